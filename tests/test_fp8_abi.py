"""fp8 dense uploads on the CPU: the header and the library agree on the new symbols, the size
rule (and its collision with bf16 at d = 9..12), the shape plan of FLTEE_OPT_FP8 with every
refusal read through fltee_debug_plan, the route word appended behind every existing one, the
format bit of the AAD, and the numpy model of the format (tests/fp8_model.py).  No device is
touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import bf16_model as BM
import fp8_model as FM
import packed_model as PM
from conftest import ROOT
from test_bf16_abi import R_BF16, R_TRIM_DENSE, R_TRIM_PACKED
from test_packed_abi import R_PACKED, host_tag
from test_plan import R_ADVANCED, R_BUBBLE, R_NIPS19, R_OPTIMIZED, R_TREE, R_TREE_LAZY, WS, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_TRIM_SELECT_DENSE, R_TRIM_SELECT_PACKED = 16, 17
R_FP8 = 18  # engine.h Route: appended after kRouteTrimSelectPacked (17)
INVALID = 0x2
NEW_SYMBOLS = ("fltee_set_upload_fp8", "fltee_upload_is_fp8", "fltee_fp8_slice_bytes",
               "fltee_unpack_fp8_device", "fltee_client_pack_fp8_device")


def test_header_declares_and_library_exports_the_fp8_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_FP8\s+0x1000u", text)
    assert re.search(r"#define\s+FLTEE_AAD_FP8_BIT\s+0x20000000u", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(L.lib(), name), f"{name} not exported"
        assert name in L.SIGNATURES
    assert L.OPT_FP8 == 0x1000 and L.AAD_FP8_BIT == 0x20000000
    # the words before the new ones keep their values
    assert (L.OPT_PACKED, L.OPT_TRIM, L.OPT_BF16, L.OPT_TRIM_SELECT) == (0x100, 0x200, 0x400, 0x800)
    assert L.AAD_PACKED_BIT == 0x80000000 and L.AAD_BF16_BIT == 0x40000000


DS = [1, 7, 8, 9, 12, 13, 16, 17, 24, 25, 1031, 50890]


@pytest.mark.parametrize("d", DS)
def test_slice_bytes(d):
    from fltee import _lib as L
    from fltee import device as D
    assert L.lib().fltee_fp8_slice_bytes(d) == FM.slice_bytes(d) == 8 * ((d + 7) // 8 + 1) == D.fp8_row(d)


# ------------------------------------------------------------------ the rule ----
@pytest.mark.parametrize("d", DS)
def test_the_fp8_call_rule(d):
    """every k_req class (0, d, another), the four slice sizes and 8 bytes on each side of them"""
    from fltee.ecalls import upload_is_bf16, upload_is_fp8, upload_is_packed
    sizes = {0}
    for base in (FM.slice_bytes(d), BM.slice_bytes(d), PM.slice_bytes(d), 8 * d):
        sizes |= {base - 8, base, base + 8, base + 4}
    for k_req in (0, d, d - 1, d + 1, 1):
        for ct in sorted(s for s in sizes if s >= 0):
            want = FM.is_fp8(True, d, k_req, ct)
            assert want == (d >= 13 and k_req in (0, d) and ct == 8 * ((d + 7) // 8 + 1))
            assert upload_is_fp8(True, d, k_req, ct) is want, (d, k_req, ct)
            assert upload_is_fp8(False, d, k_req, ct) is False  # the switch off: never
            # one payload is never two formats: every switch can be on
            assert not (want and (upload_is_packed(True, d, k_req, ct) or upload_is_bf16(True, d, k_req, ct)))
    if d >= 13:  # the four sizes differ
        assert len({FM.slice_bytes(d), BM.slice_bytes(d), PM.slice_bytes(d), 8 * d}) == 4
        assert upload_is_fp8(True, d, d, FM.slice_bytes(d)) and upload_is_fp8(True, d, 0, FM.slice_bytes(d))
    else:
        assert not upload_is_fp8(True, d, d, FM.slice_bytes(d))


def test_the_size_rule_at_the_boundary():
    """d = 9..12: an fp8 slice and a bf16 slice are both 24 bytes — such a payload is bf16 (or
    records), never fp8; from 13 on ceil(d / 4) > ceil(d / 8) + 1 at every d"""
    from fltee.ecalls import upload_is_bf16, upload_is_fp8
    for d in (9, 10, 11, 12):
        assert FM.slice_bytes(d) == BM.slice_bytes(d) == 24
        assert not upload_is_fp8(True, d, d, 24) and upload_is_bf16(True, d, d, 24)
    for d, size in ((12, 24), (13, 24), (16, 24), (17, 32)):
        assert FM.slice_bytes(d) == size
        assert upload_is_fp8(True, d, d, size) is (d >= 13)
    for d in range(13, 4200):
        assert BM.units(d) > FM.units(d)
    for d in range(1, 13):  # below: the size of a bf16 slice or more somewhere in every P class
        assert FM.units(d) >= BM.units(d)


# ------------------------------------------------------------------ the plan ----
SHAPES = [(5, 257), (5, 1026), (100, 50890), (3, 13)]


@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_flat_algs_take_the_fp8_route_with_no_scratch(alg, n, d):
    from fltee import device as D
    p = Plan(alg, n, d, d, fp8=True)
    assert p.status == 0 and p.route == R_FP8
    assert p.total == 0 and not any(p.bytes.values())
    assert D.workspace_bytes(alg, n, d, d, fp8=True) == 0
    q = Plan(alg, n, d, d, fp8=True, dense=True)  # the flag implies dense
    assert (q.status, q.route, q.bytes) == (p.status, p.route, p.bytes)
    c = Plan(alg, n, d, d, fp8=True, clip=True, clipping=0.5)  # clip: the coefficients alone
    assert c.status == 0 and c.route == R_FP8
    assert c.bytes["coef"] == n * 4 and c.total == n * 4
    assert D.workspace_bytes(alg, n, d, d, fp8=True, clip=True, clipping=0.5) == n * 4
    z = Plan(alg, n, d, d, fp8=True, trim=0)  # t = 0 is the untrimmed route itself
    assert (z.status, z.route, z.total) == (0, R_FP8, 0)


OTHER = [(1, {}, R_ADVANCED), (2, dict(seed=7), R_NIPS19), (6, dict(batch=2), R_OPTIMIZED), (7, {}, R_BUBBLE),
         (5, dict(oram_tree=True), R_TREE), (5, dict(oram_tree=True, oram_lazy=True), R_TREE_LAZY),
         (3, dict(trim=1), R_TRIM_DENSE), (4, dict(trim=2), R_TRIM_DENSE), (5, dict(trim=1), R_TRIM_DENSE),
         (3, dict(trim=2, trim_select=True), R_TRIM_SELECT_DENSE)]


@pytest.mark.parametrize("alg,kw,route", OTHER, ids=lambda x: str(x) if isinstance(x, int) else None)
@pytest.mark.parametrize("n,d", [(5, 257), (5, 1026)])
def test_other_routes_are_the_bf16_calls_plan(alg, kw, route, n, d):
    """unpack plus the existing route: every word of the plan, and the workspace bytes, are those
    of the same call with FLTEE_OPT_BF16 — the (n, d, d) records plan and n * d * 8 bytes more of
    the record scratch; a trimmed fp8 call runs the records trim (never refused, never untrimmed)"""
    from fltee import device as D
    for more in ({}, dict(clip=True, clipping=0.5)):
        b = Plan(alg, n, d, d, bf16=True, **kw, **more)
        p = Plan(alg, n, d, d, fp8=True, **kw, **more)
        assert b.status == 0 and p.status == 0 and p.route == route
        assert (p.route, p.tail, p.M, p.halo, p.bytes) == (b.route, b.tail, b.M, b.halo, b.bytes)
        assert p.bytes["rec"] == n * d * 8
        assert p.total == D.workspace_bytes(alg, n, d, d, fp8=True, **kw, **more)
        assert p.total == D.workspace_bytes(alg, n, d, d, bf16=True, **kw, **more)


@pytest.mark.parametrize("alg", [1, 2, 3, 4, 5, 6, 7])
def test_fp8_refusals(alg):
    kw = dict(batch=2) if alg == 6 else {}
    assert Plan(alg, 4, 63, 64, fp8=True, **kw).status == INVALID   # k != d
    assert Plan(alg, 4, 65, 64, fp8=True, **kw).status == INVALID
    for d in (0, 1, 2, 3, 8, 12):                                   # d < 13
        assert Plan(alg, 4, d, d, fp8=True, **kw).status == INVALID
    assert Plan(alg, 4, 13, 13, fp8=True, **kw).status == 0
    assert Plan(alg, 4, 64, 64, fp8=True, **kw).status == 0
    assert Plan(alg, 4, 64, 64, fp8=True, packed=True, **kw).status == INVALID  # with PACKED
    assert Plan(alg, 4, 64, 64, fp8=True, bf16=True, **kw).status == INVALID    # with BF16
    assert Plan(alg, 4, 64, 64, fp8=True, bf16=True, packed=True, **kw).status == INVALID
    assert Plan(alg, 4, 64, 64, packed=True, **kw).status == 0
    assert Plan(alg, 4, 64, 64, bf16=True, **kw).status == 0
    assert Plan(alg, 0, 64, 64, fp8=True, **kw).status == INVALID   # n == 0, as ever


@pytest.mark.parametrize("alg", [1, 3, 7])
def test_a_base_off_4_bytes_is_refused_by_host_arithmetic(alg):
    """the scale is read as an f32: fltee_aggregate_device refuses a base that is not 4-byte
    aligned before it touches a device (the plan itself takes no pointer); the entry points too"""
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(fp8=True)
    for ptr in (0x1001, 0x1002, 0x7F0000000003):
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(ptr), 4, 64, 64, ctypes.c_void_p(0x2000),
                                            ctypes.byref(o), None)
        assert st == INVALID
        assert L.lib().fltee_unpack_fp8_device(ctypes.c_void_p(ptr), 4, 64, ctypes.c_void_p(0x2000), None) == INVALID
        assert L.lib().fltee_client_pack_fp8_device(ctypes.c_void_p(0x2000), 4, 64, ctypes.c_void_p(ptr), None) == INVALID


def test_null_pointers_and_d_zero_are_refused():
    from fltee import _lib as L
    lib = L.lib()
    p = ctypes.c_void_p(0x2000)
    for fn in (lib.fltee_unpack_fp8_device, lib.fltee_client_pack_fp8_device):
        assert fn(None, 4, 64, p, None) == INVALID
        assert fn(p, 4, 64, None, None) == INVALID
        assert fn(p, 4, 0, p, None) == INVALID
        assert fn(p, 0, 64, p, None) == INVALID


@pytest.mark.parametrize("alg,kw", [(1, {}), (2, dict(seed=7)), (3, {}), (3, dict(dense=True)), (4, dict(dense=True)),
                                    (5, dict(oram_tree=True)), (6, dict(batch=2)), (7, {}),
                                    (3, dict(dense=True, clip=True, clipping=0.5)), (3, dict(packed=True)),
                                    (3, dict(bf16=True)), (3, dict(dense=True, trim=1)), (3, dict(bf16=True, trim=1))])
def test_plans_without_the_flag_do_not_see_it(alg, kw):
    for n, k, d in [(5, 257, 257), (5, 30, 300), (4, 13, 13)]:
        if (kw.get("dense") or kw.get("packed") or kw.get("bf16")) and k != d:
            continue
        a, b = Plan(alg, n, k, d, **kw), Plan(alg, n, k, d, fp8=False, **kw)
        assert (a.status, a.route, a.tail, a.M, a.halo, a.bytes) == (b.status, b.route, b.tail, b.M, b.halo, b.bytes)
        assert a.route != R_FP8


def test_existing_route_words_are_unchanged():
    assert R_NIPS19 == 11
    assert Plan(3, 5, 257, 257, packed=True).route == R_PACKED == 12
    assert Plan(3, 5, 257, 257, dense=True, trim=1).route == R_TRIM_DENSE == 13
    assert Plan(3, 5, 257, 257, packed=True, trim=1).route == R_TRIM_PACKED == 14
    assert Plan(3, 5, 257, 257, bf16=True).route == R_BF16 == 15
    assert Plan(3, 5, 257, 257, dense=True, trim=1, trim_select=True).route == R_TRIM_SELECT_DENSE == 16
    assert Plan(3, 5, 257, 257, packed=True, trim=1, trim_select=True).route == R_TRIM_SELECT_PACKED == 17
    assert Plan(3, 5, 257, 257, fp8=True).route == R_FP8 == 18


# ----------------------------------------------------------------- the model ----
def test_model_table_from_the_bit_fields():
    t = FM.TABLE
    assert t[0x00] == 0 and not np.signbit(t[0x00]) and t[0x80] == 0 and np.signbit(t[0x80])
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9 and t[0x08] == 2.0 ** -6
    assert t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0xFE] == -448.0
    assert t.view(np.uint32)[0x7F] == 0x7FC00000 and t.view(np.uint32)[0xFF] == 0xFFC00000
    assert np.isfinite(t[np.arange(256) & 0x7F != 0x7F]).all()  # no infinities
    assert (np.diff(t[:0x7F]) > 0).all() and np.array_equal(t[0x80:0xFF], -t[:0x7F])


def test_model_decode_then_quantise_is_the_identity():
    codes = np.arange(256, dtype=np.uint8)
    ok = (codes & 0x7F) != 0x7F
    assert np.array_equal(FM.narrow(FM.dequant(codes, np.float32(1.0)))[ok], codes[ok])
    assert np.array_equal(FM.narrow(FM.TABLE[~ok]), codes[~ok])  # a NaN keeps its sign: sign | 0x7F


def test_model_midpoints_tie_to_the_even_code_and_large_values_saturate():
    mids = FM.MIDS.astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), FM.MIDS)  # representable: exact ties
    lo = np.arange(126)
    even = np.where(lo % 2 == 0, lo, lo + 1).astype(np.uint8)
    assert np.array_equal(FM.narrow(mids), even)
    assert np.array_equal(FM.narrow(-mids), even | 0x80)
    assert np.array_equal(FM.narrow(np.nextafter(mids, np.float32(0))), lo.astype(np.uint8))
    assert np.array_equal(FM.narrow(np.nextafter(mids, np.float32(1e9))), (lo + 1).astype(np.uint8))
    big = np.array([448.0, 448.00003, 464, 480, 1e30, np.inf, -449, -np.inf], np.float32)
    assert FM.narrow(big).tolist() == [0x7E] * 6 + [0xFE] * 2
    assert FM.narrow(np.array([0.0, -0.0, 1e-45, -2.0 ** -11], np.float32)).tolist() == [0x00, 0x80, 0x00, 0x80]


def test_model_scale_and_slices():
    v = np.zeros((6, 21), np.float32)
    v[0, 3], v[0, 5] = -896.0, 2.0            # s = 2
    v[2, :4] = [np.inf, -np.inf, 4.48, 1.0]   # inf is no maximum: s = 0.01 (a / 448 rounded)
    v[3, :3] = [np.nan, -np.nan, 448.0]       # s = 1
    v[4, 0] = 1e-40                           # a / 448 is subnormal: s = 1
    v[5, 0] = 448 * 2.0 ** -126               # the smallest normal scale
    codes, s = FM.quantise(v)
    assert s.tolist() == [2.0, 1.0, float(np.float32(4.48) / np.float32(448)), 1.0, 1.0, 2.0 ** -126]
    assert codes[0, 3] == 0xFE and codes[0, 5] == 0x38 and not codes[1].any()
    assert codes[2, :3].tolist() == [0x7E, 0xFE, 0x7E] and codes[3, :3].tolist() == [0x7F, 0xFF, 0x7E]
    assert codes[4, 0] == 0 and codes[5, 0] == 0x7E
    rows = FM.pack(v)
    assert rows.dtype == np.uint8 and rows.shape == (6, 32) and rows.nbytes == 6 * FM.slice_bytes(21)
    assert not rows[:, 21:24].any() and not rows[:, 28:].any()
    assert np.array_equal(rows[:, 24:28].copy().view("<f4").reshape(-1), s)
    c2, s2 = FM.split(FM.pack(v, pad=0xFF, tail=0xFF), 21)  # padding and tail reach nothing
    assert np.array_equal(c2, codes) and np.array_equal(s2, s)
    x = FM.unpack(rows, 21)
    assert x[0, 3] == -896.0 and x[0, 5] == 2.0 and np.isnan(x[3, 0]) and x[5, 0] == v[5, 0]
    idx, val = FM.records(rows, 21)
    assert np.array_equal(idx.reshape(6, 21), np.tile(np.arange(21, dtype=np.uint32), (6, 1)))
    assert FM.same_bits(val, x.reshape(-1))


# ------------------------------------------------------------------- the AAD ----
def test_the_fp8_aad_word():
    from fltee import client as C
    ids = [7, 260, 65535]
    plain = C.ecall_aad(9, 4, ids, 3)
    assert plain == C.ecall_aad(9, 4, ids, 3, fp8=False)
    f8 = C.ecall_aad(9, 4, ids, 3, fp8=True)
    assert len({plain, f8, C.ecall_aad(9, 4, ids, 3, packed=True), C.ecall_aad(9, 4, ids, 3, bf16=True)}) == 4
    for c, cid in enumerate(ids):
        assert f8[16 * c:16 * c + 16] == FM.aad(9, 4, cid, 3, True)
        assert plain[16 * c:16 * c + 16] == FM.aad(9, 4, cid, 3, False)
        assert f8[16 * c + 12:16 * c + 16] == bytes([0x20, 0, 0, 3])


def test_an_fp8_slice_sealed_under_each_format_word():
    from fltee import client as C
    ct = np.random.default_rng(5).integers(0, 256, FM.slice_bytes(17), dtype=np.uint8).tobytes()
    iv = C.ecall_iv(11, 2)
    tags = {host_tag(300, iv, C.ecall_aad(11, 2, [300], 4, **kw), ct)
            for kw in ({}, dict(packed=True), dict(bf16=True), dict(fp8=True))}
    assert len(tags) == 4
    assert host_tag(300, iv, FM.aad(11, 2, 300, 4, True), ct) in tags
