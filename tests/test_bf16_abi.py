"""bf16 dense uploads on the CPU: the header and the library agree on the new symbols, the shape
plan of FLTEE_OPT_BF16, the numpy model of the format (tests/bf16_model.py), the bf16-call rule,
and the format bit of the AAD (host GCM tag).  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import bf16_model as BM
import packed_model as PM
from conftest import ROOT
from test_packed_abi import R_PACKED, host_tag
from test_plan import R_ADVANCED, R_BUBBLE, R_NIPS19, R_OPTIMIZED, R_TREE, R_TREE_LAZY, WS, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_TRIM_DENSE, R_TRIM_PACKED = 13, 14
R_BF16 = 15  # engine.h Route: appended after kRouteTrimPacked (14)
INVALID = 0x2
NEW_SYMBOLS = ("fltee_set_upload_bf16", "fltee_upload_is_bf16", "fltee_bf16_slice_bytes",
               "fltee_unpack_bf16_device", "fltee_client_pack_bf16_device")


def test_header_declares_and_library_exports_the_bf16_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_BF16\s+0x400u", text)
    assert re.search(r"#define\s+FLTEE_AAD_BF16_BIT\s+0x40000000u", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(L.lib(), name), f"{name} not exported"
        assert name in L.SIGNATURES
    assert L.OPT_BF16 == 0x400 and L.AAD_BF16_BIT == 0x40000000
    # the words before the new ones keep their values
    assert L.OPT_PACKED == 0x100 and L.OPT_TRIM == 0x200 and L.AAD_PACKED_BIT == 0x80000000
    assert R_NIPS19 == 11 and R_PACKED == 12


DS = list(range(1, 10)) + [50890]


@pytest.mark.parametrize("d", DS)
def test_slice_bytes(d):
    from fltee import _lib as L
    assert L.lib().fltee_bf16_slice_bytes(d) == BM.slice_bytes(d) == 8 * ((d + 3) // 4)


# ------------------------------------------------------------------ the rule ----
@pytest.mark.parametrize("d", DS)
def test_the_bf16_call_rule(d):
    """every k_req class (0, d, another), the three slice sizes and 8 bytes on each side of them"""
    from fltee.ecalls import upload_is_bf16, upload_is_packed
    sizes = set()
    for base in (BM.slice_bytes(d), PM.slice_bytes(d), 8 * d):
        sizes |= {base - 8, base, base + 8, base + 4}
    sizes |= {0}
    for k_req in (0, d, d - 1, d + 1, 1):
        for ct in sorted(s for s in sizes if s >= 0):
            want = BM.is_bf16(True, d, k_req, ct)
            assert want == (d >= 3 and k_req in (0, d) and ct == 8 * ((d + 3) // 4))
            assert upload_is_bf16(True, d, k_req, ct) is want, (d, k_req, ct)
            assert upload_is_bf16(False, d, k_req, ct) is False  # the switch off: never
            # one payload is never both formats: both switches can be on
            assert not (want and upload_is_packed(True, d, k_req, ct))
    if d >= 3:  # the three sizes differ
        assert len({BM.slice_bytes(d), PM.slice_bytes(d), 8 * d}) == 3
        assert upload_is_bf16(True, d, d, BM.slice_bytes(d)) and upload_is_bf16(True, d, 0, BM.slice_bytes(d))
    else:
        assert not upload_is_bf16(True, d, d, BM.slice_bytes(d))


# ------------------------------------------------------------------ the plan ----
SHAPES = [(5, 257), (5, 1026), (100, 50890), (3, 3)]


@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_flat_algs_take_the_bf16_route_with_no_scratch(alg, n, d):
    from fltee import device as D
    p = Plan(alg, n, d, d, bf16=True)
    assert p.status == 0 and p.route == R_BF16
    assert p.total == 0 and not any(p.bytes.values())
    assert D.workspace_bytes(alg, n, d, d, bf16=True) == 0
    # the flag implies dense; said twice it is the same plan
    q = Plan(alg, n, d, d, bf16=True, dense=True)
    assert (q.status, q.route, q.bytes) == (p.status, p.route, p.bytes)
    # clip: the coefficients alone
    c = Plan(alg, n, d, d, bf16=True, clip=True, clipping=0.5)
    assert c.status == 0 and c.route == R_BF16
    assert c.bytes["coef"] == n * 4 and c.total == n * 4
    assert D.workspace_bytes(alg, n, d, d, bf16=True, clip=True, clipping=0.5) == n * 4
    # t = 0 is the untrimmed route itself
    z = Plan(alg, n, d, d, bf16=True, trim=0)
    assert (z.status, z.route, z.total) == (0, R_BF16, 0)


OTHER = [(1, {}, R_ADVANCED), (2, dict(seed=7), R_NIPS19), (6, dict(batch=2), R_OPTIMIZED), (7, {}, R_BUBBLE),
         (5, dict(oram_tree=True), R_TREE), (5, dict(oram_tree=True, oram_lazy=True), R_TREE_LAZY),
         (3, dict(trim=1), R_TRIM_DENSE), (4, dict(trim=2), R_TRIM_DENSE), (5, dict(trim=1), R_TRIM_DENSE)]


@pytest.mark.parametrize("alg,kw,route", OTHER, ids=lambda x: str(x) if isinstance(x, int) else None)
@pytest.mark.parametrize("n,d", [(5, 257), (5, 1026)])
def test_other_routes_keep_their_plan_plus_the_unpacked_copy(alg, kw, route, n, d):
    """unpack plus the existing route: the (n, d, d) records plan and n * d * 8 bytes more of the
    record scratch — a trimmed bf16 call too, on the records trim (never refused, never the
    packed trim, never the untrimmed accumulate)"""
    from fltee import device as D
    base = Plan(alg, n, d, d, dense=("trim" in kw), **kw)
    p = Plan(alg, n, d, d, bf16=True, **kw)
    assert base.status == 0 and p.status == 0
    assert (p.route, p.tail, p.M, p.halo) == (base.route, base.tail, base.M, base.halo) and p.route == route
    for w in WS:
        grown = n * d * 8 if w == "rec" else 0
        assert p.bytes[w] == base.bytes[w] + grown, w
    assert base.bytes["rec"] == 0
    assert p.total == D.workspace_bytes(alg, n, d, d, bf16=True, **kw)
    assert p.total == D.workspace_bytes(alg, n, d, d, dense=("trim" in kw), **kw) + n * d * 8
    # clip: the unpacked copy is clipped where it is — no second copy (the trim takes coefficients)
    c = Plan(alg, n, d, d, bf16=True, clip=True, clipping=0.5, **kw)
    cb = Plan(alg, n, d, d, dense=("trim" in kw), clip=True, clipping=0.5, **kw)
    assert c.bytes["rec"] == n * d * 8 and c.bytes["coef"] == n * 4
    assert {w: c.bytes[w] for w in WS if w != "rec"} == {w: cb.bytes[w] for w in WS if w != "rec"}
    assert c.total == D.workspace_bytes(alg, n, d, d, bf16=True, clip=True, clipping=0.5, **kw)


@pytest.mark.parametrize("alg", [1, 2, 3, 4, 5, 6, 7])
def test_bf16_refusals(alg):
    kw = dict(batch=2) if alg == 6 else {}
    assert Plan(alg, 4, 63, 64, bf16=True, **kw).status == INVALID   # k != d
    assert Plan(alg, 4, 65, 64, bf16=True, **kw).status == INVALID
    for d in (0, 1, 2):                                              # d < 3
        assert Plan(alg, 4, d, d, bf16=True, **kw).status == INVALID
    assert Plan(alg, 4, 3, 3, bf16=True, **kw).status == 0
    assert Plan(alg, 4, 64, 64, bf16=True, **kw).status == 0
    assert Plan(alg, 4, 64, 64, bf16=True, packed=True, **kw).status == INVALID  # with PACKED
    assert Plan(alg, 4, 64, 64, packed=True, **kw).status == 0
    assert Plan(alg, 0, 64, 64, bf16=True, **kw).status == INVALID   # n == 0, as ever


@pytest.mark.parametrize("alg", [1, 3, 7])
def test_an_odd_pointer_is_refused_by_host_arithmetic(alg):
    """rows are read as 2-byte halves: fltee_aggregate_device refuses an odd base before it
    touches a device (the plan itself takes no pointer); the device entry points too"""
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(bf16=True)
    for ptr in (0x1001, 0x7F0000000003):
        st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(ptr), 4, 64, 64, ctypes.c_void_p(0x2000),
                                            ctypes.byref(o), None)
        assert st == INVALID
        assert L.lib().fltee_unpack_bf16_device(ctypes.c_void_p(ptr), 4, 64, ctypes.c_void_p(0x2000), None) == INVALID
        assert L.lib().fltee_client_pack_bf16_device(ctypes.c_void_p(0x2000), 4, 64, ctypes.c_void_p(ptr), None) == INVALID


def test_null_pointers_and_d_zero_are_refused():
    from fltee import _lib as L
    lib = L.lib()
    p = ctypes.c_void_p(0x2000)
    for fn in (lib.fltee_unpack_bf16_device, lib.fltee_client_pack_bf16_device):
        assert fn(None, 4, 64, p, None) == INVALID
        assert fn(p, 4, 64, None, None) == INVALID
        assert fn(p, 4, 0, p, None) == INVALID
        assert fn(p, 0, 64, p, None) == INVALID


@pytest.mark.parametrize("alg,kw", [(1, {}), (2, dict(seed=7)), (3, {}), (3, dict(dense=True)), (4, {}),
                                    (4, dict(dense=True)), (5, dict(oram_tree=True)), (6, dict(batch=2)),
                                    (7, {}), (3, dict(dense=True, clip=True, clipping=0.5)),
                                    (3, dict(packed=True)), (3, dict(dense=True, trim=1)), (3, dict(packed=True, trim=1))])
def test_plans_without_the_flag_do_not_see_it(alg, kw):
    """the same call, twice, flag off: every word the same — and none of them the new route"""
    for n, k, d in [(5, 257, 257), (5, 30, 300), (4, 3, 3)]:
        if (kw.get("dense") or kw.get("packed")) and k != d:
            continue
        a, b = Plan(alg, n, k, d, **kw), Plan(alg, n, k, d, bf16=False, **kw)
        assert (a.status, a.route, a.tail, a.M, a.halo, a.bytes) == (b.status, b.route, b.tail, b.M, b.halo, b.bytes)
        assert a.route != R_BF16


def test_existing_route_words_are_unchanged():
    assert Plan(3, 5, 257, 257, packed=True).route == R_PACKED == 12
    assert Plan(3, 5, 257, 257, dense=True, trim=1).route == R_TRIM_DENSE == 13
    assert Plan(3, 5, 257, 257, packed=True, trim=1).route == R_TRIM_PACKED == 14


# ----------------------------------------------------------------- the model ----
def test_model_narrow_on_the_listed_patterns():
    f = BM.SPECIAL_BITS.view(np.float32)
    h = BM.narrow(f)
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82,  # ties to even
            0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x3F818001: 0x3F82, 0x3F817FFF: 0x3F81,
            0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80, 0x7F7F8000: 0x7F80, 0x7F7F7FFF: 0x7F7F,  # up to inf
            0x7F800000: 0x7F80, 0xFF800000: 0xFF80, 0x00000001: 0x0000, 0x80000001: 0x8000,
            0x00008000: 0x0000, 0x00018000: 0x0002, 0x007FFFFF: 0x0080, 0x807FFFFF: 0x8080,
            0x00000000: 0x0000, 0x80000000: 0x8000,
            0x7FC00000: 0x7FC0, 0xFFC00000: 0xFFC0, 0x7F800001: 0x7FC0, 0xFF800001: 0xFFC0,  # NaNs
            0x7FA00000: 0x7FE0, 0xFFFFFFFF: 0xFFFF, 0x7F80FFFF: 0x7FC0, 0xFF808000: 0xFFC0}
    for b, got in zip(BM.SPECIAL_BITS.tolist(), h.tolist()):
        assert got == want[b], hex(b)
    nan = np.isnan(f)
    assert np.isnan(BM.widen(h[nan])).all() and not np.isnan(BM.widen(h[~nan])).any()
    assert np.array_equal(np.signbit(BM.widen(h)), np.signbit(f))


def test_model_narrow_equals_torch_off_nan_and_widen_is_exact():
    import torch
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    ok = ~np.isnan(f)
    h = BM.narrow(f)
    t = torch.from_numpy(f[ok].copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(h[ok], t)
    # every bf16 pattern widens to the f32 with the same upper half and survives the round trip
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    w = BM.widen(every)
    assert np.array_equal(w.view(np.uint32), every.astype(np.uint32) << 16)
    back = BM.narrow(w)
    snan = (every & 0x7FFF) > 0x7F80
    assert np.array_equal(back[~snan], every[~snan])
    assert np.array_equal(back[snan], every[snan] | 0x0040)


@pytest.mark.parametrize("n,d", [(1, 3), (3, 4), (4, 5), (5, 7), (6, 1026), (3, 1027)])
def test_model_pack_unpack_and_sum(n, d):
    rng = np.random.default_rng(d * 100 + n)
    v = BM.values(rng, n, d, nans=True)
    rows = BM.pack(v)
    assert rows.dtype == np.uint16 and rows.shape == (n, 4 * ((d + 3) // 4))
    assert rows.nbytes == n * BM.slice_bytes(d)
    assert not rows[:, d:].any()  # padding +0.0
    w = BM.unpack(rows, d)
    assert np.array_equal(w.view(np.uint32), BM.narrow(v).astype(np.uint32) << 16)
    idx, val = BM.records(BM.pack(v, pad=0x7FC0), d)  # the padding reaches nothing
    assert np.array_equal(idx.reshape(n, d), np.tile(np.arange(d, dtype=np.uint32), (n, 1)))
    assert np.array_equal(val.view(np.uint32), w.reshape(-1).view(np.uint32))
    clean = BM.pack(BM.values(rng, n, d))
    assert np.array_equal(BM.inorder_mean(clean, d).view(np.uint32),
                          PM.inorder_mean(BM.unpack(clean, d)).view(np.uint32))


# ------------------------------------------------------------------- the AAD ----
def test_the_bf16_aad_word():
    from fltee import client as C
    ids = [7, 260, 65535]
    plain = C.ecall_aad(9, 4, ids, 3)
    assert plain == C.ecall_aad(9, 4, ids, 3, bf16=False)
    bf = C.ecall_aad(9, 4, ids, 3, bf16=True)
    pk = C.ecall_aad(9, 4, ids, 3, packed=True)
    assert len(bf) == len(plain) == 48 and len({plain, bf, pk}) == 3
    for c, cid in enumerate(ids):
        assert bf[16 * c:16 * c + 16] == BM.aad(9, 4, cid, 3, True)
        assert plain[16 * c:16 * c + 16] == BM.aad(9, 4, cid, 3, False)
        assert bf[16 * c:16 * c + 12] == plain[16 * c:16 * c + 12]
        assert bf[16 * c + 12:16 * c + 16] == bytes([0x40, 0, 0, 3])


@pytest.mark.parametrize("d", [6, 7])
def test_a_bf16_slice_sealed_under_each_format_word(d):
    from fltee import client as C
    rng = np.random.default_rng(d)
    ct = rng.integers(0, 256, BM.slice_bytes(d), dtype=np.uint8).tobytes()  # (any ciphertext bytes)
    iv = C.ecall_iv(11, 2)
    a = host_tag(300, iv, C.ecall_aad(11, 2, [300], 4, bf16=True), ct)
    b = host_tag(300, iv, C.ecall_aad(11, 2, [300], 4), ct)
    c = host_tag(300, iv, C.ecall_aad(11, 2, [300], 4, packed=True), ct)
    assert len({a, b, c}) == 3
    assert a == host_tag(300, iv, BM.aad(11, 2, 300, 4, True), ct)
