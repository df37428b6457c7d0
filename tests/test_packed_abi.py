"""Packed dense uploads on the CPU: the header and the library agree on the new symbols, the
shape plan of FLTEE_OPT_PACKED, the numpy model of the format (tests/packed_model.py), the
packed-call rule, and the format bit of the AAD (host GCM tag).  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import packed_model as PM
from conftest import ROOT
from test_plan import R_ADVANCED, R_BUBBLE, R_NIPS19, R_OPTIMIZED, R_TREE, R_TREE_LAZY, WS, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_PACKED = 12  # engine.h Route: appended after kRouteNips19 (11)
INVALID = 0x2
NEW_SYMBOLS = ("fltee_set_upload_packed", "fltee_upload_is_packed", "fltee_packed_slice_bytes",
               "fltee_unpack_dense_device", "fltee_client_pack_dense_device")


def test_header_declares_and_library_exports_the_packed_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_PACKED\s+0x100u", text)
    assert re.search(r"#define\s+FLTEE_AAD_PACKED_BIT\s+0x80000000u", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(L.lib(), name), f"{name} not exported"
        assert name in L.SIGNATURES
    assert L.OPT_PACKED == 0x100 and L.AAD_PACKED_BIT == 0x80000000
    assert R_NIPS19 == 11  # the routes before the new one keep their words


@pytest.mark.parametrize("d", [2, 3, 4, 5, 1026, 50890])
def test_slice_bytes(d):
    from fltee import _lib as L
    assert L.lib().fltee_packed_slice_bytes(d) == PM.slice_bytes(d) == 8 * ((d + 1) // 2)


# ------------------------------------------------------------------ the plan ----
SHAPES = [(5, 257), (5, 1026), (100, 50890), (3, 2)]


@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_flat_algs_take_the_packed_route_with_no_scratch(alg, n, d):
    p = Plan(alg, n, d, d, packed=True)
    assert p.status == 0 and p.route == R_PACKED
    assert p.total == 0 and not any(p.bytes.values())
    from fltee import device as D
    assert D.workspace_bytes(alg, n, d, d, packed=True) == 0
    # the flag implies dense; said twice it is the same plan
    q = Plan(alg, n, d, d, packed=True, dense=True)
    assert (q.status, q.route, q.bytes) == (p.status, p.route, p.bytes)
    # clip: the coefficients alone
    c = Plan(alg, n, d, d, packed=True, clip=True, clipping=0.5)
    assert c.status == 0 and c.route == R_PACKED
    assert c.bytes["coef"] == n * 4 and c.total == n * 4
    assert D.workspace_bytes(alg, n, d, d, packed=True, clip=True, clipping=0.5) == n * 4


OTHER = [(1, {}, R_ADVANCED), (2, dict(seed=7), R_NIPS19), (6, dict(batch=2), R_OPTIMIZED), (7, {}, R_BUBBLE),
         (5, dict(oram_tree=True), R_TREE), (5, dict(oram_tree=True, oram_lazy=True), R_TREE_LAZY)]


@pytest.mark.parametrize("alg,kw,route", OTHER, ids=lambda x: str(x) if isinstance(x, int) else None)
@pytest.mark.parametrize("n,d", [(5, 257), (5, 1026)])
def test_other_routes_keep_their_plan_plus_the_unpacked_copy(alg, kw, route, n, d):
    from fltee import device as D
    base = Plan(alg, n, d, d, **kw)
    p = Plan(alg, n, d, d, packed=True, **kw)
    assert base.status == 0 and p.status == 0
    assert (p.route, p.tail, p.M, p.halo) == (base.route, base.tail, base.M, base.halo) and p.route == route
    for w in WS:
        grown = n * d * 8 if w == "rec" else 0
        assert p.bytes[w] == base.bytes[w] + grown, w
    assert base.bytes["rec"] == 0
    assert p.total == D.workspace_bytes(alg, n, d, d, packed=True, **kw)
    # clip: the unpacked copy is clipped where it is — no second copy
    c = Plan(alg, n, d, d, packed=True, clip=True, clipping=0.5, **kw)
    cb = Plan(alg, n, d, d, clip=True, clipping=0.5, **kw)
    assert c.bytes == cb.bytes and c.bytes["rec"] == n * d * 8
    assert c.total == D.workspace_bytes(alg, n, d, d, packed=True, clip=True, clipping=0.5, **kw)


@pytest.mark.parametrize("alg", [1, 2, 3, 4, 5, 6, 7])
def test_packed_refusals(alg):
    kw = dict(batch=2) if alg == 6 else {}
    assert Plan(alg, 4, 63, 64, packed=True, **kw).status == INVALID   # k != d
    assert Plan(alg, 4, 65, 64, packed=True, **kw).status == INVALID
    assert Plan(alg, 4, 1, 1, packed=True, **kw).status == INVALID     # d < 2
    assert Plan(alg, 4, 0, 0, packed=True, **kw).status == INVALID
    assert Plan(alg, 4, 2, 2, packed=True, **kw).status == 0
    assert Plan(alg, 0, 64, 64, packed=True, **kw).status == INVALID   # n == 0, as ever


@pytest.mark.parametrize("alg,kw", [(1, {}), (2, dict(seed=7)), (3, {}), (3, dict(dense=True)), (4, {}),
                                    (4, dict(dense=True)), (5, dict(oram_tree=True)), (6, dict(batch=2)),
                                    (7, {}), (3, dict(dense=True, clip=True, clipping=0.5))])
def test_plans_without_the_flag_do_not_see_it(alg, kw):
    """the same call, twice, flag off: every word the same — and none of them the new route"""
    for n, k, d in [(5, 257, 257), (5, 30, 300), (4, 1, 1)]:
        if kw.get("dense") and k != d:
            continue
        a, b = Plan(alg, n, k, d, **kw), Plan(alg, n, k, d, packed=False, **kw)
        assert (a.status, a.route, a.tail, a.M, a.halo, a.bytes) == (b.status, b.route, b.tail, b.M, b.halo, b.bytes)
        assert a.route != R_PACKED


# ----------------------------------------------------------------- the model ----
@pytest.mark.parametrize("n,d", [(1, 2), (3, 3), (4, 4), (5, 7), (6, 1026), (3, 1027)])
def test_model_pack_unpack_and_sum(n, d):
    rng = np.random.default_rng(d * 100 + n)
    v = PM.values(rng, n, d)
    rows = PM.pack(v)
    assert rows.shape == (n, 2 * ((d + 1) // 2)) and rows.nbytes == n * PM.slice_bytes(d)
    assert rows.nbytes * 2 == n * d * 8 + (n * 8 if d % 2 else 0)  # half the records' bytes
    if d % 2:
        assert not rows[:, d].view(np.uint32).any()  # padding +0.0
    assert np.array_equal(PM.unpack(rows, d).view(np.uint32), v.view(np.uint32))
    idx, val = PM.records(PM.pack(v, pad=np.nan), d)  # the padding reaches nothing
    assert np.array_equal(idx.reshape(n, d), np.tile(np.arange(d, dtype=np.uint32), (n, 1)))
    assert np.array_equal(val.view(np.uint32), v.reshape(-1).view(np.uint32))
    # the in-order sum, column by column in python floats rounded to f32 at each step
    want = np.zeros(d, np.float32)
    for j in range(d):
        acc = np.float32(0)
        for c in range(n):
            acc = np.float32(acc + v[c, j])
        want[j] = acc
    assert np.array_equal(PM.inorder_sum(v).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(PM.inorder_mean(v).view(np.uint32),
                          (want * (np.float32(1) / np.float32(n))).view(np.uint32))


# ------------------------------------------------------------------ the rule ----
RULE = [
    # d, k_req, ct_bytes, packed?
    (2, 2, 8, True), (2, 0, 8, True), (2, 2, 16, False),          # d = 2: U = 1; 8 d bytes: records
    (3, 3, 16, True), (3, 0, 16, True), (3, 3, 24, False), (3, 3, 8, False),
    (1, 1, 8, False), (1, 0, 8, False),                           # d = 1 is never packed
    (1026, 1026, 8 * 513, True), (1026, 0, 8 * 513, True),
    (1026, 1026, 8 * 1026, False),                                # a dense upload of records
    (1026, 513, 8 * 513, False),                                  # a k = d / 2 sparse upload
    (1027, 1027, 8 * 514, True), (1027, 1027, 8 * 513, False), (1027, 1027, 8 * 514 + 4, False),
    (1026, 1026, 0, False),                                       # not n equal slices
    (50890, 0, 8 * 25445, True), (50890, 5089, 8 * 5089, False),
]


@pytest.mark.parametrize("d,k_req,ct,want", RULE)
def test_the_packed_call_rule(d, k_req, ct, want):
    from fltee.ecalls import upload_is_packed
    assert upload_is_packed(True, d, k_req, ct) is want
    assert PM.is_packed(True, d, k_req, ct) is want
    assert upload_is_packed(False, d, k_req, ct) is False  # the switch off: never


# ------------------------------------------------------------------- the AAD ----
def test_the_packed_aad_word():
    from fltee import client as C
    ids = [7, 260, 65535]
    plain = C.ecall_aad(9, 4, ids, 3)
    assert plain == C.ecall_aad(9, 4, ids, 3, packed=False)
    packed = C.ecall_aad(9, 4, ids, 3, packed=True)
    assert len(packed) == len(plain) == 48
    for c, cid in enumerate(ids):
        assert packed[16 * c:16 * c + 16] == PM.aad(9, 4, cid, 3, True)
        assert plain[16 * c:16 * c + 16] == PM.aad(9, 4, cid, 3, False)
        assert packed[16 * c:16 * c + 12] == plain[16 * c:16 * c + 12]
        assert packed[16 * c + 12:16 * c + 16] == bytes([0x80, 0, 0, 3])


def host_tag(client_id, iv, aad, ct):
    from fltee import _lib as L
    tag = (ctypes.c_uint8 * 16)()
    st = L.lib().fltee_debug_gcm_tag_host(client_id, (ctypes.c_uint8 * 12)(*iv), (ctypes.c_uint8 * len(aad))(*aad),
                                          len(aad), (ctypes.c_uint8 * len(ct))(*ct), len(ct), tag)
    assert st == 0
    return bytes(tag)


@pytest.mark.parametrize("d", [6, 7])
def test_a_packed_slice_sealed_with_and_without_the_format_bit(d):
    from fltee import client as C
    rng = np.random.default_rng(d)
    ct = rng.integers(0, 256, PM.slice_bytes(d), dtype=np.uint8).tobytes()  # (any ciphertext bytes)
    iv = C.ecall_iv(11, 2)
    a = host_tag(300, iv, C.ecall_aad(11, 2, [300], 4, packed=True), ct)
    b = host_tag(300, iv, C.ecall_aad(11, 2, [300], 4, packed=False), ct)
    assert a != b
    assert a == host_tag(300, iv, PM.aad(11, 2, 300, 4, True), ct)
