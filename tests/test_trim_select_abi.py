"""FLTEE_OPT_TRIM_SELECT on the CPU: the header and the library agree on the new flag, the cap
and the switch; the shape plan of a call trimmed by selection — routes 16 / 17, the list
route's scratch and nothing more — and every refusal, read through fltee_debug_plan (18
words, as before) / fltee_workspace_bytes / fltee_reserve: host arithmetic, no device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_bf16_abi import R_BF16
from test_packed_abi import R_PACKED
from test_plan import R_DENSE, WS, Plan
from test_trim_abi import R_TRIM_DENSE, R_TRIM_PACKED

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_SELECT_DENSE, R_SELECT_PACKED = 16, 17  # engine.h Route: appended after kRouteBf16 (15)
INVALID = 0x2
D_ = 64
RECORDS, PACKED, BF16 = dict(dense=True), dict(packed=True), dict(bf16=True)
LAYOUTS = [RECORDS, PACKED, BF16]
IDS = ["records", "packed", "bf16"]


def test_header_declares_and_library_exports_the_switch():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_TRIM_SELECT\s+0x800u", text)
    assert re.search(r"#define\s+FLTEE_TRIM_SELECT_MAX_N\s+4096\b", text)
    assert re.search(r"#define\s+FLTEE_TRIM_MAX\s+64\b", text)  # the list kernel's cap keeps its meaning
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bvoid\s+fltee_set_dense_trim_select\s*\(\s*int\s+on\s*\)", code)
    assert hasattr(L.lib(), "fltee_set_dense_trim_select")
    assert L.SIGNATURES["fltee_set_dense_trim_select"] == (None, [ctypes.c_int])
    assert L.OPT_TRIM_SELECT == 0x800 and L.TRIM_SELECT_MAX_N == 4096 and L.TRIM_MAX == 64
    assert (R_PACKED, R_TRIM_DENSE, R_TRIM_PACKED, R_BF16) == (12, 13, 14, 15)  # the words before keep their values
    assert len(WS) + 4 == 18  # fltee_debug_plan's words


def test_opts_sets_the_flag():
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True, trim=70, trim_select=True)
    assert o.flags == L.OPT_DENSE | L.OPT_TRIM | L.OPT_TRIM_SELECT and o.trim == 70
    assert D.opts(dense=True, trim=70).flags == L.OPT_DENSE | L.OPT_TRIM
    assert D.opts(trim_select=True).flags == L.OPT_TRIM_SELECT


def test_the_python_switch_and_the_server_flag():
    from fltee import ecalls as E
    try:
        E.set_dense_trim_select(True)
        E.set_dense_trim_select(False)
        assert callable(E.Enclave.set_dense_trim_select)
    finally:
        E.set_dense_trim_select(False)
    import inspect

    from fltee.server import Aggregator
    assert inspect.signature(Aggregator.__init__).parameters["trim_select"].default is False


def refused(alg, n, k, d, **kw):
    """the plan's status, and fltee_reserve answering the same before it looks for a device"""
    from fltee import _lib as L
    from fltee import device as D
    st = Plan(alg, n, k, d, **kw).status
    assert st in (0, INVALID)
    o = D.opts(**kw)
    rs = L.lib().fltee_reserve(alg, n, k, d, ctypes.byref(o))
    assert (rs == INVALID) == (st == INVALID)
    return st == INVALID


@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,t", [(131, 65), (1000, 499), (4096, 2047), (1000, 100), (100, 49), (3, 1)])
def test_flat_algs_take_the_selection_routes(alg, n, t):
    d = D_
    for layout, route in ((RECORDS, R_SELECT_DENSE), (PACKED, R_SELECT_PACKED), (BF16, R_SELECT_DENSE)):
        p = Plan(alg, n, d, d, trim=t, trim_select=True, **layout)
        assert p.status == 0 and p.route == route, (layout, p.status, p.route)
        # without the flag: the list route up to FLTEE_TRIM_MAX, refused past it
        q = Plan(alg, n, d, d, trim=t, **layout)
        assert (q.status == INVALID) == (t > 64)
        if t <= 64:
            assert q.route == (R_TRIM_PACKED if layout is PACKED else R_TRIM_DENSE)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
@pytest.mark.parametrize("clip", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
@pytest.mark.parametrize("n,t", [(131, 65), (1000, 499), (4096, 2047), (129, 64), (17, 3)])
def test_the_scratch_is_the_list_routes(layout, clip, n, t):
    """no buffer of its own: every size, and fltee_workspace_bytes, equal those of the same
    call with t = min(t, 64) on the list route — nothing; coef under CLIP; rec = n d 8 for bf16"""
    from fltee import device as D
    d = D_
    sel = Plan(3, n, d, d, trim=t, trim_select=True, **layout, **clip)
    lst = Plan(3, n, d, d, trim=min(t, 64), **layout, **clip)
    assert sel.status == 0 and lst.status == 0
    assert sel.bytes == lst.bytes
    want = dict.fromkeys(WS, 0)
    if clip:
        want["coef"] = n * 4
    if layout is BF16:
        want["rec"] = n * d * 8
    assert sel.bytes == want
    assert D.workspace_bytes(3, n, d, d, trim=t, trim_select=True, **layout, **clip) == \
        D.workspace_bytes(3, n, d, d, trim=min(t, 64), **layout, **clip) == sum(want.values())


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_refusals(layout):
    d = D_
    sel = dict(trim_select=True, **layout)
    for n, t in [(131, 65), (1000, 499)]:
        assert not refused(3, n, d, d, trim=t, **sel)
        assert refused(3, n, d, d, trim=t, **layout)            # without the flag: past the lists
    assert not refused(3, 4096, d, d, trim=2047, **sel)        # FLTEE_TRIM_SELECT_MAX_N
    assert refused(3, 4097, d, d, trim=2047, **sel)            # past it
    assert refused(3, 4097, d, d, trim=1, **sel)
    assert not refused(3, 4097, d, d, trim=1, **layout)        # (the list route has no cap on n)
    assert refused(3, 130, d, d, trim=65, **sel)               # 2 t >= n
    assert not refused(3, 131, d, d, trim=65, **sel)
    assert refused(3, 1000, d, d, trim=500, **sel)
    assert refused(3, 2, d, d, trim=1, **sel)
    assert refused(3, 1000, d, d, trim=2 ** 63, **sel)         # (2 t wraps to 0: still refused)
    assert refused(3, 1000, d, d, trim=2 ** 63 + 1, **sel)
    assert refused(3, 1000, d, d, trim=2 ** 64 - 1, **sel)
    for alg, kw in [(1, {}), (2, dict(seed=7)), (6, dict(batch=2)), (7, {})]:  # any other alg
        assert refused(alg, 10, d, d, trim=1, **sel, **kw)
        assert refused(alg, 10, d, d, trim=0, **sel, **kw)
        assert refused(alg, 10, d, d, **sel, **kw)             # the flag without TRIM
        assert Plan(alg, 10, d, d, **layout, **kw).status == 0
    for tree in (dict(oram_tree=True), dict(oram_tree=True, oram_lazy=True), dict(oram_lazy=True)):
        assert refused(5, 10, d, d, trim=1, **sel, **tree)
    assert refused(9, 10, d, d, trim=1, **sel)
    for alg in (3, 4, 5):
        assert refused(alg, 131, d, d, **sel)                  # the flag without FLTEE_OPT_TRIM
        assert not refused(alg, 131, d, d, **layout)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_a_call_that_is_not_dense_is_refused(alg):
    assert refused(alg, 200, 8, 64, trim=70, trim_select=True)               # sparse
    assert refused(alg, 200, 64, 64, trim=70, trim_select=True)              # dense-sized, not declared dense
    assert refused(alg, 200, 8, 64, trim=70, trim_select=True, dense=True)   # k != d
    assert refused(alg, 200, 64, 64, trim=0, trim_select=True)


@pytest.mark.parametrize("layout,plain", [(RECORDS, R_DENSE), (PACKED, R_PACKED), (BF16, R_BF16)], ids=IDS)
def test_t_zero_is_the_untrimmed_route(layout, plain):
    for n in (5, 131, 1000):
        z = Plan(3, n, D_, D_, trim=0, trim_select=True, **layout)
        u = Plan(3, n, D_, D_, **layout)
        assert z.status == 0 and z.route == plain == u.route and z.bytes == u.bytes and z.total == 0


@pytest.mark.parametrize("alg,kw", [(1, {}), (3, {}), (3, dict(dense=True)), (3, dict(packed=True)),
                                    (3, dict(dense=True, trim=3)), (3, dict(packed=True, trim=64)),
                                    (4, dict(dense=True, clip=True, clipping=0.5)), (5, dict(oram_tree=True)), (7, {})])
def test_plans_without_the_flag_never_take_the_new_routes(alg, kw):
    for n, k, d in [(200, 257, 257), (5, 30, 300)]:
        if (kw.get("dense") or kw.get("packed")) and k != d:
            continue
        assert Plan(alg, n, k, d, **kw).route not in (R_SELECT_DENSE, R_SELECT_PACKED)
