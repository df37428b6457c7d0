"""FLTEE_OPT_TRIM on the CPU: the header and the library agree on the new flag, field and
symbols; the shape plan of a trimmed call (route, no scratch) and every refusal, read through
fltee_debug_plan / fltee_workspace_bytes / fltee_reserve — host arithmetic, no device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_packed_abi import R_PACKED
from test_plan import R_DENSE, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_TRIM_DENSE, R_TRIM_PACKED = 13, 14  # engine.h Route: appended after kRoutePacked (12)
INVALID = 0x2
NEW_SYMBOLS = ("fltee_trim_count", "fltee_set_dense_trim")


def test_header_declares_and_library_exports_the_trim_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_TRIM\s+0x200u", text)
    assert re.search(r"#define\s+FLTEE_TRIM_MAX\s+64\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(L.lib(), name), f"{name} not exported"
        assert name in L.SIGNATURES
    assert L.SIGNATURES["fltee_trim_count"] == (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_uint32])
    assert L.SIGNATURES["fltee_set_dense_trim"] == (None, [ctypes.c_uint32])
    assert L.OPT_TRIM == 0x200 and L.TRIM_MAX == 64
    assert R_PACKED == 12  # the routes before the new ones keep their words


def test_trim_is_the_last_field_of_the_options():
    from fltee import _lib as L
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct fltee_device_opts \{(.*?)\} fltee_device_opts;", code, re.S).group(1)
    fields = [re.split(r"[\s\*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in L.DeviceOpts._fields_]
    assert fields[-1] == "trim" and fields[-2] == "d_status"
    assert L.DeviceOpts.trim.offset + ctypes.sizeof(ctypes.c_size_t) == ctypes.sizeof(L.DeviceOpts)
    assert L.DeviceOpts.d_status.offset == 56  # what was there has not moved


def test_opts_sets_flag_and_field():
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True, trim=3)
    assert o.flags == L.OPT_DENSE | L.OPT_TRIM and o.trim == 3
    assert D.opts(dense=True).flags == L.OPT_DENSE and D.opts(dense=True).trim == 0
    assert D.opts(trim=0).flags == L.OPT_TRIM


def test_a_caller_of_the_old_struct_is_not_read_past_its_end():
    """without the flag the field is never read: a plan asked with garbage in it is the plan"""
    from fltee import device as D
    o = D.opts(dense=True)
    o.trim = 0xDEADBEEF
    from fltee import _lib as L
    out = (ctypes.c_uint64 * 18)()
    assert L.lib().fltee_debug_plan(3, 5, 257, 257, ctypes.byref(o), out) == 0 and out[0] == R_DENSE


# ------------------------------------------------------------------ the plan ----
@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,d,t", [(3, 2, 1), (5, 257, 2), (100, 50890, 49), (129, 1101, 64), (130, 64, 64)])
def test_flat_algs_take_the_trimmed_routes_with_no_scratch(alg, n, d, t):
    from fltee import device as D
    for layout, route, plain in ((dict(dense=True), R_TRIM_DENSE, R_DENSE),
                                 (dict(packed=True), R_TRIM_PACKED, R_PACKED)):
        p = Plan(alg, n, d, d, trim=t, **layout)
        assert p.status == 0 and p.route == route
        assert p.total == 0 and not any(p.bytes.values())
        # the same figure as the untrimmed dense call
        assert D.workspace_bytes(alg, n, d, d, trim=t, **layout) == D.workspace_bytes(alg, n, d, d, **layout) == 0
        # clip: the coefficients alone, no clipped copy of the records
        c = Plan(alg, n, d, d, trim=t, clip=True, clipping=0.5, **layout)
        assert c.status == 0 and c.route == route and c.bytes["coef"] == n * 4 and c.total == n * 4
        assert D.workspace_bytes(alg, n, d, d, trim=t, clip=True, clipping=0.5, **layout) == \
            D.workspace_bytes(alg, n, d, d, clip=True, clipping=0.5, **layout) == n * 4
        # t = 0: the untrimmed route itself
        z = Plan(alg, n, d, d, trim=0, **layout)
        assert z.status == 0 and z.route == plain and z.total == 0


def refused(alg, n, k, d, **kw):
    """the plan's status, and fltee_reserve answering the same before it looks for a device"""
    from fltee import _lib as L
    from fltee import device as D
    st = Plan(alg, n, k, d, **kw).status
    o = D.opts(**kw)
    rs = L.lib().fltee_reserve(alg, n, k, d, ctypes.byref(o))
    assert (rs == INVALID) == (st == INVALID)
    return st == INVALID


@pytest.mark.parametrize("layout", [dict(dense=True), dict(packed=True)], ids=["records", "packed"])
def test_trim_refusals(layout):
    n, d = 10, 64
    assert not refused(3, n, d, d, trim=4, **layout)
    assert refused(3, n, d, d, trim=5, **layout)             # 2 t >= n
    assert refused(3, 2, d, d, trim=1, **layout)
    assert not refused(3, 3, d, d, trim=1, **layout)
    assert not refused(3, 129, d, d, trim=64, **layout)      # FLTEE_TRIM_MAX
    assert refused(3, 131, d, d, trim=65, **layout)          # past it
    assert refused(3, 1000, d, d, trim=65, **layout)
    assert refused(3, n, d, d, trim=2 ** 63, **layout)       # (2 t wraps: still refused)
    for alg, kw in [(1, {}), (2, dict(seed=7)), (6, dict(batch=2)), (7, {})]:  # any other alg
        assert refused(alg, n, d, d, trim=1, **layout, **kw)
        assert refused(alg, n, d, d, trim=0, **layout, **kw)
        assert Plan(alg, n, d, d, **layout, **kw).status == 0
    for tree in (dict(oram_tree=True), dict(oram_tree=True, oram_lazy=True), dict(oram_lazy=True)):
        assert refused(5, n, d, d, trim=1, **layout, **tree)
    assert refused(9, n, d, d, trim=1, **layout)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_a_call_that_is_not_dense_is_refused(alg):
    assert refused(alg, 10, 8, 64, trim=1)                   # sparse
    assert refused(alg, 10, 64, 64, trim=1)                  # dense-sized, not declared dense
    assert refused(alg, 10, 8, 64, trim=1, dense=True)       # k != d
    assert refused(alg, 10, 64, 64, trim=0)


@pytest.mark.parametrize("alg,kw", [(1, {}), (3, {}), (3, dict(dense=True)), (3, dict(packed=True)),
                                    (4, dict(dense=True, clip=True, clipping=0.5)), (5, dict(oram_tree=True)), (7, {})])
def test_plans_without_the_flag_do_not_see_it(alg, kw):
    for n, k, d in [(5, 257, 257), (5, 30, 300)]:
        if (kw.get("dense") or kw.get("packed")) and k != d:
            continue
        a, b = Plan(alg, n, k, d, **kw), Plan(alg, n, k, d, trim=None, **kw)
        assert (a.status, a.route, a.tail, a.M, a.halo, a.bytes) == (b.status, b.route, b.tail, b.M, b.halo, b.bytes)
        assert a.route not in (R_TRIM_DENSE, R_TRIM_PACKED)


def test_the_switch_clamps_and_the_python_wrappers_validate():
    from fltee import ecalls as E
    from fltee.server import per_mille
    import argparse
    try:
        E.set_dense_trim(500)
        E.set_dense_trim(0)
        for bad in (-1, 501):
            with pytest.raises(ValueError):
                E.set_dense_trim(bad)
    finally:
        E.set_dense_trim(0)
    assert per_mille("0") == 0 and per_mille("500") == 500
    for bad in ("501", "-1", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            per_mille(bad)
