"""FLTEE_OPT_GMED on the CPU: the header and the library agree on the flag, the iteration cap, the
options struct of a geometric-median call (fltee_device_opts untouched, two fields behind it) and
the new symbols; the shape plan of such a call — routes 21 / 22, its scratch in the `mat` slot
from (n, d) alone — and every refusal, read through fltee_debug_plan (18 words, as before) /
fltee_workspace_bytes / fltee_reserve: host arithmetic, no device."""
import ctypes
import os
import re

import pytest

import gmed_model as M
from conftest import ROOT
from test_krum_abi import (BF16, FP8, IDS, LAYOUTS, PACKED, R_KRUM_DENSE, R_KRUM_PACKED, RECORDS, OldOpts,
                           geometry)
from test_plan import WS, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_GMED_DENSE, R_GMED_PACKED = 21, 22  # engine.h Route: appended after kRouteKrumPacked (20)
INVALID = 0x2
D_ = 64
NU = M.NU


def scratch_bytes(n, d):
    """Krum's layout for the chunks' NP x NP f64 partials and G, then NP-sized w, u, rho (f64),
    alpha (f32) and valid (u32)"""
    g = geometry(n, d)
    return (g["chunks"] + 1) * g["np"] ** 2 * 8 + g["np"] * (8 + 8 + 8 + 4 + 4)


def test_header_declares_and_library_exports_the_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_GMED\s+0x4000u", text)
    assert re.search(r"#define\s+FLTEE_GMED_MAX_ITERS\s+64\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bvoid\s+fltee_set_dense_gmed\s*\(\s*uint32_t\s+iters\s*,\s*double\s+nu\s*\)", code)
    assert re.search(r"\bfltee_gmed_weights_device\s*\(", code)
    for name in ("fltee_set_dense_gmed", "fltee_gmed_weights_device"):
        assert hasattr(L.lib(), name) and name in L.SIGNATURES
    assert L.SIGNATURES["fltee_set_dense_gmed"] == (None, [ctypes.c_uint32, ctypes.c_double])
    assert L.OPT_GMED == 0x4000 and L.GMED_MAX_ITERS == 64 == M.GMED_MAX_ITERS and L.KRUM_MAX_N == M.GMED_MAX_N
    flags = [v for k, v in vars(L).items() if k.startswith("OPT_")]
    assert len(set(flags)) == len(flags)  # no flag shares a bit with another
    assert (R_KRUM_DENSE, R_KRUM_PACKED) == (19, 20)  # the words before keep their values
    assert len(WS) + 4 == 18  # fltee_debug_plan's words


def test_the_two_fields_follow_trim_in_a_struct_of_their_own():
    from fltee import _lib as L
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct fltee_device_opts \{(.*?)\} fltee_device_opts;", code, re.S).group(1)
    fields = [re.split(r"[\s\*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in L.DeviceOpts._fields_] and fields[-1] == "trim"
    assert ctypes.sizeof(L.DeviceOpts) == 72
    body = re.search(r"typedef struct fltee_device_opts_gmed \{(.*?)\} fltee_device_opts_gmed;", code, re.S).group(1)
    decls = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert decls == ["fltee_device_opts base", "size_t gmed_iters", "double gmed_nu"]
    assert issubclass(L.DeviceOptsGmed, L.DeviceOpts)
    assert (L.DeviceOptsGmed.trim.offset, L.DeviceOptsGmed.gmed_iters.offset, L.DeviceOptsGmed.gmed_nu.offset) == \
        (64, 72, 80)
    assert ctypes.sizeof(L.DeviceOptsGmed) == 88


def test_opts_sets_the_flag_and_the_fields():
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True, gmed=(3, 0.5))
    assert o.flags == L.OPT_DENSE | L.OPT_GMED and (o.gmed_iters, o.gmed_nu) == (3, 0.5)
    assert isinstance(o, L.DeviceOptsGmed)
    o = D.opts(dense=True)
    assert o.flags == L.OPT_DENSE and type(o) is L.DeviceOpts
    with pytest.raises(ValueError):
        D.opts(dense=True, gmed=(3, 0.5), krum=(1, 3))


def test_weights_without_the_flag_is_refused_before_the_fields_are_read():
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True)
    anything = ctypes.c_void_p(16)
    assert L.lib().fltee_gmed_weights_device(anything, 10, 8, ctypes.byref(o), anything, anything, None) == INVALID
    assert L.lib().fltee_gmed_weights_device(anything, 10, 8, None, anything, anything, None) == INVALID


def test_a_struct_that_ends_at_trim_is_accepted_without_the_flag():
    """the old struct at the very end of a buffer, poison behind it where the new fields would
    lie: without the flag the plan is the plan, and nothing behind the struct changes it"""
    from fltee import _lib as L
    fn = L.lib().fltee_debug_plan
    want = Plan(3, 5, 257, 257, dense=True, trim=1)
    for poison in (0x00, 0xFF):
        raw = (ctypes.c_uint8 * 88)(*([poison] * 88))
        old = OldOpts.from_buffer(raw)
        ctypes.memset(ctypes.addressof(old), 0, ctypes.sizeof(OldOpts))
        old.flags, old.trim = L.OPT_DENSE | L.OPT_TRIM, 1
        out = (ctypes.c_uint64 * 18)()
        st = fn(3, 5, 257, 257, ctypes.cast(ctypes.addressof(old), ctypes.POINTER(L.DeviceOpts)), out)
        assert st == 0 and out[0] == want.route and list(out)[4:] == list(want.bytes.values())


def test_the_python_switch_and_the_server_flags():
    from fltee import ecalls as E
    try:
        E.set_dense_gmed(3, 0.5)
        E.set_dense_gmed(0)
        assert callable(E.Enclave.set_dense_gmed)
        with pytest.raises(ValueError):
            E.set_dense_gmed(-1, 0.5)
    finally:
        E.set_dense_gmed(0, 0.0)
    import inspect

    from fltee.server import Aggregator
    assert inspect.signature(Aggregator.__init__).parameters["gmed"].default is None
    src = open(os.path.join(ROOT, "fl-tee_amd", "fltee", "grpc_server.py")).read()
    assert '"--gmed-iters"' in src and '"--gmed-nu"' in src


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
@pytest.mark.parametrize("n,iters", [(1, 1), (2, 3), (7, 8), (100, 64), (129, 1), (1024, 2)])
def test_flat_algs_take_the_gmed_routes(alg, n, iters):
    d = D_
    for layout, route in ((RECORDS, R_GMED_DENSE), (PACKED, R_GMED_PACKED), (BF16, R_GMED_DENSE),
                          (FP8, R_GMED_DENSE)):
        p = Plan(alg, n, d, d, gmed=(iters, NU), **layout)
        assert p.status == 0 and p.route == route, (layout, p.status, p.route)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
@pytest.mark.parametrize("clip", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
@pytest.mark.parametrize("n,d", [(1, 1), (16, 4), (17, 64), (100, 1000000), (128, 257), (129, 50890), (300, 50890),
                                 (1000, 100000), (1024, 64), (5, (1 << 18) + 7)])
def test_the_scratch_is_the_mat_slot_from_n_and_d(layout, clip, n, d):
    from fltee import device as D
    if (layout is FP8 and d < 13) or (layout is BF16 and d < 3) or (layout is PACKED and d < 2):
        return
    p = Plan(3, n, d, d, gmed=(3, NU), **layout, **clip)
    assert p.status == 0
    want = dict.fromkeys(WS, 0)
    want["mat"] = scratch_bytes(n, d)
    if clip:
        want["coef"] = n * 4
    if layout in (BF16, FP8):
        want["rec"] = n * d * 8
    assert p.bytes == want
    assert D.workspace_bytes(3, n, d, d, gmed=(3, NU), **layout, **clip) == sum(want.values())
    # R and nu do not move a byte
    assert Plan(3, n, d, d, gmed=(64, 1e300), **layout, **clip).bytes == want
    assert Plan(3, n, d, d, gmed=(1, 5e-324), **layout, **clip).bytes == want


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_refusals(layout):
    d = D_
    ok = dict(gmed=(3, NU))
    assert not refused(3, 10, d, d, **ok, **layout)
    for alg, kw in [(1, {}), (2, dict(seed=7)), (6, dict(batch=2)), (7, {})]:  # an alg other than 3, 4, 5
        assert refused(alg, 10, d, d, **ok, **layout, **kw)
        assert Plan(alg, 10, d, d, **layout, **kw).status == 0
    assert refused(9, 10, d, d, **ok, **layout)
    for tree in (dict(oram_tree=True), dict(oram_tree=True, oram_lazy=True), dict(oram_lazy=True)):
        assert refused(5, 10, d, d, **ok, **layout, **tree)
    assert refused(3, 0, d, d, **ok, **layout)                      # n = 0
    assert not refused(3, 1, d, d, **ok, **layout)
    assert not refused(3, 1024, d, d, **ok, **layout)               # FLTEE_KRUM_MAX_N
    assert refused(3, 1025, d, d, **ok, **layout)
    for iters in (0, 65, 2 ** 32, 2 ** 64 - 1):                     # R = 0, R > 64
        assert refused(3, 10, d, d, gmed=(iters, NU), **layout) == M.refused(10, iters, NU) is True
    for iters in (1, 64):
        assert not refused(3, 10, d, d, gmed=(iters, NU), **layout)
    for nu in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan")):  # not a finite value above 0
        assert refused(3, 10, d, d, gmed=(3, nu), **layout) and M.refused(10, 3, nu)
    for nu in (5e-324, 1.0, 1.7e308):
        assert not refused(3, 10, d, d, gmed=(3, nu), **layout)
    # together with the trim, Multi-Krum or NO_AVERAGE
    assert refused(3, 10, d, d, trim=1, **ok, **layout)
    assert refused(3, 10, d, d, trim=0, **ok, **layout)
    assert refused(3, 10, d, d, trim=1, trim_select=True, **ok, **layout)
    assert refused(3, 10, d, d, no_average=True, **ok, **layout)
    assert refused(3, 10, d, d, no_average=True, accumulate=True, **ok, **layout)
    assert not refused(3, 10, d, d, accumulate=True, n_avg=7, **ok, **layout)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_the_flag_together_with_krum_is_refused(layout):
    """two flags, one pointer: a struct that holds Krum's counts where the median's fields lie —
    whatever they read as, the pair is refused"""
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(krum=(1, 3), **layout)
    o.flags |= L.OPT_GMED
    out = (ctypes.c_uint64 * 18)()
    assert L.lib().fltee_debug_plan(3, 10, D_, D_, ctypes.byref(o), out) == INVALID
    assert L.lib().fltee_reserve(3, 10, D_, D_, ctypes.byref(o)) == INVALID
    o = D.opts(gmed=(3, NU), **layout)
    o.flags |= L.OPT_KRUM
    assert L.lib().fltee_debug_plan(3, 10, D_, D_, ctypes.byref(o), out) == INVALID


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_a_call_that_is_not_dense_is_refused(alg):
    assert refused(alg, 20, 8, 64, gmed=(3, NU))               # sparse
    assert refused(alg, 20, 64, 64, gmed=(3, NU))              # dense-sized, not declared dense
    assert refused(alg, 20, 8, 64, gmed=(3, NU), dense=True)   # k != d


@pytest.mark.parametrize("alg,kw", [(1, {}), (3, {}), (3, dict(dense=True)), (3, dict(packed=True)),
                                    (3, dict(dense=True, trim=3)), (3, dict(fp8=True)),
                                    (4, dict(dense=True, clip=True, clipping=0.5)), (5, dict(oram_tree=True)), (7, {})])
def test_plans_without_the_flag_never_take_the_new_routes_and_ignore_the_fields(alg, kw):
    from fltee import _lib as L
    from fltee import device as D
    for n, k, d in [(200, 257, 257), (5, 30, 300)]:
        if (kw.get("dense") or kw.get("packed") or kw.get("fp8")) and k != d:
            continue
        p = Plan(alg, n, k, d, **kw)
        assert p.route not in (R_GMED_DENSE, R_GMED_PACKED)
        o = D.opts(gmed=(0xDEADBEEF, float("nan")), **kw)
        o.flags &= ~L.OPT_GMED  # the fields are there, the flag is not: never read
        out = (ctypes.c_uint64 * 18)()
        assert L.lib().fltee_debug_plan(alg, n, k, d, ctypes.byref(o), out) == p.status
        assert out[0] == p.route and list(out)[4:] == list(p.bytes.values())
