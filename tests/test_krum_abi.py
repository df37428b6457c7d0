"""FLTEE_OPT_KRUM on the CPU: the header and the library agree on the flag, the cap, the options
struct of a Krum call (fltee_device_opts untouched, two fields behind it) and the new symbols; the shape plan of a Multi-Krum call — routes 19 / 20, its
scratch in the `mat` slot from (n, d) alone — and every refusal, read through fltee_debug_plan
(18 words, as before) / fltee_workspace_bytes / fltee_reserve: host arithmetic, no device."""
import ctypes
import os
import re

import pytest

import krum_model as KM
from conftest import ROOT
from test_fp8_abi import R_FP8
from test_packed_abi import R_PACKED
from test_plan import R_DENSE, WS, Plan

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

HEADER = os.path.join(ROOT, "include", "fltee_agg.h")
R_KRUM_DENSE, R_KRUM_PACKED = 19, 20  # engine.h Route: appended after kRouteFp8 (18)
INVALID = 0x2
D_ = 64
RECORDS, PACKED, BF16, FP8 = dict(dense=True), dict(packed=True), dict(bf16=True), dict(fp8=True)
LAYOUTS = [RECORDS, PACKED, BF16, FP8]
IDS = ["records", "packed", "bf16", "fp8"]


def geometry(n, d):
    """the Gram pass's geometry as k_krum.hip states it: 16-row tiles, 128-row macro-tiles, column
    chunks of a multiple of 16 and at least 256 columns aiming at 512 blocks"""
    tiles = (n + 15) // 16
    macros = (tiles + 7) // 8
    target = max(1, 512 // (macros * (macros + 1) // 2))
    cols = max(256, ((d + target - 1) // target + 15) // 16 * 16)
    return dict(np=tiles * 16, tiles=tiles, macros=macros, cols=cols, chunks=max(1, (d + cols - 1) // cols))


def scratch_bytes(n, d):
    """the chunks' NP x NP f64 partials, G, NP f64 scores, NP u32 keep words"""
    g = geometry(n, d)
    return (g["chunks"] + 1) * g["np"] ** 2 * 8 + g["np"] * 8 + g["np"] * 4


def test_header_declares_and_library_exports_the_symbols():
    from fltee import _lib as L
    text = open(HEADER).read()
    assert re.search(r"#define\s+FLTEE_OPT_KRUM\s+0x2000u", text)
    assert re.search(r"#define\s+FLTEE_KRUM_MAX_N\s+1024\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bvoid\s+fltee_set_dense_krum\s*\(\s*uint32_t\s+f\s*,\s*uint32_t\s+m\s*\)", code)
    assert re.search(r"\bfltee_krum_select_device\s*\(", code)
    for name in ("fltee_set_dense_krum", "fltee_krum_select_device"):
        assert hasattr(L.lib(), name) and name in L.SIGNATURES
    assert L.SIGNATURES["fltee_set_dense_krum"] == (None, [ctypes.c_uint32, ctypes.c_uint32])
    assert L.OPT_KRUM == 0x2000 and L.KRUM_MAX_N == 1024 == KM.KRUM_MAX_N
    flags = [v for k, v in vars(L).items() if k.startswith("OPT_")]
    assert len(set(flags)) == len(flags)  # no flag shares a bit with another
    assert (R_DENSE, R_PACKED, R_FP8) == (1, 12, 18)  # the words before keep their values
    assert len(WS) + 4 == 18  # fltee_debug_plan's words


def test_the_two_fields_follow_trim_in_a_struct_of_their_own():
    """fltee_device_opts still ends at trim (72 bytes); fltee_device_opts_krum is that struct
    with krum_f, krum_m behind it, and ctypes mirrors both"""
    from fltee import _lib as L
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct fltee_device_opts \{(.*?)\} fltee_device_opts;", code, re.S).group(1)
    fields = [re.split(r"[\s\*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in L.DeviceOpts._fields_] and fields[-1] == "trim"
    assert ctypes.sizeof(L.DeviceOpts) == 72
    body = re.search(r"typedef struct fltee_device_opts_krum \{(.*?)\} fltee_device_opts_krum;", code, re.S).group(1)
    decls = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert decls == ["fltee_device_opts base", "size_t krum_f", "size_t krum_m"]
    assert issubclass(L.DeviceOptsKrum, L.DeviceOpts)
    assert (L.DeviceOptsKrum.trim.offset, L.DeviceOptsKrum.krum_f.offset, L.DeviceOptsKrum.krum_m.offset) == (64, 72, 80)
    assert ctypes.sizeof(L.DeviceOptsKrum) == 88


def test_opts_sets_the_flag_and_the_fields():
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True, krum=(2, 5))
    assert o.flags == L.OPT_DENSE | L.OPT_KRUM and (o.krum_f, o.krum_m) == (2, 5)
    assert isinstance(o, L.DeviceOptsKrum)
    o = D.opts(dense=True)
    assert o.flags == L.OPT_DENSE and type(o) is L.DeviceOpts


def test_select_without_the_flag_is_refused_before_the_fields_are_read():
    """the flag is the caller's word that krum_f, krum_m lie behind the struct: a plain
    fltee_device_opts is answered 0x2 by host arithmetic, no device touched"""
    from fltee import _lib as L
    from fltee import device as D
    o = D.opts(dense=True)
    anything = ctypes.c_void_p(16)
    assert L.lib().fltee_krum_select_device(anything, 10, 8, ctypes.byref(o), anything, anything, None) == INVALID
    assert L.lib().fltee_krum_select_device(anything, 10, 8, None, anything, anything, None) == INVALID


class OldOpts(ctypes.Structure):
    """fltee_device_opts as it ended at `trim`"""
    _fields_ = [("flags", ctypes.c_uint32), ("sigma", ctypes.c_float), ("clipping", ctypes.c_float),
                ("seed", ctypes.c_uint64), ("k_req", ctypes.c_size_t), ("batch", ctypes.c_size_t),
                ("n_avg", ctypes.c_size_t), ("fold_halo", ctypes.c_size_t), ("d_status", ctypes.c_void_p),
                ("trim", ctypes.c_size_t)]


def test_a_struct_that_ends_at_trim_is_accepted_without_the_flag():
    """the old struct at the very end of a buffer, poison behind it where the new fields would
    lie: without the flag the plan is the plan, and nothing behind the struct changes it"""
    from fltee import _lib as L
    assert ctypes.sizeof(OldOpts) == 72
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


def test_the_python_switch_and_the_server_flag():
    from fltee import ecalls as E
    try:
        E.set_dense_krum(2, 5)
        E.set_dense_krum(0, 0)
        assert callable(E.Enclave.set_dense_krum)
        with pytest.raises(ValueError):
            E.set_dense_krum(-1, 3)
    finally:
        E.set_dense_krum(0, 0)
    import inspect

    from fltee.server import Aggregator
    assert inspect.signature(Aggregator.__init__).parameters["krum"].default is None
    src = open(os.path.join(ROOT, "fl-tee_amd", "fltee", "grpc_server.py")).read()
    assert '"--krum-f"' in src and '"--krum-m"' in src


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
@pytest.mark.parametrize("n,f,m", [(3, 0, 1), (7, 2, 5), (100, 10, 90), (129, 63, 1), (1024, 100, 924)])
def test_flat_algs_take_the_krum_routes(alg, n, f, m):
    d = D_
    for layout, route in ((RECORDS, R_KRUM_DENSE), (PACKED, R_KRUM_PACKED), (BF16, R_KRUM_DENSE),
                          (FP8, R_KRUM_DENSE)):
        p = Plan(alg, n, d, d, krum=(f, m), **layout)
        assert p.status == 0 and p.route == route, (layout, p.status, p.route)


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
@pytest.mark.parametrize("clip", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
@pytest.mark.parametrize("n,d", [(3, 1), (16, 4), (17, 64), (100, 1000000), (128, 257), (129, 50890), (300, 50890),
                                 (1000, 100000), (1024, 64), (5, (1 << 18) + 7)])
def test_the_scratch_is_the_mat_slot_from_n_and_d(layout, clip, n, d):
    from fltee import _lib as L
    from fltee import device as D
    if (layout is FP8 and d < 13) or (layout is BF16 and d < 3) or (layout is PACKED and d < 2):
        return
    f, m = (n - 3) // 2, 1
    p = Plan(3, n, d, d, krum=(f, m), **layout, **clip)
    assert p.status == 0
    want = dict.fromkeys(WS, 0)
    want["mat"] = scratch_bytes(n, d)
    if clip:
        want["coef"] = n * 4
    if layout in (BF16, FP8):
        want["rec"] = n * d * 8
    assert p.bytes == want
    assert D.workspace_bytes(3, n, d, d, krum=(f, m), **layout, **clip) == sum(want.values())
    # (f, m) do not move a byte: q and m are compare constants
    assert Plan(3, n, d, d, krum=(0, n), **layout, **clip).bytes == want
    out = (ctypes.c_uint64 * 6)()
    L.lib().fltee_debug_krum_geometry(n, d, out)
    g = geometry(n, d)
    assert list(out) == [g["np"], g["tiles"], g["macros"], g["cols"], g["chunks"], scratch_bytes(n, d)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_refusals(layout):
    d = D_
    for n in range(3, 40):
        for f in range(0, 20):
            for m in (0, 1, n - f - 1, n - f, n - f + 1):
                if m < 0:
                    continue
                assert refused(3, n, d, d, krum=(f, m), **layout) == KM.refused(n, f, m), (n, f, m)
    assert not refused(3, 1024, d, d, krum=(0, 1), **layout)       # FLTEE_KRUM_MAX_N
    assert refused(3, 1025, d, d, krum=(0, 1), **layout)
    assert refused(3, 2, d, d, krum=(0, 1), **layout)              # n < 3
    assert refused(3, 100, d, d, krum=(2 ** 63, 1), **layout)      # (2 f wraps to 0: still refused)
    assert refused(3, 100, d, d, krum=(2 ** 64 - 1, 1), **layout)
    assert refused(3, 100, d, d, krum=(1, 2 ** 64 - 1), **layout)
    for alg, kw in [(1, {}), (2, dict(seed=7)), (6, dict(batch=2)), (7, {})]:  # any other alg
        assert refused(alg, 10, d, d, krum=(1, 3), **layout, **kw)
        assert Plan(alg, 10, d, d, **layout, **kw).status == 0
    for tree in (dict(oram_tree=True), dict(oram_tree=True, oram_lazy=True), dict(oram_lazy=True)):
        assert refused(5, 10, d, d, krum=(1, 3), **layout, **tree)
    assert refused(9, 10, d, d, krum=(1, 3), **layout)
    # the two robust aggregates are alternatives
    assert refused(3, 10, d, d, krum=(1, 3), trim=1, **layout)
    assert refused(3, 10, d, d, krum=(1, 3), trim=0, **layout)
    assert refused(3, 10, d, d, krum=(1, 3), trim=1, trim_select=True, **layout)
    assert not refused(3, 10, d, d, trim=1, **layout) and not refused(3, 10, d, d, krum=(1, 3), **layout)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_a_call_that_is_not_dense_is_refused(alg):
    assert refused(alg, 20, 8, 64, krum=(1, 3))               # sparse
    assert refused(alg, 20, 64, 64, krum=(1, 3))              # dense-sized, not declared dense
    assert refused(alg, 20, 8, 64, krum=(1, 3), dense=True)   # k != d


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
        assert p.route not in (R_KRUM_DENSE, R_KRUM_PACKED)
        o = D.opts(krum=(0xDEADBEEF, 0xDEADBEEF), **kw)
        o.flags &= ~L.OPT_KRUM  # the fields are there, the flag is not: never read
        out = (ctypes.c_uint64 * 18)()
        assert L.lib().fltee_debug_plan(alg, n, k, d, ctypes.byref(o), out) == p.status
        assert out[0] == p.route and list(out)[4:] == list(p.bytes.values())
