"""FLTEE_OPT_KRUM on the GPU (k_krum.hip) through the device API, bit for bit against
tests/krum_model.py.

Exact inputs are small integers, |v| <= 8: every Gram entry is then exact in any summation
order, so scores, keep words and [out] must equal the model's exactly.  General inputs are
N(0, 1) with f shifted clients; before the GPU is touched the model's own scores are asserted to
be well separated (krum_model.well_separated: every deciding gap above 1000 times the reordering
bound (d - 1) 2^-53 sum_j |x_a x_b|), then the keep words and [out] are compared bit for bit and
each score within krum_model.score_bound of the model's."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_model as BM
import fp8_model as FM
import krum_model as KM
from conftest import gpu_available
from options_model import GENERAL_CLIPPING
from stable_model import bits_equal
from test_gpu_trim import DENSE_ORDER, LAYOUTS, SEED, on_device, run
from test_krum_abi import R_KRUM_DENSE, R_KRUM_PACKED, geometry
from test_plan import Plan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CHUNK = 256  # the shortest Gram chunk (k_krum.hip kKrumMinChunk): d = CHUNK + 1 is two chunks


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def ints(n, d, seed=0):
    """n x d integers in [-8, 8], rows distinct where d allows: built once, never modified"""
    rng = np.random.default_rng(1000003 * n + d + seed)
    v = rng.integers(-8, 9, (n, d)).astype(np.float32)
    v.setflags(write=False)
    return v


def fm_for(n):
    f = (n - 3) // 3
    return f, max(1, (n - f) // 2)


def select_on(dev, layout, buf, n, d, f, m, **kw):
    lay = dict(packed=True) if layout == "packed" else {}
    s, k = dev.krum_select(buf, n, d, f, m, **lay, **kw)
    s, k = s.cpu().numpy(), k.cpu().numpy()
    assert dev.status() == 0
    assert set(np.unique(k)) <= {0, -1}
    return s, k != 0


def check_exact(dev, v, f, m, layouts=LAYOUTS, offset=0, what=""):
    n, d = v.shape
    want_s, want_k = KM.select(v, f, m)
    want = KM.krum(v, f, m, keep=want_k)
    for layout in layouts:
        if layout == "packed" and d < 2:
            continue
        buf = on_device(layout, v, offset) if layout == "packed" else on_device(layout, v)
        s, k = select_on(dev, layout, buf, n, d, f, m)
        bad = int((s.view(np.uint64) != want_s.view(np.uint64)).sum())
        print(f"{what}{layout} n={n} d={d} f={f} m={m}: {bad} of {n} scores, "
              f"{int((k != want_k).sum())} keep words differ from the model")
        assert np.array_equal(s.view(np.uint64), want_s.view(np.uint64)), (layout, n, d)
        assert np.array_equal(k, want_k), (layout, n, d)
        got = run(dev, layout, buf, n, d, krum=(f, m))
        assert bits_equal(got, want), (layout, n, d)


# ------------------------------------------------------------------ exact inputs ----
def test_first_the_mfma_layout(dev):
    """n = 16, d = 4: one tile, one instruction.  The f32 row formula on the f64 result would put
    3 of 4 results in the wrong row; distinct small integers make every such slip visible."""
    v = (np.arange(64, dtype=np.float32).reshape(16, 4) % 17) - 8
    v[:, 0] = np.arange(16) - 8  # rows distinct
    assert len({tuple(r) for r in v}) == 16
    for f, m in ((0, 16), (3, 1), (6, 10)):
        check_exact(dev, v, f, m, what="layout ")


@pytest.mark.parametrize("d", [1, 3, 4, 5, CHUNK + 1, 1027])
@pytest.mark.parametrize("n", [3, 7, 17, 100, 129])
def test_exact_inputs_equal_the_model(dev, n, d):
    if n == 3:
        f, m = 0, 1
    else:
        f, m = fm_for(n)
    assert Plan(3, n, d, d, dense=True, krum=(f, m)).route == R_KRUM_DENSE
    if d >= 2:
        assert Plan(3, n, d, d, packed=True, krum=(f, m)).route == R_KRUM_PACKED
    assert geometry(n, CHUNK + 1)["chunks"] == 2 and geometry(n, CHUNK)["chunks"] == 1
    check_exact(dev, ints(n, d), f, m)


def test_the_cap_on_n(dev):
    n, d = 1024, 64
    assert geometry(n, d)["macros"] == 8
    check_exact(dev, ints(n, d), 100, 500)


def test_the_macro_tile_boundary(dev):
    """128 clients are one macro-tile, 129 two (the second a single partial tile), 257 three"""
    for n in (128, 257):
        f, m = fm_for(n)
        check_exact(dev, ints(n, 37), f, m, what="macro ")


def test_the_accumulates_large_d_shape(dev):
    n, d = 5, (1 << 18) + 7
    check_exact(dev, ints(n, d), 1, 2)


@pytest.mark.parametrize("offset", [0, 2, 1], ids=["16B", "8B", "4B"])
@pytest.mark.parametrize("n,d", [(17, 1027), (7, 64), (129, 30)])
def test_packed_rows_at_every_alignment(dev, n, d, offset):
    f, m = fm_for(n)
    check_exact(dev, ints(n, d), f, m, layouts=["packed"], offset=offset)


def test_records_off_16_bytes(dev):
    """an 8-byte aligned record base (and an odd d) takes the 8-byte loads"""
    import torch
    n, d = 17, 64
    f, m = fm_for(n)
    v = ints(n, d)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    buf = torch.zeros(n * d + 1, dtype=torch.int64, device="cuda")
    rec = buf[1:]
    rec.copy_(torch.from_numpy(dev.pack_records(idx, v.reshape(-1))))
    assert rec.data_ptr() % 16 == 8
    want_s, want_k = KM.select(v, f, m)
    s, k = select_on(dev, "records", rec, n, d, f, m)
    assert np.array_equal(s.view(np.uint64), want_s.view(np.uint64)) and np.array_equal(k, want_k)
    assert bits_equal(run(dev, "records", rec, n, d, krum=(f, m)), KM.krum(v, f, m))


def test_the_other_flat_algs_take_the_same_route(dev):
    n, d = 17, 33
    f, m = fm_for(n)
    v = ints(n, d)
    want = KM.krum(v, f, m)
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        for alg in (4, 5):
            assert bits_equal(run(dev, layout, buf, n, d, alg=alg, krum=(f, m)), want)


# ----------------------------------------------------------------- general inputs ----
GENERAL = [(20, 300, 3, 9, 11), (100, 1027, 10, 60, 12), (150, 513, 20, 100, 13)]  # n, d, f, m, seed


@functools.lru_cache(maxsize=None)
def general_values(n, d, f, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    bad = rng.choice(n, f, replace=False)
    v[bad] += rng.normal(0.5, 0.1, (f, 1)).astype(np.float32)
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("n,d,f,m,seed", GENERAL)
def test_general_inputs(dev, n, d, f, m, seed):
    v = general_values(n, d, f, seed)
    # a condition on the input, asserted before the GPU is touched (the seeds were picked for it)
    assert KM.well_separated(v, f, m)
    want_s, want_k = KM.select(v, f, m)
    bound = KM.score_bound(v, f)
    want = KM.krum(v, f, m, keep=want_k)
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        s, k = select_on(dev, layout, buf, n, d, f, m)
        err = np.abs(s - want_s)
        print(f"{layout} n={n} d={d}: max |score - model| = {err.max():.3e}, bound there "
              f"{bound[err.argmax()]:.3e}; largest err / bound = {(err / bound).max():.3f}")
        assert np.array_equal(k, want_k)
        assert (err <= bound).all()
        assert bits_equal(run(dev, layout, buf, n, d, krum=(f, m)), want)


def test_run_to_run(dev):
    n, d, f, m, seed = GENERAL[1]
    v = general_values(n, d, f, seed)
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        a = select_on(dev, layout, buf, n, d, f, m)[0]
        b = select_on(dev, layout, buf, n, d, f, m)[0]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # and the two layouts add in the same order
    r = select_on(dev, "records", on_device("records", v), n, d, f, m)[0]
    assert np.array_equal(a.view(np.uint64), r.view(np.uint64))


# ------------------------------------------------------------------------- edges ----
def test_nan_and_inf_clients(dev):
    n, d, f = 19, 65, 3
    v = ints(n, d).copy()
    v[4, 7] = np.nan
    v[11, 0] = np.inf
    v[12, 64] = -np.inf
    for m in (1, n - f):
        want_s, want_k = KM.select(v, f, m)
        assert np.isinf(want_s[[4, 11, 12]]).all() and not want_k[[4, 11, 12]].any()
        want = KM.krum(v, f, m, keep=want_k)
        assert np.isfinite(want).all()
        for layout in LAYOUTS:
            buf = on_device(layout, v)
            s, k = select_on(dev, layout, buf, n, d, f, m)
            assert np.array_equal(s.view(np.uint64), want_s.view(np.uint64)) and np.array_equal(k, want_k)
            assert bits_equal(run(dev, layout, buf, n, d, krum=(f, m)), want)
    # with f = 0 every client's q = n - 2 nearest include a non-finite one: every score is +inf,
    # and clients with s = +inf rank in upload order
    want_s, want_k = KM.select(v, 0, n - 2)
    assert np.isinf(want_s).all() and list(np.flatnonzero(~want_k)) == [n - 2, n - 1]
    s, k = select_on(dev, "records", on_device("records", v), n, d, 0, n - 2)
    assert np.array_equal(s.view(np.uint64), want_s.view(np.uint64)) and np.array_equal(k, want_k)


def test_huge_clients(dev):
    n, d, f = 9, 16, 2
    v = ints(n, d).copy()
    v[2] = np.float32(3e38)
    v[6] = np.float32(-3e38)
    for m in (1, n - f):
        check_exact(dev, v, f, m, what="3e38 ")
    _, k = KM.select(v, f, n - f)
    assert not k[2] and not k[6]


def test_minus_zero_columns(dev):
    n, d = 7, 9
    v = ints(n, d).copy()
    v[:, 3] = np.float32(-0.0)
    v[:, 8] = np.float32(-0.0)
    check_exact(dev, v, 0, n, what="-0.0 ")  # everyone kept: +0.0 + -0.0 ... = +0.0
    out = KM.krum(v, 0, n)
    assert not np.signbit(out[[3, 8]]).any()
    check_exact(dev, v, 2, 1, what="-0.0 ")


def test_identical_clients(dev):
    n, d, f = 9, 33, 1
    v = ints(n, d).copy()
    v[6] = v[2]
    s, _ = KM.select(v, f, 1)
    assert s[2] == s[6]
    order = sorted(range(n), key=lambda a: (s[a], a))
    for m in (order.index(2) + 1, order.index(6) + 1, 1, n - f):  # the tie at the edge: the earlier one
        check_exact(dev, v, f, m, what="copies ")
    allsame = np.tile(ints(1, d), (n, 1))
    check_exact(dev, allsame, f, 3, what="all equal ")


def test_f_zero_and_everyone_kept_is_the_dense_route(dev):
    n, d = 23, 1027
    v = general_values(100, 1027, 10, 12)[:n]
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        plain = run(dev, layout, buf, n, d)
        assert bits_equal(run(dev, layout, buf, n, d, krum=(0, n)), plain)


# ----------------------------------------------------------------------- options ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_options(dev, layout, clip):
    n, d, f, m, seed = GENERAL[0]
    v = general_values(n, d, f, seed) * np.float32(0.029)  # norms around 0.5: the clip bites on some
    c = GENERAL_CLIPPING if clip else None
    x = KM.clipped(v, c)
    assert KM.well_separated(x, f, m)
    if clip:
        from options_model import clip_coefs
        coef = clip_coefs(v.reshape(-1), n, d, c)[0]
        assert (coef < 1).any() and (coef == 1).any()
    keep = KM.select(x, f, m)[1]
    buf = on_device(layout, v)
    more = dict(clip=True, clipping=GENERAL_CLIPPING) if clip else {}
    lay = dict(packed=True) if layout == "packed" else {}
    k = dev.krum_select(buf, n, d, f, m, **lay, **more)[1].cpu().numpy() != 0
    assert np.array_equal(k, keep)
    prev = np.random.default_rng(3).normal(0, 1, d).astype(np.float32)
    kw = dict(krum=(f, m), **more)
    model = functools.partial(KM.krum, v, f, m, clip=c, keep=None)
    assert bits_equal(run(dev, layout, buf, n, d, prev=prev, accumulate=True, **kw), model(prev=prev))
    assert bits_equal(run(dev, layout, buf, n, d, prev=prev, accumulate=True, n_avg=7, no_average=True, **kw),
                      model(prev=prev))
    assert bits_equal(run(dev, layout, buf, n, d, no_average=True, **kw), model(no_average=True))
    assert bits_equal(run(dev, layout, buf, n, d, n_avg=7, **kw), model(n_avg=7))
    assert bits_equal(run(dev, layout, buf, n, d, **kw), model())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_avg", [0, 7])
def test_dp_noise_takes_the_divisor_m(dev, layout, n_avg):
    """the same seed: the noise fltee_dp_noise_device adds for the divisor m (or n_avg)"""
    import torch
    n, d, f, m, seed = GENERAL[0]
    v = general_values(n, d, f, seed)
    buf = on_device(layout, v)
    kw = dict(krum=(f, m), seed=SEED, sigma=1.12, clipping=GENERAL_CLIPPING, n_avg=n_avg)
    base = run(dev, layout, buf, n, d, **kw)
    got = run(dev, layout, buf, n, d, dp=True, **kw)
    want = dev.dp_noise(torch.from_numpy(base.copy()).cuda(), 1.12, GENERAL_CLIPPING, n_avg or m, seed=SEED)
    assert bits_equal(got, want.cpu().numpy()) and not bits_equal(got, base)
    other = dev.dp_noise(torch.from_numpy(base.copy()).cuda(), 1.12, GENERAL_CLIPPING, n, seed=SEED)
    assert not bits_equal(got, other.cpu().numpy())


def test_bf16_and_fp8_calls_equal_the_records_call_on_the_widened_values(dev):
    import torch
    n, d, f, m, seed = GENERAL[0]
    v = general_values(n, d, f, seed)
    for name, M in (("bf16", BM), ("fp8", FM)):
        rows = M.pack(v)
        wide = M.unpack(rows, d)
        buf = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).cuda()
        rec = on_device("records", np.ascontiguousarray(wide, np.float32))
        flag = {name: True}
        assert Plan(3, n, d, d, krum=(f, m), **flag).route == R_KRUM_DENSE
        s0, k0 = dev.krum_select(rec, n, d, f, m)
        s1, k1 = dev.krum_select(buf, n, d, f, m, **flag)
        assert torch.equal(s0.view(torch.int64), s1.view(torch.int64)) and torch.equal(k0, k1)
        for more in ({}, dict(clip=True, clipping=GENERAL_CLIPPING)):
            want = dev.aggregate(3, rec, n, d, d, dense=True, krum=(f, m), **more).cpu().numpy()
            got = dev.aggregate(3, buf, n, d, d, krum=(f, m), **flag, **more).cpu().numpy()
            assert dev.status() == 0 and bits_equal(got, want)


# -------------------------------------------------------------- status, scratch ----
def test_a_record_out_of_position_sets_the_status(dev):
    import torch
    n, d = 17, 257
    f, m = fm_for(n)
    v = ints(n, d)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    idx[(n - 1) * d + d // 2] += 1
    rec = torch.from_numpy(dev.pack_records(idx, v.reshape(-1))).cuda()
    run(dev, "records", rec, n, d, krum=(f, m), want_status=DENSE_ORDER)  # ... and the call returned


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
def test_a_reserved_call_grows_no_scratch(dev, layout, kw):
    import torch

    from fltee import _lib as L
    n, d = 129, 1027
    f, m = fm_for(n)
    buf = on_device(layout, ints(n, d))
    lay = dict(packed=True) if layout == "packed" else dict(dense=True)
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(3, n, d, d, krum=(f, m), **lay, **kw)
    assert L.lib().fltee_debug_scratch_grown() != 0 and dev.workspace_bytes(3, n, d, d, krum=(f, m), **lay, **kw) > 0
    run(dev, layout, buf, n, d, krum=(f, m), **kw)
    select_on(dev, layout, buf, n, d, f, m, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


def test_refusals_launch_nothing_and_leave_out_alone(dev):
    import torch

    from fltee import _lib as L
    from test_gpu_oblivious import traced
    buf = torch.zeros(1025 * 8, dtype=torch.int64, device="cuda")
    out = torch.full((64,), 7.5, dtype=torch.float32, device="cuda")
    cases = [(3, 1025, 8, 8, dict(dense=True, krum=(1, 3))), (3, 4, 8, 8, dict(dense=True, krum=(1, 1))),
             (3, 20, 8, 8, dict(dense=True, krum=(1, 0))), (3, 20, 8, 8, dict(dense=True, krum=(1, 20))),
             (3, 20, 8, 8, dict(dense=True, krum=(2 ** 63, 1))), (1, 20, 8, 8, dict(dense=True, krum=(1, 3))),
             (4, 20, 8, 64, dict(krum=(1, 3))), (5, 20, 8, 8, dict(dense=True, oram_tree=True, krum=(1, 3))),
             (3, 20, 8, 8, dict(dense=True, trim=1, krum=(1, 3))), (3, 20, 8, 8, dict(packed=True, trim=0, krum=(1, 3)))]

    def calls():
        for alg, n, k, d, kw in cases:
            o = dev.opts(**kw)
            st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(buf.data_ptr()), n, k, d,
                                                ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
            assert st == L.ERROR_INVALID_PARAMETER, (alg, n, k, d, kw)
        scores = torch.zeros(1025, dtype=torch.float64, device="cuda")
        keep = torch.zeros(1025, dtype=torch.int32, device="cuda")
        for n, f, m in [(1025, 1, 3), (4, 1, 1), (20, 1, 0), (20, 1, 20)]:
            o = dev.opts(krum=(f, m))
            st = L.lib().fltee_krum_select_device(ctypes.c_void_p(buf.data_ptr()), n, 8, ctypes.byref(o),
                                                  ctypes.c_void_p(scores.data_ptr()),
                                                  ctypes.c_void_p(keep.data_ptr()), None)
            assert st == L.ERROR_INVALID_PARAMETER, (n, f, m)

    tr = traced(calls)
    assert not any(line.startswith("launch") for line in tr), tr
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(7.5)).all()
