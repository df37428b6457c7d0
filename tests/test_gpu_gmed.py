"""FLTEE_OPT_GMED on the GPU (k_gmed.hip) through the device API, against tests/gmed_model.py.

Exact inputs are small integers, |v| <= 8: every Gram entry is then exact in any summation order,
and from G on the definition fixes every operation and its order (sum64, no contraction), so
alpha, rho and [out] must equal the model's bit for bit.

General inputs are N(0, 1) rows.  [out] is compared bit for bit with the model's step 6 run on the
device's own alpha, and the device's alpha lies within 1 f32 ulp of the model's.  That bound is
derived, not measured: a reordered f64 Gram sum moves an entry by a relative O(d 2^-53), rho by a
relative O(n d 2^-53) when rho^2 ~ d, and so w / s by the same — far below the 2^-24 of alpha's one
rounding to f32, which alone can therefore flip, by one ulp.  For the seeds used here the model
itself was checked on the CPU to stay within that 1 ulp under two Gram orders, numpy's product and
a sequential longdouble sum (tests/test_gmed_model.py runs that check)."""
import ctypes
import functools

import numpy as np
import pytest

import bf16_model as BM
import fp8_model as FM
import gmed_model as M
from conftest import gpu_available
from options_model import GENERAL_CLIPPING
from stable_model import bits_equal
from test_gmed_abi import R_GMED_DENSE, R_GMED_PACKED
from test_gmed_model import GENERAL, general_values
from test_gpu_trim import DENSE_ORDER, LAYOUTS, SEED, on_device, run
from test_krum_abi import geometry
from test_plan import Plan

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CHUNK = 256  # the shortest Gram chunk (k_krum.hip kKrumMinChunk): d = CHUNK + 1 is two chunks
NU = M.NU    # 2^-20


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@functools.lru_cache(maxsize=None)
def ints(n, d, seed=0):
    """n x d integers in [-8, 8]: built once, never modified"""
    rng = np.random.default_rng(1000003 * n + d + seed)
    v = rng.integers(-8, 9, (n, d)).astype(np.float32)
    v.setflags(write=False)
    return v


def weights_on(dev, layout, buf, n, d, iters, nu=NU, **kw):
    lay = dict(packed=True) if layout == "packed" else {}
    a, r = dev.gmed_weights(buf, n, d, iters, nu, **lay, **kw)
    a, r = a.cpu().numpy(), r.cpu().numpy()
    assert dev.status() == 0
    return a, r


def same64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_exact(dev, v, iters, nu=NU, layouts=LAYOUTS, offset=0, what=""):
    n, d = v.shape
    want_a, want_r, valid = M.weights(v, iters, nu)
    want = M.gmed(v, iters, nu, alpha=want_a, valid=valid)
    for layout in layouts:
        if layout == "packed" and d < 2:
            continue
        buf = on_device(layout, v, offset) if layout == "packed" else on_device(layout, v)
        a, r = weights_on(dev, layout, buf, n, d, iters, nu)
        print(f"{what}{layout} n={n} d={d} R={iters}: {int((a.view(np.uint32) != want_a.view(np.uint32)).sum())} "
              f"of {n} alpha, {int((r.view(np.uint64) != want_r.view(np.uint64)).sum())} rho differ from the model")
        assert bits_equal(a, want_a), (layout, n, d, iters)
        assert same64(r, want_r), (layout, n, d, iters)
        got = run(dev, layout, buf, n, d, gmed=(iters, nu))
        assert bits_equal(got, want), (layout, n, d, iters)


# ------------------------------------------------------------------ exact inputs ----
@pytest.mark.parametrize("d", [1, 3, 4, 5, CHUNK + 1, 1027])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 100, 129])
def test_exact_inputs_equal_the_model(dev, n, d):
    """n = 65 crosses sum64's 64-lane stride, n = 129 the Gram pass's macro-tile"""
    assert Plan(3, n, d, d, dense=True, gmed=(1, NU)).route == R_GMED_DENSE
    if d >= 2:
        assert Plan(3, n, d, d, packed=True, gmed=(1, NU)).route == R_GMED_PACKED
    assert geometry(n, CHUNK + 1)["chunks"] == 2 and geometry(n, CHUNK)["chunks"] == 1
    for iters in (1, 3):
        check_exact(dev, ints(n, d), iters)


def test_the_cap_on_n(dev):
    n, d = 1024, 16
    assert geometry(n, d)["macros"] == 8
    check_exact(dev, ints(n, d), 3)


def test_the_cap_on_the_iterations(dev):
    check_exact(dev, ints(17, 33), 64, layouts=["records"])


def test_the_accumulates_large_d_shape(dev):
    n, d = 5, (1 << 18) + 7
    check_exact(dev, ints(n, d), 2)


@pytest.mark.parametrize("offset", [0, 2, 1], ids=["16B", "8B", "4B"])
@pytest.mark.parametrize("n,d", [(17, 1027), (7, 64), (129, 30)])
def test_packed_rows_at_every_alignment(dev, n, d, offset):
    check_exact(dev, ints(n, d), 3, layouts=["packed"], offset=offset)


def test_records_off_16_bytes(dev):
    """an 8-byte aligned record base takes the 8-byte loads"""
    import torch
    n, d, iters = 17, 64, 3
    v = ints(n, d)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    buf = torch.zeros(n * d + 1, dtype=torch.int64, device="cuda")
    rec = buf[1:]
    rec.copy_(torch.from_numpy(dev.pack_records(idx, v.reshape(-1))))
    assert rec.data_ptr() % 16 == 8
    want_a, want_r, _ = M.weights(v, iters)
    a, r = weights_on(dev, "records", rec, n, d, iters)
    assert bits_equal(a, want_a) and same64(r, want_r)
    assert bits_equal(run(dev, "records", rec, n, d, gmed=(iters, NU)), M.gmed(v, iters))


def test_the_other_flat_algs_take_the_same_route(dev):
    n, d, iters = 17, 33, 3
    v = ints(n, d)
    want = M.gmed(v, iters)
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        for alg in (3, 4, 5):
            assert Plan(alg, n, d, d, gmed=(iters, NU), **(dict(packed=True) if layout == "packed" else
                                                            dict(dense=True))).route in (R_GMED_DENSE, R_GMED_PACKED)
            assert bits_equal(run(dev, layout, buf, n, d, alg=alg, gmed=(iters, NU)), want)


# ----------------------------------------------------------------- general inputs ----
def ulps(a, b):
    """f32 ulps between non-negative finite values"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("n,d,iters,seed", GENERAL)
def test_general_inputs(dev, n, d, iters, seed):
    v = general_values(n, d, seed)
    want_a, want_r, valid = M.weights(v, iters)
    assert valid.all()
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        a, r = weights_on(dev, layout, buf, n, d, iters)
        u = ulps(a, want_a)
        print(f"{layout} n={n} d={d} R={iters}: alpha differs from the model by at most {u.max()} ulp "
              f"({int((u != 0).sum())} of {n}); max relative rho difference {np.abs(r / want_r - 1).max():.3e}")
        assert (u <= 1).all()
        got = run(dev, layout, buf, n, d, gmed=(iters, NU))
        assert bits_equal(got, M.gmed(v, iters, alpha=a, valid=valid))


def test_run_to_run(dev):
    n, d, iters, seed = GENERAL[1]
    v = general_values(n, d, seed)
    outs = []
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        a0, r0 = weights_on(dev, layout, buf, n, d, iters)
        a1, r1 = weights_on(dev, layout, buf, n, d, iters)
        assert bits_equal(a0, a1) and same64(r0, r1)
        o0, o1 = (run(dev, layout, buf, n, d, gmed=(iters, NU)) for _ in range(2))
        assert bits_equal(o0, o1)
        outs.append((a0, r0, o0))
    # and the two layouts add in the same order
    assert bits_equal(outs[0][0], outs[1][0]) and same64(outs[0][1], outs[1][1]) and bits_equal(outs[0][2], outs[1][2])


# ------------------------------------------------------------------------- edges ----
def test_nan_and_inf_clients(dev):
    n, d = 19, 65
    v = ints(n, d).copy()
    v[4, 7] = np.nan
    v[11, 0] = np.inf
    v[12, 64] = -np.inf
    bad = [4, 11, 12]
    good = [c for c in range(n) if c not in bad]
    for iters in (1, 3):
        want_a, want_r, valid = M.weights(v, iters)
        assert not valid[bad].any() and valid[good].all() and not want_a[bad].any() and np.isinf(want_r[bad]).all()
        # the rest: the model on the valid clients alone (19 clients: a lane each, the zeros move no sum)
        assert bits_equal(want_a[good], M.weights(v[good], iters)[0])
        want = M.gmed(v, iters)
        assert np.isfinite(want).all() and bits_equal(want, M.gmed(v[good], iters))
        check_exact(dev, v, iters, what="nan / inf ")


def test_a_huge_client_gets_a_finite_tiny_weight(dev):
    n, d = 9, 16
    v = ints(n, d).copy()
    v[2] = np.float32(1e30)
    for iters in (1, 3, 32):  # (the weight falls by the factor n - 1 an iteration, from 1 / 65)
        a, _, valid = M.weights(v, iters)
        assert valid.all() and 0 < a[2] < 0.02 and np.isfinite(M.gmed(v, iters)).all()
        check_exact(dev, v, iters, what="1e30 ")
    assert a[2] < 1e-25 and np.abs(M.gmed(v, 32)).max() <= 8
    v[6] = np.float32(-3e38)  # G_66 = 16 * 9e76 is still finite in f64: a valid client
    check_exact(dev, v, 3, what="3e38 ")


def test_identical_clients(dev):
    """n a power of two: s, inv and every product are exact, D = (G - 2 G) + G = 0 — rho = 0 and
    w = 1 / nu each, alpha = 1 / n; any n: the model's bits"""
    d = 33
    for n in (8, 64):
        v = np.tile(ints(1, d), (n, 1))
        for layout in LAYOUTS:
            a, r = weights_on(dev, layout, on_device(layout, v), n, d, 2)
            assert not r.view(np.uint64).any() and bits_equal(a, np.full(n, 1.0 / n, np.float32))
        check_exact(dev, v, 2, what="all equal ")
    check_exact(dev, np.tile(ints(1, d), (9, 1)), 3, what="all equal ")
    v = ints(9, d).copy()
    v[6] = v[2]
    want_a = M.weights(v, 3)[0]
    assert want_a[2] == want_a[6]
    check_exact(dev, v, 3, what="copies ")


def test_all_clients_invalid_is_a_zero_vector(dev):
    n, d = 5, 37
    v = ints(n, d).copy()
    v[:, 3] = np.nan
    v[1, 5] = np.inf
    want_a, want_r, valid = M.weights(v, 2)
    assert not valid.any() and not want_a.any()
    for layout in LAYOUTS:
        buf = on_device(layout, v)
        a, r = weights_on(dev, layout, buf, n, d, 2)
        assert not a.view(np.uint32).any() and np.isposinf(r).all()
        assert not run(dev, layout, buf, n, d, gmed=(2, NU)).view(np.uint32).any()
        prev = np.arange(d, dtype=np.float32)
        assert bits_equal(run(dev, layout, buf, n, d, prev=prev, accumulate=True, gmed=(2, NU)), prev)


def test_minus_zero_columns(dev):
    n, d = 7, 9
    v = ints(n, d).copy()
    v[:, 3] = np.float32(-0.0)
    v[:, 8] = np.float32(-0.0)
    out = M.gmed(v, 2)
    assert not np.signbit(out[[3, 8]]).any()  # +0.0 + -0.0 ... = +0.0
    check_exact(dev, v, 2, what="-0.0 ")


# ----------------------------------------------------------------------- options ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
def test_options(dev, layout, clip):
    n, d, iters, seed = GENERAL[0]
    v = general_values(n, d, seed) * np.float32(0.029)  # norms around 0.5: the clip bites on some
    c = GENERAL_CLIPPING if clip else None
    if clip:
        from options_model import clip_coefs
        coef = clip_coefs(v.reshape(-1), n, d, c)[0]
        assert (coef < 1).any() and (coef == 1).any()
    want_a, _, valid = M.weights(v, iters, clip=c)  # G on the clipped rows
    buf = on_device(layout, v)
    more = dict(clip=True, clipping=GENERAL_CLIPPING) if clip else {}
    a, _ = weights_on(dev, layout, buf, n, d, iters, **more)
    assert (ulps(a, want_a) <= 1).all()
    if clip:
        assert not bits_equal(a, weights_on(dev, layout, buf, n, d, iters)[0])
    prev = np.random.default_rng(3).normal(0, 1, d).astype(np.float32)
    kw = dict(gmed=(iters, NU), **more)
    model = functools.partial(M.gmed, v, iters, clip=c, alpha=a, valid=valid)
    assert bits_equal(run(dev, layout, buf, n, d, **kw), model())
    assert bits_equal(run(dev, layout, buf, n, d, n_avg=7, **kw), model())  # n_avg: the DP divisor alone
    assert bits_equal(run(dev, layout, buf, n, d, prev=prev, accumulate=True, **kw), model(prev=prev))
    assert bits_equal(run(dev, layout, buf, n, d, prev=prev, accumulate=True, n_avg=7, **kw), model(prev=prev))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_avg", [0, 7])
def test_dp_noise_takes_the_divisor_n(dev, layout, n_avg):
    """the same seed: the noise fltee_dp_noise_device adds for the divisor n (or n_avg)"""
    import torch
    n, d, iters, seed = GENERAL[0]
    v = general_values(n, d, seed)
    buf = on_device(layout, v)
    kw = dict(gmed=(iters, NU), seed=SEED, sigma=1.12, clipping=GENERAL_CLIPPING, n_avg=n_avg)
    base = run(dev, layout, buf, n, d, **kw)
    got = run(dev, layout, buf, n, d, dp=True, **kw)
    want = dev.dp_noise(torch.from_numpy(base.copy()).cuda(), 1.12, GENERAL_CLIPPING, n_avg or n, seed=SEED)
    assert bits_equal(got, want.cpu().numpy()) and not bits_equal(got, base)
    other = dev.dp_noise(torch.from_numpy(base.copy()).cuda(), 1.12, GENERAL_CLIPPING, n + 1, seed=SEED)
    assert not bits_equal(got, other.cpu().numpy())


def test_bf16_and_fp8_calls_equal_the_records_call_on_the_widened_values(dev):
    import torch
    n, d, iters, seed = GENERAL[0]
    v = general_values(n, d, seed)
    for name, F in (("bf16", BM), ("fp8", FM)):
        rows = F.pack(v)
        wide = F.unpack(rows, d)
        buf = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).cuda()
        rec = on_device("records", np.ascontiguousarray(wide, np.float32))
        flag = {name: True}
        assert Plan(3, n, d, d, gmed=(iters, NU), **flag).route == R_GMED_DENSE
        a0, r0 = dev.gmed_weights(rec, n, d, iters, NU)
        a1, r1 = dev.gmed_weights(buf, n, d, iters, NU, **flag)
        assert torch.equal(a0.view(torch.int32), a1.view(torch.int32))
        assert torch.equal(r0.view(torch.int64), r1.view(torch.int64))
        for more in ({}, dict(clip=True, clipping=GENERAL_CLIPPING)):
            want = dev.aggregate(3, rec, n, d, d, dense=True, gmed=(iters, NU), **more).cpu().numpy()
            got = dev.aggregate(3, buf, n, d, d, gmed=(iters, NU), **flag, **more).cpu().numpy()
            assert dev.status() == 0 and bits_equal(got, want)


# -------------------------------------------------------------- status, scratch ----
def test_a_record_out_of_position_sets_the_status(dev):
    import torch
    n, d = 17, 257
    v = ints(n, d)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    idx[(n - 1) * d + d // 2] += 1
    rec = torch.from_numpy(dev.pack_records(idx, v.reshape(-1))).cuda()
    run(dev, "records", rec, n, d, gmed=(2, NU), want_status=DENSE_ORDER)  # ... and the call returned


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kw", [{}, dict(clip=True, clipping=0.5)], ids=["plain", "clip"])
def test_a_reserved_call_grows_no_scratch(dev, layout, kw):
    import torch

    from fltee import _lib as L
    n, d = 129, 1027
    buf = on_device(layout, ints(n, d))
    lay = dict(packed=True) if layout == "packed" else dict(dense=True)
    L.lib().fltee_debug_scratch_release()
    L.lib().fltee_debug_scratch_grown()
    dev.reserve(3, n, d, d, gmed=(1, NU), **lay, **kw)
    assert L.lib().fltee_debug_scratch_grown() != 0 and dev.workspace_bytes(3, n, d, d, gmed=(1, NU), **lay, **kw) > 0
    run(dev, layout, buf, n, d, gmed=(8, 0.5), **kw)  # (R and nu move no byte)
    weights_on(dev, layout, buf, n, d, 3, **kw)
    torch.cuda.synchronize()
    assert L.lib().fltee_debug_scratch_grown() == 0


def test_refusals_launch_nothing_and_leave_out_alone(dev):
    import torch

    from fltee import _lib as L
    from test_gpu_oblivious import traced
    buf = torch.zeros(1025 * 8, dtype=torch.int64, device="cuda")
    out = torch.full((64,), 7.5, dtype=torch.float32, device="cuda")
    g = (3, NU)
    cases = [(3, 1025, 8, 8, dict(dense=True, gmed=g)), (3, 0, 8, 8, dict(dense=True, gmed=g)),
             (3, 20, 8, 8, dict(dense=True, gmed=(0, NU))), (3, 20, 8, 8, dict(dense=True, gmed=(65, NU))),
             (3, 20, 8, 8, dict(dense=True, gmed=(3, 0.0))), (3, 20, 8, 8, dict(dense=True, gmed=(3, float("nan")))),
             (3, 20, 8, 8, dict(dense=True, gmed=(3, float("inf")))), (3, 20, 8, 8, dict(dense=True, gmed=(3, -1.0))),
             (1, 20, 8, 8, dict(dense=True, gmed=g)), (4, 20, 8, 64, dict(gmed=g)),
             (5, 20, 8, 8, dict(dense=True, oram_tree=True, gmed=g)), (3, 20, 8, 8, dict(dense=True, trim=1, gmed=g)),
             (3, 20, 8, 8, dict(packed=True, trim=0, gmed=g)), (3, 20, 8, 8, dict(dense=True, no_average=True, gmed=g)),
             (4, 20, 8, 8, dict(packed=True, no_average=True, accumulate=True, gmed=g))]

    def calls():
        for alg, n, k, d, kw in cases:
            o = dev.opts(**kw)
            st = L.lib().fltee_aggregate_device(alg, ctypes.c_void_p(buf.data_ptr()), n, k, d,
                                                ctypes.c_void_p(out.data_ptr()), ctypes.byref(o), None)
            assert st == L.ERROR_INVALID_PARAMETER, (alg, n, k, d, kw)
        o = dev.opts(dense=True, krum=(1, 3))
        o.flags |= L.OPT_GMED  # together with Multi-Krum
        assert L.lib().fltee_aggregate_device(3, ctypes.c_void_p(buf.data_ptr()), 20, 8, 8,
                                              ctypes.c_void_p(out.data_ptr()), ctypes.byref(o),
                                              None) == L.ERROR_INVALID_PARAMETER
        alpha = torch.zeros(1025, dtype=torch.float32, device="cuda")
        rho = torch.zeros(1025, dtype=torch.float64, device="cuda")
        for n, iters, nu in [(1025, 3, NU), (0, 3, NU), (20, 0, NU), (20, 65, NU), (20, 3, 0.0), (20, 3, float("nan"))]:
            o = dev.opts(gmed=(iters, nu))
            st = L.lib().fltee_gmed_weights_device(ctypes.c_void_p(buf.data_ptr()), n, 8, ctypes.byref(o),
                                                   ctypes.c_void_p(alpha.data_ptr()),
                                                   ctypes.c_void_p(rho.data_ptr()), None)
            assert st == L.ERROR_INVALID_PARAMETER, (n, iters, nu)

    tr = traced(calls)
    assert not any(line.startswith("launch") for line in tr), tr
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == np.float32(7.5)).all()
