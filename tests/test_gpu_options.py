"""FLTEE_OPT_CLIP, _ACCUMULATE, _NO_AVERAGE, n_avg and _DP on every route of aggregate(),
bit for bit against references that do not come from the library: the numpy clip model
(tests/options_model.py, checked on the CPU against the reference's recorded clip results),
each alg's own CPU reference on the model-clipped records, and — for the un-averaged
results — an f64 bincount of lattice inputs whose every sum is exact in any order.

Shapes: test_plan.OPTION_SHAPES, the fourteen routes at their smallest shapes (k >= 16 for the
lattice) and the dense-flagged uploads of algs 1, 2, 6 and 7; tests/test_plan.py pins their
routes.  The semantics pinned: accumulate is out += sums on every route, whatever the
averaging options say; the clip applies on every route, whatever FLTEE_OPT_DENSE says.

advanced's second sort is reached through k_req != k, whose result is not the plain sum
(advanced.rs:70: unfolded records compete for the prefix): there the un-averaged reference
is n * oracle.advanced(k_req, ...) with n = 4 — exact, since every lattice value / 4 is a
multiple of 2^-6 below 2^8."""
import functools

import numpy as np
import pytest

from conftest import gpu_available
from options_model import (GENERAL_CLIPPING, LATTICE_CLIPPING, bincount_sums, clip_coefs, general, lattice,
                           lattice_prev, reference)
from stable_model import bits_equal
from test_plan import OPTION_SHAPES, R_SWEEP, Plan

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

SEED = 0x5EED0001F00D
ids = dict(ids=lambda c: c[0])


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


def cuda_records(dev, idx, val):
    import torch
    return torch.from_numpy(dev.pack_records(idx, val)).cuda()


def run(dev, alg, idx, val, n, k, d, kw, prev=None, **more):
    import torch
    out = None if prev is None else torch.from_numpy(prev.copy()).cuda()
    got = dev.aggregate(alg, cuda_records(dev, idx, val), n, k, d, out=out, **dict(kw, **more)).cpu().numpy()
    assert dev.status() == 0
    return got


def equal_with_nans(a, b):
    """bit equality, except that a NaN matches any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and bits_equal(a[~nan], b[~nan])


# ------------------------------------------------- clip, averaged, general ----
@functools.lru_cache(maxsize=None)
def general_reference(oracle, case):
    _, alg, n, k, d, kw, _, _ = case
    kw = dict(kw)
    idx, val, _ = general(n, k, d, kw.get("dense", False))
    _, clipped = clip_coefs(val, n, k, GENERAL_CLIPPING)
    return reference(oracle, alg, idx, clipped, n, k, d, kw), reference(oracle, alg, idx, val, n, k, d, kw)


def hashable(case):
    return case[:5] + (tuple(sorted(case[5].items())),) + case[6:]


@pytest.mark.parametrize("case", OPTION_SHAPES, **ids)
def test_clip_equals_the_reference_on_model_clipped_records(dev, oracle, case):
    _, alg, n, k, d, kw, _, _ = case
    idx, val, _ = general(n, k, d, kw.get("dense", False))
    want, unclipped = general_reference(oracle, hashable(case))
    got = run(dev, alg, idx, val, n, k, d, kw, clip=True, clipping=GENERAL_CLIPPING)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{case[0]}: {diff} of {d} differ from the reference on clipped records")
    assert bits_equal(got, want)
    if n * k:  # (no records: nothing to clip)
        assert not bits_equal(got, unclipped)
        assert bits_equal(run(dev, alg, idx, val, n, k, d, kw), unclipped)


# ------------------------------- accumulate, no_average, n_avg: the lattice ----
def lattice_sums(oracle, case, clip):
    _, alg, n, k, d, kw, _, _ = case
    idx, val, coef = lattice(n, k, d, kw.get("dense", False))
    if clip:
        got, val = clip_coefs(val, n, k, LATTICE_CLIPPING)
        assert np.array_equal(got, coef)
    if "k_req" in kw:  # not the plain sum: see the module docstring
        assert n == 4
        return reference(oracle, alg, idx, val, n, k, d, kw) * np.float32(n)
    return bincount_sums(idx, val, d)


@pytest.mark.parametrize("mode", ["accumulate", "no_average", "n_avg"])
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip"])
@pytest.mark.parametrize("case", OPTION_SHAPES, **ids)
def test_unaveraged_options_on_the_lattice(dev, oracle, case, clip, mode):
    _, alg, n, k, d, kw, _, _ = case
    idx, val, _ = lattice(n, k, d, kw.get("dense", False))
    sums = lattice_sums(oracle, case, clip)
    more = dict(clip=True, clipping=LATTICE_CLIPPING) if clip else {}
    if mode == "accumulate":
        prev = lattice_prev(d)
        want = prev + sums
        # the averaging options change nothing under accumulate
        got = run(dev, alg, idx, val, n, k, d, kw, prev=prev, accumulate=True, **more)
        assert bits_equal(run(dev, alg, idx, val, n, k, d, kw, prev=prev, accumulate=True, n_avg=7, **more), want)
    elif mode == "no_average":
        want = sums
        got = run(dev, alg, idx, val, n, k, d, kw, no_average=True, **more)
    else:
        want = sums * (np.float32(1) / np.float32(7))
        got = run(dev, alg, idx, val, n, k, d, kw, n_avg=7, **more)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{case[0]} {mode} clip={clip}: {diff} of {d} differ")
    assert bits_equal(got, want)
    if clip and k >= 16:
        assert not bits_equal(sums, lattice_sums(oracle, case, False))


# ------------------------------------------------------------------- DP ----
@pytest.mark.parametrize("case", OPTION_SHAPES, **ids)
def test_dp_composes_with_clip_and_n_avg(dev, oracle, case):
    """dp on top of clip and n_avg = 7: the same call without dp, then one f32 add of
    f32(f64(clipping * sigma) * z / 7) with the oracle's draws z of that seed (the way
    test_gpu_parity.py::test_dp_noise_matches_oracle_draws takes them: on zeros)."""
    _, alg, n, k, d, kw, _, _ = case
    idx, val, _ = general(n, k, d, kw.get("dense", False))
    kw = dict(kw, seed=SEED, clip=True, clipping=GENERAL_CLIPPING, n_avg=7, sigma=1.12)
    base = run(dev, alg, idx, val, n, k, d, kw)
    got = run(dev, alg, idx, val, n, k, d, kw, dp=True)
    noise = oracle.dp_noise(np.zeros(d, np.float32), 1.12, GENERAL_CLIPPING, 7, seed=SEED)
    assert noise.any() or d == 0
    want = base + noise
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{case[0]}: {diff} of {d} differ from base + the oracle's draws")
    assert bits_equal(got, want)


# ---------------------------------------------------- the clip kernels alone ----
def l2clip(dev, idx, val, n, k, clipping):
    import torch

    from fltee import client as C
    rec = cuda_records(dev, idx, val) if n * k else torch.zeros(0, dtype=torch.int64, device="cuda")
    C.l2clipping(rec, n, k, clipping)
    assert dev.status() == 0
    gi, gv = dev.unpack_records(rec.cpu().numpy())
    assert np.array_equal(gi, idx)
    return gv


@pytest.mark.parametrize("n,k", [(3, k) for k in (1, 63, 64, 65, 255, 256, 257, 1000)] + [(2, (1 << 23) + 1000)])
def test_l2clipping_equals_the_model(dev, n, k):
    """lanes with no element, partial waves, more than one element a lane; n * k > 65536 * 256:
    apply_clip_kernel's grid-stride loop and its 64-bit e / k run past one pass"""
    idx, val, _ = general(n, k, k, True)
    coef, want = clip_coefs(val, n, k, GENERAL_CLIPPING)
    assert (coef < 1).all() and len(set(coef)) == n
    got = l2clip(dev, idx, val, n, k, GENERAL_CLIPPING)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"l2clipping ({n}, {k}): {diff} of {n * k} differ from the model; coef {coef}")
    assert bits_equal(got, want)


def test_l2clipping_of_no_records_touches_nothing(dev):
    import torch

    from fltee import client as C
    rec = torch.full((8,), 0x3F8000000000002A, dtype=torch.int64, device="cuda")
    C.l2clipping(rec, 3, 0, 0.5)
    assert dev.status() == 0
    assert (rec.cpu().numpy() == 0x3F8000000000002A).all()


# --------------------------------------------------------- special values ----
def special_values():
    """four clients of four: one with a NaN (cf 1: the others keep their bits), one with
    +inf (norm inf, cf 0: signed zeros, inf * 0 = NaN), one of 3e38s (t finite in f64, its
    root past f32: norm inf, cf 0), one ordinary; every client on indices of its own"""
    val = np.array([1, np.nan, -2, 0.5,  1, np.inf, -2, -0.0,  3e38, 3e38, 3e38, 3e38,  3, -4, 0, 0], np.float32)
    idx = (np.arange(16) * 5 + 3).astype(np.uint32)
    coef, want = clip_coefs(val, 4, 4, GENERAL_CLIPPING)
    assert list(coef) == [1, 0, 0, np.float32(0.5) / np.float32(5)]
    assert np.isnan(want[[1, 5]]).all() and not want[6:12].any()
    return idx, val, want


def test_special_values_through_l2clipping(dev):
    idx, val, want = special_values()
    assert equal_with_nans(l2clip(dev, idx, val, 4, 4, GENERAL_CLIPPING), want)


def test_special_values_through_the_sweep(dev, oracle):
    idx, val, want = special_values()
    n, k, d = 4, 4, 100
    assert Plan(3, n, k, d, clip=True).route == R_SWEEP
    got = run(dev, 3, idx, val, n, k, d, {}, clip=True, clipping=GENERAL_CLIPPING)
    ref = oracle.baseline(oracle.as_weights(idx, want), d, n)
    assert np.isnan(ref).sum() == 2
    assert equal_with_nans(got, ref)
