"""tests/options_model.py on the CPU: the clip model against the reference's recorded results
(tests/golden/l2clip.npz, client_producer.npz — within 2e-6 relative: torch.norm's f32
accumulation is itself ~1e-6 off the exactly rounded norm at d = 5e4, see
tests/test_gpu_client.py), and the two input families' own conditions."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from options_model import (GENERAL_CLIPPING, LATTICE, LATTICE_CLIPPING, LATTICE_SMALL, bincount_sums,
                           clip_coefs, clip_model, general, general_ok, general_values, lattice, lattice_prev,
                           midpoint_margin)
from test_plan import OPTION_SHAPES

# the clip kernels' own shapes of tests/test_gpu_options.py (n, k)
CLIP_KERNEL_SHAPES = [(3, k) for k in (1, 63, 64, 65, 255, 256, 257, 1000)] + [(2, (1 << 23) + 1000)]


def _vals(b):
    return b.reshape(-1, 8)[:, 4:].copy().view("<f4").ravel()


def test_model_matches_the_reference_l2clip():
    fx = np.load(os.path.join(GOLDEN, "l2clip.npz"))
    got = clip_model(fx["flat_in"], 1, float(fx["clipping"]))
    assert not np.array_equal(got, fx["flat_in"])
    np.testing.assert_allclose(got, fx["flat_out"], rtol=2e-6, atol=0)


def test_model_matches_the_reference_client_clip():
    fx = np.load(os.path.join(GOLDEN, "client_producer.npz"))
    n = len(fx["client_ids"])
    got = clip_model(_vals(fx["plain"]), n, float(fx["clipping"]))
    np.testing.assert_allclose(got, _vals(fx["plain_clip"]), rtol=2e-6, atol=0)
    got = clip_model(fx["flats"].ravel(), n, float(fx["dense_clipping"]))
    np.testing.assert_allclose(got, _vals(fx["dense_clip"]), rtol=2e-6, atol=0)


def test_lattice_tables_state_their_own_coefficients():
    for table in (LATTICE, LATTICE_SMALL):
        for q, a, cf in table:
            norm = a * np.sqrt(q)
            assert norm == int(norm)
            want = min(1.0, LATTICE_CLIPPING / norm) if norm else 1.0
            assert cf == want and np.float32(cf) == cf
            assert (a * cf * 16) == int(a * cf * 16)  # a multiple of 2^-4
        cfs = [(cf, a * cf) for _, a, cf in table]
        assert all(x != y for x, y in zip(cfs, cfs[1:] + cfs[:1]))  # neighbours differ
    assert {cf for _, _, cf in LATTICE} == {0.75, 0.5, 0.375, 1.0}
    assert {a * np.sqrt(q) for q, a, _ in LATTICE} == {4, 6, 8, 1, 3, 0}


@pytest.mark.parametrize("case", OPTION_SHAPES, ids=lambda c: c[0])
def test_lattice_is_exact_under_any_order(case):
    _, alg, n, k, d, kw, _, _ = case
    idx, val, coef = lattice(n, k, d, kw.get("dense", False))
    got, clipped = clip_coefs(val, n, k, LATTICE_CLIPPING)
    assert np.array_equal(got, coef)
    rng = np.random.default_rng(1)
    for c in range(n):
        v = val[c * k:(c + 1) * k].astype(np.float64)
        t = np.sum(v * v)
        for _ in range(3):  # the sum of squares is the same under three shuffles
            p = rng.permutation(k)
            assert np.sum((v * v)[p]) == t and float(np.add.reduce((v * v)[p][::-1])) == t
    assert np.array_equal(clipped * 16, np.round(clipped * 16))
    for v in (val, clipped):
        sums = bincount_sums(idx, v, d)  # (asserts that f32 holds the f64 sums exactly)
        assert np.abs(sums).max(initial=0) < 1024
        prev = lattice_prev(d)
        assert np.array_equal((prev + sums).astype(np.float64), prev.astype(np.float64) + sums)
    if n >= 6 and k >= 16:
        assert set(coef) == {0.75, 0.5, 0.375, 1.0}


@pytest.mark.parametrize("case", OPTION_SHAPES, ids=lambda c: c[0])
def test_general_keeps_the_margin_at_the_first_seed(case):
    _, alg, n, k, d, kw, _, _ = case
    idx, val, seed = general(n, k, d, kw.get("dense", False))
    assert seed == 0
    assert len(idx) == len(val) == n * k
    coef, _ = clip_coefs(val, n, k, GENERAL_CLIPPING)
    assert k == 0 or (coef < 1).all()  # every client with records is clipped


@pytest.mark.parametrize("n,k", CLIP_KERNEL_SHAPES)
def test_general_keeps_the_margin_for_the_clip_kernels_shapes(n, k):
    assert general(n, k, k, True)[2] == 0


def test_margin_condition_tells_a_midpoint():
    a = np.float32(1234.5)
    mid = (np.float64(a) + np.float64(np.nextafter(a, np.float32(np.inf)))) / 2
    assert midpoint_margin(mid * mid) < 2.0 ** -36
    assert midpoint_margin(np.float64(a) ** 2) > 2.0 ** -26
    assert not general_ok(np.array([mid, 0.0]), 1, 2) and general_ok(np.array([float(a), 0.0]), 1, 2)
    assert general_values(3, 5, 17, False, 0)[1].tobytes() == general_values(3, 5, 17, False, 0)[1].tobytes()


def test_special_values_follow_from_the_arithmetic():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    val = np.array([1, nan, -2, 0.5,  1, inf, -2, -0.0,  3e38, 3e38, 3e38, 3e38,  0, 0, 0, 0], np.float32)
    coef, out = clip_coefs(val, 4, 4, 0.5)
    assert list(coef) == [1, 0, 0, 1]
    assert np.array_equal(out[:4].view(np.uint32), val[:4].view(np.uint32))
    assert np.isnan(out[5]) and np.array_equal(out[[4, 6, 7]].view(np.uint32),
                                               np.array([0.0, -0.0, -0.0], np.float32).view(np.uint32))
    assert not out[8:].any()
    assert clip_coefs(np.zeros(0, np.float32), 3, 0, 0.5)[0].tolist() == [1, 1, 1]
