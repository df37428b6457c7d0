"""tests/gmed_model.py itself: the numpy definition of FLTEE_OPT_GMED behaves like a geometric
median before any kernel is held to it."""
import functools

import numpy as np

import gmed_model as M


def test_sum64_is_the_stated_order():
    """lane partials over i = l (mod 64) in ascending i, then the partials in ascending l — on
    values where every other association rounds differently"""
    rng = np.random.default_rng(64)
    for n in (1, 2, 63, 64, 65, 129, 1000):
        v = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
        p = [0.0] * 64
        for i in range(n):
            p[i % 64] = p[i % 64] + v[i]
        s = 0.0
        for lane in range(64):
            s = s + p[lane]
        assert M.sum64(v) == s
        assert np.array_equal(M.sum64(np.stack([v, 2 * v])), [s, 2 * s])
    assert M.sum64(np.zeros(0)) == 0.0 and not np.signbit(M.sum64(np.array([-0.0])))


def test_three_collinear_points_concentrate_on_the_middle_one():
    direction = np.array([3, -4, 12, 0, 5], np.float32)
    v = np.stack([0 * direction, 1 * direction, 3 * direction]).astype(np.float32)
    last = 0.0
    for iters in (1, 2, 4, 8):
        alpha, rho, valid = M.weights(v, iters)
        assert valid.all() and alpha[1] > last and alpha[1] > alpha[0] and alpha[1] > alpha[2]
        last = alpha[1]
    assert last > 0.999 and rho[1] < 1e-3  # the iterate sits on the middle point
    out = M.gmed(v, 8)
    assert np.abs(out - v[1]).max() < 1e-4


def test_the_smoothed_objective_does_not_increase():
    """sum_c max(nu, |x_c - z|) along the iterates z_r = sum w x / sum w, z_0 the mean, over the
    first six iterations, where every step still descends by far more than the objective's own
    rounding (the later steps are below 1e-9 and would compare noise)"""
    for seed in range(5):
        rng = np.random.default_rng(seed)
        n, d = 30, 17
        v = rng.normal(0, 1, (n, d)).astype(np.float32)
        v[:5] += 4
        G, valid, w = M.gram(v), np.ones(n, bool), np.ones(n)
        x = v.astype(np.float64)
        obj = [M.objective(v, (w / w.sum()) @ x, M.NU)]
        for _ in range(6):
            w, _ = M.iterate(G, valid, w, M.NU)
            obj.append(M.objective(v, (w / w.sum()) @ x, M.NU))
        assert all(b <= a for a, b in zip(obj, obj[1:])), obj


def test_a_minority_of_huge_clients_does_not_move_it_out_of_the_inliers_ball():
    for seed, n, b in ((5, 21, 8), (6, 9, 4), (7, 100, 49)):
        rng = np.random.default_rng(seed)
        d = 40
        v = rng.normal(0, 1, (n, d)).astype(np.float32)
        bad = rng.choice(n, b, replace=False)
        v[bad] = (rng.normal(0, 1, (b, d)) * 1e6).astype(np.float32)
        inl = np.setdiff1d(np.arange(n), bad)
        c = v[inl].astype(np.float64).mean(0)
        radius = np.sqrt(((v[inl] - c) ** 2).sum(1)).max()
        dist = lambda z: np.sqrt(((z - c) ** 2).sum())
        assert dist(M.gmed(v, 32)) < radius
        assert dist(v.astype(np.float64).mean(0)) > 1000 * radius


GENERAL = [(20, 300, 3, 11), (100, 1027, 8, 12), (150, 513, 4, 13)]  # n, d, R, seed (tests/test_gpu_gmed.py)


@functools.lru_cache(maxsize=None)
def general_values(n, d, seed):
    """N(0, 1) rows, a tenth of them shifted: built once, never modified"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    bad = rng.choice(n, n // 10, replace=False)
    v[bad] += rng.normal(0.5, 0.1, (n // 10, 1)).astype(np.float32)
    v.setflags(write=False)
    return v


def test_the_general_seeds_stay_within_one_ulp_under_two_gram_orders():
    """what tests/test_gpu_gmed.py allows the device: a conforming Gram order (numpy's product, a
    sequential longdouble sum rounded once) moves alpha by at most its one rounding to f32 —
    and rho by a relative O(n d 2^-53), far below 2^-24"""
    for n, d, iters, seed in GENERAL:
        v = general_values(n, d, seed)
        a0, r0, _ = M.weights_from(M.gram(v), iters, M.NU)
        a1, r1, _ = M.weights_from(M.gram_longdouble(v), iters, M.NU)
        ulp = np.abs(a0.view(np.int32).astype(np.int64) - a1.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, (n, d, ulp.max())
        assert np.abs(r1 / r0 - 1).max() < n * d * 2.0 ** -53
        assert abs(float(a0.astype(np.float64).sum()) - 1) < n * 2.0 ** -24


def test_invalid_clients_reach_nothing():
    rng = np.random.default_rng(9)
    v = rng.integers(-8, 9, (7, 11)).astype(np.float32)
    v[2, 3], v[5, 0] = np.nan, np.inf
    alpha, rho, valid = M.weights(v, 3)
    assert list(valid) == [True, True, False, True, True, False, True]
    assert alpha[2] == 0 and alpha[5] == 0 and np.isinf(rho[[2, 5]]).all()
    keep = [0, 1, 3, 4, 6]
    a2, r2, _ = M.weights(v[keep], 3)
    assert np.array_equal(alpha[keep], a2)  # (7 clients: one lane each, the zeros change no sum)
    assert np.isfinite(M.gmed(v, 3)).all()
    none = np.full((3, 4), np.nan, np.float32)
    out = M.gmed(none, 2)
    assert not out.view(np.uint32).any()


def test_identical_clients_sit_on_the_floor():
    v = np.tile(np.arange(5, dtype=np.float32), (6, 1))
    alpha, rho, _ = M.weights(v, 2, nu=0.25)
    assert not rho.any() and np.array_equal(alpha, np.full(6, 4.0 / 24.0, np.float32))
