"""tests/krum_model.py on constructed inputs: the definition of FLTEE_OPT_KRUM pinned on the CPU,
before any kernel is asked for it."""
import numpy as np
import pytest

import krum_model as KM
from stable_model import bits_equal


def honest(n, d, seed=1):
    return np.random.default_rng(seed).integers(-8, 9, (n, d)).astype(np.float32)


@pytest.mark.parametrize("n,f", [(7, 2), (17, 3), (33, 10)])
def test_clients_far_away_are_never_kept(n, f):
    v = honest(n, 24)
    bad = [1, n // 2, n - 1][:min(f, 3)] + list(range(2, 2 + max(0, f - 3)))
    v[bad] += np.float32(1e6)
    for m in (1, n - f):
        s, keep = KM.select(v, f, m)
        assert keep.sum() == m and not keep[bad].any()
        assert min(s[bad]) > max(np.delete(s, bad))
        want = KM.in_order_sum(v[keep], np.ones(m, bool)) * (np.float32(1) / np.float32(m))
        assert bits_equal(KM.krum(v, f, m), want.astype(np.float32))


def test_exact_copies_tie_and_are_kept_in_upload_order():
    n, f = 9, 1
    v = np.tile(honest(1, 16), (n, 1))
    s, keep = KM.select(v, f, 3)
    assert (s == 0).all() and list(np.flatnonzero(keep)) == [0, 1, 2]
    # two copies among distinct clients: distance exactly 0, equal scores, the earlier one first
    v = honest(n, 16, seed=5)
    v[6] = v[2]
    D = KM.distances(KM.gram(v)[0])
    assert D[2, 6] == 0 and D[6, 2] == 0
    s, _ = KM.select(v, f, 1)
    assert s[2] == s[6]
    order = sorted(range(n), key=lambda a: (s[a], a))
    assert order.index(2) + 1 == order.index(6)


def test_everyone_kept_is_the_in_order_sum():
    n, d = 11, 40
    v = np.random.default_rng(2).normal(0, 1, (n, d)).astype(np.float32)
    s, keep = KM.select(v, 0, n)
    assert keep.all()
    acc = np.zeros(d, np.float32)
    for c in range(n):
        acc = (acc + v[c]).astype(np.float32)
    assert bits_equal(KM.krum(v, 0, n, no_average=True), acc)
    assert bits_equal(KM.krum(v, 0, n), (acc * (np.float32(1) / np.float32(n))).astype(np.float32))
    assert bits_equal(KM.krum(v, 0, n, n_avg=3), (acc * (np.float32(1) / np.float32(3))).astype(np.float32))
    prev = np.arange(d, dtype=np.float32)
    assert bits_equal(KM.krum(v, 0, n, prev=prev), (prev + acc).astype(np.float32))


def test_nan_and_inf_clients_score_inf_and_come_last_in_upload_order():
    n, f = 9, 2
    v = honest(n, 12, seed=3)
    v[7, 4] = np.nan
    v[3, 0] = np.inf
    s, keep = KM.select(v, f, n - f)
    assert np.isinf(s[3]) and np.isinf(s[7]) and np.isfinite(np.delete(s, [3, 7])).all()
    assert not keep[3] and not keep[7]
    out = KM.krum(v, f, n - f)
    assert np.isfinite(out).all()  # a dropped NaN reaches no sum
    # with room for one of them the earlier upload is taken: +inf scores rank in upload order
    order = sorted(range(n), key=lambda a: (s[a], a))
    assert order[-2:] == [3, 7]


def test_a_distance_below_zero_counts_as_zero_and_minus_zero_columns_sum_to_plus_zero():
    G = np.array([[1.0, 1.0 + 2.0 ** -40], [1.0 + 2.0 ** -40, 1.0]])
    D = KM.distances(G)
    assert (D == 0).all() and not np.signbit(D).any()
    v = honest(5, 6, seed=4)
    v[:, 2] = np.float32(-0.0)
    out = KM.krum(v, 0, 5)
    assert out[2] == 0 and not np.signbit(out[2])


def test_huge_clients_do_not_overflow_the_gram_matrix():
    v = honest(7, 8, seed=6)
    v[5] = np.float32(3e38)
    v[6] = np.float32(-3e38)
    G, _ = KM.gram(v)
    assert np.isfinite(G).all()
    s, keep = KM.select(v, 2, 5)
    assert np.isfinite(s).all() and not keep[5] and not keep[6]


def test_refusals():
    assert KM.refused(4, 1, 1) and not KM.refused(5, 1, 1)        # n < 2 f + 3
    assert KM.refused(3, 0, 0) and KM.refused(3, 0, 4) and not KM.refused(3, 0, 3)
    assert KM.refused(9, 2, 8) and not KM.refused(9, 2, 7)        # m > n - f
    assert KM.refused(1025, 0, 1) and not KM.refused(1024, 0, 1)


def test_the_separation_condition_and_the_bounds():
    rng = np.random.default_rng(7)
    n, d, f, m = 12, 64, 2, 5
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    v[:f] += np.float32(4)
    assert KM.well_separated(v, f, m)
    assert (KM.score_bound(v, f) < 1e-9).all() and (KM.gram_bound(v) >= 0).all()
    w = v.copy()
    w[7] = w[6]  # a tie at the selection's edge cannot be separated
    s, _ = KM.select(w, f, m)
    order = sorted(range(n), key=lambda a: (s[a], a))
    assert not KM.well_separated(w, f, order.index(6) + 1)
