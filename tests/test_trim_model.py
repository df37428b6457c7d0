"""tests/trim_model.py, the numpy definition of FLTEE_OPT_TRIM, against a brute-force Python
implementation of the same words, the median, the untrimmed oracle, and the library's
fltee_trim_count.  No device is touched."""
import os
import statistics

import numpy as np
import pytest

import trim_model as TM
from conftest import ROOT
from stable_model import bits_equal

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")

SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0, 2.0 ** 24, 1e30], np.float32)


def columns(rng, n, d):
    """random columns with ties, signed zeros, infinities and NaNs of both signs mixed in"""
    v = rng.integers(-4, 5, (n, d)).astype(np.float32) * np.float32(0.5)
    v = np.where(rng.random((n, d)) < 0.5, rng.normal(0, 100, (n, d)).astype(np.float32), v)
    v = np.where(rng.random((n, d)) < 0.15, SPECIAL[rng.integers(0, len(SPECIAL), (n, d))], v)
    return np.ascontiguousarray(v, np.float32)


def test_ord_is_the_total_order_of_the_definition():
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
    pos_nan = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    chain = np.array([neg_nan, -np.inf, -1e30, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 1e30, np.inf, pos_nan],
                     np.float32)
    o = TM.ord_key(chain).astype(np.int64)
    assert (np.diff(o) > 0).all()
    assert int(TM.ord_key(np.float32(0.0))) == 0x80000000 and int(TM.ord_key(np.float32(-0.0))) == 0x7FFFFFFF


@pytest.mark.parametrize("n,t", [(3, 1), (7, 0), (7, 2), (7, 3), (8, 3), (16, 5), (17, 8)])
def test_model_equals_brute_force_on_1000_columns(n, t):
    v = columns(np.random.default_rng(n * 100 + t), n, 1000)
    got = TM.sums(v, t)
    want = np.array([TM.brute_column(v[:, j], t) for j in range(1000)], np.float32)
    assert bits_equal(got, want)
    assert (TM.kept(v, t).sum(axis=0) == n - 2 * t).all()


@pytest.mark.parametrize("n", [3, 5, 17, 33])
def test_odd_n_with_the_largest_t_is_the_median(n):
    v = np.random.default_rng(n).normal(0, 1, (n, 300)).astype(np.float32)
    got = TM.trimmed(v, (n - 1) // 2)
    assert bits_equal(got, np.median(v, axis=0).astype(np.float32))
    assert got[7] == np.float32(statistics.median(float(x) for x in v[:, 7]))


def test_even_n_is_the_mean_of_the_two_middle_values():
    n = 6
    v = np.random.default_rng(6).integers(-50, 50, (n, 300)).astype(np.float32)
    s = np.sort(v, axis=0)
    # (the in-order sum of two small integers is exact either way round)
    assert bits_equal(TM.trimmed(v, n // 2 - 1), (s[2] + s[3]) * (np.float32(1) / np.float32(2)))


def test_the_tie_rule_removes_the_earliest_uploads_on_both_sides():
    big, one = np.float32(2.0 ** 24), np.float32(1)
    # t = 1: two copies of the minimum (1) and of the maximum (2^24); the first of each goes
    col = np.array([big, one, one, big, one + one], np.float32)[:, None]
    keep = TM.kept(col, 1)[:, 0]
    assert keep.tolist() == [False, False, True, True, True]
    # all equal: low takes clients 0, 1, high the next two
    assert TM.kept(np.ones((5, 1), np.float32), 2)[:, 0].tolist() == [False, False, False, False, True]


def test_nans_are_trimmed_first_and_a_surplus_one_survives():
    v = np.array([[1.0], [np.nan], [2.0], [-np.nan], [3.0]], np.float32)
    assert TM.trimmed(v, 1)[0] == np.float32(2.0)
    v[2, 0] = np.nan  # two +NaN, t = 1: one stays
    assert np.isnan(TM.trimmed(v, 1)[0])


@pytest.mark.parametrize("n,d", [(4, 257), (7, 64)])
def test_t_zero_is_the_oracles_baseline(oracle, n, d):
    v = np.random.default_rng(d).normal(0, 1, (n, d)).astype(np.float32)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    ref = oracle.baseline(oracle.as_weights(idx, v.reshape(-1)), d, n)
    assert bits_equal(TM.trimmed(v, 0), ref)


COUNT_N = [0, 1, 2, 3, 10, 100, 129, 130, 1000, 2 ** 40]
COUNT_PM = [0, 1, 100, 499, 500, 501, 1000, 0xFFFFFFFF]
TABLE = {  # (n, per_mille) -> t, by hand
    (1, 500): 0, (2, 500): 0, (3, 500): 1, (3, 100): 0, (3, 499): 1, (100, 0): 0, (100, 100): 10,
    (100, 499): 49, (100, 500): 49, (129, 100): 12, (129, 499): 64, (129, 500): 64, (130, 100): 13,
    (130, 499): 64, (130, 500): 64, (1, 0): 0, (2, 100): 0, (2, 499): 0, (1, 100): 0, (1, 499): 0,
    (3, 0): 0, (129, 0): 0, (130, 0): 0, (2, 0): 0, (10, 100): 1, (10, 500): 4,
}


@needs_lib
def test_fltee_trim_count():
    from fltee import _lib as L
    from fltee import ecalls as E
    for (n, pm), t in TABLE.items():
        assert L.lib().fltee_trim_count(n, pm) == t == TM.trim_count(n, pm), (n, pm)
    for n in COUNT_N:
        for pm in COUNT_PM:
            t = E.trim_count(n, pm)
            assert t == TM.trim_count(n, pm)
            assert t == 0 if n == 0 else 2 * t < n
