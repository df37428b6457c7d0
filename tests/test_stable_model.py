"""The model of aggregation_alg 7 the GPU tests compare against (tests/stable_model.py):
the stable sort by idx with the zero entries last, each run left-folded in float32.  It is
the in-order client sum — oracle.non_oblivious bit for bit — and it is sensitive to the
order of the clients on the order-sensitive input, which is what makes the GPU check
against it discriminating.  CPU only."""
import numpy as np
import pytest

from stable_model import bits_equal, distinct_indices, model, order_sensitive


@pytest.mark.parametrize("n,k,d", [(1, 1, 1), (3, 5, 17), (30, 500, 5000), (7, 64, 64)])
def test_model_equals_non_oblivious_on_random_uploads(oracle, n, k, d):
    rng = np.random.default_rng(n * 1000 + k)
    idx = distinct_indices(rng, n, k, d)
    val = rng.normal(0, 0.01, n * k).astype(np.float32)
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0 and bits_equal(model(idx, val, n, d), ref)


def test_model_equals_non_oblivious_with_repeats_and_signed_zeros(oracle):
    rng = np.random.default_rng(5)
    n, k, d = 6, 40, 50
    idx = rng.integers(0, d, n * k).astype(np.uint32)  # clients repeat indices
    val = rng.normal(0, 1, n * k).astype(np.float32)
    val[::7] = -0.0
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0 and bits_equal(model(idx, val, n, d), ref)


def test_model_ignores_out_of_range_records():
    idx = np.array([3, 9, 3, 2 ** 31 - 1, 10], np.uint32)
    val = np.array([1, 2, 3, 4, 5], np.float32)
    out = model(idx, val, 1, 10)
    assert out[3] == 4 and out[9] == 2 and out.sum() == 6


@pytest.mark.parametrize("n,k,d", [(3, 5, 17), (30, 500, 5000), (400, 1000, 20000), (30, 5089, 50890)])
def test_order_sensitive_input_separates_advanced(oracle, n, k, d):
    """The enclave model of advanced (the bitonic network's tie order) is another float32
    value than the in-order sum on this input, at every shape of tests/test_gpu_alg7.py
    with more than one client: what its alg 7 != advanced check relies on."""
    idx, val = order_sensitive(n, k, d)
    adv, st = oracle.advanced(k, oracle.as_weights(idx, val), d, n)
    assert st == 0 and not bits_equal(adv, model(idx, val, n, d))


# (n a multiple of four: whole cycles.  A partial cycle can read the same from both ends —
# 1e8 absorbs the small terms next to it — as at n = 3 and n = 30.)
@pytest.mark.parametrize("n,k,d", [(4, 5, 17), (32, 500, 5000)])
def test_order_sensitive_input_shows_the_client_order(oracle, n, k, d):
    idx, val = order_sensitive(n, k, d)
    fwd = model(idx, val, n, d)
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0 and bits_equal(fwd, ref)
    ridx = idx.reshape(n, k)[::-1].reshape(-1)
    rval = val.reshape(n, k)[::-1].reshape(-1)
    rev = model(ridx, rval, n, d)
    assert not bits_equal(fwd, rev), "the reversed client order must change some parameter"
