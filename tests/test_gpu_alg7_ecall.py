"""ecall_secure_aggregation with aggregation_alg 7 (lib.rs:389): encrypted uploads on the
small staged path and on the large pipelined path (payload > 16 MB), against the model
(tests/stable_model.py) and oracle.non_oblivious of the same plaintext, bit for bit; the
round counter; the alg check against ecall_fl_init; a 2-virtual-rank eid (alg 7 runs on
the root: the same bits).  The ECALL answers alg 7 once the host has opted in
(fltee_set_bubble_ecall): the tests switch it on for themselves and off again, and one
checks that it is off by default (0x2, as before)."""
import numpy as np
import pytest

from conftest import gpu_available
from stable_model import bits_equal, distinct_indices, model

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ALG_BUBBLE = 7
SMALL, LARGE = (30, 500, 5000), (30, 70000, 100000)


@pytest.fixture(scope="module")
def cases(oracle):
    """shape -> (ids, ciphertext, expected): built once, shared, never modified"""
    out = {}
    for n, k, d in (SMALL, LARGE):
        rng = np.random.default_rng(n + k)
        idx = distinct_indices(rng, n, k, d)
        val = rng.normal(0, 0.01, n * k).astype(np.float32)
        ids = np.arange(200, 200 + n, dtype=np.uint32)
        w = oracle.as_weights(idx, val).reshape(n, k)
        enc = oracle.encrypt_clients(ids, [w[c].tobytes() for c in range(n)])
        ref = model(idx, val, n, d)
        plain, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
        assert st == 0 and bits_equal(ref, plain)
        out[(n, k, d)] = (ids, enc, ref)
    return out


@pytest.fixture
def bubble_on():
    from fltee.ecalls import set_bubble_ecall
    set_bubble_ecall(True)
    try:
        yield
    finally:
        set_bubble_ecall(False)


def start(E, fl_id, ids, d, k, alg, dp=0):
    assert E.ecall_fl_init(fl_id, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, dp) == (0, 0)
    assert E.ecall_start_round(fl_id, 0, len(ids))[:2] == (0, 0)


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_ecall_alg7_equals_the_model(cases, bubble_on, shape):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    n, k, d = shape
    ids, enc, ref = cases[shape]
    assert (n * k * 8 > (16 << 20)) == (shape == LARGE)
    E = Enclave(0)
    try:
        start(E, 7100 + n + k, ids, d, k, ALG_BUBBLE)
        st, rv, out, times = E.ecall_secure_aggregation(7100 + n + k, 0, ids, enc, d, k, ALG_BUBBLE)
    finally:
        E.destroy()
    assert (st, rv) == (0, 0)
    assert bits_equal(out, ref)
    assert np.isfinite(times).all()


def test_ecall_alg7_round_counter_alg_check_and_k_req(cases, bubble_on):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    n, k, d = SMALL
    ids, enc, ref = cases[SMALL]
    E = Enclave(0)
    try:
        start(E, 7200, ids, d, k, ALG_BUBBLE)
        # another alg than ecall_fl_init's: 0x2, [out] zero-filled, the round stays
        st, rv, out, _ = E.ecall_secure_aggregation(7200, 0, ids, enc, d, k, 1)
        assert (st, rv) == (0, 2) and not out.any()
        st, rv, out, _ = E.ecall_secure_aggregation(7200, 0, ids, enc, d, k, ALG_BUBBLE)
        assert (st, rv) == (0, 0) and bits_equal(out, ref)
        # the round advanced: round 0 is refused, round 1 answered
        st, rv, out, _ = E.ecall_secure_aggregation(7200, 0, ids, enc, d, k, ALG_BUBBLE)
        assert (st, rv) == (0, 2)
        assert E.ecall_start_round(7200, 1, n)[:2] == (0, 0)
        st, rv, out, _ = E.ecall_secure_aggregation(7200, 1, ids, enc, d, k, ALG_BUBBLE)
        assert (st, rv) == (0, 0) and bits_equal(out, ref)
        # a config made for advanced refuses alg 7
        start(E, 7201, ids, d, k, 1)
        st, rv, out, _ = E.ecall_secure_aggregation(7201, 0, ids, enc, d, k, ALG_BUBBLE)
        assert (st, rv) == (0, 2) and not out.any()
        # k_req past the payload (advanced.rs:72's panic) and k_req != k: 0x2
        for fl, k_req in ((7202, k + 1), (7203, k - 1)):
            start(E, fl, ids, d, k_req, ALG_BUBBLE)
            st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k_req, ALG_BUBBLE)
            assert (st, rv) == (0, 2) and not out.any()
    finally:
        E.destroy()


def test_ecall_alg7_dp_adds_the_seeded_noise(cases, bubble_on):
    import torch

    from fltee import device as D
    from fltee.ecalls import Enclave, set_debug_seed
    torch.cuda.init()
    n, k, d = SMALL
    ids, enc, ref = cases[SMALL]
    E = Enclave(0)
    outs = []
    try:
        for fl in (7300, 7301):
            set_debug_seed(4242)
            try:
                start(E, fl, ids, d, k, ALG_BUBBLE, dp=1)
                st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, ALG_BUBBLE)
            finally:
                set_debug_seed(0)
            assert (st, rv) == (0, 0)
            outs.append(out)
    finally:
        E.destroy()
    assert bits_equal(outs[0], outs[1])           # the same seed: the same noise
    noise = outs[0] - ref
    assert noise.any() and abs(float(noise.std()) - 1.12 / n) < 0.2 * 1.12 / n
    assert D.status() == 0


def test_ecall_alg7_two_virtual_ranks_same_bits(cases, bubble_on):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    n, k, d = SMALL
    ids, enc, ref = cases[SMALL]
    E = Enclave([0, 0])
    try:
        assert E.device_count() == 2
        start(E, 7400, ids, d, k, ALG_BUBBLE)
        st, rv, out, _ = E.ecall_secure_aggregation(7400, 0, ids, enc, d, k, ALG_BUBBLE)
    finally:
        E.destroy()
    assert (st, rv) == (0, 0) and bits_equal(out, ref)


def test_ecall_alg7_is_off_until_the_host_opts_in(cases):
    import torch

    from fltee.ecalls import Enclave, set_bubble_ecall
    torch.cuda.init()
    n, k, d = SMALL
    ids, enc, ref = cases[SMALL]
    E = Enclave(0)
    try:
        start(E, 7500, ids, d, k, ALG_BUBBLE)
        st, rv, out, _ = E.ecall_secure_aggregation(7500, 0, ids, enc, d, k, ALG_BUBBLE)
        assert (st, rv) == (0, 2) and not out.any()       # the default: refused, round kept
        set_bubble_ecall(True)
        try:
            st, rv, out, _ = E.ecall_secure_aggregation(7500, 0, ids, enc, d, k, ALG_BUBBLE)
        finally:
            set_bubble_ecall(False)
        assert (st, rv) == (0, 0) and bits_equal(out, ref)
    finally:
        E.destroy()
