"""The ECALLs with authenticated uploads (fltee_set_upload_aead): the same bits as the CTR
ECALL on the same plaintext for algs 1, 3, 4 and 6; every tamper, a replayed round and an
algorithm downgrade end with retval 0x3001 and an all-zero [out], the round not advanced; the
size refusals stay 0x2; with the switch off the calls behave as before; an eid of two virtual
ranks runs the authenticated ECALL on its root: the one-GPU bits and the same refusals."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D, K = 8, 300, 30
MAC_MISMATCH = 0x3001
IDS = np.arange(500, 500 + N, dtype=np.uint32)
# a dense upload of more than one GHASH segment (8 KB) with a partial last block, for the
# tampers that need a second segment
TN, TD = 3, 1101
TIDS = np.array([7, 260, 65535], np.uint32)
TB = TD * 8


def records(n, d, k, seed):
    rng = np.random.default_rng(seed)
    if k == d:
        idx = np.tile(np.arange(d, dtype=np.uint32), n)
    else:
        idx = np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)
    val = rng.normal(0, 0.01, n * k).astype(np.float32)
    return idx, val


@pytest.fixture
def aead_on():
    from fltee.ecalls import set_upload_aead
    set_upload_aead(True)
    try:
        yield
    finally:
        set_upload_aead(False)


def auth_payload(oracle, idx, val, ids, fl_id, round_, alg):
    """host bytes of the authenticated upload (the library's producer; checked against
    OpenSSL in tests/test_gpu_gcm.py)"""
    import torch

    from fltee import client as C
    rec = torch.from_numpy(oracle.as_weights(idx, val).view(np.int64).copy()).cuda()
    return C.encrypt_parameters_auth(rec, ids, fl_id, round_, alg).cpu().numpy()


def ctr_payload(oracle, idx, val, ids, k):
    w = oracle.as_weights(idx, val).reshape(len(ids), k)
    return oracle.encrypt_clients(ids, [w[c].tobytes() for c in range(len(ids))])


def start(E, fl_id, ids, d, k, alg):
    assert E.ecall_fl_init(fl_id, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, 0) == (0, 0)
    assert E.ecall_start_round(fl_id, 0, len(ids))[:2] == (0, 0)


def call(E, fl_id, round_, ids, enc, d, k, alg):
    if alg == 6:
        return E.ecall_client_size_optimized_secure_aggregation(fl_id, round_, 3, ids, enc, d, k, alg)
    return E.ecall_secure_aggregation(fl_id, round_, ids, enc, d, k, alg)


@pytest.mark.parametrize("device", [0, [0, 0]], ids=["one_gpu", "two_virtual_ranks"])
@pytest.mark.parametrize("alg,k", [(1, K), (3, K), (4, K), (6, K), (3, D)])
def test_aead_ecall_equals_the_ctr_ecall(oracle, alg, k, device):
    import torch

    from fltee.ecalls import Enclave, set_upload_aead
    torch.cuda.init()
    idx, val = records(N, D, k, 10 * alg + k)
    fl = 8000 + 10 * alg + (k == D)
    E = Enclave(device)
    try:
        start(E, fl, IDS, D, k, alg)
        st, rv, ref, _ = call(E, fl, 0, IDS, ctr_payload(oracle, idx, val, IDS, k), D, k, alg)
        assert (st, rv) == (0, 0)
        enc = auth_payload(oracle, idx, val, IDS, fl, 0, alg)
        assert enc.nbytes == N * (k * 8 + 16)
        set_upload_aead(True)
        try:
            start(E, fl, IDS, D, k, alg)
            st, rv, out, times = call(E, fl, 0, IDS, enc, D, k, alg)
        finally:
            set_upload_aead(False)
    finally:
        E.destroy()
    assert (st, rv) == (0, 0)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    assert np.isfinite(times).all()


def flip(enc, stride, client, offset, bit=1):
    e = enc.copy()
    e[client * stride + offset] ^= bit
    return e


def swapped(enc, stride):
    e = enc.copy()
    e[:stride], e[stride:2 * stride] = enc[stride:2 * stride], enc[:stride]
    return e


TAMPERS = [
    ("ciphertext first byte", lambda e, s: flip(e, s, 1, 0)),
    ("last byte of the partial block", lambda e, s: flip(e, s, 2, TB - 1, 0x80)),
    ("a byte in the second segment", lambda e, s: flip(e, s, 0, 8192 + 77, 4)),
    ("tag byte 0", lambda e, s: flip(e, s, 1, TB)),
    ("tag byte 15", lambda e, s: flip(e, s, 1, TB + 15, 0x80)),
    ("two clients' slices swapped", lambda e, s: swapped(e, s)),
]


@pytest.fixture(scope="module")
def tamper_case(oracle):
    """(idx, val) of the two-segment dense upload: built once, never modified"""
    assert TB > 8192 and TB % 16 == 8
    return records(TN, TD, TD, 77)


@pytest.mark.parametrize("device", [0, [0, 0]], ids=["one_gpu", "two_virtual_ranks"])
def test_aead_ecall_tampers_are_mac_mismatches(oracle, tamper_case, aead_on, device):
    """every tamper: 0x3001, [out] all zero, the timers written, the round kept — the good
    payload is then answered for the same round"""
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    idx, val = tamper_case
    alg, fl = 4, 8200
    good = auth_payload(oracle, idx, val, TIDS, fl, 0, alg)
    stride = TB + 16
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), TD, TN)
    assert st == 0
    E = Enclave(device)
    try:
        start(E, fl, TIDS, TD, TD, alg)
        for what, change in TAMPERS:
            st, rv, out, times = E.ecall_secure_aggregation(fl, 0, TIDS, change(good, stride), TD, TD, alg)
            assert (st, rv) == (0, MAC_MISMATCH), what
            assert not out.view(np.uint32).any(), what
            assert np.isfinite(times).all()
        # the AAD binds the client id: client 0's slice under another id list position
        other = auth_payload(oracle, idx, val, TIDS[[1, 0, 2]], fl, 0, alg)
        st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, TIDS, other, TD, TD, alg)
        assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
        st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, TIDS, good, TD, TD, alg)
        assert (st, rv) == (0, 0)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    finally:
        E.destroy()


@pytest.mark.parametrize("device", [0, [0, 0]], ids=["one_gpu", "two_virtual_ranks"])
def test_aead_ecall_replay_downgrade_and_sizes(oracle, aead_on, device):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    idx, val = records(N, D, K, 5)
    fl = 8300
    r0 = auth_payload(oracle, idx, val, IDS, fl, 0, 1)
    r1 = auth_payload(oracle, idx, val, IDS, fl, 1, 1)
    E = Enclave(device)
    try:
        start(E, fl, IDS, D, K, 1)
        # a wrong total size: 0x2 as before (too short for k records; not n whole slices)
        for bad in (r0[:-8 * N], r0[:-1], r0[:N * 8]):
            st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, IDS, bad, D, K, 1)
            assert (st, rv) == (0, 2) and not out.view(np.uint32).any()
        st, rv, ref, _ = E.ecall_secure_aggregation(fl, 0, IDS, r0, D, K, 1)
        assert (st, rv) == (0, 0)
        # round 0's payload replayed at round 1
        assert E.ecall_start_round(fl, 1, N)[:2] == (0, 0)
        st, rv, out, _ = E.ecall_secure_aggregation(fl, 1, IDS, r0, D, K, 1)
        assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
        st, rv, out, _ = E.ecall_secure_aggregation(fl, 1, IDS, r1, D, K, 1)
        assert (st, rv) == (0, 0) and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
        # encrypted for alg 1, submitted as alg 4 (the config re-initialised accordingly)
        start(E, fl, IDS, D, K, 4)
        st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, IDS, r0, D, K, 4)
        assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
        # alg 6: a tampered slice, and the wrong alg in the AAD
        start(E, fl, IDS, D, K, 6)
        a6 = auth_payload(oracle, idx, val, IDS, fl, 0, 6)
        for bad in (flip(a6, K * 8 + 16, 5, 3), r0):
            st, rv, out, _ = E.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, IDS, bad, D, K, 6)
            assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
        st, rv, out, _ = E.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, IDS, a6, D, K, 6)
        assert (st, rv) == (0, 0)
    finally:
        E.destroy()


def test_aead_off_behaves_as_before(oracle):
    """The switch off (the default): a CTR payload is answered, and an authenticated payload
    is just a longer CTR payload (no 0x3001 exists on this path)."""
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    idx, val = records(N, D, K, 6)
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), D, N)
    E = Enclave(0)
    try:
        start(E, 8400, IDS, D, K, 4)
        st, rv, out, _ = E.ecall_secure_aggregation(8400, 0, IDS, ctr_payload(oracle, idx, val, IDS, K), D, K, 4)
        assert (st, rv) == (0, 0) and np.array_equal(out.view(np.uint32), ref.view(np.uint32))
        start(E, 8400, IDS, D, K, 4)
        st, rv, out, _ = E.ecall_secure_aggregation(8400, 0, IDS, auth_payload(oracle, idx, val, IDS, 8400, 0, 4),
                                                    D, K, 4)
        assert rv != MAC_MISMATCH
    finally:
        E.destroy()
