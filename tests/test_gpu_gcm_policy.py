"""Authenticated rounds with a failure policy (fltee_set_upload_aead_policy; the shapes and
helpers of tests/test_gpu_gcm_ecall.py, restated here): n = 8, d = 256, k = 32, on one GPU and
on an eid of two virtual ranks.

  1. DROP aggregates exactly the verified clients: retval 0 and [out] bit-equal to the oracle's
     aggregate of the survivors' plaintext with n' — algs 1, 3, 4, 5 (sweep and tree), 7, 3
     dense and 6 (batches of 3: six survivors are 3 + 3, one survivor a single batch of one) —
     for the tamper sets {0}, {7}, {2, 5}, {0..6} (a ciphertext bit on even clients, a tag bit
     on odd ones); the round advanced and the next round's clean call is answered; the report
     names the tampered ids in upload order with the call's round.
  2. nips19 and DP draw from the call's seed: the tampered DROP call equals, bit for bit, a
     clean authenticated call of the survivors alone under the same seed — n' in the threshold
     and in the noise divisor.
  3. Below the quorum (all eight tampered; {0..6} with min_survivors = 2): 0x3001, zeros,
     timers written, round kept, report filled.
  4. REPORT: the tampered call ends as under ABORT, the report is filled, and a clean call
     stores an empty one.
  5. ABORT (the default): 0x3001 and nothing stored.
  6. The launch trace under DROP: up to and including the verdict readback a function of the
     public sizes (clean, adversarial, tampered); after it a function of the sizes and the
     failed set; a clean DROP call is the clean ABORT call but for that readback's byte count.
"""
import numpy as np
import pytest

from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced, uploads

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D, K = 8, 256, 32
BATCH = 3
MAC_MISMATCH = 0x3001
IDS = np.arange(500, 500 + N, dtype=np.uint32)
DEVICES = [0, [0, 0]]
DEVICE_IDS = ["one_gpu", "two_virtual_ranks"]
TAMPER_SETS = [(0,), (7,), (2, 5), (0, 1, 2, 3, 4, 5, 6)]
# (name, alg, k): "5t" = path_oram as the tree, "3d" = dense uploads
VARIANTS = [("1", 1, K), ("3", 3, K), ("4", 4, K), ("5", 5, K), ("5t", 5, K), ("7", 7, K),
            ("3d", 3, D), ("6", 6, K)]


def records(n, d, k, seed):
    rng = np.random.default_rng(seed)
    if k == d:
        idx = np.tile(np.arange(d, dtype=np.uint32), n)
    else:
        idx = np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)
    val = rng.normal(0, 0.01, n * k).astype(np.float32)
    return idx, val


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


def tamper(enc, k, clients):
    """one flipped bit per client: in the ciphertext of an even client, in the tag of an odd one"""
    e = enc.copy()
    stride = k * 8 + 16
    for c in clients:
        off = (13 + 8 * c) % (k * 8) if c % 2 == 0 else k * 8 + (c % 16)
        e[c * stride + off] ^= 1 << (c % 8)
    return e


def survivors(idx, val, k, dropped):
    keep = [c for c in range(N) if c not in dropped]
    return keep, idx.reshape(N, k)[keep].reshape(-1), val.reshape(N, k)[keep].reshape(-1)


def oracle_aggregate(oracle, alg, ids, idx, val, d, k, fl):
    """the oracle call of the existing ECALL tests on these clients alone: its ECALL mirror on
    their CTR payload (tests/test_gpu_ecalls.py), alg 7 by the in-order sum
    (tests/test_gpu_alg7_ecall.py)"""
    n = len(ids)
    if alg == 7:
        ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
        assert st == 0
        return ref
    enc = ctr_payload(oracle, idx, val, ids, k)
    O = oracle.OracleEnclave(seed=1)
    assert O.fl_init(fl, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg) == 0
    O.start_round(fl, 0, n)
    if alg == 6:
        st, ref, _ = O.client_size_optimized_secure_aggregation(fl, 0, BATCH, ids, enc, d, k, alg)
    else:
        st, ref, _ = O.secure_aggregation(fl, 0, ids, enc, d, k, alg)
    assert st == 0
    return ref


def start(E, fl_id, ids, d, k, alg, dp=0):
    assert E.ecall_fl_init(fl_id, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, dp) == (0, 0)
    assert E.ecall_start_round(fl_id, 0, len(ids))[:2] == (0, 0)


def call(E, fl_id, round_, ids, enc, d, k, alg):
    if alg == 6:
        return E.ecall_client_size_optimized_secure_aggregation(fl_id, round_, BATCH, ids, enc, d, k, alg)
    return E.ecall_secure_aggregation(fl_id, round_, ids, enc, d, k, alg)


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module", params=DEVICES, ids=DEVICE_IDS)
def enclave(request):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    E = Enclave(request.param)
    yield E
    E.destroy()


@pytest.fixture
def switches():
    """AEAD on; the policy and every other process-wide switch restored after each test"""
    from fltee import ecalls as X
    X.set_upload_aead(True)
    try:
        yield X
    finally:
        X.set_upload_aead_policy("abort", 1)
        X.set_upload_aead(False)
        X.set_bubble_ecall(False)
        X.set_path_oram_tree(False)
        X.set_debug_seed(0)


@pytest.fixture(scope="module")
def uploads_by_variant(oracle):
    """name -> (idx, val) of the eight clients; built once, never modified"""
    return {name: records(N, D, k, 100 + i) for i, (name, _, k) in enumerate(VARIANTS)}


@pytest.mark.parametrize("dropped", TAMPER_SETS, ids=lambda s: "tamper_" + "".join(map(str, s)))
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "alg_" + v[0])
def test_drop_aggregates_the_verified_clients(oracle, enclave, switches, uploads_by_variant, variant, dropped):
    name, alg, k = variant
    idx, val = uploads_by_variant[name]
    fl = 8700 + 10 * VARIANTS.index(variant) + TAMPER_SETS.index(dropped)
    switches.set_bubble_ecall(alg == 7)
    switches.set_path_oram_tree(name == "5t")
    switches.set_upload_aead_policy("drop")
    keep, sidx, sval = survivors(idx, val, k, dropped)
    if alg == 6:  # the batches re-formed over S in order: 3 + 3, or a single batch of one
        assert len(keep) in (7, 6, 1)
    want = oracle_aggregate(oracle, alg, IDS[keep], sidx, sval, D, k, fl)
    enc = tamper(auth_payload(oracle, idx, val, IDS, fl, 0, alg), k, dropped)
    start(enclave, fl, IDS, D, k, alg)
    st, rv, out, times = call(enclave, fl, 0, IDS, enc, D, k, alg)
    assert (st, rv) == (0, 0)
    assert bits_equal(out, want)
    assert np.isfinite(times).all() and (times >= 0).all()
    assert enclave.auth_report(fl) == (0, [int(IDS[c]) for c in dropped])
    # the round advanced: round 0 is refused now, and the clean upload of round 1 is answered
    # with all eight clients; its (empty) verdict replaces the stored one
    st, rv, out0, _ = call(enclave, fl, 0, IDS, enc, D, k, alg)
    assert (st, rv) == (0, 2) and not out0.view(np.uint32).any()
    assert enclave.ecall_start_round(fl, 1, N)[:2] == (0, 0)
    st, rv, out1, _ = call(enclave, fl, 1, IDS, auth_payload(oracle, idx, val, IDS, fl, 1, alg), D, k, alg)
    assert (st, rv) == (0, 0)
    assert bits_equal(out1, oracle_aggregate(oracle, alg, IDS, idx, val, D, k, fl))
    assert enclave.auth_report(fl) == (1, [])


@pytest.mark.parametrize("dropped", [(0,), (2, 5)], ids=lambda s: "tamper_" + "".join(map(str, s)))
@pytest.mark.parametrize("alg", [2, 1], ids=["nips19_dp", "advanced_dp"])
def test_drop_takes_n_survivors_in_threshold_and_noise(oracle, enclave, switches, alg, dropped):
    """the seed set before each call: nips19's Laplace counts and shuffle, then the DP noise,
    are the same draws in both calls, so equal bits mean n' in nips19_threshold(d, k, n') and
    in the noise's divisor"""
    idx, val = records(N, D, K, 31 + alg)
    keep, sidx, sval = survivors(idx, val, K, dropped)
    fl = 8900 + 10 * alg + len(dropped)
    switches.set_upload_aead_policy("drop")
    start(enclave, fl, IDS, D, K, alg, dp=1)
    enc = tamper(auth_payload(oracle, idx, val, IDS, fl, 0, alg), K, dropped)
    switches.set_debug_seed(0xC0FFEE)
    st, rv, out, _ = call(enclave, fl, 0, IDS, enc, D, K, alg)
    assert (st, rv) == (0, 0)
    assert enclave.auth_report(fl) == (0, [int(IDS[c]) for c in dropped])
    # the survivors alone, clean, under a fresh fl_id
    sids = IDS[keep]
    start(enclave, fl + 5, sids, D, K, alg, dp=1)
    clean = auth_payload(oracle, sidx, sval, sids, fl + 5, 0, alg)
    switches.set_debug_seed(0xC0FFEE)
    st, rv, ref, _ = call(enclave, fl + 5, 0, sids, clean, D, K, alg)
    assert (st, rv) == (0, 0)
    assert bits_equal(out, ref)
    # (and the noise is there: the un-noised aggregate differs)
    if alg == 1:
        assert not bits_equal(out, oracle_aggregate(oracle, alg, sids, sidx, sval, D, K, fl))


@pytest.mark.parametrize("alg", [1, 6, 3])
@pytest.mark.parametrize("dropped,min_survivors", [(tuple(range(8)), 1), (tuple(range(7)), 2)],
                         ids=["all_eight", "one_left_of_two"])
def test_drop_below_the_quorum_ends_as_a_mac_mismatch(oracle, enclave, switches, alg, dropped, min_survivors):
    idx, val = records(N, D, K, 50 + alg)
    fl = 9000 + alg + 10 * min_survivors
    switches.set_upload_aead_policy("drop", min_survivors)
    good = auth_payload(oracle, idx, val, IDS, fl, 0, alg)
    start(enclave, fl, IDS, D, K, alg)
    st, rv, out, times = call(enclave, fl, 0, IDS, tamper(good, K, dropped), D, K, alg)
    assert (st, rv) == (0, MAC_MISMATCH)
    assert not out.view(np.uint32).any()
    assert np.isfinite(times).all() and times[0] > 0  # the timers are written
    assert enclave.auth_report(fl) == (0, [int(IDS[c]) for c in dropped])
    # the round is kept: the good upload is answered for round 0
    st, rv, out, _ = call(enclave, fl, 0, IDS, good, D, K, alg)
    assert (st, rv) == (0, 0)
    assert bits_equal(out, oracle_aggregate(oracle, alg, IDS, idx, val, D, K, fl))
    assert enclave.auth_report(fl) == (0, [])


@pytest.mark.parametrize("alg", [1, 6, 3])
def test_report_aborts_and_names_the_failed_clients(oracle, enclave, switches, alg):
    idx, val = records(N, D, K, 60 + alg)
    fl = 9100 + alg
    switches.set_upload_aead_policy("report")
    good = auth_payload(oracle, idx, val, IDS, fl, 0, alg)
    start(enclave, fl, IDS, D, K, alg)
    assert enclave.auth_report(fl) == (0, [])  # nothing stored yet
    st, rv, out, times = call(enclave, fl, 0, IDS, tamper(good, K, (2, 5)), D, K, alg)
    assert (st, rv) == (0, MAC_MISMATCH)
    assert not out.view(np.uint32).any() and np.isfinite(times).all()
    assert enclave.auth_report(fl) == (0, [int(IDS[2]), int(IDS[5])])
    # cap smaller than the list: the full count, the first id
    import ctypes
    rnd, nf, one = ctypes.c_uint32(9), ctypes.c_size_t(0), (ctypes.c_uint32 * 1)()
    assert enclave.lib.fltee_auth_report(enclave.eid, fl, ctypes.byref(rnd), one, 1, ctypes.byref(nf)) == 0
    assert (rnd.value, nf.value, one[0]) == (0, 2, int(IDS[2]))
    # the round is kept; the clean call is answered and stores an empty report
    st, rv, out, _ = call(enclave, fl, 0, IDS, good, D, K, alg)
    assert (st, rv) == (0, 0)
    assert bits_equal(out, oracle_aggregate(oracle, alg, IDS, idx, val, D, K, fl))
    assert enclave.auth_report(fl) == (0, [])


@pytest.mark.parametrize("alg", [1, 6])
def test_abort_is_the_default_and_stores_nothing(oracle, enclave, switches, alg):
    idx, val = records(N, D, K, 70 + alg)
    fl = 9200 + alg
    good = auth_payload(oracle, idx, val, IDS, fl, 0, alg)
    start(enclave, fl, IDS, D, K, alg)
    st, rv, out, _ = call(enclave, fl, 0, IDS, tamper(good, K, (2, 5)), D, K, alg)
    assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
    assert enclave.auth_report(fl) == (0, [])
    st, rv, out, _ = call(enclave, fl, 0, IDS, good, D, K, alg)
    assert (st, rv) == (0, 0)
    # the switch has no effect while AEAD is off: a CTR call under "drop" is the CTR call
    switches.set_upload_aead(False)
    switches.set_upload_aead_policy("drop")
    start(enclave, fl, IDS, D, K, alg)
    st, rv, out2, _ = call(enclave, fl, 0, IDS, ctr_payload(oracle, idx, val, IDS, K), D, K, alg)
    assert (st, rv) == (0, 0) and bits_equal(out, out2)
    assert enclave.auth_report(fl) == (1, [])  # nothing stored: the config's current round


def test_auth_report_of_an_unknown_fl_id(enclave):
    with pytest.raises(RuntimeError, match="0x1"):
        enclave.auth_report(0xDEAD0002)


# ---- the launch trace (the hook of tests/test_gpu_gcm_trace.py) --------------------------
READBACK_ABORT = "memcpy||4|2|0"               # the word gathering the failures
READBACK_KEPT = f"memcpy||{(N + 1) * 4}|2|0"   # the n fail words and that word: n alone


def split_at_readback(lines, readback):
    """(the lines through the verdict readback and its synchronisation, the lines after)"""
    last = max(i for i, line in enumerate(lines) if "ghash_finish_kernel" in line)
    i = lines.index(readback, last)
    assert lines[i + 1].startswith("sync|stream"), lines[i + 1]
    return lines[:i + 2], lines[i + 2:]


def trace_payloads(oracle, alg, fl):
    """random and all-one-index uploads of one shape, and each with clients 2 and 5 tampered"""
    encs = []
    for i, kind in enumerate(("random", "one_index")):
        idx, val = uploads(np.random.default_rng(80 + i), N, D, K, kind)
        encs.append(auth_payload(oracle, idx, val, IDS, fl, 0, alg))
    return encs, [tamper(e, K, (2, 5)) for e in encs]


@pytest.mark.parametrize("alg", [1, 6])
def test_drop_trace_depends_on_sizes_and_the_failed_set_only(oracle, switches, alg):
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    fl = 9300 + alg
    (rnd, one), (t_rnd, t_one) = trace_payloads(oracle, alg, fl)
    E = Enclave(0)

    def run(enc):
        start(E, fl, IDS, D, K, alg)
        st, rv, _, _ = call(E, fl, 0, IDS, enc, D, K, alg)
        assert (st, rv) == (0, 0)

    try:
        run(rnd)  # the shape's scratch
        tr_abort = traced(lambda: run(rnd))
        switches.set_upload_aead_policy("drop")
        run(rnd)
        run(t_rnd)  # ... and the survivors' buffer
        tr = {name: traced(lambda e=e: run(e))
              for name, e in (("random", rnd), ("one_index", one), ("t_random", t_rnd), ("t_one_index", t_one))}
        assert E.auth_report(fl) == (0, [int(IDS[2]), int(IDS[5])])
    finally:
        E.destroy()
    head, tail = split_at_readback(tr["random"], READBACK_KEPT)
    assert any("ghash_bulk_kernel" in line for line in head)
    # up to and including the readback: the public sizes alone
    assert_same_trace(tr["random"], tr["one_index"], f"DROP alg {alg}: clean, one_index")
    for name in ("t_random", "t_one_index"):
        assert_same_trace(head, split_at_readback(tr[name], READBACK_KEPT)[0], f"DROP alg {alg}: {name} head")
    # after it: the sizes and the failed set
    t_tail = split_at_readback(tr["t_random"], READBACK_KEPT)[1]
    assert any("gather_clients_kernel" in line for line in t_tail)
    assert_same_trace(t_tail, split_at_readback(tr["t_one_index"], READBACK_KEPT)[1],
                      f"DROP alg {alg}: the same failed set, other data")
    assert not any("gather_clients_kernel" in line for line in tr["random"])
    # a clean DROP call is the clean ABORT call, but for the bytes of that one readback
    a_head, a_tail = split_at_readback(tr_abort, READBACK_ABORT)
    assert_same_trace(a_head[:-2] + [READBACK_KEPT] + a_head[-1:], head, f"DROP alg {alg}: clean head vs ABORT")
    assert_same_trace(a_tail, tail, f"DROP alg {alg}: clean tail vs ABORT")


@pytest.mark.parametrize("variant", [("1", 1, K), ("3d", 3, D), ("6", 6, K)], ids=lambda v: "alg_" + v[0])
def test_clean_drop_call_runs_the_group_paths_as_abort_does(oracle, switches, variant):
    """two virtual ranks: a clean call under DROP takes the group path it takes under ABORT
    (the ranks' verdict words are read as before: the trace is the same line for line)"""
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    name, alg, k = variant
    fl = 9400 + alg + (k == D)
    idx, val = records(N, D, k, 90 + alg)
    enc = auth_payload(oracle, idx, val, IDS, fl, 0, alg)
    E = Enclave([0, 0])

    def run():
        start(E, fl, IDS, D, k, alg)
        st, rv, out, _ = call(E, fl, 0, IDS, enc, D, k, alg)
        assert (st, rv) == (0, 0)
        return out

    try:
        run()
        tr_abort = traced(run)
        switches.set_upload_aead_policy("drop")
        run()
        tr_drop = traced(run)
    finally:
        E.destroy()
    norm = [READBACK_ABORT if line == READBACK_KEPT else line for line in tr_drop]
    assert_same_trace(tr_abort, norm, f"two ranks, alg {name}: clean DROP vs ABORT")


def test_server_keeps_and_logs_the_failed_clients(oracle, switches, capsys):
    """fltee.server.Aggregator(aead_policy="drop"): the round is answered from the verified
    clients, the failed ids are kept in last_failed_clients and logged; "report": the MAC
    mismatch is a ServerPanic and the ids are kept all the same"""
    import torch

    from fltee.ecalls import Enclave
    from fltee.server import Aggregator, ServerPanic
    torch.cuda.init()
    idx, val = records(N, D, K, 97)
    fl, alg = 9500, 1
    keep, sidx, sval = survivors(idx, val, K, (2, 5))
    want = oracle_aggregate(oracle, alg, IDS[keep], sidx, sval, D, K, fl)
    bad = tamper(auth_payload(oracle, idx, val, IDS, fl, 0, alg), K, (2, 5))
    E = Enclave(0)
    try:
        A = Aggregator(enclave=E, aead=True, aead_policy="drop")
        assert A.start(fl, IDS, 1.12, 1.0, 0.1, 1.0, alg, D, K)["round"] == 0
        r = A.aggregate(fl, 0, bad, D, K, 3, alg, IDS)
        assert r["round"] == 1 and bits_equal(r["updated_parameters"], want)
        assert A.last_failed_clients == [int(IDS[2]), int(IDS[5])]
        assert "failed authentication" in capsys.readouterr().out
        r = A.aggregate(fl, 1, auth_payload(oracle, idx, val, IDS, fl, 1, alg), D, K, 3, alg, IDS)
        assert r["round"] == 2 and A.last_failed_clients == []
        A = Aggregator(enclave=E, aead=True, aead_policy="report")
        A.start(fl, IDS, 1.12, 1.0, 0.1, 1.0, alg, D, K)
        with pytest.raises(ServerPanic, match="MAC mismatch"):
            A.aggregate(fl, 0, bad, D, K, 3, alg, IDS)
        assert A.last_failed_clients == [int(IDS[2]), int(IDS[5])]
    finally:
        E.destroy()
