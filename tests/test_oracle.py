"""Pin the CPU oracle (oracle/) before trusting it as the checker.

Pins available for this path:
  * the reference's own AES library (src/cpp/encryption.cpp -> oracle/_ref/),
    its src/ffi_test.py round trip, and payloads produced by the reference
    Python client (tests/golden/, made by tests/golden/make_fixtures.py);
  * the reference bench checksum (benchmark.rs:226-239) and the cross-algorithm
    identities of SURVEY §4;
  * pure-Python transcriptions of advanced.rs / common.rs for tiny inputs.
The Rust enclave itself cannot run here: aggregation arithmetic beyond these
pins is "parity unpinned" (DESIGN.md §Oracle).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

U32MAX = 0xFFFFFFFF


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def rand_sparse(rng, n, d, k, scale=0.01):
    idx = np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)
    val = rng.normal(0, scale, n * k).astype(np.float32)
    return idx, val


# ------------------------------------------------------------------ RNG ----
def test_philox_known_answers(oracle):
    # Random123 kat_vectors for philox4x32-10
    assert list(oracle.philox([0, 0, 0, 0], [0, 0])) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert list(oracle.philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == [
        0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert list(oracle.philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344],
                              [0xA4093822, 0x299F31D0])) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


# --------------------------------------------------------------- crypto ----
def test_session_key_layout(oracle):
    # session_key_store.rs:21-22: bytes[4..8] = client_id big-endian
    assert list(oracle.session_key(0x01020304)) == [0, 0, 0, 0, 1, 2, 3, 4] + [0] * 8
    # utils.py:276-278 writes 2-byte BE into [6..8]: identical for id < 65536
    assert list(oracle.session_key(513)) == [0] * 6 + [2, 1] + [0] * 8


def test_ffi_test_known_answer(oracle):
    kat = load("ffi_test_kat")
    ct = oracle.aes128_ctr(bytes(16), kat["plaintext"].tobytes())
    assert ct == kat["ciphertext"].tobytes()
    assert oracle.aes128_ctr(bytes(16), ct) == kat["plaintext"].tobytes()  # src/ffi_test.py round trip


def test_fips197_block(oracle):
    # FIPS-197 C.1: the CTR keystream block 0 under key k is AES_k(0^16)
    key = bytes(range(16))
    pt = bytes.fromhex("00112233445566778899aabbccddeeff")
    # AES-CTR with IV=0 encrypting 16 zero bytes yields AES_k(0); check via the KAT of
    # AES_k(pt): encrypt pt as counter is not expressible, so compare with reference lib
    ks = oracle.aes128_ctr(key, bytes(16))
    assert len(ks) == 16 and ks != bytes(16)
    if oracle.ref_aes_available():
        assert ks == oracle.ref_aes_ctr_encrypt(key, bytes(16))
    assert pt  # (block KAT for the device tables lives in test_abi.py)


def test_aes_matches_reference_library(oracle):
    # tests/golden/aes_ref_ctr.npz: the reference library's own ciphertexts of these
    # inputs (make_fixtures.py aes_reference_fixtures), so the pin holds where oracle/_ref
    # is not built; where it is, the library itself is asked as well
    fx = load("aes_ref_ctr")
    cases = [(0, 1), (5, 15), (17, 16), (99, 1000), (65535, 4097), (70000, 8 * 5089)]
    assert [(int(c), int(ln)) for c, ln in zip(fx["client_ids"], fx["lengths"])] == cases
    off = 0
    for cid, ln in cases:
        data = fx["plaintext"][off:off + ln].tobytes()  # default_rng(7) bytes, as before
        assert len(data) == ln
        key = oracle.session_key(cid)
        ct = oracle.aes128_ctr(key, data)
        assert ct == fx["ciphertext"][off:off + ln].tobytes()
        if oracle.ref_aes_available():
            assert ct == oracle.ref_aes_ctr_encrypt(key, data)
        off += ln


@pytest.mark.parametrize("name", ["mnist_sparse", "mnist_sparse_clip"])
def test_reference_client_payloads_decrypt(oracle, name):
    fx = load(name)
    ids, d, k = fx["client_ids"], int(fx["d"]), int(fx["k"])
    w = oracle.decrypt_and_parse(ids, fx["ciphertext"].tobytes())
    assert w.tobytes() == fx["plaintext"].tobytes()          # serialize_sparse bytes
    assert len(w) == len(ids) * k
    # upload order = top-k order (|v| descending, utils.py:346-353)
    for c in range(len(ids)):
        cw = w[c * k:(c + 1) * k]
        assert np.array_equal(cw["idx"], fx["topk"][c])
        assert np.all(np.diff(np.abs(cw["val"])) <= 0)
        assert len(np.unique(cw["idx"])) == k and cw["idx"].max() < d


def test_reference_dense_payload(oracle):
    fx = load("dense_small")
    ids, d = fx["client_ids"], int(fx["d"])
    w = oracle.decrypt_and_parse(ids, fx["ciphertext"].tobytes())
    assert w.tobytes() == fx["plaintext"].tobytes()
    assert np.array_equal(w["idx"], np.tile(np.arange(d, dtype=np.uint32), len(ids)))
    g = oracle.baseline(w, d, len(ids))
    assert np.array_equal(g, fx["oracle_baseline"])


@pytest.mark.parametrize("name", ["mnist_sparse", "mnist_sparse_clip"])
def test_oracle_regression_on_golden(oracle, name):
    fx = load(name)
    ids, d, k = fx["client_ids"], int(fx["d"]), int(fx["k"])
    w = oracle.decrypt_and_parse(ids, fx["ciphertext"].tobytes())
    g_non, st = oracle.non_oblivious(w, d, len(ids))
    assert st == 0 and np.array_equal(g_non, fx["oracle_non_oblivious"])
    g_adv, st = oracle.advanced(k, w, d, len(ids))
    assert st == 0 and np.array_equal(g_adv, fx["oracle_advanced"])


# ---------------------------------------------------------- invariants ----
def inorder_sum(idx, val, d, n):
    g = np.zeros(d, dtype=np.float32)
    for i, v in zip(idx.tolist(), val.tolist()):
        g[i] = np.float32(g[i] + np.float32(v))
    return g * np.float32(np.float32(1.0) / np.float32(n))


def test_flat_algorithms_identical(oracle):
    rng = np.random.default_rng(1)
    n, d, k = 6, 777, 50
    idx, val = rand_sparse(rng, n, d, k)
    w = oracle.as_weights(idx, val)
    g_non, st = oracle.non_oblivious(w, d, n)
    assert st == 0
    assert np.array_equal(g_non, inorder_sum(idx, val, d, n))
    assert np.array_equal(oracle.baseline(w, d, n), g_non)
    g_oram, st = oracle.path_oram(w, d, n)
    assert st == 0 and np.array_equal(g_oram, g_non)


def test_oblivious_algorithms_close(oracle):
    rng = np.random.default_rng(2)
    n, d, k = 9, 1500, 120
    idx, val = rand_sparse(rng, n, d, k)
    w = oracle.as_weights(idx, val)
    ref, _ = oracle.non_oblivious(w, d, n)
    tol = 1e-6 * np.abs(val).max() * (n + 1)
    g, st = oracle.advanced(k, w, d, n)
    assert st == 0 and np.abs(g - ref).max() <= tol
    g, st = oracle.nips19(k, w, d, n, seed=11)
    assert st == 0 and np.abs(g - ref).max() <= tol
    g, st = oracle.client_size_optimized(4, k, w, d, n)
    assert st == 0 and np.abs(g - ref).max() <= tol


def test_bench_checksum_invariant(oracle):
    # benchmark.rs:286-297 data (k distinct idx per client, val = idx * 0.001) and the
    # printed check `sum(aggregate) == sum(raw) / n` (benchmark.rs:226-239)
    rng = np.random.default_rng(13)
    n, d, k = 10, 10000, 1000
    idx = np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)
    val = (idx.astype(np.float32) * np.float32(0.001)).astype(np.float32)
    w = oracle.as_weights(idx, val)
    raw = float(np.sum(val, dtype=np.float64)) / n
    for g in (oracle.non_oblivious(w, d, n)[0], oracle.baseline(w, d, n),
              oracle.advanced(k, w, d, n)[0], oracle.path_oram(w, d, n)[0]):
        assert abs(float(np.sum(g, dtype=np.float64)) - raw) <= 1e-5 * raw


def test_errors_mirror_panics(oracle):
    w = oracle.as_weights(np.array([0, 5], np.uint32), np.array([1, 2], np.float32))
    assert oracle.non_oblivious(w, 5, 1)[1] == oracle.ENCLAVE_CRASHED   # g[5] out of bounds
    assert oracle.path_oram(w, 5, 1)[1] == 0                             # block 5 < next_pow2(5)
    w2 = oracle.as_weights(np.array([9], np.uint32), np.array([1], np.float32))
    assert oracle.path_oram(w2, 5, 1)[1] == oracle.ENCLAVE_CRASHED
    g = oracle.baseline(w2, 5, 1)                                        # baseline ignores it
    assert not g.any()


# -------------------------------------------- pure-Python transcriptions ----
def py_bitonic(keys_vals):
    s = list(keys_vals)
    size = len(s)
    i = 2
    while i <= size:
        j = i >> 1
        while j > 0:
            for k in range(size >> 1):
                l = ((k & ~(j - 1)) << 1) | (k & (j - 1))
                m = l + j
                if ((l & i) == 0) ^ (s[l][0] < s[m][0]):
                    s[l], s[m] = s[m], s[l]
            j >>= 1
        i <<= 1
    return s


def test_bitonic_network_matches_transcription(oracle):
    rng = np.random.default_rng(3)
    for size in (2, 4, 16, 64, 256):
        idx = rng.integers(0, max(2, size // 4), size).astype(np.uint32)   # many equal keys
        val = np.arange(size, dtype=np.float32)                               # track identity
        got = oracle.bitonic_sort(oracle.as_weights(idx, val))
        exp = py_bitonic(list(zip(idx.tolist(), val.tolist())))
        assert got["idx"].tolist() == [e[0] for e in exp]
        assert got["val"].tolist() == [e[1] for e in exp]
        assert np.all(np.diff(got["idx"].astype(np.int64)) >= 0)


def py_fold(s, fold_len):
    s = [list(x) for x in s]
    pre_idx, pre_val = s[0]
    dummy = U32MAX
    for i in range(1, fold_len):
        eq = pre_idx == s[i][0]
        s[i - 1] = [dummy, 0.0] if eq else [pre_idx, pre_val]
        if eq:
            pre_val = float(np.float32(np.float32(pre_val) + np.float32(s[i][1])))
        else:
            pre_idx, pre_val = s[i]
        dummy -= 1
    s[fold_len - 1] = [pre_idx, pre_val]
    return s


def test_fold_matches_transcription(oracle):
    rng = np.random.default_rng(4)
    idx = np.sort(rng.integers(0, 20, 64)).astype(np.uint32)
    val = rng.normal(0, 1, 64).astype(np.float32)
    for fold_len in (64, 40, 1):
        got = oracle.fold(oracle.as_weights(idx, val), fold_len)
        exp = py_fold(list(zip(idx.tolist(), val.tolist())), fold_len)
        assert got["idx"].tolist() == [e[0] for e in exp]
        assert got["val"].tolist() == [float(np.float32(e[1])) for e in exp]


def test_advanced_dense_k0_quirk(oracle):
    # fl_main.py:100-103 sends k = 0 without --alpha; advanced.rs:70 then folds only d
    # entries.  The oracle must reproduce the (wrong) reference output, not fix it.
    rng = np.random.default_rng(5)
    n, d = 3, 8
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    val = rng.normal(0, 1, n * d).astype(np.float32)
    g0, st = oracle.advanced(0, oracle.as_weights(idx, val), d, n)
    assert st == 0
    s = list(zip(idx.tolist(), val.tolist())) + [(i, 0.0) for i in range(d)]
    L = len(s)
    M = 1 << (L - 1).bit_length()
    s = py_bitonic(s + [(U32MAX, 0.0)] * (M - L))[:L]
    s = py_fold(s, d)
    s = py_bitonic([tuple(x) for x in s] + [(U32MAX, 0.0)] * (M - L))[:L]
    exp = np.array([x[1] for x in s[:d]], np.float32) * np.float32(1.0 / np.float32(n))
    assert np.array_equal(g0, exp)
    g_ok, _ = oracle.advanced(d, oracle.as_weights(idx, val), d, n)
    assert not np.array_equal(g0, g_ok)


def test_nips19_pad_and_threshold(oracle):
    d, k, n = 44964, 4496, 300                               # C4 shape
    T = oracle.nips19_threshold(d, k, n)
    assert int(T) == 1476                                    # floor(T) = 1476
    r, T2 = oracle.laplace_r(200, 50, 30, seed=9)
    assert T2 == oracle.nips19_threshold(200, 50, 30)
    pad = oracle.oblivious_pad(r, 200, T2)
    tf = int(T2)
    assert len(pad) == 200 * tf
    for i in (0, 57, 199):
        ent = pad[i * tf:(i + 1) * tf]["idx"]
        exp = [i if r[i] < j else U32MAX for j in range(tf)]  # common.rs:189-197
        assert ent.tolist() == exp
    assert not pad["val"].any()


def test_shuffles_are_permutations(oracle):
    rng = np.random.default_rng(6)
    idx = rng.integers(0, 1000, 1024).astype(np.uint32)
    val = np.arange(1024, dtype=np.float32)
    for s in (oracle.shuffle_keyed(oracle.as_weights(idx, val), 123),
              oracle.shuffle_fxhash(oracle.as_weights(idx, val))):
        assert sorted(s["val"].tolist()) == val.tolist()
        assert not np.array_equal(s["val"], val)
        order = s["val"].astype(np.int64)
        assert np.array_equal(s["idx"], idx[order])


def test_l2clip_matches_reference_torch(oracle):
    fx = load("l2clip")
    got = oracle.l2_clip(fx["flat_in"], float(fx["clipping"]))
    # torch.norm reduces in fp32 (its norm is 2 ulp off the exact one here); the
    # oracle accumulates in f64: north-star tolerance 1e-6 relative.
    assert np.allclose(got, fx["flat_out"], rtol=1e-6, atol=0)


def test_sampling_reservoir(oracle):
    ids = np.arange(100, 200, dtype=np.uint32)
    assert np.array_equal(oracle.sample_client_ids(ids, 100, seed=1), ids)  # amount == m: all, in order
    s = oracle.sample_client_ids(ids, 30, seed=2)
    assert len(set(s.tolist())) == 30 and set(s.tolist()) <= set(ids.tolist())
    assert not np.array_equal(s, oracle.sample_client_ids(ids, 30, seed=3))


# --------------------------------------------------- ECALL state machine ----
def test_oracle_ecall_state_machine(oracle):
    fx = load("mnist_sparse")
    ids, d, k = fx["client_ids"], int(fx["d"]), int(fx["k"])
    E = oracle.OracleEnclave(seed=42)
    assert E.fl_init(0, ids, d, k, 1.12, 1.0, 0.1, 1.0, 4) == 0
    assert E.start_round(0, 1, len(ids))[0] == oracle.INVALID_PARAMETER   # wrong round
    assert E.start_round(0, 0, 3)[0] == oracle.INVALID_PARAMETER          # wrong sample size
    assert E.start_round(7, 0, len(ids))[0] == oracle.UNEXPECTED          # unknown fl_id
    st, sampled = E.start_round(0, 0, len(ids))
    assert st == 0 and np.array_equal(np.sort(sampled), np.sort(ids))
    enc = fx["ciphertext"].tobytes()
    assert E.secure_aggregation(0, 0, ids, enc, d, k, 1)[0] == oracle.INVALID_PARAMETER  # alg
    assert E.secure_aggregation(0, 1, ids, enc, d, k, 4)[0] == oracle.INVALID_PARAMETER  # round
    assert E.secure_aggregation(0, 0, ids[:3], enc, d, k, 4)[0] == oracle.INVALID_PARAMETER
    st, out, times = E.secure_aggregation(0, 0, ids, enc, d, k, 4)
    assert st == 0 and np.array_equal(out, fx["oracle_non_oblivious"])
    assert (times >= 0).all()
    assert E.secure_aggregation(0, 0, ids, enc, d, k, 4)[0] == oracle.INVALID_PARAMETER  # round++


def test_numpy_axis0_sum_is_in_order(oracle):
    # test_gpu_parity's full-size check uses np.sum(axis=0) as the in-order reference
    rng = np.random.default_rng(8)
    n, d = 37, 513
    v = (rng.normal(0, 1, (n, d)) * 10.0 ** rng.integers(-3, 4, (n, d))).astype(np.float32)
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    ref, _ = oracle.non_oblivious(oracle.as_weights(idx, v.reshape(-1)), d, n)
    got = np.sum(v, axis=0, dtype=np.float32) * np.float32(np.float32(1) / np.float32(n))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_dp_noise_distribution_matches_reference(oracle):
    # update.py:207-224 with zero diffs (numpy RandomState(seed+5), fl_main.py:49) vs the
    # restated common.rs:56-72 mechanism: same N(0, C*sigma)/n law (two-sample KS)
    from scipy import stats
    fx = load("dp_reference")
    ref = fx["noise"]
    n, sigma, clipping = int(fx["n"]), float(fx["sigma"]), float(fx["clipping"])
    got = oracle.dp_noise(np.zeros(ref.size, np.float32), sigma, clipping, n, seed=123)
    assert stats.ks_2samp(got, ref).pvalue > 1e-3
    assert abs(got.std() / ref.std() - 1) < 0.02
