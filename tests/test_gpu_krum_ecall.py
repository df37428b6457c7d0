"""fltee_set_dense_krum through ecall_secure_aggregation on the GPU: the staged and the pipelined
path, CTR and GCM, records and packed slices, against tests/krum_model.py bit for bit (the values
are small integers beside the hostile clients': every Gram entry is exact); DROP on the n'
survivors; every 0x2 refusal with the round kept; a two-virtual-rank eid; the switch-off trace;
and a launch trace that does not depend on the values."""
import functools

import numpy as np
import pytest

import krum_model as KM
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced
from test_gpu_trim_ecall import LARGE, ids_of, payload, same_bits, start

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D, F, M = 10, 1101, 2, 5
SEED = 0xC0FFEE5EED


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    rng = np.random.default_rng(seed + d)
    v = rng.integers(-8, 9, (n, d)).astype(np.float32)
    if n >= 7:
        v[1] += np.float32(1e6)              # a hostile client, inside no honest client's reach
        v[3, 3::11] = np.nan                 # and one that seals NaNs
    v.setflags(write=False)
    return v


@pytest.fixture
def switches():
    from fltee import ecalls as EC
    EC.set_bubble_ecall(True)
    EC.set_upload_packed(True)
    try:
        yield EC
    finally:
        EC.set_dense_krum(0, 0)
        EC.set_dense_trim(0)
        EC.set_upload_packed(False)
        EC.set_bubble_ecall(False)
        EC.set_upload_aead_policy("abort")
        EC.set_upload_aead(False)
        EC.set_path_oram_tree(False)
        EC.set_debug_seed(0)


@pytest.fixture(scope="module")
def enclave():
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    E = Enclave(0)
    yield E
    E.destroy()


def fresh_call(EC, E, fl, ids, enc, d, k, alg):
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, k, alg)
    return E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)


def plain_mean(v):
    return KM.krum(v, 0, v.shape[0], keep=np.ones(v.shape[0], bool))


# ------------------------------------------------------------------ the result ----
@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
@pytest.mark.parametrize("alg", [3, 4, 5])
def test_krum_ecall_equals_the_model(enclave, switches, alg, packed, aead):
    n, d = N, D
    v, ids, fl = host_values(n, d), ids_of(n), 9800 + alg
    switches.set_upload_aead(aead)
    switches.set_dense_krum(F, M)
    enc = payload(v, ids, packed, (fl, 0, alg) if aead else None)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    s, keep = KM.select(v, F, M)
    assert not keep[1] and not keep[3] and keep.sum() == M
    want = KM.krum(v, F, M)
    assert same_bits(out, want)
    assert np.isfinite(out).all() and np.abs(out).max() <= 8  # the 1e6 and the NaNs are gone
    # the round advanced
    st, rv, again, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()
    # switched off, the same upload is the plain mean it always was
    switches.set_dense_krum(0, 0)
    st, rv, off, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(off, plain_mean(v)) and not same_bits(off, want)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_pipelined_path_is_scored(enclave, switches, packed):
    n, d = 7, LARGE[1]  # 7 packed slices of 4,194,312 bytes > 16 MiB
    v, ids, fl = host_values(n, d, 1), ids_of(n), 9820
    switches.set_dense_krum(2, 3)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert same_bits(out, KM.krum(v, 2, 3))


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_drop_scores_the_survivors(enclave, switches, packed):
    n, d, alg, fl, failed = N, D, 3, 9840, [6]
    v, ids = host_values(n, d), ids_of(n)
    keep = [c for c in range(n) if c not in failed]
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    switches.set_dense_krum(F, 7)  # m = n' - f: possible for the 9 survivors
    enc = payload(v, ids, packed, (fl, 0, alg)).copy()
    stride = enc.nbytes // n
    for c in failed:
        enc[c * stride + 8 * c + 5] ^= 1
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    assert enclave.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    assert same_bits(out, KM.krum(v[keep], F, 7))  # n' = 9 in the selection, the divisor m = 7


def test_dp_noise_is_divided_by_m(enclave, switches):
    """the same debug seed: the DP call is the plain Krum call plus the noise of divisor m"""
    n, d, fl = N, D, 9845
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, False)
    switches.set_dense_krum(F, M)
    switches.set_debug_seed(SEED)
    assert enclave.ecall_fl_init(fl, ids, d, d, 1.12, 1.0, 0.1, 1.0, 3, 0, 1) == (0, 0)
    assert enclave.ecall_start_round(fl, 0, n)[:2] == (0, 0)
    st, rv, out, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0)
    base = KM.krum(v, F, M)
    noise = out.astype(np.float64) - base
    # N(0, clipping * sigma) / m per output: the spread says which divisor was used
    assert abs(noise.std() * M / 1.12 - 1) < 0.15 and abs(noise.mean()) < 0.05


# ------------------------------------------------------------------- refusals ----
def refused_then_kept(EC, E, fl, ids, enc, d, k, alg, f=1, m=2, trim=0):
    """the call ends with 0x2 and a zero [out] under the switch, and the round was kept: with
    the switch off the same request is answered"""
    EC.set_dense_krum(f, m)
    EC.set_dense_trim(trim)
    st, rv, out, times = fresh_call(EC, E, fl, ids, enc, d, k, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    EC.set_dense_krum(0, 0)
    EC.set_dense_trim(0)
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)
    assert (st, rv) == (0, 0)


@pytest.mark.parametrize("alg", [1, 2, 7])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_sort_based_algs_are_refused(enclave, switches, alg, packed):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    refused_then_kept(switches, enclave, 9850 + alg, ids, payload(v, ids, packed), d, d, alg)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_sparse_uploads_are_refused(enclave, switches, alg):
    import torch

    from fltee import client as C
    n, d, k = 5, 258, 64
    v, ids = host_values(n, d, 2), ids_of(n)
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    refused_then_kept(switches, enclave, 9860 + alg, ids, enc, d, k, alg)


def test_the_tree_the_counts_the_cap_and_the_trim_are_refused(enclave, switches):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    enc = payload(v, ids, False)
    switches.set_path_oram_tree(True)
    refused_then_kept(switches, enclave, 9870, ids, enc, d, d, 5)
    switches.set_path_oram_tree(False)
    refused_then_kept(switches, enclave, 9871, ids, enc, d, d, 3, f=2, m=1)   # n < 2 f + 3
    refused_then_kept(switches, enclave, 9872, ids, enc, d, d, 3, f=1, m=5)   # m > n - f
    refused_then_kept(switches, enclave, 9873, ids, enc, d, d, 3, f=1, m=0)   # m = 0
    refused_then_kept(switches, enclave, 9874, ids, enc, d, d, 3, trim=100)   # both robust switches on
    # and the same request is answered once it can be
    switches.set_dense_krum(1, 4)
    st, rv, out, _ = fresh_call(switches, enclave, 9875, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, KM.krum(v, 1, 4))
    n, d = 1025, 4  # past FLTEE_KRUM_MAX_N; 1024 clients are answered
    v, ids = host_values(n, d, 3), ids_of(n, 2000)
    refused_then_kept(switches, enclave, 9876, ids, payload(v, ids, False), d, d, 3, f=1, m=2)
    switches.set_dense_krum(100, 500)
    st, rv, out, _ = fresh_call(switches, enclave, 9877, ids[:1024], payload(v[:1024], ids[:1024], False), d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, KM.krum(v[:1024], 100, 500))


def test_too_few_survivors_are_refused(enclave, switches):
    """n = 8 answers f = 2 (2 f + 3 = 7); with two failed clients n' = 6 does not"""
    n, d, alg, fl = 8, 258, 3, 9880
    v, ids = host_values(n, d, 5), ids_of(n)
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    switches.set_dense_krum(2, 2)
    enc = payload(v, ids, False, (fl, 0, alg)).copy()
    stride = enc.nbytes // n
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(out, KM.krum(v, 2, 2))
    for c in (0, 5):
        enc[c * stride + 8 * c + 5] ^= 1
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    # m > n' - f likewise: 7 survivors, f = 2, m = 6
    switches.set_dense_krum(2, 6)
    enc = payload(v, ids, False, (fl, 0, alg)).copy()
    enc[5] ^= 1
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any()


def test_alg_6_is_refused(enclave, switches):
    import torch

    from fltee import client as C
    n, d, k = 6, 258, 32
    v, ids, fl = host_values(n, d, 2), ids_of(n), 9885
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    switches.set_dense_krum(1, 2)
    start(enclave, fl, ids, d, k, 6)
    st, rv, out, times = enclave.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, ids, enc, d, k, 6)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    switches.set_dense_krum(0, 0)
    st, rv, out, _ = enclave.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, ids, enc, d, k, 6)
    assert (st, rv) == (0, 0)


def test_records_out_of_position_are_refused(enclave, switches):
    """a dense-sized upload whose records are not in position reruns sparse without the switch;
    under it the call ends with 0x2 after the one status readback"""
    import torch

    from fltee import client as C
    n, d = 5, 258
    v, ids = host_values(n, d, 4), ids_of(n)
    rec = C.serialize_dense(torch.from_numpy(np.array(v, np.float32)).cuda()).reshape(n, d).clone()
    rec[2, [0, 1]] = rec[2, [1, 0]]  # client 2's first two records swapped
    enc = C.encrypt_parameters(rec.reshape(-1), ids).cpu().numpy()
    switches.set_dense_krum(1, 2)
    tr = traced(lambda: fresh_call(switches, enclave, 9890, ids, enc, d, d, 4))
    assert sum("krum_gram_kernel" in line and line.startswith("launch") for line in tr) == 1  # once: no rerun
    assert not any("scatter" in line or "fold_sorted" in line for line in tr)
    refused_then_kept(switches, enclave, 9890, ids, enc, d, d, 4)


# ---------------------------------------------------------------------- traces ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_off_trace_and_bits_are_the_untouched_ones(enclave, switches, packed):
    n, d, fl = N, D, 9900
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    fresh_call(switches, enclave, fl, ids, enc, d, d, 3)  # the shape's scratch
    out0 = []
    before = traced(lambda: out0.append(fresh_call(switches, enclave, fl, ids, enc, d, d, 3)[2]))
    switches.set_dense_krum(F, M)
    on = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    switches.set_dense_krum(0, 0)
    out1 = []
    after = traced(lambda: out1.append(fresh_call(switches, enclave, fl, ids, enc, d, d, 3)[2]))
    assert_same_trace(before, after, "the switch never touched vs switched off again")
    assert same_bits(out0[0], out1[0]) and same_bits(out0[0], plain_mean(v))
    assert any("krum_gram_kernel" in line for line in on)
    assert not any("krum" in line for line in before)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_on_trace_does_not_depend_on_the_values(enclave, switches, packed):
    n, d, fl = N, D, 9910
    ids = ids_of(n)
    rnd = host_values(n, d)
    equal = np.full((n, d), 0.25, np.float32)
    nans = rnd.copy()
    nans[::2] = np.nan
    nans[1::4] = -np.nan
    switches.set_dense_krum(F, M)
    fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3)
    tr = [traced(lambda v=v: fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    for k in ("krum_gram_kernel", "krum_reduce_kernel", "krum_score_kernel", "krum_rank_kernel",
              "krum_accumulate_kernel"):
        assert any(k in line for line in tr[0]), k


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_two_virtual_ranks_return_the_one_gpu_bits(enclave, switches, packed):
    from fltee.ecalls import Enclave
    n, d, fl = N, D, 9920
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    switches.set_dense_krum(F, M)
    st, rv, ref, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(ref, KM.krum(v, F, M))
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, fl, ids, enc, d, d, 3)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
    finally:
        G.destroy()
