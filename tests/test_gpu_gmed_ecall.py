"""fltee_set_dense_gmed through ecall_secure_aggregation on the GPU: the staged and the pipelined
path, CTR and GCM, records and packed slices, against tests/gmed_model.py bit for bit (the values
are small integers beside the hostile clients': every Gram entry is exact); DROP on the n'
survivors; every 0x2 refusal with the round kept; a two-virtual-rank eid; the switch-off trace;
and a launch trace that depends on the shape and R, never on the values."""
import functools

import numpy as np
import pytest

import gmed_model as M
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced
from test_gpu_trim_ecall import LARGE, ids_of, payload, same_bits, start

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D, R = 10, 1101, 3
NU = M.NU
SEED = 0xC0FFEE5EED
KERNELS = ("krum_gram_kernel", "krum_reduce_kernel", "gmed_init_kernel", "gmed_matvec_kernel", "gmed_update_kernel",
           "gmed_accumulate_kernel")


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    rng = np.random.default_rng(seed + d)
    v = rng.integers(-8, 9, (n, d)).astype(np.float32)
    if n >= 7:
        # a hostile client, far outside the honest ones — by 2^20, or by 64 where d is so large that
        # sums of 2^40 d would leave f64's exact integers (every Gram entry stays exact in any order)
        v[1] += np.float32(1048576.0 if d < 4096 else 64.0)
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
        EC.set_dense_gmed(0, 0.0)
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
    v = np.ascontiguousarray(v, np.float32)
    acc = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for c in range(v.shape[0]):
            acc = (acc + v[c]).astype(np.float32)
        return (acc * (np.float32(1) / np.float32(v.shape[0]))).astype(np.float32)


# ------------------------------------------------------------------ the result ----
@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
@pytest.mark.parametrize("alg", [3, 4, 5])
def test_gmed_ecall_equals_the_model(enclave, switches, alg, packed, aead):
    n, d = N, D
    v, ids, fl = host_values(n, d), ids_of(n), 9700 + alg
    switches.set_upload_aead(aead)
    switches.set_dense_gmed(R, NU)
    enc = payload(v, ids, packed, (fl, 0, alg) if aead else None)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    alpha, _, valid = M.weights(v, R, NU)
    assert not valid[3] and alpha[3] == 0 and 0 < alpha[1] < alpha[0] / 100
    want = M.gmed(v, R, NU)
    assert same_bits(out, want)
    # the NaNs are gone, and three iterations in the 2^20 weighs 1 / 4000 (the plain mean: 2^20 / 10)
    assert np.isfinite(out).all() and np.abs(out).max() < 2.0 ** 20 / 1000
    # the round advanced
    st, rv, again, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()
    # switched off, the same upload is the plain mean it always was
    switches.set_dense_gmed(0, NU)
    st, rv, off, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(off, plain_mean(v)) and not same_bits(off, want)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_pipelined_path_is_weighted(enclave, switches, packed):
    n, d = 7, LARGE[1]  # 7 packed slices of 4,194,312 bytes > 16 MiB
    v, ids, fl = host_values(n, d, 1), ids_of(n), 9720
    switches.set_dense_gmed(2, NU)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert same_bits(out, M.gmed(v, 2, NU))


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_drop_aggregates_the_survivors(enclave, switches, packed):
    n, d, alg, fl, failed = N, D, 3, 9740, [6]
    v, ids = host_values(n, d), ids_of(n)
    keep = [c for c in range(n) if c not in failed]
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    switches.set_dense_gmed(R, NU)
    enc = payload(v, ids, packed, (fl, 0, alg)).copy()
    stride = enc.nbytes // n
    for c in failed:
        enc[c * stride + 8 * c + 5] ^= 1
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    assert enclave.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    want = M.gmed(v[keep], R, NU)  # n' = 9
    assert same_bits(out, want) and not same_bits(want, M.gmed(v, R, NU))


def test_dp_noise_is_divided_by_the_clients_aggregated(enclave, switches):
    """the same debug seed: the DP call is the plain geometric-median call plus the noise of
    divisor n' — under DROP with one failed client n' = n - 1"""
    n, d, fl, alg = N, 11011, 9745, 3
    v, ids = host_values(n, d), ids_of(n)
    keep = [c for c in range(n) if c != 6]
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    enc = payload(v, ids, False, (fl, 0, alg)).copy()
    enc[6 * (enc.nbytes // n) + 8 * 6 + 5] ^= 1
    switches.set_dense_gmed(R, NU)
    switches.set_debug_seed(SEED)
    assert enclave.ecall_fl_init(fl, ids, d, d, 1.12, 1.0, 0.1, 1.0, alg, 0, 1) == (0, 0)
    assert enclave.ecall_start_round(fl, 0, n)[:2] == (0, 0)
    st, rv, out, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    noise = out.astype(np.float64) - M.gmed(v[keep], R, NU)
    # N(0, clipping * sigma) / n' per output: the spread says which divisor was used (11011
    # samples: the estimate's own relative spread is 1 / sqrt(2 * 11011) = 0.7 %; the divisor n
    # instead of n' would read 10 % low)
    assert abs(noise.std() * (n - 1) / 1.12 - 1) < 0.05 and abs(noise.mean()) < 0.05


# ------------------------------------------------------------------- refusals ----
def refused_then_kept(EC, E, fl, ids, enc, d, k, alg, iters=R, nu=NU, trim=0, krum=(0, 0)):
    """the call ends with 0x2 and a zero [out] under the switch — never a plain mean — and the
    round was kept: with the switch off the same request is answered"""
    EC.set_dense_gmed(iters, nu)
    EC.set_dense_trim(trim)
    EC.set_dense_krum(*krum)
    st, rv, out, times = fresh_call(EC, E, fl, ids, enc, d, k, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    EC.set_dense_gmed(0, nu)
    EC.set_dense_trim(0)
    EC.set_dense_krum(0, 0)
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)
    assert (st, rv) == (0, 0)


@pytest.mark.parametrize("alg", [1, 2, 7])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_sort_based_algs_are_refused(enclave, switches, alg, packed):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    refused_then_kept(switches, enclave, 9750 + alg, ids, payload(v, ids, packed), d, d, alg)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_sparse_uploads_are_refused(enclave, switches, alg):
    import torch

    from fltee import client as C
    n, d, k = 5, 258, 64
    v, ids = host_values(n, d, 2), ids_of(n)
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    refused_then_kept(switches, enclave, 9760 + alg, ids, enc, d, k, alg)


def test_the_tree_the_cap_and_the_other_robust_switches_are_refused(enclave, switches):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    enc = payload(v, ids, False)
    switches.set_path_oram_tree(True)
    refused_then_kept(switches, enclave, 9770, ids, enc, d, d, 5)
    switches.set_path_oram_tree(False)
    refused_then_kept(switches, enclave, 9771, ids, enc, d, d, 3, trim=100)        # together with the trim
    refused_then_kept(switches, enclave, 9772, ids, enc, d, d, 3, krum=(1, 2))     # together with Multi-Krum
    refused_then_kept(switches, enclave, 9773, ids, enc, d, d, 3, iters=65)        # R > 64
    refused_then_kept(switches, enclave, 9774, ids, enc, d, d, 3, nu=0.0)          # nu not above 0
    refused_then_kept(switches, enclave, 9775, ids, enc, d, d, 3, nu=float("nan"))
    # and the same request is answered once it can be
    switches.set_dense_gmed(64, NU)
    st, rv, out, _ = fresh_call(switches, enclave, 9776, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, M.gmed(v, 64, NU))
    n, d = 1025, 4  # past FLTEE_KRUM_MAX_N; 1024 clients are answered
    v, ids = host_values(n, d, 3), ids_of(n, 2000)
    refused_then_kept(switches, enclave, 9777, ids, payload(v, ids, False), d, d, 3)
    switches.set_dense_gmed(2, NU)
    st, rv, out, _ = fresh_call(switches, enclave, 9778, ids[:1024], payload(v[:1024], ids[:1024], False), d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, M.gmed(v[:1024], 2, NU))


def test_alg_6_is_refused(enclave, switches):
    import torch

    from fltee import client as C
    n, d, k = 6, 258, 32
    v, ids, fl = host_values(n, d, 2), ids_of(n), 9785
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    switches.set_dense_gmed(R, NU)
    start(enclave, fl, ids, d, k, 6)
    st, rv, out, times = enclave.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, ids, enc, d, k, 6)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    switches.set_dense_gmed(0, NU)
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
    switches.set_dense_gmed(R, NU)
    tr = traced(lambda: fresh_call(switches, enclave, 9790, ids, enc, d, d, 4))
    assert sum("krum_gram_kernel" in line and line.startswith("launch") for line in tr) == 1  # once: no rerun
    assert not any("scatter" in line or "fold_sorted" in line for line in tr)
    refused_then_kept(switches, enclave, 9790, ids, enc, d, d, 4)


# ---------------------------------------------------------------------- traces ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_off_trace_and_bits_are_the_untouched_ones(enclave, switches, packed):
    n, d, fl = N, D, 9800
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    fresh_call(switches, enclave, fl, ids, enc, d, d, 3)  # the shape's scratch
    out0 = []
    before = traced(lambda: out0.append(fresh_call(switches, enclave, fl, ids, enc, d, d, 3)[2]))
    switches.set_dense_gmed(R, NU)
    on = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    switches.set_dense_gmed(0, NU)  # (0, anything) is off
    out1 = []
    after = traced(lambda: out1.append(fresh_call(switches, enclave, fl, ids, enc, d, d, 3)[2]))
    assert_same_trace(before, after, "the switch never touched vs switched off again")
    assert same_bits(out0[0], out1[0]) and same_bits(out0[0], plain_mean(v))
    assert any("gmed_matvec_kernel" in line for line in on)
    assert not any("gmed" in line or "krum" in line for line in before)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_on_trace_depends_on_r_and_not_on_the_values(enclave, switches, packed):
    n, d, fl = N, D, 9810
    ids = ids_of(n)
    rnd = host_values(n, d)
    equal = np.full((n, d), 0.25, np.float32)
    nans = rnd.copy()
    nans[::2] = np.nan
    nans[1::4] = -np.nan
    switches.set_dense_gmed(R, NU)
    fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3)
    tr = [traced(lambda v=v: fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    for k in KERNELS:
        assert any(k in line for line in tr[0]), k
    # nu changes nothing; R changes the number of iterations' launches and nothing else
    switches.set_dense_gmed(R, 0.5)
    other_nu = traced(lambda: fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3))
    assert_same_trace(tr[0], other_nu, "nu = 2^-20 vs nu = 0.5")

    def launches(trace, name):
        return sum(name in line and line.startswith("launch") for line in trace)

    switches.set_dense_gmed(R + 2, NU)
    more = traced(lambda: fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3))
    for name in ("gmed_matvec_kernel", "gmed_update_kernel"):
        assert launches(tr[0], name) == R and launches(more, name) == R + 2
    for name in ("krum_reduce_kernel", "gmed_init_kernel", "gmed_accumulate_kernel"):
        assert launches(tr[0], name) == launches(more, name) == 1
    rest = [[line for line in t if "gmed_matvec_kernel" not in line and "gmed_update_kernel" not in line]
            for t in (tr[0], more)]
    assert_same_trace(rest[0], rest[1], "R = 3 vs R = 5 without the iterations' launches")


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_two_virtual_ranks_return_the_one_gpu_bits(enclave, switches, packed):
    from fltee.ecalls import Enclave
    n, d, fl = N, D, 9820
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    switches.set_dense_gmed(R, NU)
    st, rv, ref, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(ref, M.gmed(v, R, NU))
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, fl, ids, enc, d, d, 3)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
    finally:
        G.destroy()
