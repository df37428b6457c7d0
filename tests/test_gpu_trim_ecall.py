"""fltee_set_dense_trim through ecall_secure_aggregation: [out] bit for bit tests/trim_model.py
on the plaintext with the divisor n - 2 t, for records and packed uploads, CTR (the staged
path, and the pipelined one at a payload past 16 MiB) and AEAD (the verdict first, then the
unstaged path); DROP trimming the survivors with t from n'; every call that cannot be trimmed
refused with 0x2, [out] zero and the round kept; the launch trace with the switch off, and on
for random, all-equal and NaN-laden values; and a two-virtual-rank eid."""
import functools

import numpy as np
import pytest

import packed_model as PM
import trim_model as TM
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D = 10, 1101
LARGE = (5, (1 << 20) + 2)  # pipelined: 5 packed slices of 4,194,312 bytes > 16 MiB
SEED = 0xF17EE5EED


def ids_of(n, base=700):
    return np.arange(base, base + n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    rng = np.random.default_rng(seed + d)
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    v[:, ::7] = np.round(v[:, ::7])          # ties
    if n >= 4:
        v[1, ::5] = np.float32(1e30)         # a hostile client
        v[3, 3::11] = np.nan
    v.setflags(write=False)
    return v


def payload(v, ids, packed, aead=None):
    """aead: (fl_id, round, alg) for an authenticated payload"""
    import torch

    from fltee import client as C
    t = torch.from_numpy(np.array(v, np.float32)).cuda()
    if aead is None:
        return C.produce_payloads(t, ids, packed=packed).cpu().numpy()
    body = C.pack_dense(t) if packed else C.serialize_dense(t)
    return C.encrypt_parameters_auth(body, ids, *aead, packed=packed).cpu().numpy()


@pytest.fixture
def switches():
    from fltee import ecalls as EC
    EC.set_bubble_ecall(True)
    EC.set_upload_packed(True)
    try:
        yield EC
    finally:
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


def start(E, fl_id, ids, d, k, alg):
    assert E.ecall_fl_init(fl_id, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, 0) == (0, 0)
    assert E.ecall_start_round(fl_id, 0, len(ids))[:2] == (0, 0)


def fresh_call(EC, E, fl, ids, enc, d, k, alg):
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, k, alg)
    return E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ the result ----
@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
@pytest.mark.parametrize("per_mille", [100, 500])
@pytest.mark.parametrize("alg", [3, 4, 5])
def test_trimmed_ecall_equals_the_model(enclave, switches, alg, per_mille, packed, aead):
    n, d = N, D
    v, ids, fl = host_values(n, d), ids_of(n), 9600 + alg
    t = TM.trim_count(n, per_mille)
    assert t == {100: 1, 500: 4}[per_mille] == switches.trim_count(n, per_mille)
    switches.set_upload_aead(aead)
    switches.set_dense_trim(per_mille)
    enc = payload(v, ids, packed, (fl, 0, alg) if aead else None)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    want = TM.trimmed(v, t)
    assert same_bits(out, want)
    if per_mille == 500:
        assert np.isfinite(out).all() and np.abs(out).max() < 10  # the 1e30 and the NaNs are gone
    # the round advanced
    st, rv, again, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()
    # switched off, the same upload is the plain mean it always was
    switches.set_dense_trim(0)
    st, rv, off, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(off, TM.trimmed(v, 0)) and not same_bits(off, want)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_pipelined_path_is_trimmed(enclave, switches, packed):
    n, d = LARGE
    v, ids, fl = host_values(n, d, 1), ids_of(n), 9620
    switches.set_dense_trim(500)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert same_bits(out, TM.trimmed(v, TM.trim_count(n, 500)))


def test_a_tiny_per_mille_and_one_client_run_untrimmed(enclave, switches):
    v, ids = host_values(N, D), ids_of(N)
    switches.set_dense_trim(99)  # 10 * 99 / 1000 = 0
    st, rv, out, _ = fresh_call(switches, enclave, 9630, ids, payload(v, ids, True), D, D, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v, 0))
    switches.set_dense_trim(500)
    st, rv, out, _ = fresh_call(switches, enclave, 9631, ids[:1], payload(v[:1], ids[:1], False), D, D, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v[:1], 0))


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_drop_trims_the_survivors(enclave, switches, packed):
    n, d, alg, fl, failed = N, D, 3, 9640, [0, 6]
    v, ids = host_values(n, d), ids_of(n)
    keep = [c for c in range(n) if c not in failed]
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    switches.set_dense_trim(500)
    enc = payload(v, ids, packed, (fl, 0, alg)).copy()
    stride = enc.nbytes // n
    for c in failed:
        enc[c * stride + 8 * c + 5] ^= 1
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    assert enclave.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    t = TM.trim_count(len(keep), 500)
    assert t == 3
    assert same_bits(out, TM.trimmed(v[keep], t))


# ------------------------------------------------------------------- refusals ----
def refused_then_kept(EC, E, fl, ids, enc, d, k, alg, per_mille=100):
    """the call ends with 0x2 and a zero [out] under the switch, and the round was kept: with
    the switch off the same request is answered"""
    EC.set_dense_trim(per_mille)
    st, rv, out, times = fresh_call(EC, E, fl, ids, enc, d, k, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    EC.set_dense_trim(0)
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)
    assert (st, rv) == (0, 0)


@pytest.mark.parametrize("alg", [1, 2, 7])
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_sort_based_algs_are_refused(enclave, switches, alg, packed):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    refused_then_kept(switches, enclave, 9650 + alg, ids, payload(v, ids, packed), d, d, alg)


@pytest.mark.parametrize("alg", [3, 4, 5])
def test_sparse_uploads_are_refused(enclave, switches, alg):
    import torch

    from fltee import client as C
    n, d, k = 5, 258, 64
    v, ids = host_values(n, d, 2), ids_of(n)
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    refused_then_kept(switches, enclave, 9660 + alg, ids, enc, d, k, alg)


def test_the_tree_and_a_trim_count_past_the_lists_are_refused(enclave, switches):
    n, d = 5, 258
    v, ids = host_values(n, d, 2), ids_of(n)
    switches.set_path_oram_tree(True)
    refused_then_kept(switches, enclave, 9670, ids, payload(v, ids, False), d, d, 5)
    switches.set_path_oram_tree(False)
    n, d = 131, 4  # t = 65 > FLTEE_TRIM_MAX; 129 clients (t = 64) are answered
    v, ids = host_values(n, d, 3), ids_of(n, 1000)
    refused_then_kept(switches, enclave, 9671, ids, payload(v, ids, False), d, d, 3, per_mille=500)
    switches.set_dense_trim(500)
    st, rv, out, _ = fresh_call(switches, enclave, 9672, ids[:129], payload(v[:129], ids[:129], False), d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v[:129], 64))


def test_alg_6_is_refused(enclave, switches):
    import torch

    from fltee import client as C
    n, d, k = 6, 258, 32
    v, ids, fl = host_values(n, d, 2), ids_of(n), 9680
    enc = C.produce_payloads(torch.from_numpy(np.array(v, np.float32)).cuda(), ids, k=k).cpu().numpy()
    switches.set_dense_trim(100)
    start(enclave, fl, ids, d, k, 6)
    st, rv, out, times = enclave.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, ids, enc, d, k, 6)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    switches.set_dense_trim(0)
    st, rv, out, _ = enclave.ecall_client_size_optimized_secure_aggregation(fl, 0, 3, ids, enc, d, k, 6)
    assert (st, rv) == (0, 0)


@pytest.mark.parametrize("shape", [(5, 258), LARGE], ids=["staged", "pipelined"])
def test_records_out_of_position_are_refused(enclave, switches, shape):
    """a dense-sized upload whose records are not in position reruns sparse without the
    switch; under it the call ends with 0x2 after the one status readback"""
    import torch

    from fltee import client as C
    n, d = shape
    v, ids = host_values(n, d, 4), ids_of(n)
    rec = C.serialize_dense(torch.from_numpy(np.array(v, np.float32)).cuda()).reshape(n, d).clone()
    rec[2, [0, 1]] = rec[2, [1, 0]]  # client 2's first two records swapped
    enc = C.encrypt_parameters(rec.reshape(-1), ids).cpu().numpy()
    switches.set_dense_trim(500)
    tr = traced(lambda: fresh_call(switches, enclave, 9690, ids, enc, d, d, 4))
    assert any("trimmed_mean_kernel" in line for line in tr)  # it ran trimmed, once: no rerun follows
    assert not any("scatter" in line or "fold_sorted" in line for line in tr)
    refused_then_kept(switches, enclave, 9690, ids, enc, d, d, 4, per_mille=500)


# ---------------------------------------------------------------------- traces ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_off_trace_is_the_untouched_trace(enclave, switches, packed):
    n, d, fl = N, D, 9700
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    fresh_call(switches, enclave, fl, ids, enc, d, d, 3)  # the shape's scratch
    before = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    switches.set_dense_trim(500)
    on = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    switches.set_dense_trim(0)
    after = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    assert_same_trace(before, after, "the switch never touched vs switched off again")
    assert any("trimmed_mean_kernel" in line for line in on)
    assert not any("trimmed_mean_kernel" in line for line in before)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_switch_on_trace_does_not_depend_on_the_values(enclave, switches, packed):
    n, d, fl = N, D, 9710
    ids = ids_of(n)
    rnd = host_values(n, d)
    equal = np.full((n, d), 0.25, np.float32)
    nans = rnd.copy()
    nans[::2] = np.nan
    nans[1::4] = -np.nan
    switches.set_dense_trim(500)
    fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3)
    tr = [traced(lambda v=v: fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    assert any("trimmed_mean_kernel" in line for line in tr[0])


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_two_virtual_ranks_return_the_one_gpu_bits(enclave, switches, packed):
    from fltee.ecalls import Enclave
    n, d, fl = N, D, 9720
    v, ids = host_values(n, d), ids_of(n)
    enc = payload(v, ids, packed)
    switches.set_dense_trim(100)
    st, rv, ref, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(ref, TM.trimmed(v, 1))
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, fl, ids, enc, d, d, 3)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
    finally:
        G.destroy()
