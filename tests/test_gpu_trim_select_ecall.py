"""fltee_set_dense_trim_select through ecall_secure_aggregation: the 131-client median — 0x2
with the switch off, as ever — answered bit for bit tests/trim_model.py with it on, for records,
packed and bf16 uploads; DROP computing t from n'; the cap on n; a call with t <= 64 staying on
the list kernel; the launch trace at t > 64 for random, all-equal and NaN-laden values; a
two-virtual-rank eid; and the server's flag."""
import functools

import numpy as np
import pytest

import bf16_model as BM
import trim_model as TM
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced
from test_gpu_trim_ecall import fresh_call, ids_of, payload, same_bits, start

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

N, D = 131, 4
T = 65  # fltee_trim_count(131, 500): one past FLTEE_TRIM_MAX


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    """bf16-representable values (every format carries them exactly), ties, a hostile client
    and NaNs"""
    rng = np.random.default_rng(seed + 131 * d + n)
    v = BM.widen(BM.narrow(rng.normal(0, 1, (n, d)).astype(np.float32)))
    v[::3, 0] = np.float32(0.5)         # ties
    v[1, :] = np.float32(1e30)          # a hostile client (bf16: rounds to a finite value or inf; still an extreme)
    v[1] = BM.widen(BM.narrow(v[1]))
    v[3, 1::2] = np.nan
    v = np.ascontiguousarray(v, np.float32)
    v.setflags(write=False)
    return v


@pytest.fixture
def switches():
    from fltee import ecalls as EC
    EC.set_upload_packed(True)
    EC.set_upload_bf16(True)
    try:
        yield EC
    finally:
        EC.set_dense_trim_select(False)
        EC.set_dense_trim(0)
        EC.set_upload_bf16(False)
        EC.set_upload_packed(False)
        EC.set_upload_aead_policy("abort")
        EC.set_upload_aead(False)
        EC.set_debug_seed(0)


@pytest.fixture(scope="module")
def enclave():
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    E = Enclave(0)
    yield E
    E.destroy()


def upload(v, ids, fmt, aead=None):
    """the payload of `fmt` in ("records", "packed", "bf16")"""
    import torch

    from fltee import client as C
    if fmt != "bf16":
        return payload(v, ids, fmt == "packed", aead)
    assert aead is None
    t = torch.from_numpy(np.array(v, np.float32)).cuda()
    return C.produce_payloads(t, ids, bf16=True).cpu().numpy()


# ------------------------------------------------------------------ the result ----
@pytest.mark.parametrize("fmt", ["records", "packed", "bf16"])
@pytest.mark.parametrize("alg", [3, 4, 5])
def test_the_131_client_median(enclave, switches, alg, fmt):
    n, d = N, D
    v, ids, fl = host_values(n, d), ids_of(n, 2000), 9800 + alg
    assert TM.trim_count(n, 500) == T == switches.trim_count(n, 500) and T > TM.TRIM_MAX
    enc = upload(v, ids, fmt)
    switches.set_dense_trim(500)
    # the switch off: refused as it always was, [out] zero, the round kept
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    switches.set_dense_trim_select(True)
    st, rv, out, times = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    want = TM.trimmed(v, T)
    assert same_bits(out, want)
    assert np.isfinite(out).all() and np.abs(out).max() < 10  # the 1e30 and the NaNs are gone
    # the round advanced
    st, rv, again, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()
    # off again: refused again
    switches.set_dense_trim_select(False)
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any()


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_pipelined_path(enclave, switches, packed):
    """131 slices past 16 MiB in all: the chunked load, then the selection route"""
    n, d = N, 33001  # 131 x 132,008 packed bytes > 16 MiB
    v, ids, fl = host_values(n, d, 1), ids_of(n, 2000), 9810
    switches.set_dense_trim(500)
    switches.set_dense_trim_select(True)
    tr = traced(lambda: fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3))
    assert any("trim_select_kernel" in line for line in tr)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert same_bits(out, TM.trimmed(v, T))


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_drop_computes_t_from_the_survivors(enclave, switches, packed):
    n, d, alg, fl, failed = 140, D, 3, 9820, [17]
    v, ids = host_values(n, d), ids_of(n, 2000)
    keep = [c for c in range(n) if c not in failed]
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    switches.set_dense_trim(500)
    switches.set_dense_trim_select(True)
    enc = payload(v, ids, packed, (fl, 0, alg)).copy()
    stride = enc.nbytes // n
    for c in failed:
        enc[c * stride + 5] ^= 1
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    assert enclave.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    t = TM.trim_count(len(keep), 500)
    assert len(keep) == 139 and t == 69 and TM.trim_count(n, 500) == 69
    assert same_bits(out, TM.trimmed(v[keep], t))
    assert not same_bits(out, TM.trimmed(v, 69))


def test_past_the_cap_on_n_is_refused(enclave, switches):
    n, d, fl = 4097, D, 9830
    v, ids = host_values(n, d), ids_of(n, 2000)
    enc = payload(v, ids, True)
    switches.set_dense_trim(500)
    switches.set_dense_trim_select(True)
    st, rv, out, times = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all()
    # the round was kept: with trimming off the same request is answered
    switches.set_dense_trim(0)
    st, rv, out, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0)
    # 4096 clients are answered
    switches.set_dense_trim(500)
    st, rv, out, _ = fresh_call(switches, enclave, fl + 1, ids[:4096], payload(v[:4096], ids[:4096], True), d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v[:4096], 2047))


# ---------------------------------------------------------------------- traces ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_t_up_to_64_stays_on_the_list_kernel(enclave, switches, packed):
    n, d, fl = 100, 257, 9840
    v, ids = host_values(n, d), ids_of(n, 2000)
    enc = payload(v, ids, packed)
    switches.set_dense_trim(500)
    fresh_call(switches, enclave, fl, ids, enc, d, d, 3)  # the shape's scratch
    off = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    switches.set_dense_trim_select(True)
    on = traced(lambda: fresh_call(switches, enclave, fl, ids, enc, d, d, 3))
    assert_same_trace(off, on, "the 100-client median (t = 49), the selection switch off vs on")
    assert any("trimmed_mean_kernel" in line for line in on)
    assert not any("trim_select_kernel" in line for line in on)
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v, 49))


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_trace_does_not_depend_on_the_values(enclave, switches, packed):
    n, d, fl = N, 257, 9850
    ids = ids_of(n, 2000)
    rnd = host_values(n, d)
    equal = np.full((n, d), 0.25, np.float32)
    nans = rnd.copy()
    nans[::2] = np.nan
    nans[1::4] = -np.nan
    # both switches off: the trace every earlier build gives
    fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3)
    plain = traced(lambda: fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3))
    assert not any("trim" in line for line in plain)
    switches.set_dense_trim_select(True)  # alone it changes nothing
    alone = traced(lambda: fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3))
    assert_same_trace(plain, alone, "both switches off vs the selection switch alone")
    switches.set_dense_trim(500)
    fresh_call(switches, enclave, fl, ids, payload(rnd, ids, packed), d, d, 3)
    tr = [traced(lambda v=v: fresh_call(switches, enclave, fl, ids, payload(v, ids, packed), d, d, 3))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    assert any("trim_select_kernel" in line for line in tr[0])
    assert not any("trimmed_mean_kernel" in line for line in tr[0])


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_two_virtual_ranks_return_the_one_gpu_bits(enclave, switches, packed):
    from fltee.ecalls import Enclave
    n, d, fl = N, 257, 9860
    v, ids = host_values(n, d), ids_of(n, 2000)
    enc = payload(v, ids, packed)
    switches.set_dense_trim(500)
    switches.set_dense_trim_select(True)
    st, rv, ref, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(ref, TM.trimmed(v, T))
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, fl, ids, enc, d, d, 3)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
    finally:
        G.destroy()


# --------------------------------------------------------------------- server ----
def test_the_servers_flag_reaches_the_switch(enclave, switches):
    from fltee.server import Aggregator
    n, d, fl = N, D, 9870
    v, ids = host_values(n, d), ids_of(n, 2000)
    enc = payload(v, ids, True)
    Aggregator(enclave=enclave, packed=True, trim_per_mille=500)
    st, rv, out, _ = fresh_call(switches, enclave, fl, ids, enc, d, d, 3)
    assert (st, rv) == (0, 2)
    Aggregator(enclave=enclave, packed=True, trim_per_mille=500, trim_select=True)
    st, rv, out, _ = enclave.ecall_secure_aggregation(fl, 0, ids, enc, d, d, 3)
    assert (st, rv) == (0, 0) and same_bits(out, TM.trimmed(v, T))
