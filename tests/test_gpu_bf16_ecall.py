"""bf16 dense uploads through ecall_secure_aggregation (fltee_set_upload_bf16): [out] bit for bit
the records ECALL on the widened values for algs 3, 4, 5 and alg 1, plain and authenticated; the
format bit of the AAD against the other two formats; DROP on the survivors alone; the switch off
reading the same bytes as records; one server with both switches on answering all three formats;
fltee_set_dense_trim on a bf16 call; and an eid of two virtual ranks against the one-GPU eid."""
import functools

import numpy as np
import pytest

import bf16_model as BM
import packed_model as PM
import trim_model as TM
from conftest import gpu_available
from test_gpu_oblivious import traced

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MAC_MISMATCH = 0x3001
SHAPES = [(17, 3), (17, 257), (6, 1101)]
SEED = 0xF17EE5EED


def ids_of(n, base=700):
    return np.arange(base, base + n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    """(f32 values as a client holds them, their bf16 rows): built once, never modified"""
    v = BM.values(np.random.default_rng(seed + d), n, d)
    r = BM.pack(v)
    v.setflags(write=False)
    r.setflags(write=False)
    return v, r


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def ctr_payloads(n, d, seed=0):
    """(records, packed, bf16) payloads as host bytes: the bf16 slices of the values, and the
    widened values as records and as packed slices"""
    from fltee import client as C
    v, r = host_values(n, d, seed)
    ids = ids_of(n)
    wide = cuda(BM.unpack(r, d))
    rec = C.produce_payloads(wide, ids).cpu().numpy()
    pk = C.produce_payloads(wide, ids, packed=True).cpu().numpy()
    bf = C.produce_payloads(cuda(v), ids, bf16=True).cpu().numpy()
    assert rec.nbytes == n * d * 8 and pk.nbytes == n * PM.slice_bytes(d) and bf.nbytes == n * BM.slice_bytes(d)
    for a in (rec, pk, bf):
        a.setflags(write=False)
    return rec, pk, bf


@pytest.fixture
def switches():
    """every process-wide switch this module turns, back off afterwards"""
    from fltee import ecalls as EC
    EC.set_upload_bf16(True)
    try:
        yield EC
    finally:
        EC.set_upload_bf16(False)
        EC.set_upload_packed(False)
        EC.set_dense_trim(0)
        EC.set_upload_aead_policy("abort")
        EC.set_upload_aead(False)
        EC.set_debug_seed(0)


def start(E, fl_id, ids, d, k, alg):
    assert E.ecall_fl_init(fl_id, ids, d, k, 1.12, 1.0, 0.1, 1.0, alg, 0, 0) == (0, 0)
    assert E.ecall_start_round(fl_id, 0, len(ids))[:2] == (0, 0)


def fresh_call(EC, E, fl, ids, enc, d, k, alg):
    """round 0 of a config made for the call; the same seed sequence every time"""
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, k, alg)
    return E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def enclave():
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    E = Enclave(0)
    yield E
    E.destroy()


# --------------------------------------------------------- bf16 == records ----
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("alg", [1, 3, 4, 5])
def test_bf16_ecall_equals_the_records_ecall(enclave, switches, alg, n, d):
    rec, _, bf = ctr_payloads(n, d)
    ids, fl, E = ids_of(n), 9600 + alg, enclave
    for k in (d, 0):  # what the request declares: a dense upload either way
        if k == 0 and alg == 1:
            continue  # (advanced folds over the request's k)
        st, rv, ref, _ = fresh_call(switches, E, fl, ids, rec, d, k, alg)   # 8 d bytes: records
        assert (st, rv) == (0, 0)
        st, rv, out, times = fresh_call(switches, E, fl, ids, bf, d, k, alg)
        assert (st, rv) == (0, 0)
        assert same_bits(out, ref)
        assert ref.any() and np.isfinite(times).all() and times.sum() > 0
        if alg in (3, 4, 5):
            assert BM.same_bits(out, BM.inorder_mean(host_values(n, d)[1], d))
    # the round advanced: round 0 is over
    st, rv, again, _ = E.ecall_secure_aggregation(fl, 0, ids, bf, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()


def test_the_bf16_call_runs_the_bf16_kernels(enclave, switches):
    n, d = 17, 257
    rec, _, bf = ctr_payloads(n, d)
    ids, E = ids_of(n), enclave
    fresh_call(switches, E, 9610, ids, bf, d, d, 3)
    t3 = traced(lambda: fresh_call(switches, E, 9610, ids, bf, d, d, 3))
    t1 = traced(lambda: fresh_call(switches, E, 9611, ids, bf, d, d, 1))
    tr = traced(lambda: fresh_call(switches, E, 9610, ids, rec, d, d, 3))
    assert any("dense_accumulate_h" in line for line in t3) and not any("unpack" in line for line in t3)
    assert any("unpack_bf16_kernel" in line for line in t1)
    assert not any("bf16" in line or "accumulate_h" in line for line in tr)
    # a records call's trace does not see the switch
    switches.set_upload_bf16(False)
    assert tr == traced(lambda: fresh_call(switches, E, 9610, ids, rec, d, d, 3))


# ----------------------------------------------------------------------- AEAD ----
def auth(rows_or_rec, ids, fl, alg, **fmt):
    from fltee import client as C
    return C.encrypt_parameters_auth(rows_or_rec, ids, fl, 0, alg, **fmt).cpu().numpy()


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("alg", [1, 3, 4, 5])
def test_authenticated_bf16_ecall_equals_the_records_ecall(enclave, switches, alg, n, d):
    from fltee import client as C
    ids, E, fl = ids_of(n), enclave, 9700 + alg
    v, r = host_values(n, d, 1)
    wide = cuda(BM.unpack(r, d))
    switches.set_upload_aead(True)
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, auth(C.serialize_dense(wide), ids, fl, alg), d, d, alg)
    assert (st, rv) == (0, 0)
    good = auth(C.pack_dense_bf16(cuda(v)), ids, fl, alg, bf16=True)
    assert good.nbytes == n * (BM.slice_bytes(d) + 16)
    st, rv, out, times = fresh_call(switches, E, fl, ids, good, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(out, ref) and ref.any() and np.isfinite(times).all()


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES[1:])
def test_a_slice_sealed_for_one_format_verifies_under_no_other(enclave, switches, alg, n, d):
    from fltee import client as C
    ids, E, fl = ids_of(n), enclave, 9720 + alg
    v, r = host_values(n, d, 1)
    wide = cuda(BM.unpack(r, d))
    switches.set_upload_aead(True)
    switches.set_upload_packed(True)
    rows, pk, rec = C.pack_dense_bf16(cuda(v)), C.pack_dense(wide), C.serialize_dense(wide)
    good = {"bf16": auth(rows, ids, fl, alg, bf16=True), "packed": auth(pk, ids, fl, alg, packed=True),
            "records": auth(rec, ids, fl, alg)}
    bad = {"bf16 slices sealed as records": auth(rows, ids, fl, alg),
           "bf16 slices sealed as packed": auth(rows, ids, fl, alg, packed=True),
           "records sealed as bf16": auth(rec, ids, fl, alg, bf16=True),
           "packed slices sealed as bf16": auth(pk, ids, fl, alg, bf16=True)}
    stride = BM.slice_bytes(d) + 16
    flipped = good["bf16"].copy()
    flipped[2 * stride + 9] ^= 0x10
    bad["a flipped bit"] = flipped
    moved = good["bf16"].copy()
    moved[:stride], moved[stride:2 * stride] = good["bf16"][stride:2 * stride], good["bf16"][:stride]
    bad["a moved slice"] = moved
    start(E, fl, ids, d, d, alg)
    for what, enc in bad.items():
        st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
        assert (st, rv) == (0, MAC_MISMATCH), what
        assert not out.view(np.uint32).any() and np.isfinite(times).all()
    ref = None
    for what, enc in good.items():  # (the failed calls kept the round)
        st, rv, out, _ = fresh_call(switches, E, fl, ids, enc, d, d, alg)
        assert (st, rv) == (0, 0), what
        assert ref is None or same_bits(out, ref), what
        ref = out
    assert ref.any()


def drop_case(EC, E, fl, alg, n, d, failed):
    """(out of the DROP call with `failed` tampered, out of the bf16 ECALL on the survivors)"""
    from fltee import client as C
    ids = ids_of(n)
    v, _ = host_values(n, d, 2)
    keep = [c for c in range(n) if c not in failed]
    EC.set_upload_aead(True)
    EC.set_upload_aead_policy("drop")
    enc = auth(C.pack_dense_bf16(cuda(v)), ids, fl, alg, bf16=True).copy()
    stride = BM.slice_bytes(d) + 16
    for c in failed:
        enc[c * stride + (8 * c + 5) % (stride - 16)] ^= 1
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, d, alg)
    st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert E.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    ids_s = ids[keep]
    enc_s = auth(C.pack_dense_bf16(cuda(v[keep])), ids_s, fl + 1, alg, bf16=True)
    EC.set_debug_seed(SEED)
    start(E, fl + 1, ids_s, d, d, alg)
    st, rv, ref, _ = E.ecall_secure_aggregation(fl + 1, 0, ids_s, enc_s, d, d, alg)
    assert (st, rv) == (0, 0)
    return out, ref


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES)
def test_drop_equals_the_bf16_ecall_on_the_survivors(enclave, switches, alg, n, d):
    """one tampered client: the survivors' rows are gathered as Q units per client (for n' odd
    or Q odd the gathered base need not be 16-byte aligned)"""
    failed = [2]
    out, ref = drop_case(switches, enclave, 9800 + 10 * alg, alg, n, d, failed)
    assert same_bits(out, ref) and ref.any()
    if alg == 3:
        r = host_values(n, d, 2)[1][[c for c in range(n) if c not in failed]]
        assert BM.same_bits(out, BM.inorder_mean(r, d))


# ------------------------------------------------ the switch, and three formats ----
def test_switch_off_reads_the_same_bytes_as_records(enclave, switches, oracle):
    """k = Q records are exactly a bf16 slice's bytes.  Under a request that declares a dense
    upload (k_req = d): off, they are summed as the records they are (what every earlier version
    did); on, the bytes are taken for bf16 values.  Under a request that says k = Q they are
    records either way."""
    from fltee import client as C
    from fltee import device as D
    n, d = 6, 1101
    k = BM.units(d)
    ids, E = ids_of(n), enclave
    v = cuda(PM.values(np.random.default_rng(d), n, d))  # (finite: the oracle's sums are numbers)
    rec = C.zero_except_top_k_weights(v, k)
    idx, val = D.unpack_records(rec.cpu().numpy())
    want, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0
    enc = C.encrypt_parameters(rec, ids).cpu().numpy()
    assert enc.nbytes == n * BM.slice_bytes(d)
    switches.set_upload_bf16(False)
    st, rv, off, _ = fresh_call(switches, E, 9830, ids, enc, d, d, 4)
    assert (st, rv) == (0, 0) and same_bits(off, want)
    st, rv, sparse_off, _ = fresh_call(switches, E, 9831, ids, enc, d, k, 4)
    assert (st, rv) == (0, 0) and same_bits(sparse_off, want)
    switches.set_upload_bf16(True)
    st, rv, sparse_on, _ = fresh_call(switches, E, 9831, ids, enc, d, k, 4)
    assert (st, rv) == (0, 0) and same_bits(sparse_on, want)
    st, rv, on, _ = fresh_call(switches, E, 9830, ids, enc, d, d, 4)
    assert (st, rv) == (0, 0) and not same_bits(on, off)
    rows = rec.cpu().numpy().view(np.uint16).reshape(n, BM.row(d))
    assert BM.same_bits(on, BM.inorder_mean(rows, d))


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES)
def test_one_server_answers_all_three_formats(enclave, switches, alg, n, d):
    rec, pk, bf = ctr_payloads(n, d)
    ids, E, fl = ids_of(n), enclave, 9840 + alg
    switches.set_upload_bf16(False)
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, rec, d, d, alg)  # as every earlier version
    assert (st, rv) == (0, 0) and ref.any()
    switches.set_upload_bf16(True)
    switches.set_upload_packed(True)
    for turn in range(2):
        for what, enc in (("records", rec), ("packed", pk), ("bf16", bf)):
            st, rv, out, _ = fresh_call(switches, E, fl, ids, enc, d, d, alg)
            assert (st, rv) == (0, 0), what
            assert same_bits(out, ref), what


# ----------------------------------------------------------------------- trim ----
@pytest.mark.parametrize("per_mille", [100, 500], ids=["t1", "median"])
@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("d", [3, 257])
def test_trim_on_a_bf16_call_is_the_trimmed_mean_of_the_widened_values(enclave, switches, alg, d, per_mille):
    n = 17
    _, _, bf = ctr_payloads(n, d)
    wide = BM.unpack(host_values(n, d)[1], d)
    t = TM.trim_count(n, per_mille)
    assert t == {100: 1, 500: 8}[per_mille]
    switches.set_dense_trim(per_mille)
    st, rv, out, _ = fresh_call(switches, enclave, 9860 + alg, ids_of(n), bf, d, d, alg)
    assert (st, rv) == (0, 0)
    want = TM.trimmed(wide, t)
    assert BM.same_bits(out, want) and not BM.same_bits(want, TM.trimmed(wide, 0))
    switches.set_dense_trim(0)
    st, rv, off, _ = fresh_call(switches, enclave, 9860 + alg, ids_of(n), bf, d, d, alg)
    assert (st, rv) == (0, 0) and BM.same_bits(off, TM.trimmed(wide, 0))


def test_trim_refuses_what_it_refused_and_not_a_bf16_call(enclave, switches):
    """alg 1 cannot be trimmed, whatever the format: 0x2, never an untrimmed mean"""
    n, d = 17, 257
    _, _, bf = ctr_payloads(n, d)
    switches.set_dense_trim(100)
    st, rv, out, _ = fresh_call(switches, enclave, 9870, ids_of(n), bf, d, d, 1)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any()


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("alg", [1, 3])
def test_two_virtual_ranks_equal_the_one_gpu_eid(enclave, switches, alg):
    from fltee.ecalls import Enclave
    n, d = 6, 1101
    ids = ids_of(n)
    _, _, bf = ctr_payloads(n, d)
    st, rv, ref, _ = fresh_call(switches, enclave, 9900 + alg, ids, bf, d, d, alg)
    assert (st, rv) == (0, 0)
    drop_ref, _ = drop_case(switches, enclave, 9910 + 10 * alg, alg, n, d, [2])
    switches.set_upload_aead(False)
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, 9900 + alg, ids, bf, d, d, alg)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
        drop_out, drop_survivors = drop_case(switches, G, 9910 + 10 * alg, alg, n, d, [2])
        assert same_bits(drop_out, drop_ref) and same_bits(drop_survivors, drop_ref)
    finally:
        G.destroy()
