"""Packed dense uploads through ecall_secure_aggregation (fltee_set_upload_packed): [out] bit
for bit the records ECALL on the same values for algs 1, 2, 3, 4, 5 and 7, on the staged
path and on the pipelined one; records uploads through the switched-on server answered as
before; the switch off reading a packed-sized payload as records; authenticated packed calls
(the format bit of the AAD, tampers, DROP on the survivors alone); an eid of two virtual ranks
against the one-GPU eid; and the launch trace."""
import functools

import numpy as np
import pytest

import packed_model as PM
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MAC_MISMATCH = 0x3001
ALGS = [1, 2, 3, 4, 5, 7]
SMALL = (5, 1026)                 # staged: 5 x 4104 bytes
LARGE = (5, (1 << 20) + 2)        # pipelined: 5 x 4,194,312 bytes > 16 MiB (4 clients would not cross it)
SEED = 0xF17EE5EED


def ids_of(n, base=500):
    return np.arange(base, base + n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def values(n, d, seed=0):
    import torch
    if n * d > 1 << 20:  # the large shape: drawn on the device
        g = torch.Generator(device="cuda").manual_seed(seed + d)
        return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    return torch.from_numpy(PM.values(np.random.default_rng(seed + d), n, d)).cuda()


@functools.lru_cache(maxsize=None)
def ctr_payloads(n, d, seed=0):
    """(records payload, packed payload) of the same values, as host bytes: built once"""
    from fltee import client as C
    v, ids = values(n, d, seed), ids_of(n)
    rec = C.produce_payloads(v, ids).cpu().numpy()
    pk = C.produce_payloads(v, ids, packed=True).cpu().numpy()
    assert rec.nbytes == n * d * 8 and pk.nbytes == n * PM.slice_bytes(d)
    rec.setflags(write=False)
    pk.setflags(write=False)
    return rec, pk


@pytest.fixture
def switches():
    """every process-wide switch this module turns, back off afterwards"""
    from fltee import ecalls as EC
    EC.set_bubble_ecall(True)
    EC.set_upload_packed(True)
    try:
        yield EC
    finally:
        EC.set_upload_packed(False)
        EC.set_bubble_ecall(False)
        EC.set_upload_aead_policy("abort")
        EC.set_upload_aead(False)
        EC.set_path_oram_tree(False)
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


# ------------------------------------------------------- packed == records ----
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["staged", "pipelined"])
@pytest.mark.parametrize("alg", ALGS)
def test_packed_ecall_equals_the_records_ecall(enclave, switches, alg, shape):
    n, d = shape
    # what the request declares: a dense upload either way (nips19's threshold takes the
    # request's k: 0 keeps its dummies within bounds at d = 2^20)
    k = 0 if (alg == 2 and shape == LARGE) else d
    rec, pk = ctr_payloads(n, d)
    ids, fl, E = ids_of(n), 9000 + alg, enclave
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, rec, d, k, alg)   # an 8 d-byte dense upload: records
    assert (st, rv) == (0, 0)
    st, rv, out, times = fresh_call(switches, E, fl, ids, pk, d, k, alg)
    assert (st, rv) == (0, 0)
    assert same_bits(out, ref)
    assert ref.any() and np.isfinite(times).all() and times[0] > 0 and times.sum() > 0
    if alg in (3, 4, 5):
        v = values(n, d).cpu().numpy()
        assert same_bits(out, PM.inorder_mean(v))
    # the round advanced: round 0 is over, round 1 is answered
    st, rv, again, _ = E.ecall_secure_aggregation(fl, 0, ids, pk, d, k, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()
    if shape == SMALL:
        switches.set_debug_seed(SEED)
        assert E.ecall_start_round(fl, 1, n)[:2] == (0, 0)
        st, rv, out1, _ = E.ecall_secure_aggregation(fl, 1, ids, pk, d, k, alg)
        assert (st, rv) == (0, 0) and (alg == 2 or same_bits(out1, ref))
        # the records call is what it is with the switch off
        switches.set_upload_packed(False)
        st, rv, off, _ = fresh_call(switches, E, fl, ids, rec, d, k, alg)
        assert (st, rv) == (0, 0) and same_bits(off, ref)


def test_packed_alg5_takes_the_tree_when_switched_on(enclave, switches):
    n, d = SMALL
    rec, pk = ctr_payloads(n, d)
    switches.set_path_oram_tree(True)
    ids, E = ids_of(n), enclave
    st, rv, ref, _ = fresh_call(switches, E, 9010, ids, rec, d, d, 5)
    assert (st, rv) == (0, 0)
    tr = traced(lambda: fresh_call(switches, E, 9010, ids, pk, d, d, 5))
    assert any("oram" in line for line in tr) and any("unpack_dense_kernel" in line for line in tr)
    st, rv, out, _ = fresh_call(switches, E, 9010, ids, pk, d, d, 5)
    assert (st, rv) == (0, 0) and same_bits(out, ref)


# -------------------------------------- records through a switched-on server ----
@pytest.mark.parametrize("alg", [1, 4])
def test_sparse_uploads_are_answered_as_before(enclave, switches, oracle, alg):
    """a k = d / 2 sparse upload has exactly a packed slice's bytes; its request says k"""
    from fltee import client as C
    n, d = SMALL
    k = d // 2
    ids, E = ids_of(n), enclave
    enc = C.produce_payloads(values(n, d), ids, k=k).cpu().numpy()
    assert enc.nbytes == n * PM.slice_bytes(d)
    st, rv, on, _ = fresh_call(switches, E, 9020 + alg, ids, enc, d, k, alg)
    switches.set_upload_packed(False)
    st2, rv2, off, _ = fresh_call(switches, E, 9020 + alg, ids, enc, d, k, alg)
    assert (st, rv) == (st2, rv2) == (0, 0) and same_bits(on, off) and off.any()


def test_switch_off_reads_a_packed_sized_payload_as_records(enclave, switches, oracle):
    """the same k = d / 2 records under a request that declares a dense upload (k_req = d):
    off, they are summed as the records they are (what every earlier version did); on, the
    bytes are taken for packed values"""
    import torch

    from fltee import client as C
    from fltee import device as D
    n, d = SMALL
    k = d // 2
    ids, E = ids_of(n), enclave
    rec = C.zero_except_top_k_weights(values(n, d), k)
    idx, val = D.unpack_records(rec.cpu().numpy())
    want, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0
    enc = C.encrypt_parameters(rec, ids).cpu().numpy()
    switches.set_upload_packed(False)
    st, rv, off, _ = fresh_call(switches, E, 9030, ids, enc, d, d, 4)
    assert (st, rv) == (0, 0) and same_bits(off, want)
    switches.set_upload_packed(True)
    st, rv, on, _ = fresh_call(switches, E, 9030, ids, enc, d, d, 4)
    assert (st, rv) == (0, 0) and not same_bits(on, off)
    rows = rec.view(torch.float32).reshape(n, 2 * k).cpu().numpy()
    assert same_bits(on, PM.inorder_mean(rows[:, :d]))


# ----------------------------------------------------------------------- AEAD ----
def auth_packed(v, ids, fl, round_, alg, packed=True):
    from fltee import client as C
    return C.encrypt_parameters_auth(C.pack_dense(v), ids, fl, round_, alg, packed=packed).cpu().numpy()


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("d", [1026, 1027])
def test_packed_authenticated_call_verifies_and_tampers_do_not(enclave, switches, alg, d):
    from fltee import client as C
    n = 6
    ids, E, fl = ids_of(n), enclave, 9100 + alg
    v = values(n, d, 1)
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, C.produce_payloads(v, ids).cpu().numpy(), d, d, alg)
    assert (st, rv) == (0, 0)
    switches.set_upload_aead(True)
    good = auth_packed(v, ids, fl, 0, alg)
    stride = PM.slice_bytes(d) + 16
    assert good.nbytes == n * stride
    flipped = good.copy()
    flipped[2 * stride + 100] ^= 0x10
    moved = good.copy()
    moved[:stride], moved[stride:2 * stride] = good[stride:2 * stride], good[:stride]
    no_bit = auth_packed(v, ids, fl, 0, alg, packed=False)  # sealed as if the slices were records
    start(E, fl, ids, d, d, alg)
    for what, bad in (("flipped bit", flipped), ("no format bit", no_bit), ("moved slice", moved)):
        st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, bad, d, d, alg)
        assert (st, rv) == (0, MAC_MISMATCH), what
        assert not out.view(np.uint32).any() and np.isfinite(times).all()
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, good, d, d, alg)  # the round was kept
    assert (st, rv) == (0, 0) and same_bits(out, ref)
    # the other way round: records sealed with the format bit never sum as records
    rec = C.serialize_dense(v)
    start(E, fl, ids, d, d, alg)
    bad = C.encrypt_parameters_auth(rec, ids, fl, 0, alg, packed=True).cpu().numpy()
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, bad, d, d, alg)
    assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
    ok = C.encrypt_parameters_auth(rec, ids, fl, 0, alg).cpu().numpy()
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, ok, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(out, ref)


def drop_case(EC, E, fl, alg, n, d, failed):
    """(out of the DROP call with `failed` tampered, out of the packed ECALL on the survivors)"""
    ids = ids_of(n)
    v = values(n, d, 2)
    keep = [c for c in range(n) if c not in failed]
    EC.set_upload_aead(True)
    EC.set_upload_aead_policy("drop")
    enc = auth_packed(v, ids, fl, 0, alg).copy()
    stride = PM.slice_bytes(d) + 16
    for c in failed:
        enc[c * stride + 8 * c + 5] ^= 1
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, d, alg)
    st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert E.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    ids_s = ids[keep]
    enc_s = auth_packed(v[keep].contiguous(), ids_s, fl + 1, 0, alg)
    EC.set_debug_seed(SEED)
    start(E, fl + 1, ids_s, d, d, alg)
    st, rv, ref, _ = E.ecall_secure_aggregation(fl + 1, 0, ids_s, enc_s, d, d, alg)
    assert (st, rv) == (0, 0)
    return out, ref


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("d", [1026, 1027])
def test_drop_equals_the_packed_ecall_on_the_survivors(enclave, switches, alg, d):
    out, ref = drop_case(switches, enclave, 9200 + 10 * alg, alg, 6, d, [0, 3])
    assert same_bits(out, ref) and ref.any()
    if alg == 3:
        v = values(6, d, 2).cpu().numpy()[[1, 2, 4, 5]]
        assert same_bits(out, PM.inorder_mean(v))


# -------------------------------------------------------------- virtual ranks ----
@pytest.mark.parametrize("alg", [1, 3])
def test_two_virtual_ranks_equal_the_one_gpu_eid(enclave, switches, alg):
    from fltee.ecalls import Enclave
    n, d = 6, 1026
    ids = ids_of(n)
    _, pk = ctr_payloads(n, d)
    st, rv, ref, _ = fresh_call(switches, enclave, 9300 + alg, ids, pk, d, d, alg)
    assert (st, rv) == (0, 0)
    drop_ref, _ = drop_case(switches, enclave, 9310 + 10 * alg, alg, n, d, [2])
    switches.set_upload_aead(False)
    G = Enclave([0, 0])
    try:
        assert G.device_count() == 2
        st, rv, out, times = fresh_call(switches, G, 9300 + alg, ids, pk, d, d, alg)
        assert (st, rv) == (0, 0) and same_bits(out, ref) and np.isfinite(times).all()
        drop_out, drop_survivors = drop_case(switches, G, 9310 + 10 * alg, alg, n, d, [2])
        assert same_bits(drop_out, drop_ref) and same_bits(drop_survivors, drop_ref)
    finally:
        G.destroy()


# ---------------------------------------------------------------------- trace ----
def syncs(trace):
    return sum(1 for line in trace if line.startswith("sync|"))


@pytest.mark.parametrize("alg", [1, 3])
def test_small_packed_call_trace(enclave, switches, alg):
    """the staged packed call: the same trace whatever the values, and exactly the records
    call's host synchronisations; a records call's trace does not see the switch"""
    from fltee import client as C
    n, d = SMALL
    ids, E, fl = ids_of(n), enclave, 9400 + alg
    rec, pk = ctr_payloads(n, d)
    zeros = C.produce_payloads(values(n, d) * 0, ids, packed=True).cpu().numpy()
    fresh_call(switches, E, fl, ids, pk, d, d, alg)  # the shape's scratch
    fresh_call(switches, E, fl, ids, rec, d, d, alg)
    t_pk = traced(lambda: fresh_call(switches, E, fl, ids, pk, d, d, alg))
    t_zero = traced(lambda: fresh_call(switches, E, fl, ids, zeros, d, d, alg))
    t_rec = traced(lambda: fresh_call(switches, E, fl, ids, rec, d, d, alg))
    assert_same_trace(t_pk, t_zero, "packed: random vs all-zero values")
    assert syncs(t_pk) == syncs(t_rec) == 1
    switches.set_upload_packed(False)
    t_off = traced(lambda: fresh_call(switches, E, fl, ids, rec, d, d, alg))
    assert_same_trace(t_rec, t_off, "records: the switch on vs off")
    name = "dense_accumulate_p" if alg == 3 else "unpack_dense_kernel"
    assert any(name in line for line in t_pk) and not any(name in line for line in t_rec)


@pytest.mark.parametrize("alg", [1, 3])
def test_authenticated_packed_call_trace(enclave, switches, alg):
    """random, all-zero and tampered payloads: one trace up to the verdict (a tampered call
    ends there)"""
    n, d = 6, 1027
    ids, E, fl = ids_of(n), enclave, 9500 + alg
    v = values(n, d, 3)
    switches.set_upload_aead(True)
    a = auth_packed(v, ids, fl, 0, alg)
    z = auth_packed(v * 0, ids, fl, 0, alg)
    bad = a.copy()
    bad[3 * (PM.slice_bytes(d) + 16) + 9] ^= 2
    assert fresh_call(switches, E, fl, ids, a, d, d, alg)[:2] == (0, 0)
    t_a = traced(lambda: fresh_call(switches, E, fl, ids, a, d, d, alg))
    t_z = traced(lambda: fresh_call(switches, E, fl, ids, z, d, d, alg))
    t_bad = traced(lambda: fresh_call(switches, E, fl, ids, bad, d, d, alg))
    assert_same_trace(t_a, t_z, "authenticated packed: random vs all-zero values")
    assert 0 < len(t_bad) < len(t_a)
    assert_same_trace(t_bad, t_a[:len(t_bad)], "authenticated packed: tampered, up to the verdict")
    assert fresh_call(switches, E, fl, ids, bad, d, d, alg)[1] == MAC_MISMATCH
