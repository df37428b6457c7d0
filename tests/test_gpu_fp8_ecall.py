"""fp8 dense uploads through ecall_secure_aggregation (fltee_set_upload_fp8): the switch off
answering an fp8-sized payload as every earlier version did; on, [out] bit for bit the records
ECALL on the dequantised values for algs 3, 4, 5, 1 and 7, plain and authenticated; one server
answering all four formats; the format bit of the AAD against the other three; DROP on the
survivors alone; fltee_set_dense_trim(500) on an fp8 call with a client under a NaN scale; and the
launch trace of three uploads of one shape."""
import functools

import numpy as np
import pytest

import bf16_model as BM
import fp8_model as FM
import packed_model as PM
import trim_model as TM
from conftest import gpu_available
from test_gpu_oblivious import assert_same_trace, traced

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

MAC_MISMATCH = 0x3001
SHAPES = [(5, 13), (7, 1031)]
ALGS = [3, 4, 5, 1, 7]
SEED = 0xF17EE5EED


def ids_of(n, base=700):
    return np.arange(base, base + n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def host_values(n, d, seed=0):
    """(f32 values as a client holds them, their fp8 rows, the values the rows stand for): built
    once, never modified"""
    v = PM.values(np.random.default_rng(seed + d), n, d)
    r = FM.pack(v)
    x = FM.unpack(r, d)
    assert np.isfinite(x).all() and x.any()
    for a in (v, r, x):
        a.setflags(write=False)
    return v, r, x


def cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def ctr_payloads(n, d, seed=0):
    """(records, packed, bf16, fp8) payloads as host bytes: the fp8 slices of the values (the
    producer's), and the dequantised values as records and as packed slices; the bf16 payload is
    of the dequantised values narrowed once more (another upload of its own)"""
    from fltee import client as C
    v, r, x = host_values(n, d, seed)
    ids = ids_of(n)
    rec = C.produce_payloads(cuda(x), ids).cpu().numpy()
    pk = C.produce_payloads(cuda(x), ids, packed=True).cpu().numpy()
    bf = C.produce_payloads(cuda(x), ids, bf16=True).cpu().numpy()
    f8 = C.produce_payloads(cuda(v), ids, fp8=True).cpu().numpy()
    assert (rec.nbytes, pk.nbytes, bf.nbytes, f8.nbytes) == (n * d * 8, n * PM.slice_bytes(d), n * BM.slice_bytes(d),
                                                            n * FM.slice_bytes(d))
    for a in (rec, pk, bf, f8):
        a.setflags(write=False)
    return rec, pk, bf, f8


@pytest.fixture
def switches():
    """every process-wide switch this module turns, back off afterwards"""
    from fltee import ecalls as EC
    EC.set_upload_fp8(True)
    EC.set_bubble_ecall(True)
    try:
        yield EC
    finally:
        EC.set_upload_fp8(False)
        EC.set_upload_bf16(False)
        EC.set_upload_packed(False)
        EC.set_bubble_ecall(False)
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


# ---------------------------------------------------------- the switch off ----
def test_switch_off_answers_an_fp8_sized_payload_as_before(enclave, switches, oracle):
    """k = P + 1 records are exactly an fp8 slice's bytes.  Under a request that declares a dense
    upload (k_req = d): off, algs 3 and 4 sum them as the records they are and alg 1 refuses a
    fold longer than the payload (0x2) — what every earlier version did; on, the bytes are taken
    for fp8 codes and their scale.  Under a request that says k = P + 1 they are records either way."""
    from fltee import client as C
    from fltee import device as D
    n, d = 7, 1031
    k = FM.units(d)
    ids, E = ids_of(n), enclave
    v = cuda(PM.values(np.random.default_rng(d), n, d))
    rec = C.zero_except_top_k_weights(v, k)
    idx, val = D.unpack_records(rec.cpu().numpy())
    want, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0
    enc = C.encrypt_parameters(rec, ids).cpu().numpy()
    assert enc.nbytes == n * FM.slice_bytes(d)
    switches.set_upload_fp8(False)
    off = {}
    for alg in (3, 4):
        st, rv, off[alg], _ = fresh_call(switches, E, 9930 + alg, ids, enc, d, d, alg)
        assert (st, rv) == (0, 0) and same_bits(off[alg], want)
    t_off = traced(lambda: fresh_call(switches, E, 9934, ids, enc, d, d, 4))
    assert not any("fp8" in line or "accumulate_q" in line for line in t_off)
    st, rv, out, _ = fresh_call(switches, E, 9931, ids, enc, d, d, 1)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any()
    st, rv, sparse_off, _ = fresh_call(switches, E, 9932, ids, enc, d, k, 4)
    assert (st, rv) == (0, 0) and same_bits(sparse_off, want)
    switches.set_upload_fp8(True)
    st, rv, sparse_on, _ = fresh_call(switches, E, 9932, ids, enc, d, k, 4)
    assert (st, rv) == (0, 0) and same_bits(sparse_on, want)
    rows = rec.cpu().numpy().view(np.uint8).reshape(n, FM.row(d))
    for alg in (3, 4, 1):
        st, rv, on, _ = fresh_call(switches, E, 9930 + alg, ids, enc, d, d, alg)
        assert (st, rv) == (0, 0) and not same_bits(on, want)
        if alg != 1:
            assert FM.same_bits(on, FM.inorder_mean(rows, d))


# ----------------------------------------------------------- fp8 == records ----
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("alg", ALGS)
def test_fp8_ecall_equals_the_records_ecall(enclave, switches, alg, n, d):
    rec, _, _, f8 = ctr_payloads(n, d)
    ids, fl, E = ids_of(n), 9600 + alg, enclave
    for k in (d, 0):  # what the request declares: a dense upload either way
        if k == 0 and alg in (1, 7):
            continue  # (advanced and alg 7 fold over the request's k)
        st, rv, ref, _ = fresh_call(switches, E, fl, ids, rec, d, k, alg)   # 8 d bytes: records
        assert (st, rv) == (0, 0)
        st, rv, out, times = fresh_call(switches, E, fl, ids, f8, d, k, alg)
        assert (st, rv) == (0, 0)
        assert same_bits(out, ref)
        assert ref.any() and np.isfinite(times).all() and times.sum() > 0
        if alg in (3, 4, 5):
            assert same_bits(out, FM.inorder_mean(host_values(n, d)[1], d))
    # the round advanced: round 0 is over
    st, rv, again, _ = E.ecall_secure_aggregation(fl, 0, ids, f8, d, d, alg)
    assert (st, rv) == (0, 2) and not again.view(np.uint32).any()


def auth(rows_or_rec, ids, fl, alg, **fmt):
    from fltee import client as C
    return C.encrypt_parameters_auth(rows_or_rec, ids, fl, 0, alg, **fmt).cpu().numpy()


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("alg", ALGS)
def test_authenticated_fp8_ecall_equals_the_records_ecall(enclave, switches, alg, n, d):
    from fltee import client as C
    ids, E, fl = ids_of(n), enclave, 9700 + alg
    v, r, x = host_values(n, d, 1)
    switches.set_upload_aead(True)
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, auth(C.serialize_dense(cuda(x)), ids, fl, alg), d, d, alg)
    assert (st, rv) == (0, 0)
    good = auth(C.pack_dense_fp8(cuda(v)), ids, fl, alg, fp8=True)
    assert good.nbytes == n * (FM.slice_bytes(d) + 16)
    st, rv, out, times = fresh_call(switches, E, fl, ids, good, d, d, alg)
    assert (st, rv) == (0, 0) and same_bits(out, ref) and ref.any() and np.isfinite(times).all()


# ------------------------------------------------------------- four formats ----
@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES)
def test_one_server_answers_all_four_formats(enclave, switches, alg, n, d):
    rec, pk, bf, f8 = ctr_payloads(n, d)
    ids, E, fl = ids_of(n), enclave, 9840 + alg
    switches.set_upload_fp8(False)
    st, rv, ref, _ = fresh_call(switches, E, fl, ids, rec, d, d, alg)  # as every earlier version
    assert (st, rv) == (0, 0) and ref.any()
    st, rv, ref_bf, _ = fresh_call(switches, E, fl, ids, C_records_of_bf16(n, d), d, d, alg)
    assert (st, rv) == (0, 0)
    switches.set_upload_fp8(True)
    switches.set_upload_bf16(True)
    switches.set_upload_packed(True)
    for turn in range(2):
        for what, enc, want in (("records", rec, ref), ("packed", pk, ref), ("bf16", bf, ref_bf), ("fp8", f8, ref)):
            st, rv, out, _ = fresh_call(switches, E, fl, ids, enc, d, d, alg)
            assert (st, rv) == (0, 0), what
            assert same_bits(out, want), what


def C_records_of_bf16(n, d):
    """the records payload of the bf16 upload's widened values"""
    from fltee import client as C
    x = host_values(n, d)[2]
    return C.produce_payloads(cuda(BM.unpack(BM.pack(x), d)), ids_of(n)).cpu().numpy()


@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES)
def test_a_slice_sealed_for_one_format_verifies_under_no_other(enclave, switches, alg, n, d):
    from fltee import client as C
    ids, E, fl = ids_of(n), enclave, 9720 + alg
    v, r, x = host_values(n, d, 1)
    switches.set_upload_aead(True)
    switches.set_upload_packed(True)
    switches.set_upload_bf16(True)
    dx = cuda(x)
    rows, bf, pk, rec = C.pack_dense_fp8(cuda(v)), C.pack_dense_bf16(dx), C.pack_dense(dx), C.serialize_dense(dx)
    good = {"fp8": auth(rows, ids, fl, alg, fp8=True), "records": auth(rec, ids, fl, alg),
            "packed": auth(pk, ids, fl, alg, packed=True)}
    bad = {"fp8 slices sealed as records": auth(rows, ids, fl, alg),
           "fp8 slices sealed as packed": auth(rows, ids, fl, alg, packed=True),
           "fp8 slices sealed as bf16": auth(rows, ids, fl, alg, bf16=True),
           "records sealed as fp8": auth(rec, ids, fl, alg, fp8=True),
           "packed slices sealed as fp8": auth(pk, ids, fl, alg, fp8=True),
           "bf16 slices sealed as fp8": auth(bf, ids, fl, alg, fp8=True)}
    stride = FM.slice_bytes(d) + 16
    flipped = good["fp8"].copy()
    flipped[2 * stride + stride - 16 - 7] ^= 0x10  # (a bit of client 2's scale)
    bad["a flipped bit"] = flipped
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


# ----------------------------------------------------------------------- DROP ----
@pytest.mark.parametrize("alg", [1, 3])
@pytest.mark.parametrize("n,d", SHAPES)
def test_drop_equals_the_fp8_ecall_on_the_survivors(enclave, switches, alg, n, d):
    """one tampered client: the survivors' rows are gathered as P + 1 units per client"""
    from fltee import client as C
    EC, E, fl, failed = switches, enclave, 9800 + 10 * alg, [2]
    ids = ids_of(n)
    v, r, _ = host_values(n, d, 2)
    keep = [c for c in range(n) if c not in failed]
    EC.set_upload_aead(True)
    EC.set_upload_aead_policy("drop")
    enc = auth(C.pack_dense_fp8(cuda(v)), ids, fl, alg, fp8=True).copy()
    stride = FM.slice_bytes(d) + 16
    for c in failed:
        enc[c * stride + (8 * c + 5) % (stride - 16)] ^= 1
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, d, alg)
    st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isfinite(times).all()
    assert E.auth_report(fl) == (0, [int(ids[c]) for c in failed])
    ids_s = ids[keep]
    enc_s = auth(C.pack_dense_fp8(cuda(v[keep])), ids_s, fl + 1, alg, fp8=True)
    EC.set_debug_seed(SEED)
    start(E, fl + 1, ids_s, d, d, alg)
    st, rv, ref, _ = E.ecall_secure_aggregation(fl + 1, 0, ids_s, enc_s, d, d, alg)
    assert (st, rv) == (0, 0)
    assert same_bits(out, ref) and ref.any()
    if alg == 3:  # (a client's slice depends on its own values alone)
        assert same_bits(out, FM.inorder_mean(r[keep], d))


# ----------------------------------------------------------------------- trim ----
@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("n,d", SHAPES)
def test_the_median_of_an_fp8_call_trims_a_nan_scale_away(enclave, switches, alg, n, d):
    from fltee import client as C
    codes, s = FM.split(host_values(n, d)[1], d)
    s = s.copy()
    s[1] = np.nan
    r = FM.pack_codes(codes, s)
    x = FM.unpack(r, d)
    assert np.isnan(x[1]).all()
    ids = ids_of(n)
    enc = C.encrypt_parameters(cuda(r), ids).cpu().numpy()
    t = TM.trim_count(n, 500)
    assert t == (n - 1) // 2
    switches.set_dense_trim(500)
    st, rv, out, _ = fresh_call(switches, enclave, 9860 + alg, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0)
    want = TM.trimmed(x, t)
    assert np.isfinite(want).all() and same_bits(out, want)
    switches.set_dense_trim(0)
    st, rv, off, _ = fresh_call(switches, enclave, 9860 + alg, ids, enc, d, d, alg)
    assert (st, rv) == (0, 0) and np.isnan(off).all()  # the untrimmed mean is that client's


def test_trim_refuses_what_it_refused_and_not_an_fp8_call(enclave, switches):
    """alg 1 cannot be trimmed, whatever the format: 0x2, never an untrimmed mean"""
    n, d = SHAPES[0]
    f8 = ctr_payloads(n, d)[3]
    switches.set_dense_trim(100)
    st, rv, out, _ = fresh_call(switches, enclave, 9870, ids_of(n), f8, d, d, 1)
    assert (st, rv) == (0, 2) and not out.view(np.uint32).any()


# ---------------------------------------------------------------------- trace ----
@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("alg", [3, 1])
def test_the_launch_trace_does_not_depend_on_the_upload(enclave, switches, alg, aead):
    """random, all-equal and NaN-laden uploads of one shape: one trace, the fp8 kernels in it"""
    from fltee import client as C
    n, d = SHAPES[1]
    ids, E, fl = ids_of(n), enclave, 9880 + alg
    rng = np.random.default_rng(3)
    equal = FM.pack(np.full((n, d), 0.25, np.float32))
    codes = rng.integers(0, 256, (n, d), dtype=np.uint16).astype(np.uint8)
    codes[:, ::3] = 0x7F
    s = np.ones(n, np.float32)
    s[0], s[1], s[2] = np.nan, np.inf, 0.0
    uploads = [FM.random_rows(rng, n, d), equal, FM.pack_codes(codes, s)]
    switches.set_upload_aead(aead)

    def seal(r):
        if aead:
            return auth(cuda(r), ids, fl, alg, fp8=True)
        return C.encrypt_parameters(cuda(r), ids).cpu().numpy()
    encs = [seal(r) for r in uploads]
    for enc in encs:  # warm: code objects loaded, every buffer grown
        assert fresh_call(switches, E, fl, ids, enc, d, d, alg)[:2] == (0, 0)
    traces = [traced(lambda enc=enc: fresh_call(switches, E, fl, ids, enc, d, d, alg)) for enc in encs]
    if alg == 3:
        assert any("dense_accumulate_q" in line for line in traces[0])
        assert not any("unpack" in line for line in traces[0])
    else:
        assert any("unpack_fp8_kernel" in line for line in traces[0])
    for other in traces[1:]:
        assert_same_trace(traces[0], other, f"alg {alg} aead={aead}")
