"""The robust dense aggregates (trimmed mean by lists and by selection, Multi-Krum, the geometric
median) sharded by column over a multi-GPU eid — virtual ranks, so one GPU runs everything.  All
comparisons are bit for bit: the carry chain's Gram matrix against the one-GPU pass for random f32
inputs (inexact sums: the order shows) and against the numpy model where it is exact; every ECALL
against the one-GPU eid and, at one shape each, the numpy models; the launches taken; the verdict
before any aggregation launch; the refusals; the switches off; no growth on a second call.
(An eid has a power of two of ranks — three devices are refused, tests/test_gpu_group.py — so the
ECALLs run on 2, 4 and 8 ranks; three ranges are covered by the chain entry.)"""
import functools

import numpy as np
import pytest

import gmed_model as GM
import krum_model as KM
import trim_model as TM
from conftest import gpu_available
from test_gpu_gmed_ecall import host_values as gmed_values
from test_gpu_krum_ecall import host_values as krum_values
from test_gpu_oblivious import assert_same_trace, traced
from test_gpu_trim_ecall import host_values as trim_values
from test_gpu_trim_ecall import ids_of, payload, same_bits, start
from test_gpu_trim_select_ecall import host_values as select_values

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

D = 1101
F, M, R, NU = 2, 5, 3, GM.NU
SEED = 0xC0FFEE5EED
MAT_BIT = 1 << 2  # engine.h Ws: kWsMat, the bit Krum's scratch grows under
# kind -> (clients, the values, what switches it on, the numpy model of [out])
KINDS = {
    "trim": (10, trim_values, lambda EC: EC.set_dense_trim(500), lambda v: TM.trimmed(v, TM.trim_count(len(v), 500))),
    "select": (131, select_values, lambda EC: (EC.set_dense_trim(500), EC.set_dense_trim_select(True)),
               lambda v: TM.trimmed(v, TM.trim_count(len(v), 500))),
    "krum": (10, krum_values, lambda EC: EC.set_dense_krum(F, M), lambda v: KM.krum(v, F, M)),
    "gmed": (10, gmed_values, lambda EC: EC.set_dense_gmed(R, NU), lambda v: GM.gmed(v, R, NU)),
}


@pytest.fixture
def switches():
    from fltee import ecalls as EC
    EC.set_upload_packed(True)
    try:
        yield EC
    finally:
        EC.set_dense_gmed(0, 0.0)
        EC.set_dense_krum(0, 0)
        EC.set_dense_trim_select(False)
        EC.set_dense_trim(0)
        EC.set_upload_packed(False)
        EC.set_upload_aead_policy("abort")
        EC.set_upload_aead(False)
        EC.set_debug_seed(0)


@pytest.fixture(scope="module")
def eids():
    """the one-GPU eid and eids of 2, 4 and 8 virtual ranks on the same GPU"""
    import torch

    from fltee.ecalls import Enclave
    torch.cuda.init()
    E = {w: Enclave(0 if w == 1 else [0] * w) for w in (1, 2, 4, 8)}
    assert [E[w].device_count() for w in (1, 2, 4, 8)] == [1, 2, 4, 8]
    yield E
    for e in E.values():
        e.destroy()


def fresh_call(EC, E, fl, ids, enc, d, alg):
    EC.set_debug_seed(SEED)
    start(E, fl, ids, d, d, alg)
    return E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)


@functools.lru_cache(maxsize=None)
def upload(kind, d, alg, aead, fl):
    n, values = KINDS[kind][0], KINDS[kind][1]
    v, ids = values(n, d), ids_of(n, 2000)
    return v, ids, payload(v, ids, False, (fl, 0, alg) if aead else None)


def launches(trace, name):
    """(grid.x, grid.y) of every launch whose site names `name`"""
    out = []
    for line in trace:
        what, site, a = line.split("|")[:3]
        if what == "launch" and name in site:
            out.append((int(a) >> 32, int(a) & 0xFFFFFFFF))
    return out


# ---------------------------------------------------------------- chain order ----
def records_of(v):
    import torch

    from fltee import device as dev
    n, d = v.shape
    idx = np.tile(np.arange(d, dtype=np.uint32), n)
    return torch.from_numpy(dev.pack_records(idx, v.reshape(-1))).cuda()


def rows_of(v):
    import torch

    from fltee import device as dev
    n, d = v.shape
    rows = np.zeros((n, dev.packed_row(d)), np.float32)
    rows[:, :d] = v
    return torch.from_numpy(rows).cuda()


def gram_ranges(t, n, d, ranks, packed):
    import torch

    from fltee import device as dev
    G = dev.krum_gram_ranges(t, n, d, ranks, packed=packed)
    torch.cuda.synchronize()
    return G.cpu().numpy()


@pytest.mark.parametrize("n,d,packed", [(10, 1101, False), (10, 200, False), (130, 1101, False),
                                         (17, 4099, False), (17, 4099, True)],
                         ids=["5chunks", "1chunk", "offdiag", "tail", "tail-packed"])
def test_the_chain_adds_in_the_one_gpu_order(n, d, packed):
    """random normal f32 values: the Gram entries are inexact sums, so another order shows in the
    bits; ranks = 1 is launch_krum_gram itself"""
    rng = np.random.default_rng(n * 7919 + d)
    v = rng.normal(0, 1, (n, d)).astype(np.float32)
    t = rows_of(v) if packed else records_of(v)
    one = gram_ranges(t, n, d, 1, packed)
    npad = (n + 15) // 16 * 16
    assert one.shape == (npad, npad) and np.array_equal(one, one.T)
    exact = v.astype(np.float64) @ v.astype(np.float64).T
    assert np.allclose(one[:n, :n], exact, rtol=1e-12, atol=1e-9) and not one[n:].any() and not one[:, n:].any()
    for ranks in (2, 3, 8):  # (10, 200): one chunk, the ranks before the last have none
        got = gram_ranges(t, n, d, ranks, packed)
        assert np.array_equal(got.view(np.uint64), one.view(np.uint64)), f"ranks={ranks}"
    # the same sums in the wrong association differ for these inputs (what the comparison can see)
    x = v.astype(np.float64)
    halves = x[:, : d // 2] @ x[:, : d // 2].T + x[:, d // 2:] @ x[:, d // 2:].T
    assert d < 512 or not np.array_equal(halves, exact)


@pytest.mark.parametrize("packed", [False, True], ids=["records", "packed"])
def test_the_chain_equals_the_model_where_it_is_exact(packed):
    n, d = 17, 4099
    v = np.random.default_rng(5).integers(-8, 9, (n, d)).astype(np.float32)
    t = rows_of(v) if packed else records_of(v)
    want = KM.gram(v)[0]
    for ranks in (1, 2, 3, 8):
        got = gram_ranges(t, n, d, ranks, packed)
        assert np.array_equal(got[:n, :n], want) and not got[n:].any() and not got[:, n:].any()


# --------------------------------------------------------------- ECALL parity ----
@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("alg", [3, 4, 5])
@pytest.mark.parametrize("kind", list(KINDS))
def test_sharded_ecall_returns_the_one_gpu_bits(eids, switches, kind, alg, aead):
    fl = 9300 + alg
    v, ids, enc = upload(kind, D, alg, aead, fl)
    switches.set_upload_aead(aead)
    KINDS[kind][2](switches)
    st, rv, ref, _ = fresh_call(switches, eids[1], fl, ids, enc, D, alg)
    assert (st, rv) == (0, 0)
    if alg == 3:  # the hostile client and the sealed NaNs are gone, by the model
        assert same_bits(ref, KINDS[kind][3](v)) and np.isfinite(ref).all()
    for w in (2, 4, 8):
        st, rv, out, times = fresh_call(switches, eids[w], fl, ids, enc, D, alg)
        assert (st, rv) == (0, 0) and np.isfinite(times).all(), f"W={w}"
        assert same_bits(out, ref), f"W={w}"
        # the round advanced
        st, rv, again, _ = eids[w].ecall_secure_aggregation(fl, 0, ids, enc, D, D, alg)
        assert (st, rv) == (0, 2) and not again.view(np.uint32).any()


@pytest.mark.parametrize("aead", [False, True], ids=["ctr", "aead"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_most_ranks_without_columns(eids, switches, kind, aead):
    """d = 7 on eight ranks: two ranks hold the columns of a trimmed call, one rank the only chunk"""
    d, alg, fl = 7, 3, 9310
    v, ids, enc = upload(kind, d, alg, aead, fl)
    switches.set_upload_aead(aead)
    KINDS[kind][2](switches)
    st, rv, ref, _ = fresh_call(switches, eids[1], fl, ids, enc, d, alg)
    assert (st, rv) == (0, 0) and same_bits(ref, KINDS[kind][3](v))
    st, rv, out, _ = fresh_call(switches, eids[8], fl, ids, enc, d, alg)
    assert (st, rv) == (0, 0) and same_bits(out, ref)


# ------------------------------------------------------------- the path taken ----
def test_a_krum_call_runs_one_gram_pass_per_rank_and_the_chain(eids, switches):
    n, fl, alg = 10, 9320, 3
    ids = ids_of(n, 2000)
    rnd = krum_values(n, D)
    equal = np.full((n, D), 0.25, np.float32)
    nans = rnd.copy()
    nans[::2] = np.nan
    nans[1::4] = -np.nan
    switches.set_dense_krum(F, M)
    fresh_call(switches, eids[2], fl, ids, payload(rnd, ids, False), D, alg)  # the shape's scratch
    tr = [traced(lambda v=v: fresh_call(switches, eids[2], fl, ids, payload(v, ids, False), D, alg))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    # 5 chunks of 256 columns over two ranks: 2 and 3 — not the root's whole pass of 5
    assert launches(tr[0], "krum_gram_kernel") == [(1, 2), (1, 3)]
    assert len(launches(tr[0], "krum_reduce_carry_kernel")) == 2
    assert not launches(tr[0], "krum_reduce_kernel")
    assert len(launches(tr[0], "krum_score_kernel")) == 1 == len(launches(tr[0], "krum_rank_kernel"))
    assert len(launches(tr[0], "krum_accumulate_kernel")) == 2
    # every rank copied its own columns, 512 and 589 of them, and nobody the whole payload
    copies = [line.split("|") for line in tr[0] if line.startswith("memcpy2d|")]
    assert sorted(int(c[2]) for c in copies) == [512 * 8, 589 * 8] and all(int(c[3]) == n for c in copies)
    assert not any(line.startswith("memcpy|") and int(line.split("|")[2]) == n * D * 8 for line in tr[0])
    # the one-GPU eid's route, for contrast
    one = traced(lambda: fresh_call(switches, eids[1], fl, ids, payload(rnd, ids, False), D, alg))
    assert launches(one, "krum_gram_kernel") == [(1, 5)] and len(launches(one, "krum_reduce_kernel")) == 1
    assert not launches(one, "krum_reduce_carry_kernel")


def test_a_trimmed_call_trims_on_every_rank(eids, switches):
    n, fl, alg = 10, 9321, 3
    ids = ids_of(n, 2000)
    rnd = trim_values(n, D)
    equal = np.full((n, D), 0.25, np.float32)
    nans = np.array(rnd)
    nans[::2] = np.nan
    switches.set_dense_trim(500)
    fresh_call(switches, eids[2], fl, ids, payload(rnd, ids, False), D, alg)
    tr = [traced(lambda v=v: fresh_call(switches, eids[2], fl, ids, payload(v, ids, False), D, alg))
          for v in (rnd, equal, nans)]
    assert_same_trace(tr[0], tr[1], "random vs all-equal values")
    assert_same_trace(tr[0], tr[2], "random vs NaN-laden values")
    assert len(launches(tr[0], "trimmed_mean_kernel")) == 2 and not launches(tr[0], "dense_accumulate")
    copies = [line.split("|") for line in tr[0] if line.startswith("memcpy2d|")]
    assert sorted(int(c[2]) for c in copies) == [548 * 8, 553 * 8]  # the cuts (d i / W) & ~3
    assert not any(line.startswith("memcpy|") and int(line.split("|")[2]) == n * D * 8 for line in tr[0])
    one = traced(lambda: fresh_call(switches, eids[1], fl, ids, payload(rnd, ids, False), D, alg))
    assert len(launches(one, "trimmed_mean_kernel")) == 1


# --------------------------------------------------------------- verdict first ----
AGG = ("krum_gram", "krum_reduce", "krum_score", "krum_accumulate", "gmed_", "trimmed_mean", "trim_select",
       "dense_accumulate")


@pytest.mark.parametrize("kind", ["trim", "krum", "gmed"])
def test_abort_stops_before_any_aggregation_launch(eids, switches, kind):
    alg, fl = 3, 9330
    v, ids, enc = upload(kind, D, alg, True, fl)
    bad = enc.copy()
    stride = bad.nbytes // len(ids)
    bad[6 * stride + 8 * 700 + 5] ^= 1  # one bit of client 6, in the second rank's columns
    switches.set_upload_aead(True)
    KINDS[kind][2](switches)
    out = []
    tr = traced(lambda: out.append(fresh_call(switches, eids[2], fl, ids, bad, D, alg)))
    st, rv, res, _ = out[0]
    assert (st, rv) == (0, 0x3001) and not res.view(np.uint32).any()
    assert any("ghash" in line for line in tr)
    assert not any(line.startswith("launch") and any(k in line for k in AGG) for line in tr)
    # the round was kept: the untampered upload is answered
    st, rv, res, _ = eids[2].ecall_secure_aggregation(fl, 0, ids, enc, D, D, alg)
    assert (st, rv) == (0, 0) and same_bits(res, KINDS[kind][3](v))


@pytest.mark.parametrize("kind", ["trim", "krum", "gmed"])
def test_drop_aggregates_the_survivors_as_one_gpu_does(eids, switches, kind):
    alg, fl = 3, 9331
    v, ids, enc = upload(kind, D, alg, True, fl)
    bad = enc.copy()
    stride = bad.nbytes // len(ids)
    bad[6 * stride + 8 * 700 + 5] ^= 1
    switches.set_upload_aead(True)
    switches.set_upload_aead_policy("drop")
    KINDS[kind][2](switches)
    st, rv, ref, _ = fresh_call(switches, eids[1], fl, ids, bad, D, alg)
    assert (st, rv) == (0, 0) and eids[1].auth_report(fl) == (0, [int(ids[6])])
    st, rv, out, _ = fresh_call(switches, eids[2], fl, ids, bad, D, alg)
    assert (st, rv) == (0, 0) and same_bits(out, ref) and eids[2].auth_report(fl) == (0, [int(ids[6])])
    assert same_bits(out, KINDS[kind][3](np.delete(v, 6, axis=0)))


# -------------------------------------------------------------------- refusals ----
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_record_out_of_position_is_refused_on_both_eids(eids, switches, kind):
    import torch

    from fltee import client as C
    n, d, alg, fl = KINDS[kind][0], 258, 4, 9340
    v, ids = KINDS[kind][1](n, d), ids_of(n, 2000)
    rec = C.serialize_dense(torch.from_numpy(np.array(v, np.float32)).cuda()).reshape(n, d).clone()
    rec[2, [200, 201]] = rec[2, [201, 200]]  # client 2: two records swapped, in the last rank's columns
    enc = C.encrypt_parameters(rec.reshape(-1), ids).cpu().numpy()
    for w in (1, 2):
        KINDS[kind][2](switches)
        tr = []
        res = []
        tr = traced(lambda: res.append(fresh_call(switches, eids[w], fl, ids, enc, d, alg)))
        st, rv, out, times = res[0]
        assert (st, rv) == (0, 2) and not out.view(np.uint32).any() and np.isfinite(times).all(), f"W={w}"
        assert not any("scatter" in line or "fold_sorted" in line for line in tr)  # never a plain rerun
        # the round was kept: with the switches off the same request is answered
        switches.set_dense_gmed(0, 0.0), switches.set_dense_krum(0, 0)
        switches.set_dense_trim_select(False), switches.set_dense_trim(0)
        st, rv, out, _ = eids[w].ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
        assert (st, rv) == (0, 0), f"W={w}"


def test_too_few_clients_are_refused_on_both_eids(eids, switches):
    n, d, fl = 6, 258, 9341
    v, ids = krum_values(n, d, 2), ids_of(n, 2000)
    enc = payload(v, ids, False)
    switches.set_dense_krum(2, 1)  # n < 2 f + 3 = 7
    for w in (1, 2):
        st, rv, out, _ = fresh_call(switches, eids[w], fl, ids, enc, d, 3)
        assert (st, rv) == (0, 2) and not out.view(np.uint32).any(), f"W={w}"


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_packed_upload_stays_on_the_root(eids, switches, kind):
    n, values = KINDS[kind][0], KINDS[kind][1]
    v, ids, fl = values(n, D), ids_of(n, 2000), 9342
    enc = payload(v, ids, True)
    KINDS[kind][2](switches)
    st, rv, ref, _ = fresh_call(switches, eids[1], fl, ids, enc, D, 3)
    assert (st, rv) == (0, 0) and same_bits(ref, KINDS[kind][3](v))
    out = []
    tr = traced(lambda: out.append(fresh_call(switches, eids[2], fl, ids, enc, D, 3)))
    assert out[0][:2] == (0, 0) and same_bits(out[0][2], ref)
    assert not any(line.startswith("memcpy2d|") for line in tr)  # no column shards
    assert not launches(tr, "krum_reduce_carry_kernel")


# ---------------------------------------------------------------- switches off ----
def test_switches_off_is_the_plain_group_call(eids, switches):
    n, fl = 10, 9350
    v, ids = krum_values(n, D), ids_of(n, 2000)
    enc = payload(v, ids, False)
    st, rv, ref, _ = fresh_call(switches, eids[1], fl, ids, enc, D, 3)
    assert (st, rv) == (0, 0)
    fresh_call(switches, eids[2], fl, ids, enc, D, 3)
    out = []
    before = traced(lambda: out.append(fresh_call(switches, eids[2], fl, ids, enc, D, 3)[2]))
    switches.set_dense_krum(F, M)
    on = traced(lambda: fresh_call(switches, eids[2], fl, ids, enc, D, 3))
    switches.set_dense_krum(0, 0)
    after = traced(lambda: out.append(fresh_call(switches, eids[2], fl, ids, enc, D, 3)[2]))
    assert_same_trace(before, after, "never switched on vs switched off again")
    assert same_bits(out[0], ref) and same_bits(out[1], ref)
    assert not any(k in line for line in before for k in ("krum", "gmed", "trim"))
    assert len(launches(before, "dense_accumulate")) >= 2 and launches(on, "krum_reduce_carry_kernel")


# ------------------------------------------------------------------- no growth ----
@pytest.mark.parametrize("kind", ["krum", "gmed"])
def test_a_second_call_allocates_nothing(switches, kind):
    from fltee import _lib as L
    from fltee.ecalls import Enclave
    alg, fl = 3, 9360
    v, ids, enc = upload(kind, D, alg, False, fl)
    KINDS[kind][2](switches)
    G = Enclave([0, 0])  # a fresh eid: its ranks' buffers are empty
    try:
        L.lib().fltee_debug_scratch_grown()
        st, rv, first, _ = fresh_call(switches, G, fl, ids, enc, D, alg)
        assert (st, rv) == (0, 0) and L.lib().fltee_debug_scratch_grown() & MAT_BIT
        st, rv, second, _ = fresh_call(switches, G, fl, ids, enc, D, alg)
        assert (st, rv) == (0, 0) and L.lib().fltee_debug_scratch_grown() == 0
        assert same_bits(first, second) and same_bits(first, KINDS[kind][3](v))
    finally:
        G.destroy()
