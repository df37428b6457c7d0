"""aggregation_alg 7 over a multi-GPU enclave id: the stable network sharded by position range
(k_stable.hip's range kernels, group.hip group_bubble) behind the unchanged ECALL.

Ranks are virtual (Enclave([0] * w): every range on one GPU, the exchanges device copies), as
in tests/test_gpu_group.py; [0] alone opens a one-rank RCCL communicator.  Covered:

  * the five range pieces driven range by range (fltee.parallel.distributed_stable_network,
    exchanges as copies of the partner range) against fltee_stable_sort_device on the whole
    array, bit for bit: C = 2^12 (no in-range register pass), 2^13 and 2^14 (one pass of R = 1,
    R = 2), three exchange stages, the pad boundary mid-tile, mid-range and whole pad ranges;
  * the ECALL on 2, 4, 8 virtual ranks and one RCCL rank against the one-GPU eid and the
    oracle's in-order sum, bit for bit;
  * the sharded path is the one taken (the launch trace: the exchange count by the formula,
    every pass range-sized), a declined shape falls back with the same bits, the trace does
    not depend on the data, a long run across the ranges sums exactly, a ragged payload and
    DP noise equal the one-GPU eid's.

Every case holds at most 2^17 records.  References are built once and left unchanged."""
import functools

import numpy as np
import pytest

from conftest import gpu_available
from stable_model import bits_equal, distinct_indices
from stable_range_np import init_range16
from test_gpu_oblivious import KINDS, assert_same_trace, traced, uploads

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

ALG_BUBBLE = 7
SEED = 0x7A11


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@pytest.fixture(scope="module")
def enclaves():
    import torch
    torch.cuda.init()
    from fltee.ecalls import Enclave, set_bubble_ecall
    es = {1: Enclave(0), "rccl1": Enclave([0])}
    for w in (2, 4, 8):
        es[w] = Enclave([0] * w)
    set_bubble_ecall(True)
    try:
        yield es
    finally:
        set_bubble_ecall(False)
        for e in es.values():
            e.destroy()


# ------------------------------------------------------------ pieces against the whole --
VALIDS = ["M", "M-1", "M/2+1", "M/2+C/2+3"]


@pytest.mark.parametrize("vkind", VALIDS)
@pytest.mark.parametrize("M,W", [(1 << 13, 2), (1 << 14, 4), (1 << 15, 8), (1 << 16, 4)])
def test_range_pieces_equal_the_whole_network(dev, M, W, vkind):
    import torch

    from fltee import parallel as P
    C = M // W
    valid = {"M": M, "M-1": M - 1, "M/2+1": M // 2 + 1, "M/2+C/2+3": M // 2 + C // 2 + 3}[vkind]
    rng = np.random.default_rng(M + valid)
    d = valid // 4
    nrec = valid - d
    idx = rng.integers(0, d + d // 8 + 1, nrec).astype(np.uint32)   # some idx >= d
    val = rng.normal(0, 0.01, nrec).astype(np.float32)
    rec = torch.from_numpy(dev.pack_records(idx, val)).cuda()
    # init: every range from the records at its own positions (the pointer at position r * C)
    chunks = {}
    for r in range(W):
        lo = min(r * C, nrec)
        chunks[r] = dev.stable_init_range(rec[lo:] if lo < nrec else rec[:1], nrec, d, r * C, C)
        want = init_range16(idx, val, d, r * C, C)
        assert torch.equal(chunks[r].cpu(), want), f"init of range {r}"
    whole = torch.cat([chunks[r] for r in range(W)]).contiguous()
    dev.stable_sort(whole)
    out = P.distributed_stable_network(chunks, W, M, P.DeviceRangeOps(), P.VirtualRanks(W), valid=valid)
    got = torch.cat([out[r] for r in range(W)])
    assert torch.equal(got, whole), "the ranges concatenated differ from the whole-array network"
    # strip: (idx, val) of every record, a pad as (u32::MAX, +0.0)
    stripped = torch.cat([dev.stable_range_strip(out[r]) for r in range(W)]).cpu().numpy().view(np.uint64)
    w = whole.cpu().numpy().view(np.uint64)
    assert np.array_equal(stripped, (w[:, 0] >> np.uint64(32)) | ((w[:, 1] & np.uint64(0xFFFFFFFF)) << np.uint64(32)))
    assert np.all(stripped[valid:] == np.uint64(0xFFFFFFFF))
    assert dev.status() == 0


# ---------------------------------------------------------------------- the ECALL -------
SHAPES = [(8, 1500, 5000), (64, 512, 600), (4, 4000, 500), (16, 3000, 20000)]
_fl = [7700]


def ecall(E, ids, enc, d, k, dp=0, seed=SEED):
    from fltee.ecalls import set_debug_seed
    _fl[0] += 1
    set_debug_seed(seed)
    try:
        assert E.ecall_fl_init(_fl[0], ids, d, k, 1.12, 1.0, 0.1, 1.0, ALG_BUBBLE, 0, dp) == (0, 0)
        assert E.ecall_start_round(_fl[0], 0, len(ids))[:2] == (0, 0)
        st, rv, out, times = E.ecall_secure_aggregation(_fl[0], 0, ids, enc, d, k, ALG_BUBBLE)
    finally:
        set_debug_seed(0)
    assert (st, rv) == (0, 0)
    assert np.isfinite(times).all()
    return out


def encrypt(oracle, idx, val, n, k, first_id=500):
    ids = np.arange(first_id, first_id + n, dtype=np.uint32)
    w = oracle.as_weights(idx, val).reshape(n, k)
    return ids, oracle.encrypt_clients(ids, [w[c].tobytes() for c in range(n)])


_cases = {}


def case(oracle, enclaves, shape):
    """shape -> (ids, ciphertext, the oracle's in-order sum, the one-GPU eid's output)"""
    if shape not in _cases:
        n, k, d = shape
        rng = np.random.default_rng(n * 1000003 + k)
        if k <= d:
            idx = distinct_indices(rng, n, k, d)
            val = rng.normal(0, 0.01, n * k).astype(np.float32)
        else:
            # more records than parameters: a client has to repeat indices (each k / d times
            # here), so runs exceed n + 1 entries and the fold re-associates them at its walk
            # boundaries — small integers, exact under any association (as test_gpu_alg7.py's
            # repeat_int), keep "the in-order sum, bit for bit" a property of the input
            idx = np.concatenate([rng.permutation(np.arange(k) % d) for _ in range(n)]).astype(np.uint32)
            val = rng.integers(-8, 9, n * k).astype(np.float32)
        ids, enc = encrypt(oracle, idx, val, n, k)
        ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
        assert st == 0
        one = ecall(enclaves[1], ids, enc, d, k)
        ref.setflags(write=False)
        one.setflags(write=False)
        _cases[shape] = (ids, enc, ref, one)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("w", [2, 4, 8, "rccl1"])
def test_group_ecall_alg7_bit_identical(enclaves, oracle, w, shape):
    n, k, d = shape
    ids, enc, ref, one = case(oracle, enclaves, shape)
    if shape == (4, 4000, 500) and w == 8:  # ranges 5..7 are pads alone
        L, C = n * k + d, (1 << 15) // 8
        assert L == 16500 and 4 * C < L <= 5 * C
    grp = ecall(enclaves[w], ids, enc, d, k)
    assert bits_equal(grp, one)
    assert bits_equal(grp, ref)


def bytes_lines(trace):
    """(kernel, accounted bytes) of every accounted launch of a trace"""
    return [(f[1], int(f[2])) for f in (line.split("|") for line in trace) if f[0] == "bytes"]


def exchange_launches(trace):
    return sum(1 for line in trace if line.startswith("launch|stable_exchange_kernel|"))


def test_group_ecall_alg7_takes_the_sharded_path(enclaves, oracle):
    """The w = 4 ECALL at (16, 3000, 20000): L = 68,000 in M = 2^17, C = 2^15.  The trace holds
    sum over s = log2 C + 1 .. log2 M of (s - log2 C) * #{r : r C < roundup(L, 2^s)} exchange
    launches, and every pass is range-sized: no launch of the network in place (tile sort,
    register pass, tile merge: 32 B per record) nor anything else accounts more than 32 C
    bytes — on one GPU they account up to 32 M.  The exchange is accounted, as specified, at
    its three 16-byte streams per record (two loads, one store): exactly 48 C, the one
    figure above 32 C; it is checked as an equality instead."""
    shape = (16, 3000, 20000)
    n, k, d = shape
    ids, enc, ref, one = case(oracle, enclaves, shape)
    W, L = 4, n * k + d
    M = 1 << (L - 1).bit_length()
    C = M // W
    clog, mlog = C.bit_length() - 1, M.bit_length() - 1
    assert (M, C) == (1 << 17, 1 << 15)
    ecall(enclaves[W], ids, enc, d, k)  # the shape's scratch
    tr = traced(lambda: ecall(enclaves[W], ids, enc, d, k))
    want = sum((s - clog) * sum(1 for r in range(W) if r * C < min(M, -(-L // (1 << s)) * (1 << s)))
               for s in range(clog + 1, mlog + 1))
    assert want == 12
    assert exchange_launches(tr) == want
    acc = bytes_lines(tr)
    assert any(kname == "stable_tile_sort" for kname, _ in acc), "the stable network did not run"
    for kname, b in acc:
        if kname == "stable_exchange":
            assert b == 48 * C, (kname, b)
        else:
            assert b <= 32 * C, (kname, b)
    assert sum(1 for kname, _ in acc if kname == "stable_exchange") == want


def test_group_ecall_alg7_declined_shape_runs_on_the_root(enclaves, oracle):
    """(4, 300, 500) at w = 8: C = 2^11 / 8 < 2^12, declined — the root runs it: the same
    bits, no exchange launch."""
    n, k, d = 4, 300, 500
    rng = np.random.default_rng(4300500)
    idx = distinct_indices(rng, n, k, d)
    val = rng.normal(0, 0.01, n * k).astype(np.float32)
    ids, enc = encrypt(oracle, idx, val, n, k)
    ref, st = oracle.non_oblivious(oracle.as_weights(idx, val), d, n)
    assert st == 0
    one = ecall(enclaves[1], ids, enc, d, k)
    grp = ecall(enclaves[8], ids, enc, d, k)
    tr = traced(lambda: ecall(enclaves[8], ids, enc, d, k))
    assert bits_equal(grp, one) and bits_equal(grp, ref)
    assert any("stable_tile_sort_kernel" in line for line in tr)
    assert exchange_launches(tr) == 0


def test_group_ecall_alg7_trace_is_data_independent(enclaves, oracle):
    n, k, d = 16, 3000, 20000
    encs = []
    for i, kind in enumerate(KINDS):
        idx, val = uploads(np.random.default_rng(700 + i), n, d, k, kind)
        ids, enc = encrypt(oracle, idx, val, n, k)
        encs.append(enc)
    E = enclaves[4]
    ecall(E, ids, encs[0], d, k)  # the shape's scratch
    tr = [traced(lambda e=e: ecall(E, ids, e, d, k)) for e in encs]
    assert exchange_launches(tr[0]) == 12
    for t, kind in zip(tr[1:], KINDS[1:]):
        assert_same_trace(tr[0], t, f"alg 7 ECALL on 4 ranks, {kind}")


@pytest.mark.parametrize("w", [2, 8])
def test_group_ecall_alg7_long_run_across_ranges_exact(enclaves, oracle, w):
    """Every record on one index (tests/longrun.py all_one_index: a run of n k + 1 entries,
    far above n + 1, over 6 of the 8 ranges of M = 2^16) with exactly summable values: the
    carry through the ranges' totals gives bincount x 1f32/n bit for bit."""
    from longrun import assert_bits, exact_ref, exact_values, layout, run_span
    n, k, d = 16, 3000, 3000
    M = 1 << (n * k + d - 1).bit_length()
    assert M == 1 << 16
    idx, val = layout("all_one_index", n, k, d, boundary=M // 2, mid=n + 10), exact_values(n * k)
    s0 = run_span(idx, d, 7)
    assert s0[1] - s0[0] > 100 * (n + 1)
    assert (s0[1] - 1) // (M // 8) - s0[0] // (M // 8) + 1 == 6
    ids, enc = encrypt(oracle, idx, val, n, k, first_id=900)
    assert_bits(ecall(enclaves[w], ids, enc, d, k), exact_ref(idx, val, d, n))


@functools.lru_cache(maxsize=None)
def ragged(oracle):
    """client slices of 8 k + 3 bytes (lib.rs:305-306 floors bytes and records per client)"""
    rng = np.random.default_rng(77)
    n, k, d = 10, 1301, 4000   # L = 17,010 in M = 2^15: C = 2^13 on 4 ranks
    ids = np.arange(70, 70 + n, dtype=np.uint32)
    slices = []
    for i in ids:
        w = np.zeros(k, dtype=oracle.WEIGHT)
        w["idx"] = rng.permutation(d)[:k]
        w["val"] = rng.normal(0, 0.01, k).astype(np.float32)
        slices.append(oracle.aes128_ctr(oracle.session_key(int(i)), w.tobytes() + b"\x01\x02\x03"))
    return ids, b"".join(slices), n, k, d


def test_group_ecall_alg7_ragged_payload(enclaves, oracle):
    ids, enc, n, k, d = ragged(oracle)
    assert len(enc) == n * (8 * k + 3)
    one = ecall(enclaves[1], ids, enc, d, k)
    tr = traced(lambda: ecall(enclaves[4], ids, enc, d, k))
    assert exchange_launches(tr) > 0  # sharded, not declined
    assert bits_equal(ecall(enclaves[4], ids, enc, d, k), one)


def test_group_ecall_alg7_dp_same_seed_same_noise(enclaves, oracle):
    shape = (8, 1500, 5000)
    n, k, d = shape
    ids, enc, ref, one = case(oracle, enclaves, shape)
    one_dp = ecall(enclaves[1], ids, enc, d, k, dp=1, seed=4242)
    grp_dp = ecall(enclaves[4], ids, enc, d, k, dp=1, seed=4242)
    assert bits_equal(grp_dp, one_dp)
    assert not bits_equal(one_dp, one)  # the noise was added
