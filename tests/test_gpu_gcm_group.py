"""Authenticated uploads on a multi-GPU eid: GHASH sharded by window (k_ghash.hip, group.hip).

Pieces: a slice set cut into W column windows where group_dense_ecall cuts it; per window
fltee_ghash_window_device equals the host twin byte for byte, merge + finish accept the good
slices and fail exactly the tampered client, and fltee_decrypt_slice_auth_device's windows
concatenated are fltee_decrypt_auth_device's records.  ECALLs on virtual ranks [0, 0] and
[0, 0, 0, 0] (every rank on one device): the bits of Enclave(0) for dense algs 3 and 4, alg 6,
and algs 1 and 7 at shapes the group does not decline; a tamper in every rank's share, swapped
slices, a replayed round and an alg downgrade are 0x3001 with a zero [out] and the round kept.
Trace: the windowed kernel once per rank, no host copy of the whole payload, the same lines
through the fail-word readback for any payload, and nothing behind it after a failure."""
import ctypes

import numpy as np
import pytest

import gcm_model as M
from conftest import gpu_available
from test_gpu_gcm_ecall import MAC_MISMATCH, auth_payload, call, flip, records, start, swapped
from test_gpu_oblivious import assert_same_trace, traced

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

TIDS = np.array([7, 260, 65535], np.uint32)
AAD_LEN = 16


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
    from fltee.ecalls import Enclave
    es = {1: Enclave(0), 2: Enclave([0, 0]), 4: Enclave([0, 0, 0, 0])}
    try:
        yield es
    finally:
        for e in es.values():
            e.destroy()


@pytest.fixture
def aead_on():
    from fltee.ecalls import set_upload_aead
    set_upload_aead(True)
    try:
        yield
    finally:
        set_upload_aead(False)


def cuts(d, W):
    """group_dense_ecall's partition in records: p_i = (d i / W) & ~3, p_W = d"""
    return [(d * i // W) & ~3 for i in range(W)] + [d]


# ------------------------------------------------------------------------- the pieces ----
_slices = {}


def slices(dev, ids, d):
    """(ciphertext || tag rows on the device, the same on the host, aad): built once per shape"""
    import torch

    from fltee import client as C
    key = (tuple(int(i) for i in ids), d)
    if key not in _slices:
        n = len(ids)
        idx = np.tile(np.arange(d, dtype=np.uint32), n)
        val = np.random.default_rng(d).normal(0, 0.01, n * d).astype(np.float32)
        rec = torch.from_numpy(dev.pack_records(idx, val)).cuda()
        aad = b"".join(M.aad_of(int(c), AAD_LEN) for c in ids)
        enc = C.encrypt_parameters_gcm(rec, ids, M.IV, aad)
        host = enc.cpu().numpy()
        host.setflags(write=False)
        _slices[key] = (enc, host, aad)
    return _slices[key]


def host_part(lib, cid, aad, with_aad, ct, first_block, win_bytes):
    P = lib.fltee_gcm_segments(len(ct), AAD_LEN)
    out = (ctypes.c_uint8 * (16 * P))()
    lo = 16 * first_block
    w = bytes(ct[lo:lo + win_bytes])
    st = lib.fltee_debug_ghash_window_host(cid, (ctypes.c_uint8 * AAD_LEN)(*aad), AAD_LEN, 1 if with_aad else 0,
                                           (ctypes.c_uint8 * max(len(w), 1))(*w), len(ct), first_block,
                                           win_bytes, out)
    assert st == 0
    return np.frombuffer(bytes(out), np.uint8).reshape(P, 16)


def windows(enc, d, W):
    """the W column windows carved on the device, each contiguous: row stride dg * 8"""
    p = cuts(d, W)
    return p, [enc[:, p[i] * 8:p[i + 1] * 8].contiguous() for i in range(W)]


def window_parts(dev, ids, wins, p, d, aad):
    return [dev.ghash_window(ids, w, (p[i + 1] - p[i]) * 8, d * 8, p[i] // 2, (p[i + 1] - p[i]) * 8, aad,
                             aad_len=AAD_LEN, with_aad=(i == 0)) for i, w in enumerate(wins)]


def verdict(dev, ids, parts, d, tags):
    acc = parts[0].clone()
    for part in parts[1:]:
        dev.ghash_merge(acc, part)
    fail = dev.gcm_finish(ids, acc, d * 8, M.IV, AAD_LEN, tags).cpu().numpy()
    return fail, dev.status()


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("d", [1101, 4099])
def test_window_pieces_equal_the_host_twin_and_the_whole_slices(dev, d, W):
    import torch

    from fltee import _lib as L
    lib = L.lib()
    n, B = len(TIDS), d * 8
    enc, host, aad = slices(dev, TIDS, d)
    p, wins = windows(enc, d, W)
    assert all(w.shape == (n, (p[i + 1] - p[i]) * 8) for i, w in enumerate(wins))
    parts = window_parts(dev, TIDS, wins, p, d, aad)
    P = dev.gcm_segments(B, AAD_LEN)
    assert P == -(-((B + 15) // 16 + 1) // M.S) and P >= 2
    for i, part in enumerate(parts):
        got = part.cpu().numpy()
        assert got.shape == (n, P, 16)
        for c, cid in enumerate(TIDS):
            want = host_part(lib, int(cid), aad[16 * c:16 * c + 16], i == 0, host[c, :B], p[i] // 2,
                             (p[i + 1] - p[i]) * 8)
            assert np.array_equal(got[c], want), f"window {i}, client {cid}"
    tags = enc[:, B:].contiguous()
    fail, st = verdict(dev, TIDS, parts, d, tags)
    assert not fail.any() and st == 0
    # the merged vector is the whole slice's: the model's tag from it, for one client
    whole = dev.ghash_window(TIDS, enc, B + 16, B, 0, B, aad, aad_len=AAD_LEN, with_aad=True)
    acc = parts[0].clone()
    for part in parts[1:]:
        dev.ghash_merge(acc, part)
    assert torch.equal(acc, whole)
    # one flipped bit inside window 1 of client 1: that client alone
    bad = [w.clone() for w in wins]
    bad[1][1, bad[1].shape[1] // 2] ^= 0x10
    fail, st = verdict(dev, TIDS, window_parts(dev, TIDS, bad, p, d, aad), d, tags)
    assert fail.tolist() == [0, 1, 0] and st == L.DEV_ERR_AUTH
    # ... or in its tag
    bad_tags = tags.clone()
    bad_tags[1, 15] ^= 0x80
    fail, st = verdict(dev, TIDS, parts, d, bad_tags)
    assert fail.tolist() == [0, 1, 0] and st == L.DEV_ERR_AUTH
    # the CTR half per window, concatenated: the whole slices' records
    rec, f0 = dev.decrypt_auth(TIDS, enc.reshape(-1), B, M.IV, aad)
    assert not f0.cpu().numpy().any() and dev.status() == 0
    cols = [dev.decrypt_slice_auth(TIDS, w, (p[i + 1] - p[i]) * 8, p[i] // 2, (p[i + 1] - p[i]) * 8, M.IV)
            for i, w in enumerate(wins)]
    assert torch.equal(torch.cat(cols, dim=1), rec.reshape(n, d))


def test_window_pieces_with_empty_windows(dev):
    """n = 2, d = 6 on W = 4: the cuts are 0, 0, 0, 4, 6 — two empty windows, the first of them
    carrying the AAD"""
    import torch
    ids, d, W = TIDS[:2], 6, 4
    enc, host, aad = slices(dev, ids, d)
    p, wins = windows(enc, d, W)
    assert p == [0, 0, 0, 4, 6] and [w.shape[1] for w in wins] == [0, 0, 32, 16]
    parts = window_parts(dev, ids, wins, p, d, aad)
    assert parts[0].any() and not parts[1].any()
    tags = enc[:, d * 8:].contiguous()
    fail, st = verdict(dev, ids, parts, d, tags)
    assert not fail.any() and st == 0
    bad = [w.clone() for w in wins]
    bad[3][1, 15] ^= 1
    fail, st = verdict(dev, ids, window_parts(dev, ids, bad, p, d, aad), d, tags)
    assert fail.tolist() == [0, 1] and st == 0x10
    rec, _ = dev.decrypt_auth(ids, enc.reshape(-1), d * 8, M.IV, aad)
    cols = [dev.decrypt_slice_auth(ids, w, w.shape[1], p[i] // 2, w.shape[1], M.IV) for i, w in enumerate(wins)]
    assert torch.equal(torch.cat(cols, dim=1), rec.reshape(2, d))
    assert dev.status() == 0


# --------------------------------------------------------------------------- the ECALLs ----
N, D, K = 8, 300, 30
IDS = np.arange(500, 500 + N, dtype=np.uint32)
# alg 1: L = 8 * 600 + 3000 = 7800 in M = 2^13, C = 2^12 / 2^11 >= 16 W (group_advanced's bound)
# alg 7: L = 8 * 2500 + 3000 = 23000 in M = 2^15, C = 2^14 / 2^13 >= 2^12 (group_bubble's bound)
# (both: more than M / 2 records, so the second of two ranks loads clients too)
ECALL_CASES = [
    ("alg3_dense_1101", 3, 3, 1101, 1101),
    ("alg3_dense_4099", 3, 3, 4099, 4099),
    ("alg4_dense", 4, 3, 1101, 1101),
    ("alg6", 6, N, D, K),
    ("alg1", 1, N, 3000, 600),
    ("alg7", 7, N, 3000, 2500),
]
_fl = [9000]
_ecall_cases = {}


def ecall_case(oracle, enclaves, name):
    """-> (alg, ids, d, k, fl, payload, Enclave(0)'s answer): built once, never modified"""
    if name not in _ecall_cases:
        _, alg, n, d, k = next(c for c in ECALL_CASES if c[0] == name)
        ids = TIDS if n == 3 else IDS
        idx, val = records(n, d, k, 31 * alg + d)
        _fl[0] += 1
        fl = _fl[0]
        enc = auth_payload(oracle, idx, val, ids, fl, 0, alg)
        enc.setflags(write=False)
        start(enclaves[1], fl, ids, d, k, alg)
        st, rv, one, _ = call(enclaves[1], fl, 0, ids, enc, d, k, alg)
        assert (st, rv) == (0, 0)
        one.setflags(write=False)
        _ecall_cases[name] = (alg, ids, d, k, fl, enc, one)
    return _ecall_cases[name]


@pytest.fixture
def bubble_on():
    from fltee.ecalls import set_bubble_ecall
    set_bubble_ecall(True)
    try:
        yield
    finally:
        set_bubble_ecall(False)


def launches(trace, kernel):
    return sum(1 for line in trace if line.startswith(f"launch|{kernel}"))


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("name", [c[0] for c in ECALL_CASES])
def test_group_aead_ecall_has_the_one_gpu_bits(oracle, enclaves, aead_on, bubble_on, name, W):
    alg, ids, d, k, fl, enc, one = ecall_case(oracle, enclaves, name)
    E = enclaves[W]
    n = len(ids)

    def run():
        start(E, fl, ids, d, k, alg)
        st, rv, out, times = call(E, fl, 0, ids, enc, d, k, alg)
        assert (st, rv) == (0, 0) and np.isfinite(times).all()
        return out

    assert np.array_equal(run().view(np.uint32), one.view(np.uint32))
    if alg in (1, 7):
        # the group did not decline: every range was built and sorted by its own rank, and
        # every rank that loaded clients verified them itself
        tr = traced(run)
        nrec, L = n * k, n * k + d
        C = (1 << (L - 1).bit_length()) // W
        assert C >= {1: 16 * W, 7: 1 << 12}[alg]
        loaders = sum(1 for r in range(W) if r * C < nrec)
        assert loaders >= 2
        assert launches(tr, "ghash_finish_kernel<false>") == loaders
        assert launches(tr, "ghash_bulk_kernel<") == loaders
        if alg == 1:
            assert launches(tr, "advanced_init_kernel") == W
        else:
            assert launches(tr, "stable_tile_sort_kernel") >= sum(1 for r in range(W) if r * C < L) >= 2


@pytest.mark.parametrize("W", [2, 4])
def test_group_aead_dense_tampers_are_mac_mismatches(oracle, enclaves, aead_on, W):
    """a flipped bit in every rank's window (and in a tag), swapped slices, another alg's
    payload: 0x3001, [out] zero, the round kept; the good payload is then answered; its replay
    in the next round is refused, the next round's payload answered"""
    alg, ids, d, k, fl, good, one = ecall_case(oracle, enclaves, "alg3_dense_1101")
    E = enclaves[W]
    n, stride = len(ids), d * 8 + 16
    p = cuts(d, W)
    idx, val = records(n, d, k, 31 * alg + d)
    bad = [(f"rank {i}'s window", flip(good, stride, i % n, p[i] * 8 + 5, 0x20)) for i in range(W)]
    bad += [(f"rank {i}'s last byte", flip(good, stride, (i + 1) % n, p[i + 1] * 8 - 1, 0x80)) for i in range(W)]
    bad += [("a tag", flip(good, stride, 2, d * 8 + 7)),
            ("two clients' slices swapped", swapped(good, stride)),
            ("alg downgrade", auth_payload(oracle, idx, val, ids, fl, 0, 4))]
    start(E, fl, ids, d, k, alg)
    for what, enc in bad:
        st, rv, out, times = E.ecall_secure_aggregation(fl, 0, ids, enc, d, k, alg)
        assert (st, rv) == (0, MAC_MISMATCH), what
        assert not out.view(np.uint32).any(), what
        assert np.isfinite(times).all()
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 0, ids, good, d, k, alg)
    assert (st, rv) == (0, 0) and np.array_equal(out.view(np.uint32), one.view(np.uint32))
    assert E.ecall_start_round(fl, 1, n)[:2] == (0, 0)
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 1, ids, good, d, k, alg)
    assert (st, rv) == (0, MAC_MISMATCH) and not out.view(np.uint32).any()
    r1 = auth_payload(oracle, idx, val, ids, fl, 1, alg)
    st, rv, out, _ = E.ecall_secure_aggregation(fl, 1, ids, r1, d, k, alg)
    assert (st, rv) == (0, 0) and np.array_equal(out.view(np.uint32), one.view(np.uint32))


@pytest.mark.parametrize("W", [2, 4])
@pytest.mark.parametrize("name", ["alg1", "alg6"])
def test_group_aead_client_range_tampers_are_mac_mismatches(oracle, enclaves, aead_on, name, W):
    """position ranges (alg 1) and batches (alg 6): a tamper in a client of the first rank and
    in one of the last rank that loads clients, and another alg's payload"""
    alg, ids, d, k, fl, good, one = ecall_case(oracle, enclaves, name)
    E = enclaves[W]
    n, stride = len(ids), k * 8 + 16
    idx, val = records(n, d, k, 31 * alg + d)
    start(E, fl, ids, d, k, alg)
    for what, enc in [("first client", flip(good, stride, 0, 9, 2)),
                      ("last client", flip(good, stride, n - 1, k * 8 - 1, 0x40)),
                      ("last client's tag", flip(good, stride, n - 1, k * 8 + 3)),
                      ("two clients' slices swapped", swapped(good, stride)),
                      ("alg downgrade", auth_payload(oracle, idx, val, ids, fl, 0, 7 - alg))]:
        st, rv, out, _ = call(E, fl, 0, ids, enc, d, k, alg)
        assert (st, rv) == (0, MAC_MISMATCH), what
        assert not out.view(np.uint32).any(), what
    st, rv, out, _ = call(E, fl, 0, ids, good, d, k, alg)
    assert (st, rv) == (0, 0) and np.array_equal(out.view(np.uint32), one.view(np.uint32))


# ----------------------------------------------------------------------------- the trace ----
def test_group_aead_dense_trace(oracle, enclaves, aead_on):
    """[0, 0], dense alg 3, n = 5, d = 3000"""
    n, d, alg, W = 5, 3000, 3, 2
    ids = np.arange(40, 40 + n, dtype=np.uint32)
    E = enclaves[W]
    _fl[0] += 1
    fl = _fl[0]
    idx, val = records(n, d, d, 123)
    rnd = auth_payload(oracle, idx, val, ids, fl, 0, alg)
    one_index = auth_payload(oracle, np.full(n * d, 3, np.uint32), val, ids, fl, 0, alg)
    tampered = flip(rnd, d * 8 + 16, 3, cuts(d, W)[1] * 8 + 100, 8)  # in rank 1's window

    def run(enc, want):
        start(E, fl, ids, d, d, alg)
        st, rv, _, _ = E.ecall_secure_aggregation(fl, 0, ids, enc, d, d, alg)
        assert (st, rv) == (0, want)

    run(rnd, 0)  # the shape's scratch
    run(one_index, 0)
    good = traced(lambda: run(rnd, 0))
    assert launches(good, "ghash_window_kernel<") == W, "the windowed GHASH kernel: once per rank"
    assert launches(good, "ghash_bulk_kernel<") == 0
    whole = n * (d * 8 + 16)
    assert not any(t.startswith(f"memcpy||{whole}|1|") for t in good), "a host copy of the whole payload"
    assert sum(1 for t in good if t.startswith(f"memcpy2d||{d * 8 // W}|{n}|1")) == W
    # the readback of the one auth word follows the finish: a 4-byte D2H copy and the sync
    fin = next(i for i, t in enumerate(good) if t.startswith("launch|ghash_finish_kernel<false>"))
    assert good[fin + 1].startswith("memcpy||4|2|") and good[fin + 2].startswith("sync|")
    assert not any(t.startswith("launch|dense_") or "accumulate" in t for t in good[:fin + 3])
    assert any("accumulate" in t for t in good[fin + 3:])
    through = fin + 3
    assert_same_trace(good[:through], traced(lambda: run(one_index, 0))[:through], "one-index payload")
    bad = traced(lambda: run(tampered, MAC_MISMATCH))
    assert_same_trace(good[:through], bad, "tampered payload: the same lines, and nothing behind them")
