"""The counting sort and the ordered fold of fl-tee_amd/csrc/k_radix.hip in numpy, and the
constructed inputs of tests/test_gpu_radix.py (checked on the CPU by
tests/test_radix_model.py).  Test infrastructure only.

Records are uint64: low 32 bits the u32 idx, high 32 bits the f32 val's bits
(fltee.device.pack_records).

cs_plan          (passes, width) of the counting sort for d, as k_radix.hip states it.
stable_sorted    the records in order of min(idx, d), upload order within a key.
composite_sorted the order under fltee_debug_set_radix_order(0): by (idx, position) — the
                 same for every idx < d; the records with idx >= d come by idx, not by position.
ordered          the enclave's loop g[idx] += val over idx < d in list order, x coef.
runs_layout      a list whose sorted form has runs of chosen lengths at chosen positions,
                 handed over in a chosen upload order.
values           membership / association / mirror / general, per sorted position.
ordered_reversed, ordered_chunked   two WRONG folds; test_radix_model.py proves with them
                 that the association values tell a reordered or re-associated run apart.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
BIG = np.float32(2.0 ** 24)
VALUE_SETS = ("membership", "association", "mirror", "general")
# k_radix.hip: a sort tile, the fold's chunk, wave (kFoldCh chunks) and preload (one more)
TILE, CHUNK, WAVE, PRELOAD = 2048, 64, 256, 320


def cs_plan(d):
    b = 1
    while b < 32 and (1 << b) <= d:  # keys 0 .. d (d: out of range)
        b += 1
    passes = (b + 7) // 8
    return passes, (b + passes - 1) // passes


def pack(idx, val):
    idx = np.ascontiguousarray(idx, np.uint32)
    val = np.ascontiguousarray(val, np.float32)
    return idx.astype(np.uint64) | (val.view(np.uint32).astype(np.uint64) << np.uint64(32))


def rec_idx(rec):
    return (rec & MASK).astype(np.int64)


def rec_val(rec):
    return (rec >> np.uint64(32)).astype(np.uint32).view(np.float32)


def stable_sorted(rec, d):
    return rec[np.argsort(np.minimum(rec_idx(rec), d), kind="stable")]


def composite_sorted(rec):
    return rec[np.argsort(rec_idx(rec), kind="stable")]


def ordered(rec, d, coef):
    """NumpyRangeOps.ordered (np.add.at on f32 zeros, x f32(coef)) over the records with
    idx < d"""
    import torch

    from range_ops_np import NumpyRangeOps
    keep = np.ascontiguousarray(rec[rec_idx(rec) < d])
    return NumpyRangeOps().ordered(torch.from_numpy(keep.view(np.int64)), d, coef).numpy()


# ------------------------------------------------------------ wrong folds ----
def ordered_reversed(rec, d, coef):
    """every run folded back to front"""
    s = stable_sorted(rec, d)
    s = s[rec_idx(s) < d][::-1]
    return ordered(s[np.argsort(rec_idx(s), kind="stable")], d, coef)


def ordered_chunked(rec, d, c, coef):
    """the sorted records cut into pieces of c positions: each run's records inside a piece
    folded from +0.0, then the run's pieces folded from +0.0 in order"""
    s = stable_sorted(rec, d)
    s = s[rec_idx(s) < d]
    idx, val = rec_idx(s), rec_val(s)
    out = np.zeros(d, np.float32)
    if len(s) == 0:
        return out * np.float32(coef)
    piece = np.arange(len(s)) // c
    new = np.ones(len(s), bool)
    new[1:] = (idx[1:] != idx[:-1]) | (piece[1:] != piece[:-1])
    seg = np.cumsum(new) - 1
    part = np.zeros(seg[-1] + 1, np.float32)
    np.add.at(part, seg, val)
    np.add.at(out, idx[new], part)
    return out * np.float32(coef)


# ---------------------------------------------------------------- layouts ----
Layout = namedtuple("Layout", "d idx starts lengths nin order")


def filler(m):
    """run lengths 1, 2, 1, 3, 5, ... that add up to m"""
    out, i = [], 0
    while m > 0:
        out.append(min(m, (1, 2, 1, 3, 5)[i % 5]))
        m -= out[-1]
        i += 1
    return out


def oor_tail(m, d):
    """m indices >= d: d, d + 1, u32::MAX and u32::MAX - 1 mixed"""
    return [(d, d + 1, 0xFFFFFFFF, d, 0xFFFFFFFE, d + 1, d + 1)[i % 7] for i in range(m)]


def runs_layout(lengths, d, gaps=None, perm=None, tail=()):
    """A record list whose sorted form is: run j (lengths[j] records of index j * (gaps + 1))
    for every j, back to back from position 0, then the out-of-range indices `tail` in this
    order.  gaps: the unused indices between two used ones (None: as many as d allows).
    perm: a permutation of the sorted positions (None: the identity) — upload position p
    takes a record with the key of sorted record perm[p], each key's records kept in their
    sorted order, so that the stable sort by min(idx, d) returns the sorted form exactly.
    .idx: the sorted form's indices; .starts / .lengths: the runs; .nin: records with
    idx < d; .order[j]: the upload position of sorted record j."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    assert (lengths > 0).all() and all(t >= d for t in tail)
    runs = len(lengths)
    if gaps is None:
        gaps = max(d // runs - 1, 0) if runs else 0
    assert runs == 0 or (runs - 1) * (gaps + 1) < d
    idx = np.concatenate([np.repeat(np.arange(runs, dtype=np.int64) * (gaps + 1), lengths),
                          np.asarray(tail, np.int64)]).astype(np.uint32)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64) if runs else lengths
    n = len(idx)
    if perm is None:
        order = np.arange(n, dtype=np.int64)
    else:
        perm = np.asarray(perm, np.int64)
        assert np.array_equal(np.sort(perm), np.arange(n))
        order = np.argsort(np.minimum(idx.astype(np.int64), d)[perm], kind="stable")
    for a in (idx, starts, lengths, order):
        a.setflags(write=False)
    return Layout(d, idx, starts, lengths, int(lengths.sum()), order)


def values(name, lay):
    """the f32 value of every sorted position"""
    n = len(lay.idx)
    if name == "membership":
        return ((np.arange(n) % 1000) + 1).astype(np.float32)
    if name in ("association", "mirror"):
        v = np.ones(n, np.float32)
        v[lay.starts if name == "association" else lay.starts + lay.lengths - 1] = BIG
        return v
    assert name == "general"
    return (np.random.default_rng(n).normal(0, 1, n) * 100).astype(np.float32)


def upload(lay, val):
    """the records in upload order"""
    rec = np.empty(len(lay.idx), np.uint64)
    rec[lay.order] = pack(lay.idx, val)
    return rec


# the fold's layouts: name -> (lengths, d, gaps, tail length, claims); a claim is
# ("start", p): a run's first record at sorted position p; ("end", p): a run's last record
# at p - 1; ("oor", p): the first out-of-range record at p; ("n", p): p records in all
def _fold_specs():
    S = {}

    def add(name, lengths, d, claims, gaps=None, tail=0):
        S[name] = (tuple(lengths), d, gaps, tail, tuple(claims))

    ds = {1: 255, 2: 256, 63: 65535, 64: 65536, 65: 1 << 24, 256: 65536, 320: 256, 321: 65535, 384: 255}
    for L, d in ds.items():  # a run from position 0
        add(f"run{L}_at0", [L] + filler(100), d, [("start", 0), ("end", L)])
    add("ends_on_lane63_x4", filler(40) + [24] + filler(30) + [34] + filler(10) + [54] + filler(3) + [61]
        + filler(50), 65536, [("end", 64), ("end", 128), ("end", 192), ("end", 256)])
    for L, d in ((2, 65535), (66, 256), (130, 65536)):  # across the wave's end
        add(f"run{L}_at255", filler(255) + [L] + filler(60), d, [("start", 255), ("end", 255 + L)])
    for L, d in ((64, 255), (128, 65536), (129, 256)):  # to the wave's end, the preload's, one more
        add(f"run{L}_at192", filler(192) + [L] + filler(60), d, [("start", 192), ("end", 192 + L)])
    add("run3000_at700", filler(700) + [3000] + filler(100), 65536, [("start", 700), ("end", 3700)])
    # the last run ends at n; 1024 and 1025: inside the loop past the preload (832)
    for n, L in ((64, 20), (256, 100), (257, 3), (320, 130), (321, 131), (1024, 424), (1025, 425)):
        add(f"last_run_ends_at_n{n}", filler(n - L) + [L], 65535, [("start", n - L), ("end", n), ("n", n)])
    add("d1", [700], 1, [("start", 0), ("end", 700), ("n", 700)])
    add("d1_one_record", [1], 1, [("n", 1)])
    add("d7_every_index", [63, 64, 65, 1, 2, 130, 75], 7, [("end", 63), ("end", 127), ("start", 195)], gaps=0)
    f = filler(600)
    add("every_index_used", f, len(f), [("n", 600)], gaps=0)
    add("gap_between_indices", f, 2 * len(f) + 3, [("n", 600)], gaps=1)
    add("oor_on_chunk_lane0", filler(44) + [20], 65536, [("end", 64), ("oor", 64)], tail=70)
    add("oor_on_wave_lane0", filler(200) + [56], 65536, [("end", 256), ("oor", 256)], tail=70)
    add("oor_only", [], 300, [("oor", 0), ("n", 100)], tail=100)
    add("empty", [], 300, [("n", 0)])
    return S


FOLD_SPECS = _fold_specs()


def _perm(name, n):
    return np.random.default_rng(zlib.crc32(name.encode())).permutation(n)


@functools.lru_cache(maxsize=None)
def fold_layout(name, shuffled=True):
    lengths, d, gaps, tail, _ = FOLD_SPECS[name]
    t = oor_tail(tail, d)
    return runs_layout(lengths, d, gaps, _perm(name, sum(lengths) + tail) if shuffled else None, t)


# ------------------------------------------------- the sort's index patterns ----
SORT_N = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6145)
SORT_D = (1, 7, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)
PASS_SHAPES = dict(zip(SORT_D, ((1, 1), (1, 3), (1, 8), (2, 5), (2, 8), (3, 6), (3, 8), (4, 7))))
SORT_PATTERNS = ("one_index", "two_by_lane", "position_mod_digits", "later_digit_only",
                 "pass0_digit_only", "sorted", "reversed", "zeros_in_last_lanes", "out_of_range")


def _hash(p):
    return (p * 2654435761) % (1 << 32)


def sort_pattern(name, n, d):
    """n indices (int64) for the sort-alone test, or None where d has no such pattern"""
    passes, w = cs_plan(d)
    mask = (1 << w) - 1
    p = np.arange(n, dtype=np.int64)
    if name == "one_index":  # every tile, group and ballot holds one digit
        return np.full(n, d - 1)
    if name == "two_by_lane":
        return np.where(p % 2 == 0, d - 1, d // 2)
    if name == "position_mod_digits":
        return (p % (1 << w)) % d
    if name == "later_digit_only":  # pass 0 moves nothing: the order rests on the later passes
        if d >> w == 0:
            return None
        return ((_hash(p) % (d >> w)) << w) | (mask & 0x5B)  # < (d >> w) << w <= d
    if name == "pass0_digit_only":
        hi, lo = (d - 1) >> w, (d - 1) & mask
        if lo == 0 and hi > 0:
            hi, lo = hi - 1, mask
        return (hi << w) | (_hash(p) % (lo + 1))
    if name == "sorted":
        return p * d // n
    if name == "reversed":
        return (p * d // n)[::-1].copy()
    rng = np.random.default_rng(n * 31 + d % 1009)
    idx = rng.integers(min(1, d - 1), d, n)
    if name == "zeros_in_last_lanes":  # the dead lanes behind them carry record 0 too
        idx[max(n - 71, 0):] = 0
        idx[-1] = d - 1
        return idx
    assert name == "out_of_range"
    bad = np.array(oor_tail(n, d), np.int64)
    return np.where(_hash(p) % 3 == 0, bad, idx)


# ----------------------------------------- the routes that reach the same kernels ----
# name -> (alg, n, k, d, run lengths): n * k records, client-major in the shuffled order
ROUTE_SPECS = {
    # non_oblivious past the scatter rows (n * d > 2^24 cells): the run of 3000 over both clients
    "alg4_sort_path": (4, 2, 1900, (1 << 24) + 1, tuple(filler(700) + [3000] + filler(100))),
    # nips19: a run of 700 and short ones, every client repeating indices
    "alg2_repeats": (2, 12, 300, 3000, tuple(filler(500) + [700] + filler(2400))),
}


@functools.lru_cache(maxsize=None)
def route_layout(name):
    alg, n, k, d, lengths = ROUTE_SPECS[name]
    assert sum(lengths) == n * k
    return runs_layout(lengths, d, None, _perm(name, n * k))
