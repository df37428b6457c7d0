"""The counting sort and the ordered fold of k_radix.hip at constructed boundaries, bit for
bit against tests/radix_model.py (whose inputs tests/test_radix_model.py checks on the CPU).

The sort alone (fltee_debug_sort_records_device; every record's value bits are its upload
position): every n around a wave, a round of 256 and a tile of 2048, every pass shape from
(1, 1) to (4, 7), index patterns that fill tiles, groups and ballots with one digit, leave a
pass nothing to do, or put idx 0 in the last live lanes.  The (4, 8) shape needs d >= 2^28
(a 1 GB output for the fold) and is not run; neither is a list of >= 2^29 entries.

The fold (fltee_ordered_list_device, `out` pre-filled with NaNs): runs that end on lane 63
of each chunk, at the wave's end (256), the preload's end (320), one past either, at n, and
the first out-of-range record on lane 0 — each with the membership, association, mirror and
general values, in a shuffled and in the sorted upload order, under both settings of
fltee_debug_set_radix_order.  Then non_oblivious's sort path (with and without accumulate)
and nips19 on one constructed layout each, against the oracle."""
import functools
import zlib

import numpy as np
import pytest

import radix_model as M
from conftest import gpu_available

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")]

INDEX_RANGE = 0x2
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    import torch

    from fltee import device as D
    torch.cuda.init()
    return D


@pytest.fixture(params=[1, 0], ids=["counting_sort", "composite_order"])
def radix_order(request):
    """both settings of fltee_debug_set_radix_order, restored to 1"""
    from fltee import _lib as L
    L.lib().fltee_debug_set_radix_order(request.param)
    try:
        yield request.param
    finally:
        L.lib().fltee_debug_set_radix_order(1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def on_device(rec):
    import torch
    return torch.from_numpy(np.array(rec, np.uint64).view(np.int64)).cuda()  # (a writable copy)


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} differ, first at {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, want {want[bad[:5]].tolist()}"


# ------------------------------------------------------------------ the sort alone ----
@functools.lru_cache(maxsize=None)
def sort_cases(d):
    """(pattern, n, records in upload order, the stable order, the composite order): the value
    bits are the upload position"""
    out = []
    for n in M.SORT_N:
        for name in M.SORT_PATTERNS:
            idx = M.sort_pattern(name, n, d)
            if idx is None:
                continue
            rec = idx.astype(np.uint64) | (np.arange(n, dtype=np.uint64) << np.uint64(32))
            rec.setflags(write=False)
            out.append((name, n, rec, M.stable_sorted(rec, d), M.composite_sorted(rec)))
    return out


@pytest.mark.parametrize("d", M.SORT_D, ids=lambda d: "d%d_%dx%d" % ((d,) + M.PASS_SHAPES[d]))
def test_sort_alone_is_the_stable_order(dev, radix_order, d):
    """Every record lands where np.argsort(min(idx, d), kind="stable") puts it; the records
    with idx >= d come last in upload order (the composite order: by idx, then position) and
    set status bit 0x2, the others none."""
    assert dev.status() == 0
    for name, n, rec, stable, composite in sort_cases(d):
        got = dev.debug_sort_records(on_device(rec), d).cpu().numpy().view(np.uint64)
        st = dev.status()
        want = stable if radix_order else composite
        assert np.array_equal(got, want), (name, n, first_difference(got, want))
        assert st == (INDEX_RANGE if (M.rec_idx(rec) >= d).any() else 0), (name, n, st)


# ------------------------------------------------------------------------ the fold ----
def coef_of(vs):
    """the constructed sets are read un-scaled (a product may round two sums together)"""
    return float(np.float32(1) / np.float32(7)) if vs == "general" else 1.0


@functools.lru_cache(maxsize=None)
def fold_reference(name, vs):
    """(the shuffled upload, the sorted upload, the reference): built once, read-only"""
    ups = []
    for shuffled in (True, False):
        lay = M.fold_layout(name, shuffled)
        ups.append(M.upload(lay, M.values(vs, lay)))
        ups[-1].setflags(write=False)
    ref = M.ordered(ups[0], lay.d, coef_of(vs))
    assert np.array_equal(bits(ref), bits(M.ordered(ups[1], lay.d, coef_of(vs))))
    ref.setflags(write=False)
    return ups[0], ups[1], ref


def nan_filled(d):
    import torch
    out = torch.empty(d, dtype=torch.int32, device="cuda").fill_(NAN_BITS).view(torch.float32)
    return out


@pytest.mark.parametrize("vs", M.VALUE_SETS)
@pytest.mark.parametrize("name", sorted(M.FOLD_SPECS))
def test_fold_at_constructed_boundaries(dev, radix_order, name, vs):
    """out[i] = the left fold from +0.0 of index i's records in list order, x coef; +0.0
    (not the NaN that was there) for an index without records; status 0x2 exactly when the
    list holds an index >= d, and the outputs beside those records unchanged by them."""
    shuffled, in_order, ref = fold_reference(name, vs)
    d = len(ref)
    tail = M.FOLD_SPECS[name][3]
    assert dev.status() == 0
    for what, up in (("shuffled", shuffled), ("sorted", in_order)):
        out = dev.ordered_list(on_device(up), d, coef_of(vs), out=nan_filled(d)).cpu().numpy()
        st = dev.status()
        assert np.array_equal(bits(out), bits(ref)), (what, first_difference(bits(out), bits(ref)))
        assert st == (INDEX_RANGE if tail else 0), (what, st)
    if not M.FOLD_SPECS[name][0]:  # no record in range: every output +0.0
        assert not bits(ref).any()


# -------------------------------------------- routes that reach the same kernels ----
@functools.lru_cache(maxsize=None)
def route_records(name, vs):
    lay = M.route_layout(name)
    rec = M.upload(lay, M.values(vs, lay))
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def accumulate_prev(d):
    """what accumulate finds in out: multiples of 2^-4, no -0.0"""
    prev = (((np.arange(d, dtype=np.int64) * 7919) % 2001 - 1000) / 16.0).astype(np.float32)
    prev.setflags(write=False)
    return prev


@pytest.mark.parametrize("accumulate", [False, True], ids=["plain", "accumulate"])
@pytest.mark.parametrize("vs", M.VALUE_SETS)
def test_non_oblivious_sort_path(dev, oracle, radix_order, vs, accumulate):
    """alg 4 past the scatter rows (n * d > 2^24 cells; four passes of 7 bits): the run of
    3000 split over the two clients == oracle.non_oblivious; accumulate (the fold's ACC
    instantiation): out += the un-averaged in-order sums, the other indices untouched."""
    import torch
    alg, n, k, d, _ = M.ROUTE_SPECS["alg4_sort_path"]
    rec = route_records("alg4_sort_path", vs)
    w = oracle.as_weights(M.rec_idx(rec).astype(np.uint32), M.rec_val(rec))
    if accumulate:
        sums, st = oracle.non_oblivious(w, d, 1)
        ref = accumulate_prev(d) + sums
        out = torch.from_numpy(accumulate_prev(d).copy()).cuda()
    else:
        ref, st = oracle.non_oblivious(w, d, n)
        out = nan_filled(d)
    assert st == 0
    got = dev.aggregate(alg, on_device(rec), n, k, d, out=out, accumulate=accumulate).cpu().numpy()
    assert dev.status() == 0
    assert np.array_equal(bits(got), bits(ref)), first_difference(bits(got), bits(ref))


@pytest.mark.parametrize("vs", M.VALUE_SETS)
def test_nips19_with_repeated_indices(dev, oracle, radix_order, vs):
    """alg 2 at (12, 3000, 300), every client repeating indices (a run of 700 among them):
    the shuffled list's in-order sums == oracle.nips19, bit for bit"""
    alg, n, k, d, _ = M.ROUTE_SPECS["alg2_repeats"]
    rec = route_records("alg2_repeats", vs)
    seed = 0x5EED0000 + zlib.crc32(vs.encode()) % 1000
    got = dev.aggregate(alg, on_device(rec), n, k, d, out=nan_filled(d), seed=seed).cpu().numpy()
    assert dev.status() == 0
    ref, st = oracle.nips19(k, oracle.as_weights(M.rec_idx(rec).astype(np.uint32), M.rec_val(rec)),
                            d, n, seed=seed)
    assert st == 0
    assert np.array_equal(bits(got), bits(ref)), first_difference(bits(got), bits(ref))
