"""tests/radix_model.py on the CPU: the pass shapes, that every constructed layout of
tests/test_gpu_radix.py has its run ends and starts where it claims, and that the value
sets tell a wrong fold from the right one — conditions on the inputs, asserted here, not
tolerances."""
import os

import numpy as np
import pytest

import radix_model as M
from conftest import ROOT

LIB = os.path.join(ROOT, "fl-tee_amd", "lib", "libfltee_agg.so")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pass_shapes():
    assert {d: M.cs_plan(d) for d in M.SORT_D} == M.PASS_SHAPES
    assert M.PASS_SHAPES == {1: (1, 1), 7: (1, 3), 255: (1, 8), 256: (2, 5), 65535: (2, 8),
                             65536: (3, 6), (1 << 24) - 1: (3, 8), 1 << 24: (4, 7)}
    assert M.cs_plan((1 << 24) + 1) == (4, 7) and M.cs_plan((1 << 28) - 1) == (4, 7)
    assert M.cs_plan(1 << 28) == (4, 8)  # (not run on the GPU: d >= 2^28 is a 1 GB output)
    # every shape but (4, 8) is sorted alone, and the fold's layouts cover one to four passes
    assert {M.cs_plan(s[1])[0] for s in M.FOLD_SPECS.values()} | \
           {M.cs_plan(s[3])[0] for s in M.ROUTE_SPECS.values()} == {1, 2, 3, 4}


def test_stable_sorted_and_ordered_on_a_small_list():
    idx = np.array([5, 2, 9, 2, 5, 7, 2, 8], np.uint32)
    rec = M.pack(idx, np.arange(8, dtype=np.float32))
    s = M.stable_sorted(rec, 7)  # 9, 7 and 8 are out of range: last, in upload order
    assert M.rec_idx(s).tolist() == [2, 2, 2, 5, 5, 9, 7, 8]
    assert M.rec_val(s).tolist() == [1, 3, 6, 0, 4, 2, 5, 7]
    assert M.rec_idx(M.composite_sorted(rec)).tolist() == [2, 2, 2, 5, 5, 7, 8, 9]
    out = M.ordered(rec, 7, 0.5)
    assert out.tolist() == [0, 0, 5.0, 0, 0, 2.0, 0]
    assert bits(M.ordered_reversed(rec, 7, 0.5)).tolist() == bits(out).tolist()
    assert bits(M.ordered_chunked(rec, 7, 2, 0.5)).tolist() == bits(out).tolist()


@pytest.mark.parametrize("shuffled", [True, False])
@pytest.mark.parametrize("name", sorted(M.FOLD_SPECS))
def test_layouts_are_what_they_claim(name, shuffled):
    lengths, d, gaps, tail, claims = M.FOLD_SPECS[name]
    lay = M.fold_layout(name, shuffled)
    n, idx = len(lay.idx), lay.idx.astype(np.int64)
    assert n <= 20000 and lay.nin == sum(lengths) and n == lay.nin + tail
    assert (idx[:lay.nin] < d).all() and (idx[lay.nin:] >= d).all()
    assert (np.diff(idx[:lay.nin]) >= 0).all()
    assert claims
    for what, p in claims:
        if what == "start":
            assert idx[p] < d and (p == 0 or idx[p - 1] != idx[p]) and p in lay.starts
        elif what == "end":
            assert idx[p - 1] < d and (p == n or idx[p] != idx[p - 1])
            assert p in lay.starts + lay.lengths
        elif what == "oor":
            assert idx[p] >= d and (p == 0 or idx[p - 1] < d)
        else:
            assert what == "n" and n == p
    # the gaps: d // runs - 1 unused indices between two used ones unless the layout says
    if len(lengths) > 1:
        used = np.unique(idx[:lay.nin])
        assert (np.diff(used) == (gaps if gaps is not None else d // len(lengths) - 1) + 1).all()
    # the upload order: a permutation that the stable sort undoes exactly
    val = M.values("membership", lay)
    up = M.upload(lay, val)
    want = M.pack(lay.idx, val)
    assert np.array_equal(M.stable_sorted(up, d), want)
    assert np.array_equal(M.rec_idx(M.composite_sorted(up))[:lay.nin], idx[:lay.nin])
    if shuffled and n > 8 and len(lengths) + (tail > 0) > 1:  # (one key: one order)
        assert not np.array_equal(up, want)
    else:
        assert shuffled or np.array_equal(up, want)


def test_named_boundaries_are_covered():
    """the positions the issue names, by the kernels' constants"""
    ends = {p for s in M.FOLD_SPECS.values() for w, p in s[4] if w == "end"}
    starts = {p for s in M.FOLD_SPECS.values() for w, p in s[4] if w == "start"}
    assert {M.CHUNK * c for c in (1, 2, 3, 4)} <= ends          # lane 63 of every chunk
    assert {1, 2, 63, 64, 65, 256, 320, 321, 384} <= ends       # runs from position 0
    assert {M.WAVE - 1, M.WAVE - 64} <= starts                  # 255 and 192
    assert {257, 321, 385, M.WAVE, M.PRELOAD, M.PRELOAD + 1} <= ends
    lay = M.fold_layout("run3000_at700")
    assert lay.lengths.max() == 3000 and 700 in lay.starts      # over 1024 and several waves
    oor = {p for s in M.FOLD_SPECS.values() for w, p in s[4] if w == "oor"}
    assert {0, M.CHUNK, M.WAVE} <= oor
    # a last run that ends at n inside the loop past the preload
    lengths = M.FOLD_SPECS["last_run_ends_at_n1025"][0]
    start = 1025 - lengths[-1]
    assert start // M.WAVE * M.WAVE + M.PRELOAD < 1024


def all_layouts():
    for name in sorted(M.FOLD_SPECS):
        for shuffled in (True, False):
            yield name, M.fold_layout(name, shuffled)
    for name in sorted(M.ROUTE_SPECS):
        yield name, M.route_layout(name)


def test_membership_sums_are_exact_in_any_order():
    for name, lay in all_layouts():
        v = M.values("membership", lay).astype(np.float64)
        assert len(set(v[:1000])) == min(len(v), 1000)
        sums = np.bincount(lay.idx[:lay.nin], weights=v[:lay.nin], minlength=1)
        assert sums.max(initial=0) < 2 ** 24, name
        want = sums.astype(np.float32)
        got = M.ordered(M.upload(lay, M.values("membership", lay)), lay.d, 1.0)
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any()


def test_association_values_tell_a_reversed_run():
    """the left fold of [2^24, 1, ..., 1] is 2^24 and of [1, ..., 1, 2^24] is 2^24 + L - 1
    rounded once; back to front they swap: other bits for every run of 3 or more"""
    seen = 0
    for name, lay in all_layouts():
        for vs in ("association", "mirror"):
            rec = M.upload(lay, M.values(vs, lay))
            ref, rev = M.ordered(rec, lay.d, 1.0), M.ordered_reversed(rec, lay.d, 1.0)
            at = lay.idx[lay.starts]
            long = lay.lengths >= 3
            assert (bits(ref)[at[long]] != bits(rev)[at[long]]).all(), (name, vs)
            assert np.array_equal(bits(ref)[at[~long]], bits(rev)[at[~long]])
            if vs == "association":
                assert (ref[at] == M.BIG).all()
            seen += int(long.sum())
    assert seen > 1000


@pytest.mark.parametrize("c", [M.CHUNK, M.WAVE])
def test_association_values_tell_a_chunked_run(c):
    """Folding pieces of c sorted positions apart gives other bits for every run that goes
    two or more records past a piece boundary.  (One record past it is no other expression:
    fold(A) + (0 + x) is the left fold itself, whatever the values; neither is a run that
    ends on the boundary.)  [2^24, 1, ..., 1] cut after its first piece: 2^24 + m with m >= 2
    ones summed first, not 2^24."""
    seen = set()
    for name, lay in all_layouts():
        rec = M.upload(lay, M.values("association", lay))
        ref, chk = M.ordered(rec, lay.d, 1.0), M.ordered_chunked(rec, lay.d, c, 1.0)
        at = lay.idx[lay.starts]
        first_cut = (lay.starts // c + 1) * c
        past = lay.starts + lay.lengths - first_cut  # records behind the run's first boundary
        split = past >= 2
        assert (bits(ref)[at[split]] != bits(chk)[at[split]]).all(), name
        assert np.array_equal(bits(ref)[at[~split]], bits(chk)[at[~split]])
        if split.any():
            seen.add(name)
    want = {"run256_at0", "run320_at0", "run321_at0", "run384_at0", "run66_at255", "run130_at255",
            "run128_at192", "run129_at192", "run3000_at700", "last_run_ends_at_n1025",
            "alg4_sort_path", "alg2_repeats"}
    if c == M.WAVE:
        want -= {"run256_at0"}
    assert want <= seen


def test_general_values_are_not_exact():
    """the breadth set: a reversed long run does change its bits (so the order is pinned)"""
    lay = M.fold_layout("run3000_at700")
    rec = M.upload(lay, M.values("general", lay))
    ref, rev = M.ordered(rec, lay.d, 1.0), M.ordered_reversed(rec, lay.d, 1.0)
    i = lay.idx[lay.starts[lay.lengths == 3000]]
    assert bits(ref)[i] != bits(rev)[i]


@pytest.mark.parametrize("d", M.SORT_D)
def test_sort_patterns(d):
    passes, w = M.cs_plan(d)
    mask = (1 << w) - 1
    for n in M.SORT_N:
        for name in M.SORT_PATTERNS:
            idx = M.sort_pattern(name, n, d)
            if idx is None:
                assert name == "later_digit_only" and passes == 1
                continue
            assert idx.shape == (n,) and idx.min() >= 0 and idx.max() <= 0xFFFFFFFF
            key = np.minimum(idx, d)
            if name == "out_of_range":
                assert (idx >= d).any() or n < 3
                continue
            assert idx.max() < d, (name, n, d)
            if name == "one_index":
                assert len(set(idx)) == 1
            elif name == "two_by_lane" and n > 1 and d > 1:
                assert idx[0] != idx[1] and (idx[::2] == idx[0]).all() and (idx[1::2] == idx[1]).all()
            elif name == "later_digit_only":
                assert len(set(key & mask)) == 1 and (n < 64 or len(set(key >> w)) > 1)
            elif name == "pass0_digit_only":
                assert len(set(key >> w)) == 1 and (n < 64 or d < 3 or len(set(key & mask)) > 1)
            elif name == "sorted":
                assert (np.diff(idx) >= 0).all()
            elif name == "reversed":
                assert (np.diff(idx) <= 0).all()
            elif name == "zeros_in_last_lanes":
                assert idx[-1] == d - 1 and (idx[max(n - 71, 0):-1] == 0).all()
                if n % M.TILE:  # a partial last tile: the dead lanes follow these zeros
                    assert n == 1 or idx[-2] == 0


@pytest.mark.skipif(not os.path.exists(LIB), reason="libfltee_agg.so not built")
def test_route_shapes_reach_the_counting_sort():
    """alg 4's shape leaves the scatter rows for the counting-sort fold (host arithmetic)"""
    from test_plan import R_COUNTING, R_NIPS19, Plan
    alg, n, k, d, _ = M.ROUTE_SPECS["alg4_sort_path"]
    assert n * d > max(1 << 24, 64 * (1 << (n * k - 1).bit_length()))
    assert Plan(alg, n, k, d).route == R_COUNTING
    assert Plan(alg, n, k, d, accumulate=True).route == R_COUNTING
    alg, n, k, d, _ = M.ROUTE_SPECS["alg2_repeats"]
    assert (alg, n, k, d) == (2, 12, 300, 3000) and Plan(alg, n, k, d, seed=5).route == R_NIPS19
    lay = M.route_layout("alg2_repeats")
    up = M.rec_idx(M.upload(lay, M.values("membership", lay))).reshape(n, k)
    assert all(len(set(row)) < k for row in up)  # repeated indices inside every client
