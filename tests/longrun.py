"""Checks for `advanced` / alg 6 on uploads with runs longer than n + 1 entries (a client
repeating an index).  The enclave folds every run left to right in the sorted order
(advanced.rs:66-101); the device folds each run of <= halo + 1 entries the same way (bit
for bit) and finishes longer ones with a sum re-associated at its fold's walk boundaries
(k_fold.hip / k_compact.hip headers) — within the per-index
re-association bound below (every partial sum of a run of c values is within
(c - 1) * 2^-24 * sum|v| of the exact sum, for either order).

That bound is the worst case of ANY summation order and grows with the run: at c = 508,901 it
lets 0.0 pass.  Two sharper checks:

* exact values (exact_values / exact_ref / assert_bits): where every partial sum is exactly
  representable, any correct carry gives the left fold's bits;
* the tree-height bound (tree_height / height_bound).  For any summation tree,
  |err| <= gamma_h * sum|v|, gamma_h = h u / (1 - h u), u = 2^-24, h = the largest number of
  additions any one input passes through.  h from the fold's geometry (fold_geometry), each
  term an upper bound read off the kernel:
  - the streaming fold + patch (k_fold.hip).  A lane's in-order walk covers Hr + C positions
    (its head run's S, its piece's Q): <= Hr + C additions.  The wave's Hillis-Steele scan of
    64 pieces: 6 levels.  In the patch, a thread folds its slice of the wave aggregates in
    front of the block left to right, <= ceil(waves / 256) additions; fp_block_scan over 256
    threads: 8 levels, twice (wave aggregates, then the block's lanes); the thread's 4 lanes
    folded in order: <= 3 + the 2 of `mine`; carry + exclusive prefix: 1; tot = run.Q + S: 1.
    h = Hr + C + 6 + ceil(waves / 256) + 8 + 2 + 3 + 8 + 1 + 1.
  - the fused fold (k_compact.hip fold_compact_first).  A lane walks back lim slots and
    through its chunk = ceil((Hr + 512 per + 1) / 512) slots: <= lim + chunk additions.  The
    window-local prefix: the wave scan's 6 levels, <= 7 wave totals in front, the exclusive
    shift and ex.Q + a2: 2.  Across tiles a piece's partial travels through the look-back
    (fa_combine with an empty operand adds nothing, so only real merges count).  A tile T
    whose nearest predecessor with a published inclusive prefix is P = T - delta reduces
    the delta entries P .. T - 1: inside a wave a reduction tree over them, <= ceil(log2
    delta) merges on any path (6 at most), then <= ceil(delta / 64) - 1 wave results and one
    running aggregate a further round in front; then its own inclusive prefix = that carry
    + its piece: 1.  In every case that is <= delta additions for a stage that advances
    delta tiles (delta = 1: 1; 2: 2; 3: 3; 5: 4; 64: 7; 512: 15), so however the tiles'
    timing chains the prefixes (fc_lookback takes whichever predecessor has published when
    it looks: the tree differs from run to run, the bound holds for every outcome), a value
    passes through <= ntiles additions on its way across the tiles.  The carry into the
    record: 1.
    h = lim + chunk + 6 + 7 + 2 + ntiles + 1.
  - alg 6 adds its batches' sums in order: + the number of batches.
  The averaging (1f32 / n rounded, one multiply) adds 3 u |result|.  At configs[2]
  (all_one_index) h is 160 for the streaming fold and 343 for the fused one, against
  c - 1 = 508,900."""
import numpy as np

U = 2.0 ** -24


def run_stats(idx, val, d):
    """per index i < d: the run length (records + the initial entry), sum |v|, exact sum"""
    idx = np.asarray(idx, np.int64)
    val = np.asarray(val, np.float32).astype(np.float64)
    sel = idx < d
    cnt = np.bincount(idx[sel], minlength=d)[:d] + 1
    absum = np.zeros(d, np.float64)
    np.add.at(absum, idx[sel], np.abs(val[sel]))
    exact = np.zeros(d, np.float64)
    np.add.at(exact, idx[sel], val[sel])
    return cnt, absum, exact


def tree_height(g, batches=0):
    """h for the device's summation tree of one run under the fold geometry g
    (fold_geometry): an upper bound on the f32 additions any one value passes through
    (module docstring); alg 6 adds its batches' sums in order: + batches."""
    if g["path"] == "one_lane":
        return g["L"] + batches
    if g["path"] == "streaming":
        waves = (g["lanes"] + 63) // 64
        return g["Hr"] + g["C"] + 6 + (waves + 255) // 256 + 8 + 2 + 3 + 8 + 1 + 1 + batches
    chunk = (g["Hr"] + 512 * g["per"] + 1 + 511) // 512
    return g["lim"] + chunk + 6 + 7 + 2 + g["ntiles"] + 1 + batches


def height_bound(h, absum, want, n):
    """|out - want| allowed by a summation tree of height h over values of sum |v| = absum
    (Higham, Accuracy and Stability, 4.2: gamma_h = h u / (1 - h u)), then the rounding of
    1f32/n and of the multiply (3 u |want| covers both and the second-order term)"""
    return h * U / (1 - h * U) * absum / n + 3 * U * np.abs(want) + 1e-45


def _assert_height(o64, idx, val, d, n, h):
    cnt, absum, exact = run_stats(idx, val, d)
    want = exact / n
    err, bound = np.abs(o64 - want), height_bound(h, absum, want, n)
    over = np.flatnonzero(err > bound)
    det = [(int(i), int(cnt[i]), float(o64[i]), float(want[i]), float(bound[i])) for i in over[:5]]
    assert over.size == 0, (f"{over.size} indices over the height-{h} bound: "
                            f"(idx, entries, out, exact, bound) {det}")


def assert_advanced(out, ref, idx, val, d, n, lim=None, h=None):
    """out vs the oracle's `advanced` (ref), both x 1f32/n: bit for bit wherever the run
    has <= lim (= n + 1) entries, within the re-association bound elsewhere; returns the
    number of long runs.  h (tree_height): every index also within the tree-height bound of
    the exact (float64) sum."""
    cnt, absum, _ = run_stats(idx, val, d)
    if h is not None:
        _assert_height(np.asarray(out, np.float32).astype(np.float64), idx, val, d, n, h)
    lim = n + 1 if lim is None else lim
    short = cnt <= lim
    o = np.asarray(out, np.float32)
    r = np.asarray(ref, np.float32)
    assert np.isfinite(o).all()
    diff = np.flatnonzero(short & (o.view(np.uint32) != r.view(np.uint32)))
    assert diff.size == 0, f"{diff.size} short runs differ (first idx {diff[:5]})"
    o64, r64 = o.astype(np.float64), r.astype(np.float64)
    bound = 2 * (cnt - 1) * U * absum / n + 2 * U * np.abs(r64) + 1e-45
    over = np.flatnonzero(~short & (np.abs(o64 - r64) > bound))
    if over.size:
        _, _, exact = run_stats(idx, val, d)
        det = [(int(i), int(cnt[i]), float(o64[i]), float(r64[i]), float(exact[i] / n), float(bound[i]))
               for i in over[:5]]
        raise AssertionError(f"{over.size} long runs over the bound: (idx, entries, out, ref, "
                             f"exact, bound) {det}")
    return int((~short).sum())


# ---------------------------------------------------------------- exact values ----
# The device only re-associates a run's sum; it never changes which records belong to a
# run.  With small positive integer values and sum|v| < 2^24 over the whole upload, every
# partial sum under any association is an integer below 2^24, exact in f32: any correct
# carry gives the left fold's bits, and x (1f32 / n) is the same one multiply on both
# sides.  Positive, so every piece of a run has a non-zero sum: a dropped, doubled or
# misattributed piece changes the answer.
def exact_values(nrec):
    """val[p] = 1 + p % 7 (neighbouring pieces of a run differ in their sums); the upload's
    total must stay below 2^24 — a condition of the method, not a tolerance."""
    val = (1 + np.arange(nrec) % 7).astype(np.float32)
    assert val.sum(dtype=np.float64) < 2 ** 24, "exact_values: choose a smaller upload"
    return val


def exact_ref(idx, val, d, n):
    """`advanced` / alg 6 of an exact_values upload, bit for bit — no sort network needed"""
    idx = np.asarray(idx, np.int64)
    sel = idx < d
    sums = np.bincount(idx[sel], weights=np.asarray(val, np.float64)[sel], minlength=d)[:d]
    assert sums.max(initial=0.0) < 2 ** 24
    return np.float32(sums) * (np.float32(1) / np.float32(n))


def assert_bits(out, ref):
    o = np.ascontiguousarray(out, np.float32)
    r = np.ascontiguousarray(ref, np.float32)
    assert o.shape == r.shape, (o.shape, r.shape)
    diff = np.flatnonzero(o.view(np.uint32) != r.view(np.uint32))
    if diff.size:
        det = [(int(i), float(o[i]), float(r[i])) for i in diff[:8]]
        raise AssertionError(f"{diff.size} of {o.size} outputs differ: (idx, out, ref) {det}")


LAYOUTS = ("one_client", "all_one_index", "two_adjacent", "index_zero", "last_and_beyond",
           "boundary")


def boundary_base(boundary, nrec, d):
    """the `boundary` layout's first index: about half the records on it, its run's last
    entry on sorted position boundary - 1"""
    return int(min(max(boundary - 1 - nrec // 2, 0), d - 3))


def layout(name, n, k, d, boundary=None, base=7, mid=None, seed=5):
    """The adversarial index layouts (u32[n * k], client-major).  In the sorted array
    (records and the d initial entries by index) index i's run starts at position
    i + #records with a smaller index (run_span), so the long runs' positions are known:
      one_client       client 0 sends index `base` k times, the others k distinct indices each
      all_one_index    every record on `base`: one run over positions [base, base + n k]
      two_adjacent     the first half on base, the rest on base + 1: a carry must stop at the
                       key change
      index_zero       every record on 0: the array's first lanes
      last_and_beyond  half on d - 1, half on d + 5 (out of range: never reaches out[d - 1])
      boundary         index b = boundary_base()'s run ends on sorted position boundary - 1
                       (the last of a piece, tile or range); index b + 1's run of `mid`
                       entries (long, yet ending inside the unit it starts: the one place a
                       carry of b's partial onto another key would land) starts on
                       `boundary`, and b + 2's takes the rest"""
    nrec = n * k
    idx = np.empty(nrec, np.uint32)
    if name == "one_client":
        rng = np.random.default_rng(seed)
        for c in range(n):
            idx[c * k:(c + 1) * k] = rng.choice(d, k, replace=False)
        idx[:k] = base
    elif name == "all_one_index":
        idx[:] = base
    elif name == "two_adjacent":
        idx[:nrec // 2] = base
        idx[nrec // 2:] = base + 1
    elif name == "index_zero":
        idx[:] = 0
    elif name == "last_and_beyond":
        idx[:nrec // 2] = d - 1
        idx[nrec // 2:] = d + 5
    elif name == "boundary":
        b = boundary_base(boundary, nrec, d)
        c0 = boundary - 1 - b  # b's run: its initial entry and c0 records on [b, boundary)
        assert 0 < c0 and c0 + mid - 1 < nrec, (boundary, nrec, d, mid)
        idx[:c0] = b
        idx[c0:c0 + mid - 1] = b + 1
        idx[c0 + mid - 1:] = b + 2
    else:
        raise ValueError(name)
    return idx


def run_span(idx, d, i):
    """[start, end) of index i's run (its records and its initial entry) in the sorted array"""
    idx = np.asarray(idx, np.int64)
    start = min(i, d) + int((idx < i).sum())
    return start, start + int((idx == i).sum()) + (1 if i < d else 0)


def fold_geometry(n, k, d, halo=0):
    """fltee_debug_fold_geometry for `advanced` of n x k records into d (halo 0: the default
    n), under the current A/B settings: the path run_advanced takes and its sizes, so a case
    can assert the regime it was written for (host code only, no GPU needed)."""
    import ctypes

    from fltee import _lib
    L = n * k + d
    M = 1 << max(0, (L - 1).bit_length())
    out = (ctypes.c_uint64 * 8)()
    _lib.lib().fltee_debug_fold_geometry(M, L, d, halo or n, out)
    v = [int(x) for x in out]
    g = dict(M=M, L=L)
    if v[0] == 1:
        g.update(path="fused", per=v[1], S=v[2], ntiles=v[3], lim=v[4], G=v[5], last=bool(v[6]),
                 Hr=v[7])
    else:
        g.update(path="streaming" if v[0] == 2 else "one_lane", Hr=v[1], C=v[2], lanes=v[3],
                 depth=v[4], patch_blocks=v[5], span=v[6])
    return g


def boundary_position(g, nrec):
    """A sorted position near nrec / 2 on which a piece of the fold g (fold_geometry) starts —
    the unit whose aggregate the carries are made of: [t S - Hr, (t + 1) S - Hr) for tile t
    of the fused pass (its look-back slot), [j C - Hr, j C - Hr + C) for lane j of the
    streaming fold — a patch block's first lane (j a multiple of 1,024) or a wave's (64)
    where the upload is long enough."""
    if g["path"] == "fused":
        unit, hr = g["S"], g["Hr"]
    else:
        C, hr = g["C"], g["Hr"]
        unit = next(u for u in (1024 * C, 64 * C, C) if nrec >= 4 * u or u == C)
    return ((nrec // 2 + hr) // unit + 1) * unit - hr


def sorted_runs(m, Hr, C, seed):
    """A pre-sorted key array (key = the run's number) with runs of 1 to 50,000 entries: the
    short ones around the halo, one long run ending on the last position of a piece
    (B - 1, B = the first position of the piece of a wave's — at these sizes also a patch
    block's — first lane near m / 2) and the next one starting on B, both crossing more
    than 64 lanes (more than 1,024 where C = 16 leaves room), random lengths elsewhere."""
    rng = np.random.default_rng(seed)
    B = (m // 2) // (64 * C) * (64 * C) - Hr
    la, lb = min(50000, B - 600), min(50000, (m - B) // 2)
    assert la > 64 * C and lb > 64 * C
    pool = np.array([1, 1, 1, 2, 3, 7, Hr, Hr + 1, Hr + 2, 2 * Hr + 5, 3 * C + 1, 700, 5000, 50000])
    lens = [1, 2, 3, Hr + 1, Hr + 2, 2 * Hr + 5]
    front = B - la
    assert sum(lens) <= front
    while sum(lens) < front:
        lens.append(int(min(rng.choice(pool), front - sum(lens))))
    lens += [la, lb]
    while sum(lens) < m:
        lens.append(int(min(rng.choice(pool), m - sum(lens))))
    lens = np.array(lens)
    assert lens.sum() == m
    idx = np.repeat(np.arange(len(lens), dtype=np.uint32), lens)
    start = np.cumsum(lens) - lens
    k = int(np.searchsorted(start, B))
    assert start[k] == B and lens[k] == lb and lens[k - 1] == la
    return idx, B


def assert_sequential_fold(gi, gv, idx, val, fold_len, halo):
    """(gi, gv) = the fold of the pre-sorted (idx = the run's number, val: exactly summable)
    equals the enclave's sequential fold bit for bit: every run of the folded part leaves
    exactly one record (its key, its sum) — at its last position when it has <= halo + 1
    entries, anywhere inside it otherwise — dummies (u32::MAX - p, +0.0) elsewhere, the
    positions past fold_len copied."""
    m = len(idx)
    fi, fv, fp = idx[:fold_len], val[:fold_len], np.arange(fold_len)
    nruns = int(fi[-1]) + 1
    sums = np.bincount(fi, weights=fv, minlength=nruns)
    assert sums.max() < 2 ** 24
    cnt = np.bincount(fi, minlength=nruns)
    last = np.cumsum(cnt) - 1
    dummy = gi[:fold_len] == (0xFFFFFFFF - fp).astype(np.uint32)
    assert (gv[:fold_len][dummy].view(np.uint32) == 0).all()
    reps = np.flatnonzero(~dummy)
    # one record a run, inside the run, with the run's key and sum
    assert reps.size == nruns and np.array_equal(gi[reps], np.arange(nruns, dtype=np.uint32)), \
        np.flatnonzero(np.bincount(fi[reps], minlength=nruns) != 1)[:8]
    assert np.array_equal(fi[reps], gi[reps])
    bad = np.flatnonzero(gv[reps] != sums.astype(np.float32))
    assert bad.size == 0, [(int(r), int(cnt[r]), float(gv[reps[r]]), float(sums[r]))
                           for r in bad[:8]]
    short = cnt <= halo + 1
    assert np.array_equal(reps[short], last[short])
    assert np.array_equal(gi[fold_len:], idx[fold_len:])
    assert m == len(gi)
    assert np.array_equal(gv[fold_len:].view(np.uint32), val[fold_len:].view(np.uint32))


def assert_near_exact(out, idx, val, d, n, h=None):
    """out (x 1f32/n) vs the exact (float64) per-index sums: within the bound every f32
    left fold obeys — the full-size property check where the oracle's network is too
    slow to run per case.  h (tree_height): also within the tree-height bound."""
    cnt, absum, exact = run_stats(idx, val, d)
    o = np.asarray(out, np.float32).astype(np.float64)
    if h is not None:
        _assert_height(o, idx, val, d, n, h)
    want = exact / n
    bound = (cnt - 1) * U * absum / n + 2 * U * np.abs(want) + 1e-45
    over = np.flatnonzero(np.abs(o - want) > bound)
    assert over.size == 0, f"{over.size} indices over the bound (first {over[:5]})"
