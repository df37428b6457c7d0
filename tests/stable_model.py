"""The model of aggregation_alg 7 (bubble_sort_based.rs) the alg-7 tests share, in numpy:
the records ++ (i, 0.0) for i < d in STABLE order by idx, each run left-folded in float32
(((v1 + v2) + ... + vc) + 0.0, the zero entry last), times 1f32 / n, the first d values.
Also the input builders of those tests."""
import numpy as np


def run_sums(idx, val, d):
    """The in-order float32 sum of every index's run (zero entry last), for idx < d."""
    idx = np.concatenate([np.asarray(idx, np.uint32), np.arange(d, dtype=np.uint32)])
    val = np.concatenate([np.asarray(val, np.float32), np.zeros(d, np.float32)])
    o = np.argsort(idx, kind="stable")
    si, sv = idx[o], val[o]
    first = np.ones(len(si), bool)
    first[1:] = si[1:] != si[:-1]
    run = np.cumsum(first) - 1                       # run number of every entry
    start = np.flatnonzero(first)
    rank = np.arange(len(si)) - start[run]           # place inside its run
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2))
    acc = np.zeros(len(start), np.float32)
    for r in range(len(bounds) - 1):                 # one left-fold step for every run
        sel = by_rank[bounds[r]:bounds[r + 1]]
        if r == 0:
            acc[run[sel]] = sv[sel]
        else:
            acc[run[sel]] = acc[run[sel]] + sv[sel]  # float32 + float32
    keys = si[start]
    out = np.zeros(d, np.float32)
    keep = keys < d
    out[keys[keep]] = acc[keep]
    return out


def model(idx, val, n, d):
    return run_sums(idx, val, d) * (np.float32(1) / np.float32(n))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def distinct_indices(rng, n, k, d):
    return np.concatenate([rng.choice(d, k, replace=False) for _ in range(n)]).astype(np.uint32)


ORDER_VALUES = np.array([1e8, 1.0, -1e8, 3.0], np.float32)


def order_sensitive(n, k, d):
    """Every client sends the same k indices; per index the values cycle 1e8, 1, -1e8, 3
    across the clients (the j-th index starting the cycle at place j), so the float32 sum
    depends on the order of addition.  Client c sends its records rotated by c places: the
    upload positions of an index's records are then spread unevenly, which is what makes
    a network without the position in its key (advanced's) leave them in another order
    even at n = 3 (checked against the enclave model of advanced at (3, 5, 17))."""
    base = np.arange(k, dtype=np.uint32) * np.uint32(max(1, d // max(k, 1))) % np.uint32(d)
    rows = [np.roll(np.arange(k), c) for c in range(n)]
    idx = np.concatenate([base[r] for r in rows])
    val = np.concatenate([ORDER_VALUES[(c + r) % 4] for c, r in enumerate(rows)])
    return idx.astype(np.uint32), val.astype(np.float32)
