"""The options of fltee_aggregate_device in numpy (include/fltee_agg.h: FLTEE_OPT_CLIP,
_ACCUMULATE, _NO_AVERAGE, n_avg), independent of the library, and the inputs on which the
option tests (tests/test_gpu_options.py) can ask for bit equality.

clip_coefs     update.py:187-204 as k_dp.hip states it: t = the f64 sum of squares of a
               client's k values, norm32 = f32(sqrt(t)), cf = f32(clipping) / norm32 in f32,
               cf = cf if cf < 1 else 1 (NaN, inf and >= 1 all give 1), v * cf in f32.
reference      a route's result = the alg's own CPU reference (the oracle, or
               stable_model.model for alg 7) on the records it is given: model-clipped ones
               for a clipped call.
lattice        inputs whose clipped values and sums are exact in f32 under ANY order of
               addition: the un-averaged sums are an f64 bincount whatever the route.
general        N(0, 1) * 100 values whose f64 norm lies clear of every f32 rounding
               midpoint, so that the device's differently ordered f64 sum rounds to the same
               f32 norm as this model's.
"""
import functools
import zlib

import numpy as np

from stable_model import distinct_indices, model


# ------------------------------------------------------------------ clip ----
def clip_coefs(val, n, k, clipping):
    """(coef f32[n], clipped f32[n * k]).  No value is treated specially: a NaN makes t, the
    norm and cf NaN, `cf < 1` false and cf 1; an inf makes the norm inf and cf 0 (inf * 0 is
    NaN, finite * 0 a signed zero); a finite t whose root is past f32 rounds to an inf norm;
    no values or all zeros divide by a zero norm, cf inf, so 1."""
    val = np.ascontiguousarray(val, np.float32)
    assert val.size == n * k
    coef = np.empty(n, np.float32)
    out = np.empty(n * k, np.float32)
    with np.errstate(all="ignore"):
        for c in range(n):
            v = val[c * k:(c + 1) * k]
            t = np.sum(v.astype(np.float64) ** 2) if k else np.float64(0)
            norm32 = np.float32(np.sqrt(t))
            cf = np.float32(np.float32(clipping) / norm32)
            coef[c] = cf if cf < 1 else np.float32(1)
            out[c * k:(c + 1) * k] = v * coef[c]
    return coef, out


def clip_model(val, n, clipping):
    """the clipped values alone, of n clients with val.size / n values each"""
    val = np.ascontiguousarray(val, np.float32).ravel()
    return clip_coefs(val, n, val.size // n, clipping)[1]


# ------------------------------------------------------------- reference ----
def reference(oracle, alg, idx, val, n, k, d, kw):
    """the alg's CPU reference on these records, averaged by 1 / n"""
    w = oracle.as_weights(idx, val)
    if alg == 1:
        ref, st = oracle.advanced(kw.get("k_req", k), w, d, n)
    elif alg == 2:
        ref, st = oracle.nips19(k, w, d, n, seed=kw["seed"])
    elif alg == 6:
        ref, st = oracle.client_size_optimized(kw["batch"], k, w, d, n)
    elif alg == 7:
        ref, st = model(idx, val, n, d), 0
    elif alg == 3:
        ref, st = oracle.baseline(w, d, n), 0
    else:
        ref, st = {4: oracle.non_oblivious, 5: oracle.path_oram}[alg](w, d, n)
    assert st == 0
    return ref


def bincount_sums(idx, val, d):
    """the un-averaged sums of the records with idx < d, in f64 -> f32: the reference of any
    route on lattice inputs (every partial sum is exact, so the order cannot matter)"""
    idx = np.asarray(idx, np.int64)
    keep = idx < d
    s = np.bincount(idx[keep], weights=np.asarray(val, np.float64)[keep], minlength=d)
    out = s.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), s)
    return out


def indices(rng, n, k, d, dense):
    """every client's k indices distinct; a dense upload has idx j in slot j"""
    if dense:
        return np.tile(np.arange(d, dtype=np.uint32), n)
    if k == 0:
        return np.zeros(0, np.uint32)
    if d > 1 << 20:  # (a permutation of d a client is too slow: distinct by construction)
        return np.concatenate([np.sort(rng.choice(d // k, k, replace=False)) * k + rng.integers(0, k, k)
                               for _ in range(n)]).astype(np.uint32)
    return distinct_indices(rng, n, k, d)


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# --------------------------------------------------------------- lattice ----
LATTICE_CLIPPING = 3.0
# (q, a, cf): q records of +-a (a a power of two), norm a * sqrt(q) exactly, clipping 3.
# Neighbouring clients have different coefficients, and different clipped magnitudes a * cf
# (1.5, 1, 0.75, 0.5, 1, 0): a coefficient read from another client changes bits.
LATTICE = [
    (4, 2.0, 0.75),    # norm 4
    (9, 2.0, 0.5),     # norm 6
    (16, 2.0, 0.375),  # norm 8
    (4, 0.5, 1.0),     # norm 1: not clipped (3 / 1 -> 1)
    (9, 1.0, 1.0),     # norm 3: cf == 1.0 exactly, the !(cf < 1) edge
    (0, 0.0, 1.0),     # all zeros: 3 / 0 = inf -> 1
]
# for k < 16: q in {1, 4}
LATTICE_SMALL = [
    (4, 2.0, 0.75),    # norm 4
    (1, 8.0, 0.375),   # norm 8
    (4, 0.5, 1.0),     # norm 1
    (0, 0.0, 1.0),
    (1, 4.0, 0.75),    # norm 4
    (4, 4.0, 0.375),   # norm 8
]


@functools.lru_cache(maxsize=None)
def lattice(n, k, d, dense=False):
    """(idx, val, coef): client c is LATTICE[c % 6] (LATTICE_SMALL where k < 16): q records
    of +-a at random places of its k, 0.0 elsewhere.  Every clipped value is a multiple of
    2^-4, and every sum of n <= 512 of them lies below 2^10: exact in f32 in any order."""
    assert n <= 512
    rng = _rng("lattice", n, k, d, dense)
    table = LATTICE if k >= 16 else LATTICE_SMALL
    idx = indices(rng, n, k, d, dense)
    val = np.zeros(n * k, np.float32)
    coef = np.ones(n, np.float32)
    for c in range(n):
        q, a, cf = table[c % len(table)]
        if k < q:
            q, a, cf = 0, 0.0, 1.0
        at = c * k + rng.choice(k, q, replace=False) if q else np.zeros(0, np.int64)
        val[at] = np.float32(a) * rng.choice(np.array([-1, 1], np.float32), q)
        coef[c] = cf
    for a in (idx, val, coef):
        a.setflags(write=False)
    return idx, val, coef


def lattice_prev(d):
    """what accumulate finds in out: multiples of 2^-4 below 2^6"""
    return (_rng("prev", d).integers(-1023, 1024, d) / 16.0).astype(np.float32)


# --------------------------------------------------------------- general ----
GENERAL_CLIPPING = 0.5
MARGIN = 2.0 ** -36


def midpoint_margin(t):
    """how far sqrt(t) (f64) lies from the nearest f32 rounding midpoint, relative to it"""
    s = np.sqrt(np.float64(t))
    f = np.float32(s)
    lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
    mids = [(np.float64(lo) + np.float64(f)) / 2, (np.float64(f) + np.float64(hi)) / 2]
    return min(abs(s - m) for m in mids) / s


def general_ok(val, n, k):
    """The device sums the squares in another order than this model (256 strided lanes, then
    shuffles): its t is within (k / 256 + 11) * 2^-53 relative of the exact sum, numpy's
    pairwise sum within (128 + log2 k) * 2^-53, and sqrt halves a relative error.  With
    sqrt(t) further than 2^-36 from every f32 midpoint both round to the same norm32 up to
    k = 2^24 (2^16 * 2^-53 = 2^-37)."""
    if k == 0:
        return True
    v = np.asarray(val, np.float64).reshape(n, k)
    return all(midpoint_margin(np.sum(r * r)) > MARGIN for r in v)


def general_values(n, k, d, dense, seed):
    rng = _rng("general", n, k, d, dense, seed)
    idx = indices(rng, n, k, d, dense)
    return idx, (rng.normal(0, 1, n * k) * 100).astype(np.float32)


@functools.lru_cache(maxsize=None)
def general(n, k, d, dense=False):
    """(idx, val, seed): deterministic in the shape; the first seed whose every client norm
    keeps the margin (a condition on the input, not a tolerance:
    tests/test_options_model.py asserts that seed 0 already does for every shape in use)."""
    for seed in range(64):
        idx, val = general_values(n, k, d, dense, seed)
        if general_ok(val, n, k):
            idx.setflags(write=False)
            val.setflags(write=False)
            return idx, val, seed
    raise AssertionError("no seed keeps the margin")
