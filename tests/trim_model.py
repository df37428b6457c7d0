"""The coordinate-wise trimmed mean of FLTEE_OPT_TRIM (include/fltee_agg.h) in numpy,
independent of the library: the one definition the kernel (k_trim.hip) is held to.

Per output j, with x_c client c's value at j (clip: v * coef_c in f32, options_model.clip_coefs):
  ord(x)  = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000), b = bits(x): a total order on every
            bit pattern, -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN;
  removal = first the t clients smallest by (ord ascending, c ascending); then, of those that
            remain, the t clients largest by (ord descending, c ascending);
  sum     = ((+0.0 + x_c1) + x_c2) + ... over the kept clients in upload order, f32;
  out[j]  = sum * (f32(1) / f32(div)), div = n_avg or n - 2 t.
"""
import numpy as np

from options_model import clip_coefs

TRIM_MAX = 64


def ord_key(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def trim_count(n, per_mille):
    """fltee_trim_count: the ECALL's trim count"""
    if n == 0:
        return 0
    return min(n * min(per_mille, 500) // 1000, (n - 1) // 2)


def kept(values, t):
    """bool [n, d]: the clients kept at each output"""
    v = np.ascontiguousarray(values, np.float32)
    n, d = v.shape
    assert 0 <= t and 2 * t < n
    o = ord_key(v).astype(np.int64)
    c = np.broadcast_to(np.arange(n)[:, None], (n, d))
    keep = np.ones((n, d), bool)
    cols = np.arange(d)
    if t:
        # np.lexsort sorts by the last key first: (ord ascending, c ascending) down each column
        low = np.lexsort((c, o), axis=0)[:t]
        keep[low, cols] = False
        # of those that remain: (ord descending, c ascending); the removed ones sort last
        o2 = np.where(keep, -o, np.int64(1) << 40)
        high = np.lexsort((c, o2), axis=0)[:t]
        keep[high, cols] = False
    assert (keep.sum(axis=0) == n - 2 * t).all()
    return keep


def sums(values, t):
    """f32 [d]: the kept clients' in-order sum"""
    v = np.ascontiguousarray(values, np.float32)
    keep = kept(v, t)
    acc = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for c in range(v.shape[0]):
            acc = np.where(keep[c], acc + v[c], acc).astype(np.float32)
    return acc


def trimmed(values, t, n_avg=0, clip=None, no_average=False, prev=None):
    """fltee_aggregate_device with FLTEE_OPT_TRIM on n dense uploads values[n, d]; clip: the
    FLTEE_OPT_CLIP bound; prev: FLTEE_OPT_ACCUMULATE on what out held"""
    v = np.ascontiguousarray(values, np.float32)
    n, d = v.shape
    if clip is not None:
        v = clip_coefs(v.reshape(-1), n, d, clip)[1].reshape(n, d)
    s = sums(v, t)
    with np.errstate(all="ignore"):
        if prev is not None:
            return (np.asarray(prev, np.float32) + s).astype(np.float32)
        if no_average:
            return s
        div = n_avg if n_avg else n - 2 * t
        return (s * (np.float32(1) / np.float32(div))).astype(np.float32)


def brute_column(col, t):
    """one column of the definition in plain Python (tests/test_trim_model.py)"""
    col = np.ascontiguousarray(col, np.float32)
    n = len(col)
    o = [int(x) for x in ord_key(col)]
    alive = list(range(n))
    for c in sorted(alive, key=lambda c: (o[c], c))[:t]:
        alive.remove(c)
    for c in sorted(alive, key=lambda c: (-o[c], c))[:t]:
        alive.remove(c)
    acc = np.float32(0)
    with np.errstate(all="ignore"):
        for c in sorted(alive):
            acc = np.float32(acc + col[c])
    return acc
