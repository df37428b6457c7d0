"""Multi-Krum of FLTEE_OPT_KRUM (include/fltee_agg.h) in numpy, independent of the library: the
one definition the kernels (k_krum.hip) are held to.

n clients, d coordinates, f assumed Byzantine clients, m clients kept.  x_c[j] is the value the
dense route would add for client c at j (clip: v * coef_c in f32, options_model.clip_coefs).
  G[a][b] = sum_j f64(x_a[j]) * f64(x_b[j])   every product exact, the order of the sum free
            (here: numpy's), the same for every entry;
  D[a][b] = (G[a][a] + G[b][b]) - 2 G[a][b]   in f64, in that association; NaN / +-inf -> +inf,
            anything not above 0 -> +0.0;
  s_a     = the f64 sum of the q = n - f - 2 smallest D[a][b], b != a, added in ascending order
            from +0.0;
  kept    = the m clients smallest by (s ascending, client ascending);
  sum     = ((+0.0 + x_c1) + x_c2) + ... over the kept clients in upload order, f32;
  out[j]  = sum * (f32(1) / f32(div)), div = n_avg or m.
"""
import numpy as np

from options_model import clip_coefs

KRUM_MAX_N = 1024


def refused(n, f, m):
    """the refusals that depend on (n, f, m) alone"""
    return n < 2 * f + 3 or m == 0 or m > n - f or n > KRUM_MAX_N


def gram(values):
    """f64 [n, n]: G, and the reordering bound's sum_j |x_a x_b| beside it"""
    x = np.ascontiguousarray(values, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return x @ x.T, np.abs(x) @ np.abs(x).T


def distances(G):
    n = G.shape[0]
    g = np.diag(G)
    with np.errstate(all="ignore"):
        D = (g[:, None] + g[None, :]) - 2.0 * G
    D = np.where(np.isfinite(D), D, np.inf)
    D = np.where(D > 0, D, 0.0)  # (an inf stays: inf > 0)
    assert D.shape == (n, n)
    return D


def sorted_rows(D):
    """f64 [n, n - 1]: every row's distances to the others, ascending"""
    n = D.shape[0]
    return np.stack([np.sort(np.delete(D[a], a)) for a in range(n)])


def scores_from(D, f):
    n = D.shape[0]
    q = n - f - 2
    rows = sorted_rows(D)
    s = np.zeros(n, np.float64)
    for i in range(q):  # ascending, from +0.0
        s = s + rows[:, i]
    return s


def keep_from(s, m):
    """bool [n]: the m clients smallest by (s, index); +inf last, in upload order"""
    n = len(s)
    order = sorted(range(n), key=lambda a: (s[a], a))
    keep = np.zeros(n, bool)
    keep[order[:m]] = True
    return keep


def clipped(values, clip):
    v = np.ascontiguousarray(values, np.float32)
    n, d = v.shape
    if clip is not None:
        v = clip_coefs(v.reshape(-1), n, d, clip)[1].reshape(n, d)
    return v


def select(values, f, m, clip=None):
    """fltee_krum_select_device: (scores f64 [n], keep bool [n])"""
    v = clipped(values, clip)
    n = v.shape[0]
    assert not refused(n, f, m)
    s = scores_from(distances(gram(v)[0]), f)
    return s, keep_from(s, m)


def in_order_sum(values, keep):
    """f32 [d]: a dropped client adds a selected +0.0, never its value"""
    v = np.ascontiguousarray(values, np.float32)
    acc = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for c in range(v.shape[0]):
            acc = (acc + (v[c] if keep[c] else np.float32(0))).astype(np.float32)
    return acc


def krum(values, f, m, n_avg=0, clip=None, no_average=False, prev=None, keep=None):
    """fltee_aggregate_device with FLTEE_OPT_KRUM on n dense uploads values[n, d]; clip: the
    FLTEE_OPT_CLIP bound; prev: FLTEE_OPT_ACCUMULATE on what out held"""
    v = clipped(values, clip)
    if keep is None:
        keep = select(v, f, m)[1]
    s = in_order_sum(v, keep)
    with np.errstate(all="ignore"):
        if prev is not None:
            return (np.asarray(prev, np.float32) + s).astype(np.float32)
        if no_average:
            return s
        div = n_avg if n_avg else m
        return (s * (np.float32(1) / np.float32(div))).astype(np.float32)


# ---- the condition on a general input, and the score tolerance -------------------------------
# A sum of d exact products in any order differs from the exact sum by at most
# (d - 1) u sum_j |x_a x_b| (1 + O(d u)), u = 2^-53: the bound e[a][b] on one G entry.  Two
# implementations therefore differ by at most 2 e.  D adds three entries: |dD[a][b]| <= 2 (e_aa +
# e_bb + 2 e_ab) plus the two roundings of its own, 2 u |terms|; a score adds q of them in the
# same order once their order agrees, each addition rounding by u s.
def gram_bound(values):
    v = np.ascontiguousarray(values, np.float32)
    d = v.shape[1]
    return (d - 1) * 2.0 ** -53 * gram(v)[1]


def distance_bound(values):
    e = gram_bound(values)
    g = np.diag(e)
    return g[:, None] + g[None, :] + 2.0 * e


def score_bound(values, f):
    """per client: what two conforming implementations' scores may differ by"""
    v = np.ascontiguousarray(values, np.float32)
    n = v.shape[0]
    q = n - f - 2
    G, A = gram(v)
    eD = 2.0 * distance_bound(v) + 4 * 2.0 ** -53 * (np.diag(A)[:, None] + np.diag(A)[None, :] + 2.0 * A)
    D = distances(G)
    bound = np.zeros(n)
    for a in range(n):
        others = np.delete(np.arange(n), a)
        pick = others[np.argsort(D[a, others], kind="stable")[:q]]
        bound[a] = eD[a, pick].sum() + (q + 1) * 2.0 ** -53 * D[a, pick].sum()
    return bound


def well_separated(values, f, m, factor=1000.0):
    """The condition a general input must meet before it is given to the GPU: the gap between
    the m-th and (m+1)-th score, and between the q-th and (q+1)-th distance of every row,
    exceeds `factor` times the reordering bound (d - 1) 2^-53 sum_j |x_a x_b| of the entries
    involved — so no conforming summation order can change a selection."""
    v = np.ascontiguousarray(values, np.float32)
    n = v.shape[0]
    q = n - f - 2
    D = distances(gram(v)[0])
    eD = distance_bound(v)
    s = scores_from(D, f)
    for a in range(n):
        others = np.delete(np.arange(n), a)
        o = others[np.argsort(D[a, others], kind="stable")]
        if q < n - 1:
            gap = D[a, o[q]] - D[a, o[q - 1]]
            if not gap > factor * max(eD[a, o[q]], eD[a, o[q - 1]]):
                return False
    order = sorted(range(n), key=lambda a: (s[a], a))
    if m < n:
        lo, hi = order[m - 1], order[m]
        sb = score_bound(v, f)
        if not s[hi] - s[lo] > factor * max(sb[lo], sb[hi]):
            return False
    return True
