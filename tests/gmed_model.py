"""The geometric median of FLTEE_OPT_GMED (include/fltee_agg.h) in numpy, independent of the
library: the one definition the kernels (k_gmed.hip) are held to.  The "RFA" of Pillutla, Kakade
and Harchaoui (2022): R iterations of the smoothed Weiszfeld iteration with the floor nu, run on
the Gram matrix alone.

n clients, d coordinates.  x_c[j] is the value the dense route would add for client c at j (clip:
v * coef_c in f32, options_model.clip_coefs).  All f64 arithmetic is numpy's round-to-nearest add,
multiply, divide and sqrt, one operation at a time.  sum64(v) over indices 0 .. n - 1:
  p_l    = the sum of v_i over i = l (mod 64), ascending, from +0.0;
  result = p_0 ... p_63 added in ascending l, from +0.0.
The steps:
  1. G[a][b] = sum_j f64(x_a[j]) * f64(x_b[j])   every product exact, the order of the sum free
               (here: numpy's), the same for every entry;
  2. valid_c = G[c][c] is finite;
  3. w_c     = valid_c ? 1.0 : 0.0;
  4. R times: s = sum64(w); u_a = sum64_b(valid_b ? G[a][b] * w_b : +0.0);
              q = sum64_a(valid_a ? w_a * u_a : +0.0); inv = s > 0 ? 1 / s : 0;
              D_a = (G_aa - 2 * (u_a * inv)) + (q * inv) * inv, not finite -> +inf, not above 0 -> +0.0;
              rho_a = sqrt(D_a); w_a = valid_a ? 1 / max(nu, rho_a) : 0;
  5. s = sum64(w); alpha_c = f32(s > 0 ? w_c / s : 0);
  6. out[j] = (((+0.0 + y_0) + y_1) + ...) in f32, y_c = valid_c ? x_c[j] * alpha_c : +0.0.
"""
import numpy as np

from options_model import clip_coefs

GMED_MAX_N = 1024
GMED_MAX_ITERS = 64
NU = 2.0 ** -20


def refused(n, iters, nu):
    """the refusals that depend on (n, R, nu) alone"""
    return n == 0 or n > GMED_MAX_N or iters == 0 or iters > GMED_MAX_ITERS or not (0 < nu < np.inf)


def sum64(v):
    """the one reduction order, along the last axis of v (f64 [..., n]) -> f64 [...]"""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    p = np.zeros(v.shape[:-1] + (64,), np.float64)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, 64):  # lane l adds i = l, l + 64, ... in ascending order
            part = v[..., i0:i0 + 64]
            p[..., :part.shape[-1]] = p[..., :part.shape[-1]] + part
        s = np.zeros(v.shape[:-1], np.float64)
        for lane in range(64):
            s = s + p[..., lane]
    return s


def clipped(values, clip):
    v = np.ascontiguousarray(values, np.float32)
    n, d = v.shape
    if clip is not None:
        v = clip_coefs(v.reshape(-1), n, d, clip)[1].reshape(n, d)
    return v


def gram(values):
    x = np.ascontiguousarray(values, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return x @ x.T


def gram_longdouble(values):
    """G by a sequential sum over j in longdouble, rounded to f64 once: another conforming order"""
    x = np.ascontiguousarray(values, np.float32).astype(np.longdouble)
    n, d = x.shape
    G = np.zeros((n, n), np.longdouble)
    for j in range(d):
        G += np.outer(x[:, j], x[:, j])
    return G.astype(np.float64)


def iterate(G, valid, w, nu):
    """one iteration of step 4 -> (w', rho)"""
    with np.errstate(all="ignore"):
        s = sum64(w)
        u = sum64(np.where(valid[None, :], G * w[None, :], 0.0))
        q = sum64(np.where(valid, w * u, 0.0))
        inv = np.float64(1.0) / s if s > 0 else np.float64(0.0)
        D = (np.diag(G) - 2.0 * (u * inv)) + (q * inv) * inv
        D = np.where(np.isfinite(D), D, np.inf)
        D = np.where(D > 0, D, 0.0)
        rho = np.sqrt(D)
        w = np.where(valid, 1.0 / np.maximum(np.float64(nu), rho), 0.0)
    return w, rho


def weights_from(G, iters, nu):
    """steps 2 - 5 on a Gram matrix -> (alpha f32 [n], rho f64 [n], valid bool [n])"""
    G = np.asarray(G, np.float64)
    valid = np.isfinite(np.diag(G))
    w = np.where(valid, 1.0, 0.0)
    rho = None
    for _ in range(iters):
        w, rho = iterate(G, valid, w, nu)
    s = sum64(w)
    with np.errstate(all="ignore"):
        alpha = (w / s if s > 0 else np.zeros_like(w)).astype(np.float32)
    return alpha, rho, valid


def weights(values, iters, nu=NU, clip=None):
    """fltee_gmed_weights_device: (alpha f32 [n], rho f64 [n], valid bool [n])"""
    v = clipped(values, clip)
    assert not refused(v.shape[0], iters, nu)
    return weights_from(gram(v), iters, nu)


def weighted_sum(values, alpha, valid):
    """step 6, f32 [d]: an invalid client adds a selected +0.0, never its value"""
    v = np.ascontiguousarray(values, np.float32)
    alpha = np.asarray(alpha, np.float32)
    acc = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for c in range(v.shape[0]):
            y = (v[c] * alpha[c]).astype(np.float32) if valid[c] else np.float32(0)
            acc = (acc + y).astype(np.float32)
    return acc


def gmed(values, iters, nu=NU, clip=None, prev=None, alpha=None, valid=None):
    """fltee_aggregate_device with FLTEE_OPT_GMED on n dense uploads values[n, d]; clip: the
    FLTEE_OPT_CLIP bound; prev: FLTEE_OPT_ACCUMULATE on what out held; alpha, valid: step 6 alone
    on given weights"""
    v = clipped(values, clip)
    if alpha is None:
        alpha, _, valid = weights(v, iters, nu)
    s = weighted_sum(v, alpha, valid)
    if prev is not None:
        with np.errstate(all="ignore"):
            return (np.asarray(prev, np.float32) + s).astype(np.float32)
    return s


# ---- the iteration in the plain (not Gram) form: what the model's own tests compare against ----
def objective(values, z, nu):
    """the smoothed objective sum_c max(nu, |x_c - z|) in f64"""
    x = np.asarray(values, np.float64)
    return np.maximum(nu, np.sqrt(((x - z[None, :]) ** 2).sum(axis=1))).sum()


def iterate_of(values, alpha):
    """z = sum_c alpha_c x_c in f64"""
    return np.asarray(alpha, np.float64) @ np.asarray(values, np.float64)
