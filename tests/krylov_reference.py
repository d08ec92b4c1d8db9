"""Exact host references for the Krylov vector kernels (tests/test_gpu_krylov_kernels.py).

exact_dot gives the correctly rounded sum of products: every product x_i y_i is split into p_i + e_i exactly (Dekker's
TwoProduct, built from plain float64 operations, no fused multiply-add needed) and math.fsum rounds the exact sum of all
p_i and e_i once.  The Gram-Schmidt references take float64 steps with such dot products, so the only rounding they hold
is the one the update itself needs; modified and classical Gram-Schmidt are kept apart on purpose (see mgs / cgs).
The CG scalars and the Chebyshev step follow the formulas of nsk_kernels.hip (cg_fused_scalars, vec_cheby_step).
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -53                   # unit roundoff of float64
_SPLITTER = 134217729.0          # 2^27 + 1
_SPLIT_MAX = 1.99 * 2.0 ** 996   # |a| below this (1.33e300): the splitter's product (2^27 + 1) a cannot overflow
_PROD_MIN = 2.0 ** -960          # |x y| at least this (or 0): no partial product of the split loses a bit to underflow


def _split(a):
    """a = hi + lo exactly, hi and lo with at most 26 significant bits each (Veltkamp)."""
    c = _SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(x, y):
    """p, e with p = fl(x y) and p + e = x y exactly (Dekker), elementwise."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    p = x * y
    xh, xl = _split(x)
    yh, yl = _split(y)
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def _check_domain(x, y, p):
    if not (np.all(np.abs(x) < _SPLIT_MAX) and np.all(np.abs(y) < _SPLIT_MAX) and np.all(np.isfinite(p))):
        raise ValueError("exact_dot: an entry or a product is too large for an exact split")
    tiny = (p != 0.0) & (np.abs(p) < _PROD_MIN)
    if np.any(tiny) or np.any((p == 0.0) & (x != 0.0) & (y != 0.0)):
        raise ValueError("exact_dot: a product is too small for an exact error term")


def exact_dot(x, y):
    """The correctly rounded value of sum_i x_i y_i."""
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    y = np.ascontiguousarray(y, dtype=np.float64).ravel()
    with np.errstate(all="ignore"):
        p, e = two_product(x, y)
    _check_domain(x, y, p)
    return math.fsum(np.concatenate([p, e]))


def abs_dot(x, y):
    """sum_i |x_i y_i| (the scale of the summation-order error of any way of adding the products)."""
    return float(np.sum(np.abs(np.asarray(x) * np.asarray(y))))


def mgs(w, V):
    """Modified Gram-Schmidt as the sweep and the chain of launches do it: for k in order, h_k = w . v_k with the w
    every earlier link has updated, then w -= h_k v_k.  Returns (h, w, w.w) with exactly rounded dot products."""
    w = np.array(w, dtype=np.float64)
    h = []
    for v in V:
        hk = exact_dot(w, v)
        w = w - hk * v
        h.append(hk)
    return np.array(h), w, exact_dot(w, w)


def cgs(w, V):
    """Classical Gram-Schmidt as the fused passes do it: every h_k = w . v_k from the w that came in, then
    w -= sum_k h_k v_k (k in order).  Returns (h, w, w.w)."""
    w0 = np.array(w, dtype=np.float64)
    h = np.array([exact_dot(w0, v) for v in V])
    w = w0.copy()
    for hk, v in zip(h, V):
        w = w - hk * v
    return h, w, exact_dot(w, w)


def pythagoras(h, ww):
    """The one-reduction norm of gs_pythagoras: max(w.w - sum h_i^2, 0) in the kernel's order, and its root."""
    q = float(ww)
    for hi in h:
        q -= float(hi) * float(hi)
    q = q if q > 0.0 else 0.0
    return q, math.sqrt(q)


def cg_fused_scalars(sc, first):
    """cg_fused_scalars: sc = {gamma_new, delta, rr | gamma, alpha, beta, norm} -> the new sc[3..7)."""
    sc = [float(v) for v in sc]
    gn, dl = sc[0], sc[1]
    if first:
        beta, alpha = 0.0, gn / dl
    else:
        beta = gn / sc[3]
        alpha = gn / (dl - beta * gn / sc[4])
    return np.array([gn, dl, sc[2], gn, alpha, beta, math.sqrt(abs(sc[2]))])


def cg_fused_update(alpha, beta, u, w, p, s, x, r):
    """vec_cg_fused_update: p = u + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s."""
    p = u + beta * p
    s = w + beta * s
    return p, s, x + alpha * p, r - alpha * s


def cheby_step(c1, c2, dinv, r, w, x, set_x):
    """vec_cheby_step: w = c1 w + c2 dinv r (w not read when c1 == 0) ; x = set_x ? w : x + w."""
    wn = (c1 * w if c1 != 0.0 else 0.0) + c2 * dinv * r
    return wn, (wn.copy() if set_x else x + wn)


def nearly_parallel_case(n, m, eps=1e-3, seed=7):
    """w and m unit vectors all within ~eps of one direction (not orthogonal), w mostly along it: h_k of modified and
    classical Gram-Schmidt differ at O(1) here (CGS: every h_k ~ 8, MGS: h_0 ~ 8 and the rest ~ eps), so a kernel doing
    the one where the other is meant cannot pass."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n)
    e /= np.linalg.norm(e)
    V = []
    for _ in range(m):
        v = e + eps / math.sqrt(n) * rng.standard_normal(n)
        V.append(v / np.linalg.norm(v))
    w = 8.0 * e + rng.standard_normal(n) / math.sqrt(n)
    return w, V


def orthonormal_basis(n, m, seed=11):
    """m orthonormal vectors of length n (QR of a random matrix)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, m)))
    return [np.ascontiguousarray(q[:, k]) for k in range(m)]
