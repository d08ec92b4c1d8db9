"""Host references for the kernels of the fp32 inner Krylov basis (tests/test_gpu_inner_basis_precision.py).

The basis vectors are fp32 values, w and every sum are float64.  exact_dot of tests/krylov_reference.py gives the correctly
rounded sum of products (fp32 values are float64 values, so it applies as it stands); integer data gives sums that every
order of additions reproduces exactly.  The error bounds are counted from the kernels in csrc/nsk_kernels.hip:

multi_dot_f32_kernel / the norm of multi_axpy_f32_kernel.  The grid is red_grid_quads(n): one workgroup of 1024 threads
per 4096 quads of four entries, at most 256.  An accumulator takes one fused multiply-add per entry (the product is not
rounded), four per trip, T = ceil(quads / (grid * 1024)) trips, and thread 0 of workgroup 0 the up to three entries behind
the last quad.  reduce_finish then adds 6 times across the wavefront (shuffles), 16 wavefront sums, and in the last
workgroup one partial per thread (the grid never exceeds 1024), 6 shuffles and 16 wavefront sums again.  Every one of these
D = 4 T + 3 + (6 + 16) + 1 + (6 + 16) operations rounds a partial sum that is at most sum |w_i v_i| (1 + D u) in size:
    |s - exact| <= D u (1 + D u) sum_i |w_i v_i|,
held as 1.01 D u sum |w_i v_i| (D <= 84 at the largest size tested).

multi_axpy_f32_kernel.  An entry takes m fused multiply-adds, w -= h_k v_k for k in order, each rounding once a value that
is at most |w| + sum_k |h_k v_k| in size (times 1 + m u):
    |w' - exact| <= m u (1 + m u) (|w| + sum_k |h_k| |v_k|),
held as 1.01 m u scale, plus one u for the rounding of the reference itself (extended precision, rounded once).

vec_equ_f32.  y = (1 / a) x in float64, exactly as vec_equ forms it (one division for the scalar, one product per entry),
then one rounding to fp32, to nearest even: np.float32(y) bit for bit; the working vector is that float widened (exact).
"""
from __future__ import annotations

import math

import numpy as np

from tests import krylov_reference as R

U = R.U
GRID_CAP = 256       # red_grid_quads
THREADS = 1024       # RBLK
QUADS_PER_GROUP = 4096


def round_f32(x):
    """x rounded to fp32 (to nearest even) and widened again."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def is_f32(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.array_equal(round_f32(x), x))


def grid_quads(n):
    """Workgroups of the two sweeps (nsk::red_grid_quads)."""
    b = ((n >> 2) + QUADS_PER_GROUP - 1) // QUADS_PER_GROUP
    return max(1, min(GRID_CAP, b))


def trips(n):
    """Trips of the busiest thread: ceil(quads / (grid * 1024))."""
    t = grid_quads(n) * THREADS
    return ((n >> 2) + t - 1) // t


def depth(n):
    """Rounding operations on the longest path into one sum of n products (see the module docstring)."""
    return 4 * trips(n) + 3 + (6 + 16) + 1 + (6 + 16)


def dot_bound(n, w, v):
    return 1.01 * depth(n) * U * R.abs_dot(w, v)


def dots(w, V, rider=False):
    """Correctly rounded w . v_k for every k, and w . w behind them with the rider."""
    out = [R.exact_dot(w, v) for v in V]
    if rider:
        out.append(R.exact_dot(w, w))
    return np.array(out)


def int_dot(w, v):
    """Exact integer sum of products of integer-valued vectors (Python integers: no overflow)."""
    wi = np.asarray(w).astype(np.int64)
    vi = np.asarray(v).astype(np.int64)
    assert np.array_equal(wi, w) and np.array_equal(vi, v), "integer-valued data expected"
    assert np.abs(wi).max(initial=0) < 2 ** 20 and np.abs(vi).max(initial=0) < 2 ** 20
    return int(np.dot(wi.astype(object), vi.astype(object))) if wi.size < 4096 else _int_dot_blocks(wi, vi)


def _int_dot_blocks(wi, vi):
    # products below 2^40; blocks of 4096 sum below 2^52 in int64, the blocks are added as Python integers
    total = 0
    for i in range(0, wi.size, 4096):
        total += int(np.dot(wi[i:i + 4096], vi[i:i + 4096]))
    return total


def axpy(w, V, h):
    """w - sum_k h_k v_k in extended precision, rounded once, and the per-entry scale |w| + sum_k |h_k| |v_k|."""
    assert np.finfo(np.longdouble).nmant >= 63, "extended precision expected"
    acc = np.asarray(w, dtype=np.longdouble).copy()
    scale = np.abs(np.asarray(w, dtype=np.float64))
    for hk, v in zip(h, V):
        acc -= np.longdouble(hk) * np.asarray(v, dtype=np.longdouble)
        scale = scale + abs(float(hk)) * np.abs(np.asarray(v, dtype=np.float64))
    return acc.astype(np.float64), scale


def axpy_bound(m, scale):
    return (1.01 * m + 1.0) * U * scale


def normalise(x, a):
    """What vec_equ stores (float64), and what vec_equ_f32 stores: that rounded to fp32, and the float widened."""
    y = (1.0 / float(a)) * np.asarray(x, dtype=np.float64)
    v = y.astype(np.float32)
    return y, v, v.astype(np.float64)


def cgs_f32(w, V, one_red):
    """One Arnoldi column on an fp32 basis the way arnoldi_column does it (classical Gram-Schmidt in two sweeps): exactly
    rounded h_k = w . v_k, w' = w - sum h_k v_k, and |w'|^2 from w' (mode 1) or as max(w.w - sum h_k^2, 0) (mode 2)."""
    h = dots(w, V)
    wn, scale = axpy(w, V, h)
    if one_red:
        q, nrm = R.pythagoras(h, R.exact_dot(w, w))
    else:
        q = R.exact_dot(wn, wn)
        nrm = math.sqrt(q)
    return h, wn, scale, q, nrm


def launches(mode, m, rider=False):
    """Launches of one sweep over m basis vectors (+ the rider's output) with NSK_IOPT_GS_ONE_LAUNCH = mode."""
    cap = {1: 32, 2: 16, 0: 8}[mode]
    return (m + (1 if rider else 0) + cap - 1) // cap
