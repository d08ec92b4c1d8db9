"""Vorticity and divergence of `nsk_state_get_record_fields` stated once more, in extended precision and
independently of the library.

Q3/Q2 — per listed cell and point pt = l (s+1) + k, with the tables D_x, D_y [(s+1)^2, 16]:

    g_cd(pt) = sum_n D_d[pt][n] u_c[node n of the cell]       vorticity = g_10 - g_01       divergence = g_00 + g_11

`gradient_tables(s, hx, hy)` builds the tables in `np.longdouble` (64-bit mantissa on x86) from the 1-D Lagrange derivatives
on the degree-3 Gauss-Lobatto nodes: D_x[pt][b*4+a] = L'_a(t_k) L_b(t_l) / hx, D_y[pt][b*4+a] = L_a(t_k) L'_b(t_l) / hy.  They
judge the double-precision tables of the product.  `q3_fields` takes the tables it is given — the tests hand it the very
doubles the library was handed, so that the bound below holds the kernel alone to account — and returns next to each value
A_pt = sum_n |D_d[pt][n]| |u_c[n]| over the elementary products of the field (32 of them).

P2/P1 — per vertex v, over the entries e of vert_ptr / vert_ent (cell t = code // 3, local vertex lv = code % 3):

    value(v) = (sum_t area_t f_t(v)) / (sum_t area_t),     f_t(v) from g_cd = sum_k u_c[node k] (sum_i dl_i(k) grad_lam[t][i][d])

with the barycentric derivatives dl of the six P2 functions (vertices 0-2, then the edges (0,1), (1,2), (2,0)) at lambda = e_lv.
`p2_fields` returns the values, A_v = (sum_t area_t sum |u_c[k]| |dl_i| |grad_lam[t][i][d]|) / (sum_t area_t) and the number
of cells m_v of each vertex.

The constants of the bound |result - exact| <= C 2^-53 A, counted from the kernels in csrc/nsk_assembly_kernels.hip as the
number of roundings an elementary product can pass.  No measured figure enters.

record_fields_kernel:
    g += D[n] * u[n], n = 0..15, one accumulator from 0.0: the product rounds once (not at all when fused), the first
    addition (to 0.0) is exact, each of the 15 later ones rounds                                                          16
    g_10 - g_01 (or g_00 + g_11)                                                                                           1
    the terms of second order ((1 + u)^17 - 1 <= 17 u (1 + 1e-14)) and the rounding of this reference (2^-64 per step)      1
                                                                                                               C_Q3 = 18
simplex_record_fields_kernel, a vertex of m cells:
    dl_i at a vertex is one of -1, 0, 3, 4: exact.  gx = dl_0 gl_0 + dl_1 gl_2 + dl_2 gl_4: a product and two additions     3
    g += u * gx, k = 0..5: a product, the first addition exact, five later ones                                            6
    g_10 - g_01 (or g_00 + g_11)                                                                                           1
    area * (...)                                                                                                           1
    the sum over the cells: the first addition exact, m - 1 later ones                                                 m - 1
    the sum of the (positive) areas: m - 1 additions, each a relative error of the denominator                         m - 1
    the division                                                                                                           1
    second order and the reference's own rounding                                                                          1
                                                                                                    C_P2(m) = 12 + 2 m

Not collected by pytest (no test_ prefix).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C_Q3 = 18


def c_p2(m):
    return 12 + 2 * np.asarray(m)


def _gll():
    r = LD(1) / np.sqrt(LD(5))
    return np.array([LD(0), (LD(1) - r) / 2, (LD(1) + r) / 2, LD(1)], LD)


def lagrange_1d(t):
    """(L [point, basis], L' [point, basis]) of the four Lagrange functions on the Gauss-Lobatto nodes, in longdouble."""
    t = np.asarray(t, LD)
    x = _gll()
    val, der = np.ones((len(t), 4), LD), np.zeros((len(t), 4), LD)
    for a in range(4):
        for b in range(4):
            if b != a:
                val[:, a] *= (t - x[b]) / (x[a] - x[b])
        for b in range(4):
            if b == a:
                continue
            term = np.ones(len(t), LD) / (x[a] - x[b])
            for c in range(4):
                if c not in (a, b):
                    term = term * (t - x[c]) / (x[a] - x[c])
            der[:, a] += term
    return val, der


def gradient_tables(s, hx, hy):
    """(D_x, D_y) [(s+1)^2, 16] in longdouble."""
    t = np.arange(s + 1).astype(LD) / LD(s)
    v, d = lagrange_1d(t)
    dx, dy = np.zeros(((s + 1) ** 2, 16), LD), np.zeros(((s + 1) ** 2, 16), LD)
    for l in range(s + 1):
        for k in range(s + 1):
            for b in range(4):
                for a in range(4):
                    dx[l * (s + 1) + k, b * 4 + a] = d[k, a] * v[l, b] / LD(hx)
                    dy[l * (s + 1) + k, b * 4 + a] = v[k, a] * d[l, b] / LD(hy)
    return dx, dy


def q3_fields(cell_u_nodes, cells, d_x, d_y, u_local):
    """(vorticity, divergence, A_vorticity, A_divergence), each [n_cells, ppc] in longdouble; u_local: [owned | ghost]."""
    cells = np.asarray(cells, np.int64)
    dx, dy = np.asarray(d_x).astype(LD), np.asarray(d_y).astype(LD)
    u = np.asarray(u_local, np.float64).astype(LD)
    un = np.asarray(cell_u_nodes, np.int64)[cells]
    ux, uy = u[2 * un], u[2 * un + 1]                                       # [cell, n]
    p00, p01 = dx[None] * ux[:, None, :], dy[None] * ux[:, None, :]          # [cell, pt, n]
    p10, p11 = dx[None] * uy[:, None, :], dy[None] * uy[:, None, :]
    g00, g01, g10, g11 = (p.sum(axis=2) for p in (p00, p01, p10, p11))
    a00, a01, a10, a11 = (np.abs(p).sum(axis=2) for p in (p00, p01, p10, p11))
    return g10 - g01, g00 + g11, a10 + a01, a00 + a11


def _p2_dl(k, lv):
    """Barycentric derivatives of P2 function k at the vertex lambda = e_lv."""
    lam = [LD(1) if i == lv else LD(0) for i in range(3)]
    dl = [LD(0)] * 3
    if k < 3:
        dl[k] = 4 * lam[k] - 1
    else:
        i, j = k - 3, (k - 2) % 3
        dl[i], dl[j] = 4 * lam[j], 4 * lam[i]
    return dl


def p2_fields(cell_u, grad_lam, area, vert_ptr, vert_ent, u):
    """(vorticity, divergence, A_vorticity, A_divergence, m) per vertex; a vertex of no cell gets 0 (and A = 0)."""
    cu = np.asarray(cell_u, np.int64)
    gl = np.asarray(grad_lam, np.float64).reshape(-1, 3, 2).astype(LD)
    ar = np.asarray(area, np.float64).astype(LD)
    u = np.asarray(u, np.float64).astype(LD)
    n = len(vert_ptr) - 1
    out = np.zeros((4, n), LD)
    m = np.diff(np.asarray(vert_ptr, np.int64))
    for v in range(n):
        sw = sd = aw = ad = sa = LD(0)
        for e in range(vert_ptr[v], vert_ptr[v + 1]):
            t, lv = divmod(int(vert_ent[e]), 3)
            g = np.zeros((2, 2), LD)
            a = np.zeros((2, 2), LD)
            for k in range(6):
                dl = _p2_dl(k, lv)
                for c in range(2):
                    uc = u[2 * cu[t, k] + c]
                    for d in range(2):
                        for i in range(3):
                            g[c, d] += uc * dl[i] * gl[t, i, d]
                            a[c, d] += abs(uc) * abs(dl[i]) * abs(gl[t, i, d])
            sw += ar[t] * (g[1, 0] - g[0, 1])
            sd += ar[t] * (g[0, 0] + g[1, 1])
            aw += ar[t] * (a[1, 0] + a[0, 1])
            ad += ar[t] * (a[0, 0] + a[1, 1])
            sa += ar[t]
        if sa > 0:
            out[:, v] = sw / sa, sd / sa, aw / sa, ad / sa
    return out[0], out[1], out[2], out[3], m
