"""The sums of `nsk_state_get_record` for subdivided patches stated once more, in extended precision, from
exactly what the library is handed: per listed cell and point pt = l (s+1) + k

    u_c(pt) = sum_n W_u[pt][n] u_c[node n of the cell]   (c = x, y; 16 nodes)      p(pt) = sum_m W_p[pt][m] p[DoF m]   (9)

evaluated in `np.longdouble` (64-bit mantissa on x86) on the double-precision tables and state.  Next to the values it
returns A_pt = sum |W state|, the sum of the absolute values of the elementary products: what a rounding error of the
double-precision evaluation is proportional to.

Not collected by pytest (no test_ prefix): tests/test_vtu_record.py and tests/test_gpu_record.py import it.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def record_sums(cell_u_nodes, cell_p_dofs, cells, w_u, w_p, u_local, p_local):
    """(vel [n_cells, ppc, 2], prs [n_cells, ppc], A_vel, A_prs) as np.longdouble; u_local / p_local: [owned | ghost]."""
    cells = np.asarray(cells, np.int64)
    wu, wp = np.asarray(w_u, np.float64).astype(LD), np.asarray(w_p, np.float64).astype(LD)
    u, p = np.asarray(u_local, np.float64).astype(LD), np.asarray(p_local, np.float64).astype(LD)
    un, pn = np.asarray(cell_u_nodes, np.int64)[cells], np.asarray(cell_p_dofs, np.int64)[cells]
    su = np.stack([u[2 * un], u[2 * un + 1]], axis=2)                       # [cell, n, c]
    prod_u = wu[None, :, :, None] * su[:, None, :, :]                        # [cell, pt, n, c]
    prod_p = wp[None, :, :] * p[pn][:, None, :]                              # [cell, pt, m]
    return prod_u.sum(axis=2), prod_p.sum(axis=2), np.abs(prod_u).sum(axis=2), np.abs(prod_p).sum(axis=2)
