"""NumPy statement of the matrix-free F (NSK_OPT_INNER_MATRIX_FREE_F), in np.longdouble.

TEST INFRASTRUCTURE ONLY.  Inputs come from problem.generate (tabulation, cells, flags) and a state; nothing is read
from the library.  With U, G = grad U the state and x_c, dx x_c, dy x_c the input at quadrature point q of a cell,
w = JxW[q]:

    a_c  = w (U0 dx x_c + U1 dy x_c + G[c][0] x_0 + G[c][1] x_1 + inv_dt x_c)     (Stokes phase: the inv_dt term only)
    bx_c = w nu dx x_c,  by_c = w nu dy x_c
    y[2n+c] = sum_{cells k of n} sum_q phi_n(q) a_c(q) + dphi_n/dx(q) bx_c(q) + dphi_n/dy(q) by_c(q)

Dirichlet rows: y = d0 x with d0 = |entry (0,0) of the uncleared block| (the cell of DoF 0, node 0, component 0).

Besides y the function returns A_i: the sum of the absolute values of EVERY elementary product of row i, the state's
interpolation included (|u_j phi_j(q)| instead of |U(q)|) — the quantity a rounding-error bound C 2^-53 A_i of any
summation order of these products is stated in, whether the products are first collected into matrix entries (the
assembled F) or into fluxes (the kernels).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# Roundings one elementary product can pass before it is part of y_i (multiplications and additions counted one each:
# an upper bound, FMA contraction only removes some).
# Kernels (nsk_assembly_kernels.hip): asm_cell_state_kernel 16 + 1 (U or G at a point); mf_cell_flux_kernel: the
# interpolation of x 16 + 1, U * dx x 1, the sum a_c 5 (inv_dt x_c, then four terms), w * a_c 1 (w nu: 2), the
# contraction 1 + 2 + 16 (product, the three terms of a point, the chain over q); mf_rows_kernel 4.  Dirichlet rows pass
# fewer (asm_d0_kernel ~ 40).
C_KERNEL = 17 + 17 + 1 + 5 + 2 + 19 + 4
# The handle's own assembled product: asm_cell_state 17; asm_F_rows_kernel: adv 2, adv + G phi_m 2, w = JxW phi_n and its
# product 2, the chain over q 16, + nu K + inv_dt M3 1 (the table entries themselves: 16 points x (2 products, 1 sum, w, the
# chain) <= 21, + 2 + 1 — the shorter path), the four cells 4; then the 2x2 node-block SpMV of a row of <= 49 blocks:
# tests/spmv_reference.py, roundings("blk_c2", 49) = 2 + 12 + 2.
C_ASSEMBLED_GPU = 17 + 2 + 2 + 2 + 16 + 1 + 4 + 16
# The host hand-off producer (problem_gen.cpp) and SciPy's CSR product: conv_element 17 (u, g), adv 2, + g phi 2, w 2,
# the chain over q 16; row_F: nu K + inv_dt M3 and the two accumulations per cell, four cells: 12; F @ x: one product
# and a chain of <= 98 entries.
C_HOST = 17 + 2 + 2 + 2 + 16 + 12 + 99
C_REFERENCE = 1   # the longdouble sums below: ~70 x 2^-64 A_i, far under one unit of 2^-53 A_i


def node_cells(cell_u, n_nodes):
    """[n_nodes, 4] cell * 16 + local node, -1 where unused; cells ascending — the order nsk_assembly_set_cells keeps."""
    out = -np.ones((n_nodes, 4), dtype=np.int64)
    cnt = np.zeros(n_nodes, dtype=np.int64)
    for c in range(cell_u.shape[0]):
        for n in range(16):
            node = cell_u[c, n]
            if node < n_nodes:
                out[node, cnt[node]] = c * 16 + n
                cnt[node] += 1
    return out


def matfree_reference(tables, cell_u, dirichlet, cell_of_dof0, state_u, x, nu, inv_dt, stokes):
    """(y, A): y = F x in longdouble, A_i the absolute sum of row i's elementary products (float64)."""
    T = np.asarray(tables, dtype=LD)
    phi, dpx, dpy, w = T[0:256].reshape(16, 16), T[256:512].reshape(16, 16), T[512:768].reshape(16, 16), T[912:928]
    tab = (phi, dpx, dpy)
    tab_a = tuple(np.abs(t) for t in tab)
    cell_u = np.asarray(cell_u, dtype=np.int64)
    n_u = len(dirichlet)
    x = np.asarray(x, dtype=LD)
    su = np.asarray(state_u, dtype=LD)
    nu, inv_dt = LD(nu), LD(inv_dt)

    def at_points(v, absolute):
        """value, d/dx, d/dy of the nodal vector v [cells, 16] at the 16 points: three [cells, 16] arrays"""
        return tuple((np.abs(v) if absolute else v) @ t for t in (tab_a if absolute else tab))

    def apply(xv, absolute, cells):
        """the shares [2][cells, 16 nodes] of `cells` [cells, 16] in their node rows, for nodal input xv [2][cells, 16]"""
        X = [at_points(xv[c], absolute) for c in range(2)]          # X[c] = (x_c, dx x_c, dy x_c)
        Us = [at_points(su[2 * cells + c], absolute) for c in range(2)]   # Us[c] = (U_c, G[c][0], G[c][1])
        ph, dx, dy = tab_a if absolute else tab
        wa = np.abs(w) if absolute else w
        out = []
        for c in range(2):
            a = inv_dt * X[c][0]
            if not stokes:
                a = a + Us[0][0] * X[c][1] + Us[1][0] * X[c][2] + Us[c][1] * X[0][0] + Us[c][2] * X[1][0]
            out.append((wa * a) @ ph.T + (wa * nu * X[c][1]) @ dx.T + (wa * nu * X[c][2]) @ dy.T)
        return out

    xv = [x[2 * cell_u + c] for c in range(2)]
    y, A = np.zeros(n_u, dtype=LD), np.zeros(n_u, dtype=LD)
    for arr, absolute in ((y, False), (A, True)):
        r = apply(xv, absolute, cell_u)
        for c in range(2):
            np.add.at(arr, (2 * cell_u + c).ravel(), r[c].ravel())
    # the Dirichlet diagonal: the bilinear form of the cell of DoF 0 on the unit vector of its node 0, component 0
    e = np.zeros((1, 16), dtype=LD)
    e[0, 0] = 1
    zero = np.zeros((1, 16), dtype=LD)
    first = cell_u[cell_of_dof0:cell_of_dof0 + 1]
    d0 = abs(apply([e, zero], False, first)[0][0, 0])
    d0_abs = apply([e, zero], True, first)[0][0, 0]
    d = np.asarray(dirichlet).astype(bool)
    y[d] = d0 * x[d]
    A[d] = d0_abs * np.abs(x[d])
    return y, A.astype(np.float64), d0
