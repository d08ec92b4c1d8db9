"""The force integral of `nsk_forces` stated once more, in extended precision, from exactly what the library is handed.

    force = - sum over the faces of boundary id 10 of (nu (grad u + grad u^T) - p I) n JxW        (drag, lift)

(`NSSolverStationary::compute_lift_drag`, NSSolverStationary.cpp:836-897) with the fluid cell's outward normal n.

`q3_forces`: congruent Q3/Q2 cells — the face list (`face_cell`, `face_side`) and the 672-entry face tabulation of the
generator (include/nsk_problem.h).  `p2_forces`: P2/P1 triangles — the edge list of `simplex.force_edges` and the cells'
grad_lambda, two Gauss points per edge.

Everything is evaluated in `np.longdouble` (64-bit mantissa on x86: its own rounding is 2^-11 of a double's) from the
double-precision tables and state, so the result is the exact value of the sum the kernels approximate, to well below
one unit of the bound the tests use.  Next to the forces both functions return A = (A_drag, A_lift): the sum of the
absolute values of every elementary product of the integral, weights and normal components included — what a rounding
error of the double-precision evaluation is proportional to:

    Q3/Q2   A_drag = sum JxW (|n_x| (2 nu sum_n |u_x,n dphi_n/dx| + sum_m |p_m psi_m|)
                              + |n_y| nu (sum_n |u_x,n dphi_n/dy| + sum_n |u_y,n dphi_n/dx|))       (A_lift alike)
    P2/P1   the same with dphi_n/dx replaced by its own elementary products sum_l |dphi_n/dlambda_l dlambda_l/dx|
            (the kernel forms the gradient from the cell's grad_lambda) and psi by the barycentric coordinates.

Not collected by pytest (no test_ prefix): tests/test_forces_reference.py and tests/test_gpu_forces.py import it.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
NORMALS = ((-1.0, 0.0), (1.0, 0.0), (0.0, -1.0), (0.0, 1.0))       # face_side -> outward normal of the fluid cell
EDGES = ((0, 1), (1, 2), (2, 0))
GAUSS2 = (0.21132486540518712, 0.78867513459481288)                 # 1/2 -+ 1/(2 sqrt 3): the kernel's constants


def local_state(pr, u_global, p_global):
    """A rank's [owned | ghost] vectors from global ones (one rank: the global vectors)."""
    i = pr.info
    u = np.concatenate([u_global[i["u_begin"]:i["u_end"]], u_global[np.asarray(pr.ghost_u, np.int64)]])
    p = np.concatenate([p_global[i["p_begin"]:i["p_end"]], p_global[np.asarray(pr.ghost_p, np.int64)]])
    return u, p


def _stress_terms(g, ga, pq, pa, nu, n, w):
    """(-(S n) w, elementary absolute sums) for S = nu (g + g^T) - pq I; ga / pa: absolute sums behind g / pq."""
    nx, ny = LD(n[0]), LD(n[1])
    nu, w = LD(nu), LD(w)
    s00, s01, s11 = nu * (g[0][0] + g[0][0]) - pq, nu * (g[0][1] + g[1][0]), nu * (g[1][1] + g[1][1]) - pq
    f = (-(s00 * nx + s01 * ny) * w, -(s01 * nx + s11 * ny) * w)
    a01 = nu * (ga[0][1] + ga[1][0])
    a = (w * (abs(nx) * (2 * nu * ga[0][0] + pa) + abs(ny) * a01), w * (abs(nx) * a01 + abs(ny) * (2 * nu * ga[1][1] + pa)))
    return f, a


def q3_forces(cell_u_nodes, cell_p_dofs, face_cell, face_side, tables672, u_local, p_local, nu):
    """((drag, lift), (A_drag, A_lift)) over the listed faces, as np.longdouble."""
    tab = np.asarray(tables672, np.float64).astype(LD)
    u, p = np.asarray(u_local, np.float64).astype(LD), np.asarray(p_local, np.float64).astype(LD)
    f_tot, a_tot = [LD(0), LD(0)], [LD(0), LD(0)]
    for c, s in zip(np.asarray(face_cell, np.int64), np.asarray(face_side, np.int64)):
        un, pn = np.asarray(cell_u_nodes[c], np.int64), np.asarray(cell_p_dofs[c], np.int64)
        ux, uy = u[2 * un], u[2 * un + 1]
        for q in range(4):
            t = tab[(s * 4 + q) * 41:(s * 4 + q + 1) * 41]
            dx, dy, psi = t[:16], t[16:32], t[32:41]
            g = ((np.sum(ux * dx), np.sum(ux * dy)), (np.sum(uy * dx), np.sum(uy * dy)))
            ga = ((np.sum(abs(ux * dx)), np.sum(abs(ux * dy))), (np.sum(abs(uy * dx)), np.sum(abs(uy * dy))))
            f, a = _stress_terms(g, ga, np.sum(p[pn] * psi), np.sum(abs(p[pn] * psi)), nu, NORMALS[s], tab[656 + s * 4 + q])
            for k in range(2):
                f_tot[k] += f[k]
                a_tot[k] += a[k]
    return tuple(f_tot), tuple(a_tot)


def p2_forces(cell_u, cell_p, grad_lam, edge_cell, edge_local, edge_nl, u, p, nu):
    """The same over the id-10 edges of a P2/P1 mesh (simplex.force_edges): ((drag, lift), (A_drag, A_lift))."""
    u, p = np.asarray(u, np.float64).astype(LD), np.asarray(p, np.float64).astype(LD)
    f_tot, a_tot = [LD(0), LD(0)], [LD(0), LD(0)]
    for e, (c, k) in enumerate(zip(np.asarray(edge_cell, np.int64), np.asarray(edge_local, np.int64))):
        gl = np.asarray(grad_lam[c], np.float64).astype(LD)                  # [3, 2]
        cu, cp = np.asarray(cell_u[c], np.int64), np.asarray(cell_p[c], np.int64)
        i, j = EDGES[k]
        for gp in GAUSS2:
            lam = np.zeros(3, LD)
            lam[i], lam[j] = LD(1) - LD(gp), LD(gp)
            dl = np.zeros((6, 3), LD)
            for v in range(3):
                dl[v, v] = 4 * lam[v] - 1
            for m, (a, b) in enumerate(EDGES):
                dl[3 + m, a], dl[3 + m, b] = 4 * lam[b], 4 * lam[a]
            grad, grad_abs = dl @ gl, abs(dl) @ abs(gl)                      # [6, 2]
            ux, uy = u[2 * cu], u[2 * cu + 1]
            g = ((np.sum(ux * grad[:, 0]), np.sum(ux * grad[:, 1])), (np.sum(uy * grad[:, 0]), np.sum(uy * grad[:, 1])))
            ga = ((np.sum(abs(ux) * grad_abs[:, 0]), np.sum(abs(ux) * grad_abs[:, 1])),
                  (np.sum(abs(uy) * grad_abs[:, 0]), np.sum(abs(uy) * grad_abs[:, 1])))
            f, a = _stress_terms(g, ga, np.sum(p[cp] * lam), np.sum(abs(p[cp] * lam)), nu, edge_nl[e][:2],
                                 LD(0.5) * LD(edge_nl[e][2]))
            for d in range(2):
                f_tot[d] += f[d]
                a_tot[d] += a[d]
    return tuple(f_tot), tuple(a_tot)
