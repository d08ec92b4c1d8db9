"""NumPy statement of the device assembly (csrc/nsk_assembly_kernels.hip), in np.longdouble.

TEST INFRASTRUCTURE ONLY, not collected by pytest.  Nothing is read from the library and neither problem.generate nor
simplex.assemble is called: the sums below are written from the weak form (include/nsk.h; the reference's
NSSolverStationary.cpp:352-537 for the cell loop, :540-575 for the Dirichlet rows, NSSolver.cpp:443-446 and :460-463
for the time terms), on a connectivity and a tabulation handed in as data.

Q3/Q2, with phi_n, psi_m the tabulated functions, w = JxW, U = sum_j u_j phi_j, G[c][d] = d_d U_c, P = sum p_m psi_m and
O = sum uold_j phi_j at the 16 points of a cell (the nine fields of `cq`):

    F[(n,c),(m,d)] = sum_cells sum_q  delta_cd (nu grad phi_n . grad phi_m + inv_dt phi_n phi_m) w
                                     + [Newton] w phi_n (delta_cd (U . grad phi_m) + G[c][d] phi_m)
    rhs_u[(n,c)]   = [Newton] sum_cells sum_q w (-nu G[c] . grad phi_n - (U . G[c]) phi_n + P d_c phi_n
                                                 - [old state] inv_dt (U_c - O_c) phi_n)
                     - [c == 0] p_out sum_{outlet cells} face_n
    rhs_p[m]       = [Newton] sum_cells sum_q w (G[0][0] + G[1][1]) psi_m
    d0             = share of cell `cell_of_dof0` in F[(its node 0, 0), (its node 0, 0)]   (signed, as asm_d0 leaves it)
    Dirichlet rows: F cleared with |d0| on the diagonal, rhs = |d0| bc, x0 = bc.

THE OLD-STATE RULE (nsk_capi_assembly.cpp, nsk_assemble: `asm_rhs_u(.., A.have_old ? inv_dt : 0.0, ..)` and
`asm_cell_state(.., A.have_old ? A.old_u : nullptr, ..)`): without a saved old state (so = None) the residual has no
time term, whatever inv_dt, the matrix keeps inv_dt M, and fields 7, 8 of cq are 0; with one, fields 7, 8 hold O and the
residual's time term is inv_dt (U - O), which at inv_dt == 0 is nothing.  The Stokes phase (.cpp:383-406, :455-458)
keeps nu K + inv_dt M in F, the outlet term and the Dirichlet rows, and nothing else.

Every output comes with A: the sum of the absolute values of EVERY elementary product of that entry, the state's
interpolation included (|u_j phi_j(q)| instead of |U(q)|), as tests/matfree_reference.py defines A_i.  A rounding-error
bound of any summation order of these products is C 2^-53 A with C the number of roundings one product can pass.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# Roundings one elementary product can pass before it is part of the output (multiplications and additions counted one
# each: an upper bound, FMA contraction only removes some).  Where two interpolated quantities are multiplied, the
# roundings of both chains count.
# asm_cell_state_kernel: the product u_j phi_j 1, the chain over 16 nodes 16 (pressure: 1 + 9).
C_CQ = 1 + 16
# asm_F_rows_kernel, starting from tests/matfree_reference.py's assembled-F part: cq 17; adv = U0 dpx + U1 dpy 2 (product,
# sum); adv + G phi_m 2 (product, sum); w = JxW phi_n and w * (..) 2; the chain over q 16; + (nu K + inv_dt M3) 1; the
# slots of the four cells 4.  (A table entry K[n][m] passes 19 on the host — product, sum, JxW, 16 points — then nu * 1,
# + inv_dt M3 1, + 1, 4 cells: the shorter path.)
C_F = 17 + 2 + 2 + 2 + 16 + 1 + 4
# asm_d0_kernel: cq 17; c * dpx 1, the sum adv 1, + G phi 1; JxW * phi and * (..) 2; the chain v += over q 16.
# (K[0][0]: 19, nu * 1, + inv_dt M3 1, then the same 16 additions: 37.)
C_D0 = 17 + 1 + 1 + 1 + 2 + 16
# asm_rhs_u_kernel, the convective product U_a G[c][a] phi_n: cq twice 17 + 17; U0 * G 1, + U1 * G 1, * phi 1; the four
# terms of the bracket 3; w * 1; ONE accumulator over 4 cells x 16 points 64, and one outlet subtraction per cell 4.
C_RHS_U = 17 + 17 + 1 + 1 + 1 + 3 + 1 + 64 + 4
# asm_rhs_p_kernel: cq 17; G00 + G11 1; JxW * 1; * psi 1; one accumulator over 4 cells x 16 points 64.
C_RHS_P = 17 + 1 + 1 + 1 + 64
# The host producer (problem_gen.cpp), the parts of matfree_reference.C_HOST without the SpMV chain: conv_element 17 (u,
# g), adv 2, + g phi 2, w 2, the chain over q 16; row_F: nu K + inv_dt M3 and the two accumulations per cell, four
# cells: 12.
C_HOST_F = 17 + 2 + 2 + 2 + 16 + 12
# nsp_assemble's d0: the conv_element entry 39, + (nu K + inv_dt M3) 1.
C_HOST_D0 = 17 + 2 + 2 + 2 + 16 + 1
# rhs_element: u and g 17 + 17; u0 g 1, + u1 g 1, * phi 1; r built by three updates 3; w * r 1; the chain over q 16; the
# row sum over four cells 4 and their outlet terms 4 (p_out * hy * face_w3 in another association than the table's: 2 more
# on that product alone, under the rest).
C_HOST_RHS_U = 17 + 17 + 1 + 1 + 1 + 3 + 1 + 16 + 8
# rhs_element's Rp: g 17, divu 1, w * divu 1, * psi 1, the chain over q 16, four cells 4.
C_HOST_RHS_P = 17 + 1 + 1 + 1 + 16 + 4
C_REFERENCE = 1   # the longdouble sums below: < 100 x 2^-64 A, far under one unit of 2^-53 A


def norm_bound(ref_norm, bounds, n):
    """What the returned ||residual|| may differ from the reference's by: the entries move by at most `bounds` (the norm
    by at most their 2-norm), and the sum of n squares in any order and the root lose (n + 1) / 2 + 1 units relative."""
    b = np.asarray(bounds, dtype=LD)
    return float(np.sqrt((b * b).sum()) + ((n + 1) / 2 + 1) * U * LD(ref_norm))


def pattern_positions(rowptr, col, rows, cols):
    """Position in a CSR pattern of the entries (rows[i], cols[i]); -1 where the pattern has none."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    width = int(max(col.max(initial=0), np.max(cols, initial=0))) + 1
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr)) * width + col
    order = np.argsort(key, kind="stable")
    ks = key[order]
    want = np.asarray(rows, np.int64) * width + np.asarray(cols, np.int64)
    i = np.minimum(np.searchsorted(ks, want), len(ks) - 1)
    return np.where(ks[i] == want, order[i], -1)


def _q3q2(dt, tables944, cell_u, cell_p, cell_flags, dirichlet, bc, cell_of_dof0, rowptr, col, su, sp, so, nu, inv_dt,
          p_out, stokes):
    T = np.asarray(tables944).astype(dt)
    phi, dpx, dpy = T[0:256].reshape(16, 16), T[256:512].reshape(16, 16), T[512:768].reshape(16, 16)
    psi, w, face = T[768:912].reshape(9, 16), T[912:928], T[928:944]
    cu, cp = np.asarray(cell_u, np.int64), np.asarray(cell_p, np.int64)
    nc = cu.shape[0]
    flags = (np.asarray(cell_flags).astype(np.int64) & 1).astype(dt)
    dirichlet = np.asarray(dirichlet).astype(bool)
    n_u, n_p = len(dirichlet), len(sp)
    su, sp = np.asarray(su).astype(dt), np.asarray(sp).astype(dt)
    so = None if so is None else np.asarray(so).astype(dt)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    nu, inv_dt, p_out = dt(nu), dt(inv_dt), dt(p_out)
    timed = so is not None and inv_dt != 0     # the old-state rule (module docstring)

    def interp(f):
        q = np.zeros((nc, 9, 16), dtype=dt)
        for c in range(2):
            v = f(su[2 * cu + c])
            q[:, c] = v @ f(phi)
            q[:, 2 + 2 * c] = v @ f(dpx)
            q[:, 3 + 2 * c] = v @ f(dpy)
            if so is not None:
                q[:, 7 + c] = f(so[2 * cu + c]) @ f(phi)
        q[:, 6] = f(sp[cp]) @ f(psi)
        return q

    def element(f, q):
        """(Fe [cell, n, c, m, d], Ru [cell, n, c], Rp [cell, m]); f = identity, or abs for the absolute sums"""
        ab = f is np.abs
        sg = dt(1) if ab else dt(-1)
        P, DX, DY, W, PSI = f(phi), f(dpx), f(dpy), f(w), f(psi)
        K = np.einsum("q,nq,mq->nm", W, DX, DX) + np.einsum("q,nq,mq->nm", W, DY, DY)
        M3 = np.einsum("q,nq,mq->nm", W, P, P)
        diag = np.broadcast_to(f(nu) * K + f(inv_dt) * M3, (nc, 16, 16)).copy()
        Fe = np.zeros((nc, 16, 2, 16, 2), dtype=dt)
        Ru = np.zeros((nc, 16, 2), dtype=dt)
        Rp = np.zeros((nc, 9), dtype=dt)
        if not stokes:
            adv = np.einsum("tq,mq->tmq", q[:, 0], DX) + np.einsum("tq,mq->tmq", q[:, 1], DY)   # (U . grad) phi_m
            diag += np.einsum("q,nq,tmq->tnm", W, P, adv)
            for c in range(2):
                g0, g1 = q[:, 2 + 2 * c], q[:, 3 + 2 * c]
                for d in range(2):
                    Fe[:, :, c, :, d] = np.einsum("q,nq,tq,mq->tnm", W, P, q[:, 2 + 2 * c + d], P)
                r = sg * f(nu) * (np.einsum("q,tq,nq->tn", W, g0, DX) + np.einsum("q,tq,nq->tn", W, g1, DY))
                r += sg * np.einsum("q,tq,nq->tn", W, q[:, 0] * g0 + q[:, 1] * g1, P)
                r += np.einsum("q,tq,nq->tn", W, q[:, 6], DX if c == 0 else DY)
                if timed:
                    du = q[:, c] + q[:, 7 + c] if ab else q[:, c] - q[:, 7 + c]
                    r += sg * f(inv_dt) * np.einsum("q,tq,nq->tn", W, du, P)
                Ru[:, :, c] = r
            Rp[:] = np.einsum("q,tq,mq->tm", W, q[:, 2] + q[:, 5], PSI)
        for c in range(2):
            Fe[:, :, c, :, c] += diag
        Ru[:, :, 0] += sg * f(p_out) * flags[:, None] * f(face)[None, :]
        return Fe, Ru, Rp

    two = np.arange(2, dtype=np.int64)
    rows = np.broadcast_to(2 * cu[:, :, None, None, None] + two[None, None, :, None, None], (nc, 16, 2, 16, 2))
    cols = np.broadcast_to(2 * cu[:, None, None, :, None] + two[None, None, None, None, :], (nc, 16, 2, 16, 2))
    pos = pattern_positions(rowptr, col, rows.ravel(), cols.ravel())
    if (pos < 0).any():
        raise ValueError("a cell couples DoFs that are not in the pattern")
    row_of = np.repeat(np.arange(n_u, dtype=np.int64), np.diff(rowptr))
    d_row = dirichlet[row_of]
    d_diag = d_row & (col == row_of)
    bcv = np.zeros(n_u, dtype=dt) if bc is None else np.asarray(bc).astype(dt)
    out = {}
    for tag, f in (("", lambda a: a), ("_A", np.abs)):
        q = interp(f)
        Fe, Ru, Rp = element(f, q)
        d0 = Fe[cell_of_dof0, 0, 0, 0, 0]
        F = np.zeros(len(col), dtype=dt)
        np.add.at(F, pos, Fe.ravel())
        F[d_row] = 0
        F[d_diag] = abs(d0)
        ru, rp = np.zeros(n_u, dtype=dt), np.zeros(n_p, dtype=dt)
        np.add.at(ru, (2 * cu[:, :, None] + two[None, None, :]).ravel(), Ru.ravel())
        np.add.at(rp, cp.ravel(), Rp.ravel())
        ru[dirichlet] = abs(d0) * f(bcv[dirichlet])
        out.update({"cq" + tag: q, "d0" + tag: d0, "F" + tag: F, "rhs_u" + tag: ru, "rhs_p" + tag: rp})
    out["x0"] = bcv
    out["dirichlet"] = dirichlet
    return out


def q3q2_reference(tables944, cell_u, cell_p, cell_flags, dirichlet, bc, cell_of_dof0, rowptr, col, su, sp, so, nu, inv_dt,
                   p_out, stokes):
    """cq [cell, 9, 16], d0, F (values on the given pattern), rhs_u, rhs_p in longdouble, x0 (the boundary values: what
    the Dirichlet rows of the initial guess hold), norm = ||(rhs_u, rhs_p)||_2, and for each of the five `<name>_A`
    (float64).  bc, so: None for none."""
    r = _q3q2(LD, tables944, cell_u, cell_p, cell_flags, dirichlet, bc, cell_of_dof0, rowptr, col, su, sp, so, nu, inv_dt,
              p_out, stokes)
    r["norm"] = np.sqrt((r["rhs_u"] ** 2).sum() + (r["rhs_p"] ** 2).sum())
    for k in ("cq", "d0", "F", "rhs_u", "rhs_p"):
        r[k + "_A"] = np.asarray(r[k + "_A"]).astype(np.float64)
    return r


def q3q2_int64(tables944, cell_u, cell_p, cell_flags, dirichlet, bc, cell_of_dof0, rowptr, col, su, sp, so, nu, inv_dt,
               p_out, stokes):
    """The same sums in plain int64, for inputs that are all integers (the integer-exact case)."""
    args = [tables944, bc, su, sp, so, nu, inv_dt, p_out]
    for a in args:
        if a is not None and not np.array_equal(np.asarray(a), np.round(np.asarray(a))):
            raise ValueError("q3q2_int64 takes integers")
    return _q3q2(np.int64, tables944, cell_u, cell_p, cell_flags, dirichlet, bc, cell_of_dof0, rowptr, col, su, sp, so, nu,
                 inv_dt, p_out, stokes)


# ------------------------------------------------------------------------------------------------ mesh builders
@dataclass
class Poly:
    cells: list               # lattice (i, j) of every cell, in the order of cell_u
    cell_u: np.ndarray        # [n, 16] velocity node ids, local node n = b * 4 + a
    cell_p: np.ndarray        # [n, 9] pressure DoF ids, local m = b * 3 + a
    n_unodes: int
    n_pdofs: int
    cell_of_dof0: int
    F: tuple                  # (rowptr, col) of each block: two interleaved DoFs per velocity node, rows sorted
    Bt: tuple
    B: tuple
    Mp: tuple


def _pattern(rows, cols, n_rows, n_cols):
    """CSR pattern coupling rows[t, :] with cols[t, :] for every cell t; columns ascending in every row."""
    r = np.repeat(rows[:, :, None], cols.shape[1], axis=2).ravel().astype(np.int64)
    c = np.repeat(cols[:, None, :], rows.shape[1], axis=1).ravel().astype(np.int64)
    key = np.unique(r * n_cols + c)
    rowptr = np.zeros(n_rows + 1, np.int64)
    np.add.at(rowptr, key // n_cols + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), (key % n_cols).astype(np.int32)


def polyomino(cells, perm_cells=None, perm_nodes=None):
    """Q3/Q2 connectivity and block patterns of a set of lattice cells (i, j).  Without permutations the cells are in
    (i, j) order and the nodes are numbered x-major over the lattice points that exist, as problem_gen.cpp numbers a
    generated mesh.  perm_nodes = (pu, pp): velocity node k becomes pu[k], pressure DoF k becomes pp[k]; perm_cells: cell k
    of the result is cell perm_cells[k] of the (i, j) order.  A node is coupled to every node of a cell it shares."""
    cells = sorted({(int(i), int(j)) for i, j in cells})

    def number(step):
        pts = sorted({(step * i + a, step * j + b) for i, j in cells for a in range(step + 1) for b in range(step + 1)})
        return {p: k for k, p in enumerate(pts)}

    uid, pid = number(3), number(2)
    cu = np.array([[uid[3 * i + a, 3 * j + b] for b in range(4) for a in range(4)] for i, j in cells], dtype=np.int64)
    cp = np.array([[pid[2 * i + a, 2 * j + b] for b in range(3) for a in range(3)] for i, j in cells], dtype=np.int64)
    if perm_nodes is not None:
        pu, pp = (np.asarray(p, np.int64) for p in perm_nodes)
        assert sorted(pu) == list(range(len(uid))) and sorted(pp) == list(range(len(pid)))
        cu, cp = pu[cu], pp[cp]
    if perm_cells is not None:
        pc = np.asarray(perm_cells, np.int64)
        assert sorted(pc) == list(range(len(cells)))
        cu, cp, cells = cu[pc], cp[pc], [cells[k] for k in pc]
    n_un, n_p = len(uid), len(pid)
    holders = np.argwhere(cu == 0)
    # DoF 0 is local node 0 of exactly one cell and belongs to no other: asm_d0 integrates that cell's (0, 0) entry
    assert len(holders) == 1 and holders[0][1] == 0, "DoF 0 must be local node 0 of exactly one cell"
    ud = (2 * cu[:, :, None] + np.arange(2)[None, None, :]).reshape(len(cells), 32)
    return Poly(cells, cu.astype(np.int32), cp.astype(np.int32), n_un, n_p, int(holders[0][0]),
                _pattern(ud, ud, 2 * n_un, 2 * n_un), _pattern(ud, cp, 2 * n_un, n_p), _pattern(cp, ud, n_p, 2 * n_un),
                _pattern(cp, cp, n_p, n_p))


def random_perms(cells, seed):
    """(perm_cells, perm_nodes) for polyomino: a shuffled cell list and a random numbering in which the lower-left corner
    of the first cell in (i, j) order — a node of that cell alone — keeps number 0."""
    base = polyomino(cells)
    rng = np.random.default_rng(seed)
    pc = rng.permutation(len(base.cells))
    pu, pp = rng.permutation(base.n_unodes), rng.permutation(base.n_pdofs)
    k = int(np.nonzero(pu == 0)[0][0])
    pu[k], pu[0] = pu[0], 0
    return pc, (pu, pp)


def add_blocks(pattern, pairs):
    """The F pattern with extra 2x2 node blocks (row node, column node) that no cell produces."""
    rowptr, col = (np.asarray(a, np.int64) for a in pattern)
    rows = [list(col[rowptr[r]:rowptr[r + 1]]) for r in range(len(rowptr) - 1)]
    for n, m in pairs:
        for c in range(2):
            assert 2 * m not in rows[2 * n + c], "the block is in the pattern already"
            rows[2 * n + c] = sorted(rows[2 * n + c] + [2 * m, 2 * m + 1])
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return rp.astype(np.int32), np.concatenate(rows).astype(np.int32)


def node_tables(cell_u, cell_p, n_unodes, n_pdofs, rowptr, col):
    """What nsk_assembly_set_cells derives: node_cells [n, 4] (cell * 16 + local node, cells ascending, -1 unused),
    node_off [n, 64] (block offset of (slot k, column node m) in the node's rows; 0 in unused slots), node_self [n],
    pdof_cells [n_p, 4] (cell * 9 + local DoF)."""
    cu, cp = np.asarray(cell_u, np.int64), np.asarray(cell_p, np.int64)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    nodes = -np.ones((n_unodes, 4), np.int64)
    pdofs = -np.ones((n_pdofs, 4), np.int64)
    for ids, out, width in ((cu, nodes, 16), (cp, pdofs, 9)):
        cnt = np.zeros(len(out), np.int64)
        for c in range(ids.shape[0]):
            for n in range(width):
                out[ids[c, n], cnt[ids[c, n]]] = c * width + n
                cnt[ids[c, n]] += 1
    off = np.zeros((n_unodes, 64), np.int64)
    self_ = np.zeros(n_unodes, np.int64)
    for r in range(n_unodes):
        blocks = list(col[rowptr[2 * r]:rowptr[2 * r + 1]:2] // 2)
        self_[r] = blocks.index(r)
        for k in range(4):
            if nodes[r, k] >= 0:
                for m in range(16):
                    off[r, k * 16 + m] = blocks.index(cu[nodes[r, k] // 16, m])
    return nodes, off, self_, pdofs


# ------------------------------------------------------------------------------------------------ P2/P1 triangles
# simplex_*_kernel (second half of nsk_assembly_kernels.hip), the reference's -M path (NSSolverStationary.cpp:144-206).
# Roundings of one elementary product, with N the longest cell list of a node and kappa the largest
# (|J00 J11| + |J01 J10|) / |det J| of a cell (what the host's double grad_lambda and area lose in the determinant):
#   a quadrature constant as written in the kernel 1 per use; phi = lam (2 lam - 1): 2 + 2 constants = 4; dphi/dlam 2; a
#   gradient dl . grad_lam 2 + 1 + 2 = 5; elem_state: u 1 + 6 + 4 = 11, grad u 1 + 6 + 5 = 12; w = area W 2.
#   geometry, per factor taken from the host: grad_lam 2 + 3 kappa, area 1 + 3 kappa; at most two gradients and the area
#   in one product: 5 + 9 kappa.
def c_geometry(kappa):
    return 5 + 9 * float(kappa)


# simplex_F_blocks_kernel, the product w phi_n G phi_m: w 2, * phi_n 1 + 4, * G 1 + 12, * phi_m 1 + 4; two additions a
# point over 7 points 14; the cells of the block N.  (Viscous: two gradients 10, product, sum, nu, + 4, w 3, 14, N: less.)
def c_sx_f(n_list, kappa):
    return 2 + 5 + 13 + 5 + 14 + n_list + c_geometry(kappa)


# simplex_rhs_u_kernel, the product U_a G[c][a] phi_n: 11 + 12, product 1, sum 1, * phi_n 1 + 4; the terms of t0 3; w 2,
# w * t0 1; the chain over 7 points 7; the cells N; the outlet term 1.
def c_sx_rhs_u(n_list, kappa):
    return 11 + 12 + 1 + 1 + 5 + 3 + 3 + 7 + n_list + 1 + c_geometry(kappa)


# simplex_rhs_p_kernel: grad u 12, the divergence 1, area W 2, * 1, * lam 1 + 1, the chain 7, the cells N.
def c_sx_rhs_p(n_list, kappa):
    return 12 + 1 + 2 + 1 + 2 + 7 + n_list + c_geometry(kappa)


# simplex.assemble (NumPy einsum and bincount): the same products; its quadrature points come from square roots
# ((6 -+ sqrt 15) / 21 and 1 - 2 a: 4 roundings a constant instead of 1, two constants in phi) and the scatter adds the
# cells one by one like the kernels: the kernels' counts + 8.
C_HOST_SX_EXTRA = 8


def _tri_rule(dt=LD):
    s15 = np.sqrt(dt(15))
    a1, a2 = (6 - s15) / 21, (6 + s15) / 21
    w1, w2 = (155 - s15) / 1200, (155 + s15) / 1200
    third = dt(1) / 3
    L = np.array([[third, third, third], [1 - 2 * a1, a1, a1], [a1, 1 - 2 * a1, a1], [a1, a1, 1 - 2 * a1],
                  [1 - 2 * a2, a2, a2], [a2, 1 - 2 * a2, a2], [a2, a2, 1 - 2 * a2]], dtype=dt)
    return L, np.array([dt(9) / 40, w1, w1, w1, w2, w2, w2], dtype=dt)


def _p2_tab(lam, absolute):
    """phi[n, q], dphi/dlam[n, q, 3] of the six P2 functions (vertices, then the midpoints of (0,1), (1,2), (2,0)); with
    `absolute` the sums of the absolute values of their terms: 2 lam^2 + lam, 4 lam + 1."""
    s = 1 if absolute else -1
    phi = np.zeros((6, len(lam)), dtype=LD)
    dl = np.zeros((6, len(lam), 3), dtype=LD)
    for i in range(3):
        phi[i] = 2 * lam[:, i] * lam[:, i] + s * lam[:, i]
        dl[i, :, i] = 4 * lam[:, i] + s
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        phi[3 + k] = 4 * lam[:, i] * lam[:, j]
        dl[3 + k, :, i] = 4 * lam[:, j]
        dl[3 + k, :, j] = 4 * lam[:, i]
    return phi, dl


def p2p1_reference(nodes, tris, cell_u, dirichlet, bc, outlet, rowptr, col, su, sp, so, nu, inv_dt, p_out, stokes):
    """The P2/P1 assembly on triangles `tris` [T, 3] of vertices `nodes` [nv, 2]; cell_u [T, 6] the velocity nodes (vertices,
    then the midpoints of the edges (0,1), (1,2), (2,0)), the pressure DoFs are the vertices.  dirichlet: per velocity DoF;
    outlet: (a, m, b, t) — the id-8 edges as vertex, midpoint node, vertex and the triangle they belong to.  grad_lambda
    and the areas are computed here, in longdouble, from the coordinates.  The time term follows simplex_assemble: in the
    residual only with an old state and inv_dt != 0, in the matrix whenever inv_dt != 0.  Returns F, rhs_u, rhs_p, d0
    (= |F[0, 0]| before clearing), x0, norm and the `_A` of each; n_list and kappa for the constants above."""
    X = np.asarray(nodes).astype(LD)
    tris = np.asarray(tris, np.int64)
    cu = np.asarray(cell_u, np.int64)
    nt = len(tris)
    dirichlet = np.asarray(dirichlet).astype(bool)
    n_u, n_p = len(dirichlet), len(sp)
    su, sp = np.asarray(su).astype(LD), np.asarray(sp).astype(LD)
    timed = so is not None and inv_dt != 0
    so = np.asarray(so).astype(LD) if timed else None
    nu, inv_dt, p_out = LD(nu), LD(inv_dt), LD(p_out)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    p = X[tris]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    kappa = float(np.max((np.abs(e1[:, 0] * e2[:, 1]) + np.abs(e1[:, 1] * e2[:, 0])) / np.abs(det)))
    g1 = np.stack([e2[:, 1], -e2[:, 0]], axis=1) / det[:, None]      # grad lam_1
    g2 = np.stack([-e1[:, 1], e1[:, 0]], axis=1) / det[:, None]      # grad lam_2
    gl = np.stack([-(g1 + g2), g1, g2], axis=1)                      # [T, 3, 2]
    area = np.abs(det) / 2
    L, W = _tri_rule()
    two = np.arange(2, dtype=np.int64)
    rows = np.broadcast_to(2 * cu[:, :, None, None, None] + two[None, None, :, None, None], (nt, 6, 2, 6, 2))
    cols = np.broadcast_to(2 * cu[:, None, None, :, None] + two[None, None, None, None, :], (nt, 6, 2, 6, 2))
    pos = pattern_positions(rowptr, col, rows.ravel(), cols.ravel())
    if (pos < 0).any():
        raise ValueError("a cell couples DoFs that are not in the pattern")
    row_of = np.repeat(np.arange(n_u, dtype=np.int64), np.diff(rowptr))
    d_row = dirichlet[row_of]
    d_diag = d_row & (col == row_of)
    pos00 = int(pattern_positions(rowptr, col, [0], [0])[0])
    bcv = np.zeros(n_u, dtype=LD) if bc is None else np.asarray(bc).astype(LD) * dirichlet
    out = dict(kappa=kappa, n_list=int(np.bincount(cu.ravel()).max()))
    for tag, ab in (("", False), ("_A", True)):
        f = np.abs if ab else (lambda a: a)
        sg = LD(1) if ab else LD(-1)
        phi, dl = _p2_tab(L, ab)
        psi = L.T
        if ab:   # grad lam_0 = -(g1 + g2): two terms
            gla = np.stack([np.abs(g1) + np.abs(g2), np.abs(g1), np.abs(g2)], axis=1)
        dphi = np.einsum("nql,tld->tnqd", dl, gla if ab else gl)
        jxw = area[:, None] * W[None, :]
        Un = np.stack([f(su[2 * cu]), f(su[2 * cu + 1])], axis=1)              # [T, 2, 6]
        u = np.einsum("tcn,nq->tcq", Un, phi)
        g = np.einsum("tcn,tnqd->tcdq", Un, dphi)
        base = f(nu) * np.einsum("tq,tnqd,tmqd->tnm", jxw, dphi, dphi) + f(inv_dt) * np.einsum("tq,nq,mq->tnm", jxw, phi, phi)
        Fe = np.zeros((nt, 6, 2, 6, 2), dtype=LD)
        re = np.zeros((nt, 6, 2), dtype=LD)
        rp_e = np.zeros((nt, 3), dtype=LD)
        if not stokes:
            adv = np.einsum("tdq,tmqd->tmq", u, dphi)
            base = base + np.einsum("tq,nq,tmq->tnm", jxw, phi, adv)
            Fe += np.einsum("tq,nq,tcdq,mq->tncmd", jxw, phi, g, phi)
            pq = np.einsum("tj,jq->tq", f(sp[tris]), psi)
            re = sg * f(nu) * np.einsum("tq,tcdq,tnqd->tnc", jxw, g, dphi) + sg * np.einsum("tq,tdq,tcdq,nq->tnc", jxw, u, g, phi)
            re += np.einsum("tq,tnqc->tnc", jxw * pq, dphi)
            if timed:
                On = np.stack([f(so[2 * cu]), f(so[2 * cu + 1])], axis=1)
                du = u + np.einsum("tcn,nq->tcq", On, phi) if ab else u - np.einsum("tcn,nq->tcq", On, phi)
                re += sg * f(inv_dt) * np.einsum("tq,tcq,nq->tnc", jxw, du, phi)
            rp_e = np.einsum("tq,tq,jq->tj", jxw, g[:, 0, 0] + g[:, 1, 1], psi)
        for c in range(2):
            Fe[:, :, c, :, c] += base
        F = np.zeros(len(col), dtype=LD)
        np.add.at(F, pos, Fe.ravel())
        d0 = abs(F[pos00])
        F[d_row] = 0
        F[d_diag] = d0
        ru, rpp = np.zeros(n_u, dtype=LD), np.zeros(n_p, dtype=LD)
        np.add.at(ru, (2 * cu[:, :, None] + two[None, None, :]).ravel(), re.ravel())
        np.add.at(rpp, tris.ravel(), rp_e.ravel())
        a, m, b, t = (np.asarray(v, np.int64) for v in outlet)
        for k in range(len(a)):   # - p_out int phi . n over an id-8 edge: Simpson, exact for P2
            tang = X[b[k]] - X[a[k]]
            length = np.sqrt(tang @ tang)
            nrm = np.array([tang[1], -tang[0]]) / length
            third = [v for v in tris[t[k]] if v not in (a[k], b[k])][0]
            if nrm @ (X[third] - X[a[k]]) > 0:
                nrm = -nrm
            for node, wgt in ((a[k], LD(1) / 6), (m[k], LD(4) / 6), (b[k], LD(1) / 6)):
                ru[2 * node:2 * node + 2] += sg * f(p_out) * wgt * length * f(nrm)
        ru[dirichlet] = d0 * f(bcv[dirichlet])
        out.update({"d0" + tag: d0, "F" + tag: F, "rhs_u" + tag: ru, "rhs_p" + tag: rpp})
    out["x0"] = bcv
    out["norm"] = np.sqrt((out["rhs_u"] ** 2).sum() + (out["rhs_p"] ** 2).sum())
    for k in ("d0", "F", "rhs_u", "rhs_p"):
        out[k + "_A"] = np.asarray(out[k + "_A"]).astype(np.float64)
    return out


# hand-made triangle meshes: (vertex coordinates, triangles counter-clockwise, boundary segments, their ids — 6 wall,
# 7 inlet, 8 outlet, as gmsh.TriMesh takes them)
TRI_MESHES = ["one", "two", "two_rotated", "fan"]


def tri_mesh(name):
    if name == "fan":   # 12 triangles round vertex 0, unequal angles and radii: a diagonal block and a node list of 12 cells
        gaps = np.array([3, 5, 4, 6, 5, 7, 4, 6, 5, 3, 6, 6], dtype=np.float64)
        ang = 2 * np.pi * np.concatenate([[0.0], np.cumsum(gaps)[:-1]]) / gaps.sum()
        rad = 0.5 + 0.03 * np.arange(12)
        nodes = np.concatenate([[[0.1, -0.05]], np.stack([0.1 + rad * np.cos(ang), -0.05 + rad * np.sin(ang)], axis=1)])
        tris = [(0, k + 1, (k + 1) % 12 + 1) for k in range(12)]
        ids = {0: 6, 1: 8, 2: 7}
        seg = [((k + 1, (k + 1) % 12 + 1), ids[k % 4]) for k in range(12) if k % 4 in ids]
    else:
        nodes = np.array([[0.0, 0.0], [1.0, 0.1], [0.3, 0.9], [1.2, 1.0]])
        if name == "one":
            nodes, tris, seg = nodes[:3], [(0, 1, 2)], [((0, 1), 6), ((1, 2), 8)]
        else:   # two triangles sharing the edge (1, 2), the second in two of its vertex orders
            tris = [(0, 1, 2), (1, 3, 2) if name == "two" else (3, 2, 1)]
            seg = [((0, 1), 6), ((1, 3), 8), ((2, 0), 7)]
    return (np.asarray(nodes, np.float64), np.asarray(tris, np.int64), np.array([s for s, _ in seg], np.int64),
            np.array([i for _, i in seg], np.int64))


# ------------------------------------------------------------------------------------------------ the cases of the tests
def rect(nx, ny):
    return [(i, j) for i in range(nx) for j in range(ny)]


# name -> (cells, velocity nodes, pressure DoFs, the cells-per-node values that occur)
MESHES = {
    "1x1": (rect(1, 1), 16, 9, {1}),
    "2x2": (rect(2, 2), 49, 25, {1, 2, 4}),
    "L": ([(0, 0), (1, 0), (0, 1)], 40, 21, {1, 2, 3}),
    "corner": ([(0, 0), (1, 1)], 31, 17, {1, 2}),
    "3x2": (rect(3, 2), 70, 35, {1, 2, 4}),
    "2x4": (rect(2, 4), 91, 45, {1, 2, 4}),
    "7x4": (rect(7, 4), 286, 135, {1, 2, 4}),
    "8x8": (rect(8, 8), 625, 289, {1, 2, 4}),
}
NU, P_OUT = 0.05, 0.7


def random_tables(seed):
    """944 entries from uniform(-1, 1), JxW positive: data without any of the symmetries of a real tabulation."""
    t = np.random.default_rng(seed).uniform(-1.0, 1.0, 944)
    t[912:928] = np.abs(t[912:928])
    return t


def random_case(poly, seed):
    """Dirichlet flags on about a quarter of the nodes (both components), outlet flags on two cells, boundary values, a
    state and an old state."""
    rng = np.random.default_rng(seed)
    nn, nc = poly.n_unodes, len(poly.cells)
    d = np.repeat(rng.uniform(size=nn) < 0.25, 2)
    if not d.any():
        d[2:4] = True
    flags = np.zeros(nc, np.uint8)
    flags[rng.choice(nc, size=min(2, nc), replace=False)] = 1
    su = rng.uniform(-1.0, 1.0, 2 * nn)
    return dict(dirichlet=d.astype(np.uint8), flags=flags, bc=rng.uniform(-1.0, 1.0, 2 * nn) * d, su=su,
                sp=rng.uniform(-1.0, 1.0, poly.n_pdofs), so=su + 0.1 * rng.uniform(-1.0, 1.0, 2 * nn))


INT_NU, INT_INV_DT, INT_P_OUT = 2.0, 4.0, 3.0
INT_TABLE, INT_JXW, INT_STATE = 2, 2, 3     # |table entries| <= 2, JxW in {1, 2}, |state|, |old state|, |p|, |bc| <= 3


def integer_case(poly, seed):
    """The integer-exact case: every input a small integer, so that every product and partial sum is an integer far
    below 2^53 (tests/test_asm_reference.py proves it for these ranges) and any summation order gives the same bits."""
    rng = np.random.default_rng(seed)
    c = random_case(poly, seed + 1)
    nn = poly.n_unodes
    t = rng.integers(-INT_TABLE, INT_TABLE + 1, 944).astype(np.float64)
    t[912:928] = rng.integers(1, INT_JXW + 1, 16)
    d = c["dirichlet"].astype(bool)
    c.update(tables=t, su=rng.integers(-INT_STATE, INT_STATE + 1, 2 * nn).astype(np.float64),
             so=rng.integers(-INT_STATE, INT_STATE + 1, 2 * nn).astype(np.float64),
             sp=rng.integers(-INT_STATE, INT_STATE + 1, poly.n_pdofs).astype(np.float64),
             bc=rng.integers(-INT_STATE, INT_STATE + 1, 2 * nn).astype(np.float64) * d)
    return c
