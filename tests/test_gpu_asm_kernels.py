"""Every kernel of the device assembly alone, against an exact statement of the weak form (csrc/nsk_assembly_kernels.hip,
tests/asm_reference.py, nsk_internal.h: nsk_debug_asm).

Hand-made meshes (tests/asm_reference.py: polyomino) go in through the public calls with NaN as the values of block
(0,0); what nsk_assemble leaves — cq and d0 through the read-only hook, every entry of F, of the residual and the
Dirichlet rows of the initial guess — is compared ENTRY BY ENTRY with the longdouble reference within
(C + C_REFERENCE) 2^-53 A, C counted from the kernels' order of operations and A the absolute sum of the entry's
elementary products.  No norm is used anywhere.  On integer inputs the same outputs must equal the reference bit for bit.
"""
import ctypes as C
import dataclasses
import time

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from tests import asm_reference as AR
from tests import matfree_reference as MR

pytestmark = pytest.mark.gpu

LD = np.longdouble
T_START = time.perf_counter()
_TALLY = set()

CQ, D0, NODE_CELLS, NODE_OFF, NODE_SELF, PDOF_CELLS = range(6)   # nsk_internal.h: NSK_DBG_ASM_*

# (stokes, inv_dt, a saved old state, inhomogeneous bc).  A saved old state stays on a handle, so the cases without one
# run first.  Numbers: the issue's list of cases.
CASES_NO_OLD = [(False, 0.0, False, False),     # 1
                (True, 0.0, False, False),      # 2
                (False, 100.0, False, False),   # 4
                (False, 0.0, False, True)]      # 6
CASES_OLD = [(False, 100.0, True, False),       # 3
             (False, 0.0, True, False)]         # 5
SMALL = ["1x1", "2x2", "L", "corner", "3x2", "2x4"]
LARGE = ["7x4", "8x8"]          # the first and the last case only
EXTRA = ["2x2", "3x2"]          # once more with blocks in the pattern that no cell produces
INTEGER = ["2x2", "L", "3x2"]   # the integer-exact case, shuffled


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


def _hook(ls, what, dtype, count):
    out = np.zeros(count, dtype=dtype)
    ls.L.nsk_debug_asm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]   # (nsk_internal.h: not in EXPORTS)
    ls.L.nsk_debug_asm.restype = C.c_int64
    rc = ls.L.nsk_debug_asm(ls.h, what, out.ctypes.data, out.nbytes)
    if rc < 0:
        raise RuntimeError(f"nsk error {rc}: {ls.last_error()}")
    assert rc == out.nbytes, (what, rc, out.nbytes)
    return out


_REAL = {}


def _real_tables():
    """the tabulation of a real cell"""
    if "t" not in _REAL:
        _REAL["t"] = P.generate(3, 2, nu=AR.NU, mode=1, state=1).cell_tables.copy()
    return _REAL["t"]


def _problem(poly, case, tables, pattern=None):
    """A LocalProblem of one rank from hand-made arrays.  F's values are NaN: whatever the assembly does not write shows.
    B, Bt and M_p are not read by the assembly: ones on the right pattern."""
    n_u, n_p = 2 * poly.n_unodes, poly.n_pdofs

    def blk(pat, rows, cols, fill):
        rp, col = pat
        return P.CsrBlock(rows, cols, np.asarray(rp, np.int32), np.asarray(col, np.int32), np.full(len(col), fill))

    info = dict(nx=0, ny=0, nranks=1, rank=0, n_cells=len(poly.cells), n_removed=0, n_u_global=n_u, n_p_global=n_p,
                u_begin=0, u_end=n_u, p_begin=0, p_end=n_p, n_ghost_u=0, n_ghost_p=0)
    z32 = np.zeros(0, np.int32)
    return P.LocalProblem(info, blk(pattern or poly.F, n_u, n_u, np.nan), blk(poly.Bt, n_u, n_p, 1.0), blk(poly.B, n_p, n_u, 1.0),
                          blk(poly.Mp, n_p, n_p, 1.0), P.CsrBlock(0, n_p, np.zeros(1, np.int32), z32, np.zeros(0)),
                          np.zeros(n_u), np.zeros(n_p), np.zeros(n_u), np.zeros(n_p), z32, z32, case["dirichlet"],
                          np.array([0, n_u]), np.array([0, n_p]), cell_u_nodes=poly.cell_u, cell_p_dofs=poly.cell_p,
                          cell_flags=case["flags"], cell_of_dof0=poly.cell_of_dof0, cell_tables=tables)


def _poly(mesh, shuffled):
    cells, n_un, n_p, per_node = AR.MESHES[mesh]
    poly = AR.polyomino(cells, *AR.random_perms(cells, 17)) if shuffled else AR.polyomino(cells)
    assert (poly.n_unodes, poly.n_pdofs, len(poly.cells)) == (n_un, n_p, len(cells))
    return poly


def _extra_pairs(poly, seed, count=3):
    """node pairs no cell couples, in rows that stay within 49 blocks"""
    rng = np.random.default_rng(seed)
    rp, col = poly.F
    pairs = []
    while len(pairs) < count:
        n, m = (int(v) for v in rng.integers(0, poly.n_unodes, 2))
        row = col[rp[2 * n]:rp[2 * n + 1]]
        if 2 * m in row or len(row) // 2 + sum(1 for a, _ in pairs if a == n) >= 49 or (n, m) in pairs:
            continue
        pairs.append((n, m))
    return pairs


class Bench:
    """One handle, one mesh: the arrays the checks need and what the library derived from the connectivity."""

    def __init__(self, mesh, variant):
        S = _S()
        self.mesh, self.variant = mesh, variant
        self.poly = _poly(mesh, variant != "lattice")
        self.case = AR.random_case(self.poly, 23)
        self.pattern = AR.add_blocks(self.poly.F, _extra_pairs(self.poly, 29)) if variant == "extra" else self.poly.F
        self.rowptr, self.col = (np.asarray(a, np.int64) for a in self.pattern)
        self.row_of = np.repeat(np.arange(2 * self.poly.n_unodes), np.diff(self.rowptr))
        self.tabs = AR.node_tables(self.poly.cell_u, self.poly.cell_p, self.poly.n_unodes, self.poly.n_pdofs, *self.pattern)
        self.ls = S.LinearSolver()
        self.ls.set_problem(_problem(self.poly, self.case, _real_tables(), self.pattern))
        self.old_saved = False

    def close(self):
        self.ls.close()

    def set_assembly(self, case, tables):
        self.ls.set_assembly(_problem(self.poly, case, tables, self.pattern), bc_u=case["bc"])

    def entry(self, w):
        """name an entry of F: (row node, component), (column node, component), the cells of the row node"""
        r, c = int(self.row_of[w]), int(self.col[w])
        cells = [int(v) // 16 for v in self.tabs[0][r // 2] if v >= 0]
        return f"F[(node {r // 2}, {r % 2}), (node {c // 2}, {c % 2})], cells {cells} of the row node"

    def node(self, i):
        cells = [int(v) // 16 for v in self.tabs[0][i // 2] if v >= 0]
        return f"(node {i // 2}, {i % 2}), cells {cells}"

    def pdof(self, i):
        return f"pressure DoF {i}, cells {[int(v) // 9 for v in self.tabs[3][i] if v >= 0]}"

    def assemble(self, case, nu, inv_dt, p_out, stokes, inhomog):
        ls, S, n = self.ls, _S(), self.poly.n_unodes
        nrm = ls.assemble(nu, inv_dt, p_out, inhomogeneous_bc=inhomog, stokes=stokes)
        rp, col, val = ls.get_block(S.BLK_F)
        assert np.array_equal(rp, self.rowptr) and np.array_equal(col, self.col)
        ru, rpp = ls.download_rhs()
        xu, _ = ls.download_solution()
        return dict(norm=nrm, F=val, rhs_u=ru, rhs_p=rpp, x0=xu,
                    cq=_hook(ls, CQ, np.float64, len(self.poly.cells) * 144).reshape(-1, 9, 16),
                    d0=_hook(ls, D0, np.float64, 1)[0],
                    node_cells=_hook(ls, NODE_CELLS, np.int32, n * 4).reshape(n, 4),
                    node_off=_hook(ls, NODE_OFF, np.uint8, n * 64).reshape(n, 64),
                    node_self=_hook(ls, NODE_SELF, np.int32, n),
                    pdof_cells=_hook(ls, PDOF_CELLS, np.int32, self.poly.n_pdofs * 4).reshape(-1, 4))

    def run(self, case, tables, nu, inv_dt, p_out, stokes, old, inhomog, label):
        """one assembly and its reference: (device outputs, reference); the structural and the bit-exact checks"""
        ls, poly = self.ls, self.poly
        assert old or not self.old_saved, "a saved old state stays on the handle: the cases without one come first"
        if old:
            ls.state_set(case["so"], case["sp"])
            ls.state_save_old()
            self.old_saved = True
        ls.state_set(case["su"], case["sp"])
        g = self.assemble(case, nu, inv_dt, p_out, stokes, inhomog)
        bc = case["bc"] if inhomog else None
        r = AR.q3q2_reference(tables, poly.cell_u, poly.cell_p, case["flags"], case["dirichlet"], bc, poly.cell_of_dof0,
                              self.rowptr, self.col, case["su"], case["sp"], case["so"] if old else None, nu, inv_dt, p_out, stokes)
        # what nsk_assembly_set_cells derived from the connectivity and the pattern
        nodes, off, self_, pdofs = self.tabs
        assert np.array_equal(g["node_cells"], MR.node_cells(poly.cell_u, poly.n_unodes)), label
        assert np.array_equal(g["node_cells"], nodes) and np.array_equal(g["pdof_cells"], pdofs), label
        assert np.array_equal(g["node_off"], off) and np.array_equal(g["node_self"], self_), label
        # Dirichlet rows, bit for bit: 0 off the diagonal, |d0| on it, rhs = |d0| * bc, x0 = bc
        d = case["dirichlet"].astype(bool)
        assert d.any() and not d.all()
        d_row = d[self.row_of]
        diag = d_row & (self.col == self.row_of)
        assert np.all(g["F"][d_row & ~diag] == 0.0) and np.all(g["F"][diag] == abs(g["d0"])), label
        bcv = r["x0"].astype(np.float64)
        assert np.array_equal(g["rhs_u"][d], abs(g["d0"]) * bcv[d]) and np.array_equal(g["x0"][d], bcv[d]), label
        assert not np.isnan(g["F"]).any(), (label, self.entry(int(np.argmax(np.isnan(g["F"])))))
        # a second assembly: the same bits
        g2 = self.assemble(case, nu, inv_dt, p_out, stokes, inhomog)
        for k in ("F", "rhs_u", "rhs_p", "cq", "d0", "norm"):
            assert np.array_equal(g[k], g2[k]), (label, k)
        return g, r

    def check(self, tables_kind, stokes, inv_dt, old, inhomog):
        case = self.case
        tables = _real_tables() if tables_kind == "real" else AR.random_tables(41)
        label = (self.mesh, self.variant, tables_kind, "stokes" if stokes else "newton", inv_dt, "old" if old else "no old",
                 "bc" if inhomog else "bc 0")
        g, r = self.run(case, tables, AR.NU, inv_dt, AR.P_OUT, stokes, old, inhomog, label)
        ratios, bounds = {}, {}
        names = dict(F=self.entry, rhs_u=self.node, rhs_p=self.pdof, cq=lambda w: f"cq[cell {w // 144}, field {w % 144 // 16}, point {w % 16}]",
                     d0=lambda w: "d0")
        for k, Cc in (("cq", AR.C_CQ), ("d0", AR.C_D0), ("F", AR.C_F), ("rhs_u", AR.C_RHS_U), ("rhs_p", AR.C_RHS_P)):
            got, ref, A = np.ravel(g[k]), np.ravel(r[k]), np.ravel(r[k + "_A"])
            err = np.abs(got.astype(LD) - ref).astype(np.float64)
            bounds[k] = (Cc + AR.C_REFERENCE) * AR.U * A
            ratios[k] = float(np.max(err / np.maximum(AR.U * A, 1e-300)))
            w = int(np.argmax(err - bounds[k]))
            assert np.all(err <= bounds[k]), (label, names[k](w), "got", got[w], "reference", float(ref[w]), "error", err[w],
                                               "bound", bounds[k][w])
        nb = AR.norm_bound(r["norm"], np.concatenate([bounds["rhs_u"], bounds["rhs_p"]]), len(g["rhs_u"]) + len(g["rhs_p"]))
        assert abs(LD(g["norm"]) - r["norm"]) <= nb, (label, g["norm"], float(r["norm"]), nb)
        if self.variant == "extra":   # entries no cell produces: exactly 0.0
            base = AR.pattern_positions(*self.poly.F, self.row_of, self.col) >= 0
            assert (~base).sum() == 12 and np.all(g["F"][~base] == 0.0), label
        print("asm " + " ".join(str(v) for v in label) + ": max err / (2^-53 A): " +
              ", ".join(f"{k} {ratios[k]:.2f} (C = {Cc})" for k, Cc in (("cq", AR.C_CQ), ("d0", AR.C_D0), ("F", AR.C_F),
                                                                         ("rhs_u", AR.C_RHS_U), ("rhs_p", AR.C_RHS_P))))
        _TALLY.add((self.mesh, self.variant, tables_kind, stokes, inv_dt, old, inhomog))

    def check_integer(self):
        """Integers in, integers far below 2^53 all the way (tests/test_asm_reference.py): the reference bit for bit,
        whatever the summation order or FMA contraction."""
        case = AR.integer_case(self.poly, 31)
        self.set_assembly(case, case["tables"])
        label = (self.mesh, self.variant, "integer")
        g, r = self.run(case, case["tables"], AR.INT_NU, AR.INT_INV_DT, AR.INT_P_OUT, False, True, True, label)
        names = dict(F=self.entry, rhs_u=self.node, rhs_p=self.pdof, cq=str, d0=str)
        for k in ("cq", "d0", "F", "rhs_u", "rhs_p"):
            got, ref = np.ravel(g[k]), np.ravel(r[k]).astype(np.float64)
            assert np.array_equal(ref.astype(LD), np.ravel(r[k]))
            w = int(np.argmax(got != ref))
            assert np.array_equal(got, ref), (label, names[k](w), "got", got[w], "reference", ref[w])
        assert np.abs(g["rhs_u"]).max() > 0 and np.abs(g["rhs_p"]).max() > 0
        print("asm " + " ".join(label) + ": cq, d0, F, rhs_u, rhs_p equal the reference bit for bit")
        _TALLY.add((self.mesh, self.variant, "integer"))


def _variants(mesh):
    return ["lattice", "shuffled"] + (["extra"] if mesh in EXTRA else [])


@pytest.mark.parametrize("mesh,variant", [(m, v) for m in SMALL + LARGE for v in _variants(m)])
def test_q3q2_kernels_entry_by_entry(mesh, variant):
    b = Bench(mesh, variant)
    try:
        cells, n_un, n_p, per_node = AR.MESHES[mesh]
        assert set(int(c) for c in (b.tabs[0] >= 0).sum(axis=1)) == per_node
        assert (2 * n_un, n_p) == (b.ls.n_u, b.ls.n_p)
        no_old, with_old = (CASES_NO_OLD, CASES_OLD) if mesh in SMALL else ([CASES_NO_OLD[0], CASES_NO_OLD[-1]], [])
        for cases in (no_old, with_old):
            for kind in ("real", "random"):
                b.set_assembly(b.case, _real_tables() if kind == "real" else AR.random_tables(41))
                for stokes, inv_dt, old, inhomog in cases:
                    b.check(kind, stokes, inv_dt, old, inhomog)
        if mesh in INTEGER and variant == "shuffled":
            b.check_integer()
    finally:
        b.close()


def test_launch_shapes_are_the_ones_meant():
    n = {m: AR.MESHES[m][1] for m in AR.MESHES}
    assert n["2x2"] % 4 == 1 and n["3x2"] % 4 == 2 and n["2x4"] % 4 == 3 and n["L"] % 4 == 0   # idle waves of asm_F_rows
    assert n["2x4"] < 256 < n["7x4"]                                          # asm_rhs_u: one thread per node
    assert AR.MESHES["7x4"][2] < 256 < AR.MESHES["8x8"][2]                    # asm_rhs_p: one thread per pressure DoF
    assert len(AR.MESHES["2x4"][0]) < 16 < len(AR.MESHES["7x4"][0])           # asm_cell_state: 16 cells per workgroup
    assert np.diff(AR.polyomino(AR.MESHES["2x2"][0]).F[0]).max() == 98        # a row of 49 blocks


# ------------------------------------------------------------------------------------------------ error returns
def test_error_returns_of_the_hand_off_leave_the_handle_usable():
    """-62 ... -65 of nsk_assembly_set_cells / nsk_assembly_set_dirichlet: the host checks run before anything is stored
    or launched, and the next assembly gives the bits of the one before."""
    b = Bench("corner", "lattice")
    try:
        ls, poly, case = b.ls, b.poly, b.case
        good = _problem(poly, case, _real_tables())
        with pytest.raises(RuntimeError, match=r"nsk error -66: nsk_debug_asm"):
            _hook(ls, D0, np.float64, 1)          # no cells yet
        ls.set_assembly(good, bc_u=case["bc"])
        with pytest.raises(RuntimeError, match=r"nsk error -66: nsk_debug_asm"):
            _hook(ls, D0, np.float64, 1)          # before the first assembly
        ls.state_set(case["su"], case["sp"])
        before = b.assemble(case, AR.NU, 0.0, AR.P_OUT, False, True)

        def same_bits():
            after = b.assemble(case, AR.NU, 0.0, AR.P_OUT, False, True)
            for k in before:
                assert np.array_equal(before[k], after[k]), k

        cu, cp = poly.cell_u, poly.cell_p
        shared = int(np.intersect1d(cu[0], cu[1])[0])
        assert (cu == shared).sum() == 2
        five = [0, 0, 0, 0, 1]                     # the cells of the shared node: one more than four
        inner = int(cu[1, 5])                     # an inner node of cell 1: coupled to no node of cell 0 but the shared one
        bad_cu, bad_range, bad_cp = cu.copy(), cu.copy(), cp.copy()
        bad_cu[0, 5] = inner
        bad_range[1, 7] = poly.n_unodes
        bad_cp[0, 4] = cp[0, 0]
        half = case["dirichlet"].copy()
        k = int(np.nonzero(half)[0][0])
        half[k] = 0
        for code, text, change in (
                (-63, "more than 4 cells touch one velocity node",
                 dict(cell_u_nodes=cu[five], cell_p_dofs=cp[five], cell_flags=case["flags"][five])),
                (-62, "velocity node id out of range", dict(cell_u_nodes=bad_range)),
                (-64, "a cell couples DoFs that are not in the sparsity pattern", dict(cell_u_nodes=bad_cu)),
                (-64, "an owned pressure DoF belongs to no cell", dict(cell_p_dofs=bad_cp)),
                (-65, "Dirichlet flags must cover both components of a node", dict(dirichlet_u=half))):
            with pytest.raises(RuntimeError, match=f"nsk error {code}: .*{text}"):
                ls.set_assembly(dataclasses.replace(good, **change), bc_u=case["bc"])
            if code == -65:   # (the cells were accepted again before the flags were refused: they are the good ones)
                ls.set_assembly(good, bc_u=case["bc"])
            same_bits()
        with pytest.raises(RuntimeError, match=r"nsk error -65: nsk_debug_asm"):
            _hook(ls, 6, np.float64, 1)
        with pytest.raises(RuntimeError, match=r"nsk error -61: nsk_debug_asm"):
            _hook(ls, NODE_SELF, np.int32, poly.n_unodes - 1)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ P2/P1 triangles
SX_MESHES = AR.TRI_MESHES + ["channel", "channel12"]


def _sx_space(name, tmp_path):
    from navier_stokes_solver_amd import gmsh as G
    from navier_stokes_solver_amd import simplex as SX
    from tests.test_simplex import channel_mesh
    if name.startswith("channel"):
        return SX.build_space(G.read_msh(channel_mesh(str(tmp_path / "c.msh"), 12 if name == "channel12" else 10, 5, jitter=0.25)))
    return SX.build_space(G.TriMesh(*AR.tri_mesh(name)))


@pytest.mark.parametrize("mesh", SX_MESHES)
def test_p2p1_kernels_entry_by_entry(mesh, tmp_path):
    """simplex_F_blocks, simplex_d0, simplex_dirichlet_rows, simplex_rhs_u, simplex_rhs_p: the cases of the Q3/Q2 list, with
    the time term as simplex_assemble applies it.  What the kernels receive (grad_lam, area, outlet_w, the block lists)
    comes from simplex.device_handoff; the reference works from the coordinates."""
    from navier_stokes_solver_amd import simplex as SX
    S = _S()
    s = _sx_space(mesh, tmp_path)
    first = SX.assemble(s, 0.1, mode=0, inlet_bc=1, U=0.1)      # the pattern; the values of F are not handed over
    first.F.val[:] = np.nan
    first.simplex = SX.device_handoff(s, first)
    if mesh == "channel":     # 10 x 5: the blocks and the 462 rows of simplex_dirichlet_rows cross 256, its 231 nodes do not;
        assert first.simplex["n_blocks"] > 256 and 2 * s.n_un > 256 >= s.n_un
    if mesh == "channel12":   # 12 x 5 has 275: a second workgroup in simplex_rhs_u
        assert first.simplex["n_blocks"] > 256 and s.n_un > 256 >= s.n_p
    if mesh == "fan":
        assert np.diff(first.simplex["blk_ptr"]).max() == 12 and np.diff(first.simplex["node_ptr"]).max() == 12
    if mesh.startswith("two"):
        assert set(np.diff(first.simplex["blk_ptr"])) == {1, 2}
    rng = np.random.default_rng(43)
    su, sp = rng.uniform(-1, 1, s.n_u), rng.uniform(-1, 1, s.n_p)
    so = su + 0.1 * rng.uniform(-1, 1, s.n_u)
    d = first.dirichlet_u.astype(bool)
    bc = rng.uniform(-1, 1, s.n_u) * d
    outlet = (s.outlet[0], s.outlet[1], s.outlet[2], s.outlet[6])
    rowptr, col = first.F.rowptr.astype(np.int64), first.F.col.astype(np.int64)
    row_of = np.repeat(np.arange(s.n_u), np.diff(rowptr))
    d_row = d[row_of]
    diag = d_row & (col == row_of)
    cells_of = [[int(t) for t in np.nonzero((s.cell_u == n).any(axis=1))[0]] for n in range(s.n_un)]
    names = dict(F=lambda w: f"F[(node {row_of[w] // 2}, {row_of[w] % 2}), (node {col[w] // 2}, {col[w] % 2})], cells "
                             f"{cells_of[row_of[w] // 2]} of the row node",
                 rhs_u=lambda w: f"(node {w // 2}, {w % 2}), cells {cells_of[w // 2]}",
                 rhs_p=lambda w: f"pressure DoF {w}, cells {cells_of[w]}")
    ls = S.LinearSolver()
    try:
        ls.set_problem(first)
        ls.set_assembly(first, bc_u=bc)
        with pytest.raises(RuntimeError, match=r"nsk error -66: nsk_debug_asm"):
            _hook(ls, D0, np.float64, 1)          # the hook covers Q3/Q2 handles
        saved = False
        for stokes, inv_dt, old, inhomog in CASES_NO_OLD + CASES_OLD:
            label = (mesh, "p2p1", "stokes" if stokes else "newton", inv_dt, "old" if old else "no old", "bc" if inhomog else "bc 0")
            assert old or not saved
            if old:
                ls.state_set(so, sp)
                ls.state_save_old()
                saved = True
            ls.state_set(su, sp)

            def assemble():
                nrm = ls.assemble(AR.NU, inv_dt, AR.P_OUT, inhomogeneous_bc=inhomog, stokes=stokes)
                rp, cl, val = ls.get_block(S.BLK_F)
                assert np.array_equal(rp, rowptr) and np.array_equal(cl, col)
                return dict(norm=nrm, F=val, x0=np.concatenate(ls.download_solution()),
                            **dict(zip(("rhs_u", "rhs_p"), ls.download_rhs())))

            g = assemble()
            r = AR.p2p1_reference(s.mesh.nodes, s.mesh.tris, s.cell_u, d, bc if inhomog else None, outlet, rowptr, col, su, sp,
                                  so if old else None, AR.NU, inv_dt, AR.P_OUT, stokes)
            n, kap = r["n_list"], r["kappa"]
            ratios, bounds = {}, {}
            consts = (("F", AR.c_sx_f(n, kap)), ("rhs_u", AR.c_sx_rhs_u(n, kap)), ("rhs_p", AR.c_sx_rhs_p(n, kap)))
            for k, Cc in consts:
                got, ref, A = g[k], r[k], r[k + "_A"]
                err = np.abs(got.astype(LD) - ref).astype(np.float64)
                bounds[k] = (Cc + AR.C_REFERENCE) * AR.U * A
                ratios[k] = float(np.max(err / np.maximum(AR.U * A, 1e-300)))
                w = int(np.argmax(err - bounds[k]))
                assert np.all(err <= bounds[k]), (label, names[k](w), "got", got[w], "reference", float(ref[w]), "error", err[w],
                                                   "bound", bounds[k][w])
            nb = AR.norm_bound(r["norm"], np.concatenate([bounds["rhs_u"], bounds["rhs_p"]]), s.n_u + s.n_p)
            assert abs(LD(g["norm"]) - r["norm"]) <= nb, (label, g["norm"], float(r["norm"]), nb)
            # Dirichlet rows, bit for bit: 0 off the diagonal, one value d0 on it (within F's bound of the reference's, above),
            # rhs = d0 * bc; the initial guess: bc there, 0 everywhere else
            d0 = g["F"][diag][0]
            assert np.all(g["F"][d_row & ~diag] == 0.0) and np.all(g["F"][diag] == d0) and d0 > 0, label
            bcv = r["x0"].astype(np.float64)
            assert np.array_equal(g["rhs_u"][d], d0 * bcv[d]), label
            assert np.array_equal(g["x0"], np.concatenate([bcv, np.zeros(s.n_p)])), label
            assert not np.isnan(g["F"]).any(), label
            g2 = assemble()
            for k in g:
                assert np.array_equal(g[k], g2[k]), (label, k)
            print("asm " + " ".join(str(v) for v in label) + f" (N = {n}, kappa = {kap:.2f}): max err / (2^-53 A): " +
                  ", ".join(f"{k} {ratios[k]:.2f} (C = {Cc:.0f})" for k, Cc in consts))
            _TALLY.add((mesh, "p2p1", stokes, inv_dt, old, inhomog))
    finally:
        ls.close()


# ------------------------------------------------------------------------------------------------ coverage
def test_zz_every_combination_ran():
    want = set()
    for mesh in SMALL + LARGE:
        cases = CASES_NO_OLD + CASES_OLD if mesh in SMALL else [CASES_NO_OLD[0], CASES_NO_OLD[-1]]
        for variant in _variants(mesh):
            want |= {(mesh, variant, kind) + c for kind in ("real", "random") for c in cases}
    want |= {(mesh, "shuffled", "integer") for mesh in INTEGER}
    want |= {(mesh, "p2p1") + c for mesh in SX_MESHES for c in CASES_NO_OLD + CASES_OLD}
    # every (mesh kind, phase, time-term rule) of the issue's list is among them
    rules = {(c[0], c[1] != 0.0, c[2]) for c in CASES_NO_OLD + CASES_OLD}
    assert rules == {(False, False, False), (True, False, False), (False, True, True), (False, True, False), (False, False, True)}
    assert any(c[3] for c in CASES_NO_OLD)
    missing = want - _TALLY
    assert not missing, sorted(missing, key=str)[:10]
    print(f"asm kernels module: {len(_TALLY)} combinations, {time.perf_counter() - T_START:.1f} s wall")
