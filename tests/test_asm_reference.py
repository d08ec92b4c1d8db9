"""tests/asm_reference.py is tested here before it judges the device assembly (tests/test_gpu_asm_kernels.py):
against the host producers entry by entry within (C_HOST + C_REFERENCE) 2^-53 A, against a plain int64 evaluation
exactly, and its mesh builder against the generated meshes.  CPU only."""
import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from tests import asm_reference as AR
from tests import matfree_reference as MR

LD = np.longdouble


def _within(name, got, ref, A, C, label):
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    bound = (C + AR.C_REFERENCE) * AR.U * np.asarray(A, dtype=np.float64)
    ratio = float(np.max(err / np.maximum(AR.U * A, 1e-300))) if np.size(err) else 0.0
    print(f"host {label} {name}: max err / (2^-53 A) = {ratio:.2f} (C = {C:.0f})")
    w = int(np.argmax(err - bound)) if np.size(err) > 1 else 0
    assert np.all(err <= bound), (label, name, w, np.ravel(err)[w], np.ravel(bound)[w])


# ------------------------------------------------------------------------------------------------ the mesh builder
@pytest.mark.parametrize("nx,ny", [(1, 1), (2, 1), (3, 2)])
def test_polyomino_of_a_rectangle_is_the_generated_mesh(nx, ny):
    assert P.mesh_info(nx, ny)["n_removed"] == 0
    g = P.generate(nx, ny, nu=0.1, mode=1, state=1)
    p = AR.polyomino(AR.rect(nx, ny))
    assert np.array_equal(p.cell_u, g.cell_u_nodes) and np.array_equal(p.cell_p, g.cell_p_dofs)
    assert p.cell_of_dof0 == g.cell_of_dof0 and 2 * p.n_unodes == g.n_u and p.n_pdofs == g.n_p
    for name in ("F", "Bt", "B", "Mp"):
        rp, col = getattr(p, name)
        blk = getattr(g, name)
        assert np.array_equal(rp, blk.rowptr) and np.array_equal(col, blk.col), name
    nodes, off, self_, pdofs = AR.node_tables(p.cell_u, p.cell_p, p.n_unodes, p.n_pdofs, *p.F)
    assert np.array_equal(nodes, MR.node_cells(g.cell_u_nodes, g.n_u // 2))


def test_the_meshes_of_the_gpu_module_have_the_shapes_their_table_says():
    for name, (cells, n_un, n_p, per_node) in AR.MESHES.items():
        for perms in (None, AR.random_perms(cells, 5)):
            p = AR.polyomino(cells) if perms is None else AR.polyomino(cells, *perms)
            assert (p.n_unodes, p.n_pdofs) == (n_un, n_p), name
            nodes, off, self_, pdofs = AR.node_tables(p.cell_u, p.cell_p, p.n_unodes, p.n_pdofs, *p.F)
            assert set(int(c) for c in (nodes >= 0).sum(axis=1)) == per_node, name
            assert np.diff(p.F[0]).max() <= 98 and off.max() <= 48
            assert p.cell_u[p.cell_of_dof0, 0] == 0 and (p.cell_u == 0).sum() == 1
    assert AR.MESHES["2x2"][1] % 4 == 1 and AR.MESHES["3x2"][1] % 4 == 2 and AR.MESHES["2x4"][1] % 4 == 3
    assert np.diff(AR.polyomino(AR.MESHES["2x2"][0]).F[0]).max() == 98   # the 49-block row


# ------------------------------------------------------------------------------------------------ against the producer
def _state(nx, ny, seed):
    i = P.mesh_info(nx, ny)
    rng = np.random.default_rng(seed)
    su = 0.1 * rng.standard_normal(i["n_u_global"])
    return su, rng.standard_normal(i["n_p_global"]), su + 0.01 * rng.standard_normal(su.size)


CASES = [   # stokes, inv_dt, old state, inlet values
    (False, 0.0, False, False), (True, 0.0, False, False), (False, 100.0, True, False), (True, 100.0, True, False),
    (False, 100.0, False, False), (False, 0.0, True, False), (False, 0.0, False, True), (True, 0.0, False, True)]


@pytest.mark.parametrize("nx,ny", [(3, 2), (16, 10)])
def test_q3q2_reference_against_the_host_producer(nx, ny):
    nu, p_out = 0.05, 0.7
    su, sp, so = _state(nx, ny, 3)
    for stokes, inv_dt, old, inlet in CASES:
        g = P.generate(nx, ny, nu=nu, mode=0 if stokes else 1, state=(su, sp), inv_dt=inv_dt, p_out=p_out,
                       inlet_bc=int(inlet), state_old=so if old else None)
        r = AR.q3q2_reference(g.cell_tables, g.cell_u_nodes, g.cell_p_dofs, g.cell_flags, g.dirichlet_u,
                              g.x0_u if inlet else None, g.cell_of_dof0, g.F.rowptr, g.F.col, su, sp, so if old else None,
                              nu, inv_dt, p_out, stokes)
        label = (nx, ny, stokes, inv_dt, old, inlet)
        assert g.cell_flags.any() and g.dirichlet_u.any()
        _within("F", g.F.val, r["F"], r["F_A"], AR.C_HOST_F, label)
        _within("rhs_u", g.rhs_u, r["rhs_u"], r["rhs_u_A"], AR.C_HOST_RHS_U, label)
        _within("rhs_p", g.rhs_p, r["rhs_p"], r["rhs_p_A"], AR.C_HOST_RHS_P, label)
        d = g.dirichlet_u.astype(bool)
        diag = g.F.val[AR.pattern_positions(g.F.rowptr, g.F.col, np.nonzero(d)[0], np.nonzero(d)[0])]
        assert np.all(diag == diag[0])
        _within("d0", diag[0], abs(r["d0"]), r["d0_A"], AR.C_HOST_D0, label)
        assert np.array_equal(g.x0_u[d], r["x0"][d].astype(np.float64))
        if inlet:
            assert np.abs(g.x0_u).max() > 0


def test_the_old_state_rule():
    """No saved old state: no time term in the residual, inv_dt M in the matrix, zeros in cq's last two fields; a saved one
    at inv_dt == 0: the residual of no time term at all."""
    g = P.generate(3, 2, nu=0.05, mode=1, state=1)
    su, sp, so = _state(3, 2, 4)
    args = (g.cell_tables, g.cell_u_nodes, g.cell_p_dofs, g.cell_flags, g.dirichlet_u, None, g.cell_of_dof0, g.F.rowptr,
            g.F.col, su, sp)
    r0 = AR.q3q2_reference(*args, None, 0.05, 0.0, 1.0, False)
    r1 = AR.q3q2_reference(*args, None, 0.05, 100.0, 1.0, False)
    r2 = AR.q3q2_reference(*args, so, 0.05, 0.0, 1.0, False)
    r3 = AR.q3q2_reference(*args, so, 0.05, 100.0, 1.0, False)
    free = ~g.dirichlet_u.astype(bool)
    assert np.array_equal(r0["rhs_u"][free], r1["rhs_u"][free]) and not np.array_equal(r0["F"], r1["F"])
    assert np.array_equal(r0["rhs_u"], r2["rhs_u"]) and np.array_equal(r0["F"], r2["F"])
    assert not np.array_equal(r3["rhs_u"][free], r1["rhs_u"][free]) and np.array_equal(r3["F"], r1["F"])
    assert not r0["cq"][:, 7:].any() and r2["cq"][:, 7:].any() and np.array_equal(r0["cq"][:, :7], r2["cq"][:, :7])


# ------------------------------------------------------------------------------------------------ the integer-exact case
def test_every_partial_sum_of_the_integer_case_stays_below_two_to_the_53():
    """A bounds every partial sum of every output, in any order and whatever is fused, and it grows with the magnitude of
    every input: its value with every input AT the end of its range, on a mesh with four cells on a node and a
    49-block row, bounds it over the whole range.  Computed, not assumed."""
    cells = AR.MESHES["2x2"][0]
    p = AR.polyomino(cells)
    t = np.full(944, float(AR.INT_TABLE))
    t[912:928] = AR.INT_JXW
    nn = p.n_unodes
    worst = 0.0
    for dirichlet in (np.zeros(2 * nn, np.uint8), np.ones(2 * nn, np.uint8)):
        r = AR.q3q2_reference(t, p.cell_u, p.cell_p, np.ones(len(cells), np.uint8), dirichlet, np.full(2 * nn, float(AR.INT_STATE)),
                              p.cell_of_dof0, *p.F, np.full(2 * nn, float(AR.INT_STATE)), np.full(p.n_pdofs, float(AR.INT_STATE)),
                              np.full(2 * nn, -float(AR.INT_STATE)), AR.INT_NU, AR.INT_INV_DT, AR.INT_P_OUT, False)
        worst = max([worst] + [float(np.max(r[k + "_A"])) for k in ("cq", "d0", "F", "rhs_u", "rhs_p")])
    print(f"integer case: the largest absolute sum any output can reach is {worst:.0f} = 2^{np.log2(worst):.1f}")
    assert 0 < worst < 2.0 ** 53 / 1024     # (the K and M3 tables the library forms on the host are partial sums of F's)


@pytest.mark.parametrize("mesh", ["2x2", "L", "3x2"])
def test_longdouble_and_int64_agree_exactly_on_the_integer_case(mesh):
    cells = AR.MESHES[mesh][0]
    p = AR.polyomino(cells, *AR.random_perms(cells, 21))
    c = AR.integer_case(p, 31)
    for so in (None, c["so"]):
        args = (c["tables"], p.cell_u, p.cell_p, c["flags"], c["dirichlet"], c["bc"], p.cell_of_dof0, *p.F, c["su"], c["sp"],
                so, AR.INT_NU, AR.INT_INV_DT, AR.INT_P_OUT, False)
        r, ri = AR.q3q2_reference(*args), AR.q3q2_int64(*args)
        for k in ("cq", "d0", "F", "rhs_u", "rhs_p"):
            assert np.array_equal(np.asarray(r[k]), np.asarray(ri[k]).astype(LD)), (mesh, k)
            assert np.array_equal(np.asarray(r[k]).astype(np.float64).astype(LD), np.asarray(r[k])), (mesh, k)
            assert np.max(np.abs(ri[k])) <= np.max(r[k + "_A"]) < 2.0 ** 53
        assert np.abs(r["rhs_u"]).max() > 0 and np.abs(r["rhs_p"]).max() > 0 and r["d0"] != 0


def test_int64_evaluation_refuses_fractions():
    p = AR.polyomino(AR.rect(1, 1))
    c = AR.integer_case(p, 1)
    with pytest.raises(ValueError):
        AR.q3q2_int64(c["tables"] + 0.5, p.cell_u, p.cell_p, c["flags"], c["dirichlet"], None, 0, *p.F, c["su"], c["sp"], None,
                      2.0, 4.0, 3.0, False)


def test_extra_blocks_keep_the_pattern_sorted_and_under_the_cap():
    p = AR.polyomino(AR.MESHES["3x2"][0])
    rp, col = AR.add_blocks(p.F, [(0, 69), (69, 0), (5, 60)])
    assert rp[-1] == p.F[0][-1] + 12 and np.diff(rp).max() <= 98
    for r in range(len(rp) - 1):
        assert np.all(np.diff(col[rp[r]:rp[r + 1]]) > 0)
    assert (AR.pattern_positions(rp, col, [0, 1, 139], [138, 139, 1]) >= 0).all()
    assert (AR.pattern_positions(rp, col, [0], [100]) == -1).all()


# ------------------------------------------------------------------------------------------------ P2/P1 triangles
def _sx_spaces(tmp_path):
    from navier_stokes_solver_amd import gmsh as G
    from navier_stokes_solver_amd import simplex as SX
    from tests.test_simplex import REF_MESH, channel_mesh
    yield "channel", SX.build_space(G.read_msh(channel_mesh(str(tmp_path / "c.msh"), 10, 5, jitter=0.25)))
    yield "gmsh", SX.build_space(G.read_msh(REF_MESH))
    for name in AR.TRI_MESHES:
        yield name, SX.build_space(G.TriMesh(*AR.tri_mesh(name)))


def test_p2p1_reference_against_the_host_producer(tmp_path):
    from navier_stokes_solver_amd import simplex as SX
    nu, p_out = 1.0 / 30.0, 0.7
    for name, s in _sx_spaces(tmp_path):
        rng = np.random.default_rng(7)
        su, sp = 0.3 * rng.uniform(-1, 1, s.n_u), rng.uniform(-1, 1, s.n_p)
        so = su + 0.1 * rng.uniform(-1, 1, s.n_u)
        outlet = (s.outlet[0], s.outlet[1], s.outlet[2], s.outlet[6])
        for stokes, inv_dt, old, inlet in CASES:
            g = SX.assemble(s, nu, mode=0 if stokes else 1, state=(su, sp), inlet_bc=int(inlet), inv_dt=inv_dt, U=0.1,
                            p_out=p_out, state_old=so if old else None)
            r = AR.p2p1_reference(s.mesh.nodes, s.mesh.tris, s.cell_u, g.dirichlet_u, g.x0_u if inlet else None, outlet,
                                  g.F.rowptr, g.F.col, su, sp, so if old else None, nu, inv_dt, p_out, stokes)
            label = (name, stokes, inv_dt, old, inlet)
            n, k = r["n_list"], r["kappa"]
            assert n == np.bincount(s.cell_u.ravel()).max() and 1.0 <= k < 50.0
            _within("F", g.F.val, r["F"], r["F_A"], AR.c_sx_f(n, k) + AR.C_HOST_SX_EXTRA, label)
            _within("rhs_u", g.rhs_u, r["rhs_u"], r["rhs_u_A"], AR.c_sx_rhs_u(n, k) + AR.C_HOST_SX_EXTRA, label)
            _within("rhs_p", g.rhs_p, r["rhs_p"], r["rhs_p_A"], AR.c_sx_rhs_p(n, k) + AR.C_HOST_SX_EXTRA, label)
            assert np.array_equal(g.x0_u, r["x0"].astype(np.float64))


def test_the_hand_made_triangle_meshes_are_what_their_names_say():
    from navier_stokes_solver_amd import gmsh as G
    from navier_stokes_solver_amd import simplex as SX
    for name in AR.TRI_MESHES:
        s = SX.build_space(G.TriMesh(*AR.tri_mesh(name)))
        assert np.all(s.area > 0) and (s.dirichlet != 0).any() and (s.dirichlet == 0).any(), name
        assert len(s.outlet[0]) > 0, name
    fan = SX.build_space(G.TriMesh(*AR.tri_mesh("fan")))
    assert len(fan.cell_u) == 12 and np.bincount(fan.cell_u.ravel())[0] == 12 and len(set(np.round(fan.area, 12))) == 12
    a, b = SX.build_space(G.TriMesh(*AR.tri_mesh("two"))), SX.build_space(G.TriMesh(*AR.tri_mesh("two_rotated")))
    assert len(a.cell_u) == 2 and np.array_equal(a.cell_u[0], b.cell_u[0]) and not np.array_equal(a.cell_u[1], b.cell_u[1])
    assert sorted(a.cell_u[1]) == sorted(b.cell_u[1])
    assert len(SX.build_space(G.TriMesh(*AR.tri_mesh("one"))).cell_u) == 1
