"""Device assembly, forces and the VTU record of P2/P1 triangle meshes on several ranks: rank threads of one
process joined by the in-process transport, every rank with its own handle, its cells in local numbering
(`simplex.device_rank_handoff`) and a resident state with a halo-refreshed ghost tail.

The assembled values are the one-rank device assembly's BITS (the lists keep the one-rank order of every sum), the forces
obey the bound of tests/test_gpu_forces.py with one more rounding per further rank, the record is the bits of the state.

Meshes: `channel_mesh(4, 3, jitter=0.25)` (24 cells; at 3 ranks the middle rank has ghosts on both sides) and the
reference's coarse mesh with its cylinder tagged 10 (122 cells, 14 obstacle edges)."""
import dataclasses
import threading
import time
from fractions import Fraction

import numpy as np
import pytest

from navier_stokes_solver_amd import gmsh as G
from navier_stokes_solver_amd import newton as N
from navier_stokes_solver_amd import partition as PT
from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import simplex as SX
from tests import forces_reference as R
from tests.test_gpu_forces import NUS, U, _within, c_p2
from tests.test_simplex import channel_mesh
from tests.test_simplex_rank_handoff import cylinder_mesh
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spaces(tmp_path_factory):
    """Per mesh: the space, the first (Stokes) hand-off and its one-rank device hand-off — computed once, never changed."""
    d = tmp_path_factory.mktemp("simplex_ranks")
    out = {}
    for name, s in (("channel", SX.build_space(G.read_msh(channel_mesh(str(d / "c.msh"), 4, 3, jitter=0.25)))),
                    ("cylinder", SX.build_space(cylinder_mesh()))):
        first = SX.assemble(s, 0.1, mode=0, inlet_bc=1, U=0.1)
        first.simplex = SX.device_handoff(s, first)
        out[name] = (s, first)
    return out


def _parts(s, first, nranks):
    from navier_stokes_solver_amd import solver as S
    lay = SX.rank_layout(s, nranks)
    parts = [SX.local_problem(first, lay, r) for r in range(nranks)]
    for r, q in enumerate(parts):
        q.simplex = SX.device_rank_handoff(s, lay, r, q)
    plans = [{S.SPACE_U: PT.build_halo_plan(r, lay.u_ranges, [q.ghost_u for q in parts]),
              S.SPACE_P: PT.build_halo_plan(r, lay.p_ranges, [q.ghost_p for q in parts])} for r in range(nranks)]
    return lay, parts, plans


def _on_ranks(nranks, fn, deadline=120.0):
    """fn(rank, uid) on `nranks` threads; the first failure takes the library's local group down, the peers are joined with
    a deadline (tests/test_gpu_simplex.py::test_multi_rank_operators_on_a_gmsh_partition)."""
    from navier_stokes_solver_amd import solver as S
    uid = S.local_group_id(nranks, on_stream=True)
    res, errs = [None] * nranks, []

    def run(r):
        try:
            res[r] = fn(r, uid)
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
            S.abort_local_group(uid)

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(nranks)]
    [t.start() for t in th]
    end = time.time() + deadline
    [t.join(max(0.0, end - time.time())) for t in th]
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a rank is still blocked after the deadline"
    return res


def _handle(q, plan, r, nranks, uid):
    from navier_stokes_solver_amd import solver as S
    ls = S.LinearSolver(r, nranks, 0, uid)
    try:
        ls.set_problem(q, plan)
        ls.set_assembly(q, bc_u=q.x0_u)
    except Exception:
        ls.close()
        raise
    return ls


def _to_layout(lay, u, p):
    """one-rank numbering -> the layout's (rank by rank)"""
    du, dp = lay.dof_new()
    ul, pl = np.empty_like(u), np.empty_like(p)
    ul[du], pl[dp] = u, p
    return ul, pl


def _owned(lay, r, ul, pl):
    return ul[lay.u_ranges[r]:lay.u_ranges[r + 1]], pl[lay.p_ranges[r]:lay.p_ranges[r + 1]]


@pytest.mark.parametrize("stokes,inv_dt", [(0, 0.0), (1, 0.0), (0, 100.0)])
@pytest.mark.parametrize("nranks", [2, 3])
def test_rank_assembly_is_the_one_rank_device_assembly_bit_for_bit(spaces, nranks, stokes, inv_dt):
    from navier_stokes_solver_amd import solver as S
    nu = 1.0 / 30.0
    for name, (s, first) in spaces.items():
        rng = np.random.default_rng(7)
        free = np.repeat(s.dirichlet == 0, 2)
        u = 0.3 * rng.uniform(-1, 1, s.n_u) * free
        p = rng.uniform(-1, 1, s.n_p)
        u_old = 0.3 * rng.uniform(-1, 1, s.n_u) * free
        host = SX.assemble(s, nu, mode=0 if stokes else 1, state=(u, p), inlet_bc=1, U=0.1, inv_dt=inv_dt,
                           state_old=u_old if inv_dt else None)
        # the one-rank device assembly first
        ls = S.LinearSolver()
        try:
            ls.set_problem(first)
            ls.set_assembly(first, bc_u=first.x0_u)
            if inv_dt:
                ls.state_set(u_old, p); ls.state_save_old()
            ls.state_set(u, p)
            nrm1 = ls.assemble(nu, inv_dt, 1.0, inhomogeneous_bc=True, stokes=bool(stokes))
            val1 = ls.get_block(S.BLK_F)[2]
            ru1, rp1 = ls.download_rhs()
        finally:
            ls.close()
        one = dataclasses.replace(first, F=P.CsrBlock(first.F.rows, first.F.cols, first.F.rowptr, first.F.col, val1),
                                  rhs_u=ru1, rhs_p=rp1)
        lay, parts, plans = _parts(s, first, nranks)
        want = [SX.local_problem(one, lay, r) for r in range(nranks)]
        want_host = [SX.local_problem(host, lay, r) for r in range(nranks)]
        ul, pl = _to_layout(lay, u, p)
        ol, _ = _to_layout(lay, u_old, p)

        def run(r, uid):
            ls = _handle(parts[r], plans[r], r, nranks, uid)
            try:
                if inv_dt:
                    ls.state_set(*_owned(lay, r, ol, pl)); ls.state_save_old()
                ls.state_set(*_owned(lay, r, ul, pl))
                nrm = ls.assemble(nu, inv_dt, 1.0, inhomogeneous_bc=True, stokes=bool(stokes))
                blk, rhs = ls.get_block(S.BLK_F), ls.download_rhs()
                nrm2 = ls.assemble(nu, inv_dt, 1.0, inhomogeneous_bc=True, stokes=bool(stokes))
                return dict(nrm=nrm, blk=blk, rhs=rhs, nrm2=nrm2, val2=ls.get_block(S.BLK_F)[2], rhs2=ls.download_rhs())
            finally:
                ls.close()

        res = _on_ranks(nranks, run)
        scale_f = np.abs(host.F.val).max()
        scale_r = max(np.abs(host.rhs_u).max(), np.abs(host.rhs_p).max())
        for r, (o, w, wh) in enumerate(zip(res, want, want_host)):
            rp, col, val = o["blk"]
            assert np.array_equal(rp, w.F.rowptr) and np.array_equal(col, w.F.col), (name, r)
            assert np.array_equal(val, w.F.val), (name, r, float(np.abs(val - w.F.val).max()))
            assert np.array_equal(o["rhs"][0], w.rhs_u) and np.array_equal(o["rhs"][1], w.rhs_p), (name, r)
            # against the host producer: the bound of test_device_assembly_of_p2p1_cells_matches_the_host_producer
            assert np.abs(val - wh.F.val).max() <= 1e-13 * scale_f
            assert np.abs(o["rhs"][0] - wh.rhs_u).max() <= 1e-13 * scale_r and np.abs(o["rhs"][1] - wh.rhs_p).max() <= 1e-13 * scale_r
            # the norm is global: the same on every rank, the one-rank norm to its bound
            print(f"{name} rank {r}/{nranks}: norm {o['nrm']!r}, one rank {nrm1!r}")
            assert o["nrm"] == res[0]["nrm"] and abs(o["nrm"] - nrm1) <= 1e-12 * nrm1
            # a second assembly: the same bits
            assert o["nrm2"] == o["nrm"] and np.array_equal(o["val2"], val)
            assert np.array_equal(o["rhs2"][0], o["rhs"][0]) and np.array_equal(o["rhs2"][1], o["rhs"][1])
        assert sum(q.simplex["pos00"] >= 0 for q in parts) == 1


@pytest.mark.parametrize("nranks", [2, 3])
def test_forces_and_record_on_the_ranks_of_the_cylinder_mesh(spaces, nranks):
    """Forces: the totals are equal on all ranks, the shares add up to them within one rounding per further rank, the total
    obeys |total - exact| <= C u A with C the P2/P1 count of tests/test_gpu_forces.py plus one per further rank (the
    additions of the all-reduce, as DESIGN 5q counts for Q3/Q2); a rank without edges reports exactly (0, 0).
    Record: every rank's bytes are the state at its points — ghost vertices on the cut included; two calls, the same bytes."""
    s, first = spaces["cylinder"]
    lay, parts, plans = _parts(s, first, nranks)
    ec, el, nl = SX.force_edges(s)
    rng = np.random.default_rng(3)
    u, p = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    ul, pl = _to_layout(lay, u, p)
    edges = [SX.force_edges_rank(s, lay, r, parts[r].simplex) for r in range(nranks)]
    points = [SX.record_points_rank(s, lay, r, parts[r].simplex) for r in range(nranks)]
    assert sum(len(e[0]) for e in edges) == 14 and min(len(e[0]) for e in edges) == (0 if nranks == 3 else 3)

    def run(r, uid):
        ls = _handle(parts[r], plans[r], r, nranks, uid)
        try:
            ls.set_force_edges_rank(s, lay, r, parts[r].simplex)
            ls.set_record_points(points[r][2], points[r][3])
            ls.state_set(*_owned(lay, r, ul, pl))
            n = len(points[r][2])
            rec = ls.state_record(n_points=n)
            rec2 = ls.state_record(n_points=n)
            return dict(forces=[ls.forces(nu, local=True) for nu in NUS], again=[ls.forces(nu, local=True) for nu in NUS],
                        rec=(rec[0].tobytes(), rec[1].tobytes()), rec2=(rec2[0].tobytes(), rec2[1].tobytes()))
        finally:
            ls.close()

    res = _on_ranks(nranks, run)
    for k, nu in enumerate(NUS):
        exact, a = R.p2_forces(s.cell_u, s.cell_p, s.grad_lam, ec, el, nl, u, p, nu)
        total = res[0]["forces"][k][0]
        shares = [res[r]["forces"][k][1] for r in range(nranks)]
        for r in range(nranks):
            assert res[r]["forces"][k][0] == total and res[r]["again"][k] == res[r]["forces"][k]
            if len(edges[r][0]) == 0:
                assert shares[r] == (0.0, 0.0)
        for c in range(2):
            exact_sum = sum(Fraction(sh[c]) for sh in shares)
            bound = (nranks - 1) * Fraction(U) * sum(abs(Fraction(sh[c])) for sh in shares)
            assert abs(Fraction(total[c]) - exact_sum) <= bound * (1 + Fraction(1, 10 ** 14)), (nu, c)
        _within(total, exact, a, c_p2(max(len(e[0]) for e in edges)) + nranks - 1, f"P2/P1 {nranks} ranks nu={nu}")
    ghost_points = 0
    for r in range(nranks):
        xy, tris, u_node, p_dof = points[r]
        verts = parts[r].simplex["vert_ids"][p_dof]
        vel3 = np.stack([u[2 * verts], u[2 * verts + 1], np.zeros(len(verts))], axis=1)
        assert res[r]["rec"] == (vel3.tobytes(), p[verts].tobytes()) and res[r]["rec2"] == res[r]["rec"]
        ghost_points += int((u_node >= parts[r].n_u // 2).sum())
    assert ghost_points > 0                       # vertices of the cut belong to the lower rank: ghosts of the higher one's cells


def test_error_cases_return_their_codes_with_text(spaces):
    from navier_stokes_solver_amd import solver as S
    s, first = spaces["channel"]
    lay, parts, plans = _parts(s, first, 2)

    def run(r, uid):
        q = parts[r]
        n_all, np_all = (q.n_u + len(q.ghost_u)) // 2, q.n_p + len(q.ghost_p)
        ls = S.LinearSolver(r, 2, 0, uid)
        try:
            ls.set_problem(q, plans[r])
            # an odd ghost count: the ghost velocity DoFs are not whole nodes
            i = q.info
            ls.set_partition(S.SPACE_U, i["u_begin"], i["u_end"], q.ghost_u[:-1])
            with pytest.raises(RuntimeError, match=r"nsk error -65: \S.*whole nodes"):
                ls.set_assembly(q, bc_u=q.x0_u)
            ls.set_partition(S.SPACE_U, i["u_begin"], i["u_end"], q.ghost_u)
            # a node / DoF id at owned + ghost: caught on the host, nothing is launched
            for key, at, what in (("cell_u", n_all, "velocity node"), ("cell_p", np_all, "pressure DoF")):
                bad = dataclasses.replace(q)
                bad.simplex = dict(q.simplex, **{key: q.simplex[key].copy()})
                bad.simplex[key][-1, -1] = at
                with pytest.raises(RuntimeError, match=rf"nsk error -64: \S.*{what} id out of range"):
                    ls.set_assembly(bad, bc_u=q.x0_u)
            ls.set_assembly(q, bc_u=q.x0_u)
            ls.state_set(np.zeros(q.n_u), np.zeros(q.n_p))
            # a record without a list on several ranks: as before
            with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*one rank"):
                ls.state_record(n_points=q.n_p)
            for un, pd in (([n_all], [0]), ([0], [np_all]), ([-1], [0]), ([0], [-1])):
                with pytest.raises(RuntimeError, match=r"nsk error -72: \S.*out of range"):
                    ls.set_record_points(un, pd)
            ls.set_record_points([n_all - 1], [np_all - 1])              # the last ghost: valid
            assert ls.state_record(n_points=1)[0].tolist() == [[0.0, 0.0, 0.0]]
            ls.set_record_points([], [])                                 # n_points = 0: valid
            assert ls.state_record(n_points=0)[1].shape == (0,)
            ls.set_assembly(q, bc_u=q.x0_u)                              # new cell data void the list
            with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*one rank"):
                ls.state_record(n_points=q.n_p)
        finally:
            ls.close()
        return True

    assert _on_ranks(2, run) == [True, True]
    # one rank: pos00 = -1 names no owner
    ls = S.LinearSolver()
    try:
        ls.set_problem(first)
        bad = dataclasses.replace(first)
        bad.simplex = dict(first.simplex, pos00=-1)
        with pytest.raises(RuntimeError, match=r"nsk error -64: \S.*pos00"):
            ls.set_assembly(bad, bc_u=first.x0_u)
    finally:
        ls.close()
    # the point list belongs to P2/P1 handles
    pr = P.generate(16, 10, nu=0.1, mode=0, state=0, inlet_bc=1)
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        with pytest.raises(RuntimeError, match=r"nsk error -69: \S.*no cells"):
            ls.set_record_points([0], [0])
        ls.set_assembly(pr, bc_u=pr.x0_u)
        with pytest.raises(RuntimeError, match=r"nsk error -71: \S.*Q3/Q2"):
            ls.set_record_points([0], [0])
    finally:
        ls.close()


def test_a_line_search_step_after_an_assembly_adds_the_solves_result(spaces):
    """solution = evaluation_point + alpha * delta_owned for every alpha of one line search: the assembly between two
    steps writes the next initial guess over the resident result, which must not take the direction with it.
    From the state 0 both steps are one product per entry: exact."""
    from navier_stokes_solver_amd import solver as S
    s, first = spaces["channel"]
    ls = S.LinearSolver()
    try:
        ls.set_problem(first)
        ls.set_assembly(first, bc_u=first.x0_u)
        ls.state_set(np.zeros(s.n_u), np.zeros(s.n_p))
        ls.assemble(0.1, 0.0, 1.0, inhomogeneous_bc=True, stokes=True)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        its, res, rc = ls.solve_resident(S.FGMRES, 1e-10, 20000)
        assert rc == 0 and its > 0
        du, dp = ls.download_solution()
        free = np.repeat(s.dirichlet == 0, 2)
        assert np.abs(du[free]).max() > 1e-3 and np.abs(dp).max() > 1e-3
        ls.state_save()
        ls.state_update(1.0)
        u, p = ls.state_get()
        assert np.array_equal(u, du) and np.array_equal(p, dp)
        for alpha in (0.1, 0.01):
            ls.assemble(0.1, 0.0, 1.0, inhomogeneous_bc=False, stokes=True)
            ls.state_update(alpha)
            u, p = ls.state_get()
            assert np.array_equal(u, alpha * du) and np.array_equal(p, alpha * dp), alpha
    finally:
        ls.close()


def test_newton_on_two_ranks_with_device_assembly_matches_the_direct_driver(tmp_path, monkeypatch):
    """solve_newton() to Re 10 on 2 ranks of the coarse mesh through the drivers' rank function (cli._gmsh_rank_main)
    against the one-rank host-assembly driver with sparse-direct solves; the bounds of
    tests/test_gpu_simplex.py::test_newton_on_several_ranks_matches_the_direct_driver."""
    from navier_stokes_solver_amd import cli
    from navier_stokes_solver_amd import solver as S
    from tests.test_simplex import REF_MESH
    s = SX.build_space(G.read_msh(REF_MESH))
    ref = N.SimplexBackend(None, s, 1, 2, 1e-11, direct=True)
    h_ref = N.solve_newton(ref, 10.0, log=lambda *_: None)
    nranks = 2
    lay = SX.rank_layout(s, nranks)
    first = SX.assemble(s, 0.1, mode=0, inlet_bc=1, U=0.1)
    grp = cli._ThreadGroup(nranks)
    cfg = dict(solver=S.FGMRES, prec=S.ASIMPLE, tol=1e-11, Re=10.0, vtu_format="ascii")
    out = {}

    def run(r, uid):
        try:
            cli._gmsh_rank_main(cfg, False, r, nranks, grp, lambda: S.LinearSolver(r, nranks, 0, uid), lambda *_a, **_k: None,
                                s, lay, first, out=out)
        except Exception:
            grp.abort()
            raise

    monkeypatch.setenv("NSK_OUTPUT_DIR", str(tmp_path))
    monkeypatch.delenv("NSK_HOST_POSTPROCESS", raising=False)
    _on_ranks(nranks, run, deadline=300.0)
    assert all((tmp_path / f"output-stokes_0.{r}.vtu").exists() for r in range(nranks)) and (tmp_path / "output-stokes_0.pvtu").exists()
    # (Re 10 is the first level: the Stokes passes up to the full inlet velocity.)  Norms and counts are global
    assert out[0]["history"] and out[0]["history"] == out[1]["history"] and len(h_ref) == len(out[0]["history"])
    ug, pg = SX.gather_solution(lay, [out[r]["solution"][0] for r in range(nranks)], [out[r]["solution"][1] for r in range(nranks)])
    ur, prr = ref.solution()
    print(f"velocity {rel_err(ug, ur):.3e}, pressure {rel_err(pg, prr):.3e}")
    assert rel_err(ug, ur) <= 1e-7 and rel_err(pg, prr) <= 1e-6
