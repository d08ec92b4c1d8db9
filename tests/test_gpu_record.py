"""`nsk_record_set_cells` / `nsk_state_get_record` on the GPU: the record in file layout against the state
(s = 1: a copy) and against the extended-precision statement of tests/record_reference.py (s > 1).

The bound for s > 1 is |result - exact| <= C u A_pt, u = 2^-53, A_pt the sum of the absolute values of the elementary
products W[pt][n] state[n] of the point, C the number of roundings an elementary product can pass, counted from
state_record_kernel in csrc/nsk_assembly_kernels.hip.  No measured constant enters.

    ux += W[n] * uv.x, n = 0..15, one accumulator starting at 0.0: the product rounds once (not at all when fused), the
    first addition (to 0.0) is exact, every later one rounds: product n passes at most 1 + 15 roundings            16
    p += Wp[m] * sp[..], m = 0..8, alike                                                                              9
    + 1 for the terms of second order ((1 + u)^16 - 1 <= 16 u (1 + 1e-14)) and the rounding of the extended-precision
    reference (2^-64 per operation)                                                        C_VEL = 17, C_PRS = 10
A row of the table that is a unit vector (a vertex point) gives 0 * x + ... + 1 * state[n] + ...: the entry itself.
"""
import threading

import numpy as np
import pytest

from navier_stokes_solver_amd import gmsh as G
from navier_stokes_solver_amd import partition as PT
from navier_stokes_solver_amd import postprocess as PP
from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import simplex as SX
from tests import forces_reference as R
from tests import record_reference as RR
from tests.test_gpu_forces import _handle, _simplex_handle, _state
from tests.test_simplex import REF_MESH

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
C_VEL, C_PRS = 17, 10
ZERO_BITS = np.zeros(1).tobytes()


def _vertices(s):
    return [0, s, s * (s + 1), (s + 1) ** 2 - 1]


def _check_copy(vel3, prs, pr, cells, ul, pl):
    """s = 1: the bits of the state at the cells' vertices, z = +0.0."""
    un, pn = pr.cell_u_nodes[cells][:, [0, 3, 12, 15]].reshape(-1), pr.cell_p_dofs[cells][:, [0, 2, 6, 8]].reshape(-1)
    assert vel3.shape == (4 * len(cells), 3) and prs.shape == (4 * len(cells),)
    assert np.ascontiguousarray(vel3[:, 0]).tobytes() == ul[2 * un].tobytes()
    assert np.ascontiguousarray(vel3[:, 1]).tobytes() == ul[2 * un + 1].tobytes()
    assert prs.tobytes() == pl[pn].tobytes()
    assert np.ascontiguousarray(vel3[:, 2]).tobytes() == ZERO_BITS * len(vel3)


def _check_sums(vel3, prs, pr, cells, s, ul, pl, what):
    """s > 1: within C u A_pt of the exact sums; the vertex points are the entries of the state."""
    wu, wp = PP.record_tables(s)
    ppc = (s + 1) ** 2
    ev, ep, av, ap = RR.record_sums(pr.cell_u_nodes, pr.cell_p_dofs, cells, wu, wp, ul, pl)
    assert vel3.shape == (len(cells) * ppc, 3) and prs.shape == (len(cells) * ppc,)
    gv, gp = vel3[:, :2].reshape(len(cells), ppc, 2), prs.reshape(len(cells), ppc)
    rv = np.abs(gv.astype(np.longdouble) - ev) / (U * av)
    rp = np.abs(gp.astype(np.longdouble) - ep) / (U * ap)
    print(f"{what}: max |error| / (u A_pt): velocity {float(rv.max()):.3f} (C = {C_VEL}), pressure {float(rp.max()):.3f} (C = {C_PRS})")
    assert (rv <= C_VEL).all() and (rp <= C_PRS).all()
    assert np.ascontiguousarray(vel3[:, 2]).tobytes() == ZERO_BITS * len(vel3)
    un, pn = pr.cell_u_nodes[cells][:, [0, 3, 12, 15]], pr.cell_p_dofs[cells][:, [0, 2, 6, 8]]
    v = _vertices(s)
    assert np.array_equal(gv[:, v, 0], ul[2 * un]) and np.array_equal(gv[:, v, 1], ul[2 * un + 1])
    assert np.array_equal(gp[:, v], pl[pn])


@pytest.fixture(scope="module")
def one_rank():
    pr = P.generate(16, 10, nu=0.1, mode=0, state=0, inlet_bc=1)
    state = _state(pr)
    ls = _handle(pr, state=state, faces=False)
    yield pr, state, ls
    ls.close()


def test_one_patch_per_cell_is_a_copy_of_the_state(one_rank):
    pr, state, ls = one_rank
    n = len(pr.cell_flags)
    assert n == 158
    for cells in (np.arange(n)[::-1].copy(), np.arange(n)[::3].copy(), np.arange(n)[5::7][::-1].copy()):
        ls.set_record(cells, 1)
        vel3, prs = ls.state_record(4 * len(cells))
        _check_copy(vel3, prs, pr, cells, *state)
        pv, pp = ls.state_patches(cells)                           # the same bytes as nsk_state_get_patches
        assert np.ascontiguousarray(vel3[:, :2]).tobytes() == pv.tobytes() and prs.tobytes() == pp.tobytes()
        again = ls.state_record(4 * len(cells))
        assert again[0].tobytes() == vel3.tobytes() and again[1].tobytes() == prs.tobytes()
    ls.set_record(np.zeros(0, np.int32), 1)
    vel3, prs = ls.state_record(0)
    assert vel3.shape == (0, 3) and prs.shape == (0,)


@pytest.mark.parametrize("s", [2, 3])
def test_subdivided_patches_against_the_exact_sums(one_rank, s):
    pr, state, ls = one_rank
    cells = np.arange(len(pr.cell_flags), dtype=np.int32)
    n_points = len(cells) * (s + 1) ** 2
    assert n_points % 256 != 0 and (s != 3 or n_points == 2528)    # the last workgroup is not full
    ls.set_record(cells, s)
    # into positions of a larger buffer, as a report fills its file image
    image = np.full(4 * n_points + 3, np.nan)
    vel3, prs = image[1:1 + 3 * n_points].reshape(-1, 3), image[2 + 3 * n_points:2 + 4 * n_points]
    ls.state_record(vel3=vel3, prs=prs)
    assert np.isnan(image[[0, 1 + 3 * n_points, -1]]).all()         # nothing next to them is touched
    _check_sums(vel3, prs, pr, cells, s, *state, what=f"16x10 s={s}")
    again = ls.state_record(n_points)
    assert again[0].tobytes() == vel3.tobytes() and again[1].tobytes() == prs.tobytes()
    # a reversed subset
    sub = cells[::-5].copy()
    ls.set_record(sub, s)
    v2, p2 = ls.state_record(len(sub) * (s + 1) ** 2)
    ppc = (s + 1) ** 2
    assert np.array_equal(v2.reshape(len(sub), ppc, 3), vel3.reshape(len(cells), ppc, 3)[sub])
    assert np.array_equal(p2.reshape(len(sub), ppc), prs.reshape(len(cells), ppc)[sub])
    ls.set_record(np.zeros(0, np.int32), s)
    assert ls.state_record(0)[1].shape == (0,)


def test_record_on_two_ranks_reads_the_ghosts_of_the_cut():
    """4 x 10 on [0, 0.44]: the cut at column 2 beside the hole at column 1; rank 1's cells use rank 0's nodes on the cut."""
    from navier_stokes_solver_amd import solver as S
    nx, ny, lx = 4, 10, 0.44
    one = P.generate(nx, ny, nu=0.1, mode=0, state=0, inlet_bc=1, lx=lx)
    parts = [P.generate(nx, ny, nu=0.1, mode=0, state=0, inlet_bc=1, lx=lx, nranks=2, rank=r) for r in range(2)]
    state = _state(one)
    plans = [{S.SPACE_U: PT.build_halo_plan(r, parts[0].u_ranges, [p.ghost_u for p in parts]),
              S.SPACE_P: PT.build_halo_plan(r, parts[0].p_ranges, [p.ghost_p for p in parts])} for r in range(2)]
    uid = S.local_group_id(2, False)
    res, errs = [None, None], []

    def run(r):
        try:
            ls = _handle(parts[r], plans[r], r, 2, uid, state, faces=False)
            try:
                own = np.nonzero(parts[r].cell_in_strip)[0]
                out = {}
                for s in (1, 3):
                    ls.set_record(own, s)
                    n = len(own) * (s + 1) ** 2
                    out[s] = (ls.state_record(n), ls.state_record(n))
                res[r] = out
            finally:
                ls.close()
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
            S.abort_local_group(uid)

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(2)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not errs, errs
    assert all(r is not None for r in res)
    for r, p in enumerate(parts):
        ul, pl = R.local_state(p, *state)
        own = np.nonzero(p.cell_in_strip)[0]
        n_own_u, n_own_p = (p.info["u_end"] - p.info["u_begin"]) // 2, p.info["p_end"] - p.info["p_begin"]
        # the nodes of the cut line are rank 0's: ghosts of rank 1's cells, at the vertices and inside the edges
        assert (p.cell_u_nodes[own] >= n_own_u).any() == (r == 1) and (p.cell_p_dofs[own] >= n_own_p).any() == (r == 1)
        assert (p.cell_u_nodes[own][:, [0, 3, 12, 15]] >= n_own_u).any() == (r == 1)
        for s in (1, 3):
            (vel3, prs), again = res[r][s]
            assert again[0].tobytes() == vel3.tobytes() and again[1].tobytes() == prs.tobytes()
            if s == 1:
                _check_copy(vel3, prs, p, own, ul, pl)
            else:
                _check_sums(vel3, prs, p, own, s, ul, pl, what=f"4x10 rank {r} s={s}")


def test_simplex_record_is_the_vertices_of_the_state():
    s = SX.build_space(G.read_msh(REF_MESH))
    rng = np.random.default_rng(4)
    u, p = rng.standard_normal(s.n_u), rng.standard_normal(s.n_p)
    ls = _simplex_handle(s, edges=False)
    try:
        ls.state_set(u, p)
        n = s.n_p
        assert n % 256 != 0 and 2 * n < s.n_u
        vel3, prs = ls.state_record(n)
        assert np.ascontiguousarray(vel3[:, 0]).tobytes() == u[0:2 * n:2].tobytes()
        assert np.ascontiguousarray(vel3[:, 1]).tobytes() == u[1:2 * n:2].tobytes()
        assert prs.tobytes() == p[:n].tobytes() and np.ascontiguousarray(vel3[:, 2]).tobytes() == ZERO_BITS * n
        again = ls.state_record(n)
        assert again[0].tobytes() == vel3.tobytes() and again[1].tobytes() == prs.tobytes()
        with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*n_points"):
            ls.state_record(n - 1)
        with pytest.raises(RuntimeError, match=r"nsk error -71: \S.*P2/P1"):
            ls.set_record([0], 1)
    finally:
        ls.close()


def test_error_cases_return_their_codes_with_text():
    from navier_stokes_solver_amd import solver as S
    pr = P.generate(16, 10, nu=0.1, mode=0, state=0, inlet_bc=1)
    n = len(pr.cell_flags)
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        # no cells on the handle
        for call in (lambda: ls.set_record([0], 1), lambda: ls.state_record(4)):
            with pytest.raises(RuntimeError, match=r"nsk error -69: \S.*cells"):
                call()
        ls.set_assembly(pr, bc_u=pr.x0_u)
        with pytest.raises(RuntimeError, match=r"nsk error -69: \S.*no record list"):
            ls.state_record(4)
        # bad arguments: subdivisions outside 1..4, s > 1 without tables
        for s in (0, 5, -1):
            with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*subdivisions"):
                ls.set_record([0], s)
        c = np.zeros(1, np.int32)
        wu, wp = PP.record_tables(2)
        for a, b in ((None, None), (wu.ctypes.data, None), (None, wp.ctypes.data)):
            with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*bad arguments"):
                ls._ck(ls.L.nsk_record_set_cells(ls.h, 1, c.ctypes.data, 2, a, b))
        with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*bad arguments"):
            ls._ck(ls.L.nsk_record_set_cells(ls.h, 1, None, 1, None, None))
        # a cell index out of range, checked at hand-off: nothing is handed over
        for cells in ([n], [-1], [0, 1, n]):
            with pytest.raises(RuntimeError, match=r"nsk error -72: \S.*out of range"):
                ls.set_record(cells, 3)
        with pytest.raises(RuntimeError, match=r"nsk error -69: \S.*no record list"):
            ls.state_record(16)
        ls.set_record([0, 1], 3)
        # no state
        with pytest.raises(RuntimeError, match=r"nsk error -73: \S.*no state"):
            ls.state_record(32)
        ls.state_set(np.ones(pr.n_u), np.full(pr.n_p, 2.0))
        vel3, prs = ls.state_record(32)
        assert vel3.shape == (32, 3) and np.isfinite(vel3).all() and np.isfinite(prs).all()
        # n_points is not n_cells (s + 1)^2
        for bad in (31, 33, 8, 0):
            with pytest.raises(RuntimeError, match=r"nsk error -60: \S.*n_points"):
                ls.state_record(bad)
        # a new cell list voids the record's, as it voids the faces
        ls.set_assembly(pr, bc_u=pr.x0_u)
        with pytest.raises(RuntimeError, match=r"nsk error -69: \S.*no record list"):
            ls.state_record(32)
    finally:
        ls.close()
