"""NSK_IOPT_FGMRES_SKIP_UNUSED: FGMRES makes its check before it builds a basis column, and does not build the
column no iterate reads — the one in front of the check that ends a solve, and the last one of a full restart cycle.

Every test runs the same calls on two fresh handles, the switch at 0 (deal.II's order) and at 1 (the default), and
compares BYTES: nothing a caller sees may depend on the switch.  The counts asserted are the ones the algorithm fixes:

* with tolerance 0 a solve of K iterations runs ceil(K / 29) restart cycles of at most 29 counted iterations; a cycle of
  r iterations builds r + 1 columns in deal.II's order, so the preconditioner is applied K + ceil(K / 29) times — and
  once less with the switch on (stationary aSIMPLE keeps state: the application at a cycle's end still runs, only the
  one in front of the last check does not);
* one application of the stationary block-diagonal preconditioner (nsk_precond_vmult) is one FGMRES solve on F and one
  CG solve on M_p: the only work the switch removes from it is one SSOR apply and one SpMV per skipped column of the F
  solve, so both counters fall by exactly `columns_skipped`.  (A whole outer solve would also lose its last
  application with everything inside it, so the identity is asserted where it is exact.)
"""
import functools
import math

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from tests.util import problem, rng_vec

pytestmark = pytest.mark.gpu

OFF, ON = 0, 1


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same(on, off, what=""):
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert same_bytes(a, b), f"{what} item {k}"


def _handle(S, pr, skip, prec, variant, gs=None, options=()):
    ls = S.LinearSolver()
    ls.set_option(S.OPT_TRI_ORDERING, 1)
    if gs is not None:
        ls.set_option(S.OPT_INNER_FUSED_GS, gs)
    for opt, v in options:
        ls.set_option(opt, v)
    ls.set_option(S.IOPT_FGMRES_SKIP_UNUSED, skip)
    ls.set_problem(pr)
    ls.setup_preconditioner(prec, variant, 0.5)
    ls.reset_stats()
    return ls


def _solve(S, ls, pr, tol, K):
    """One outer FGMRES solve from the problem's initial guess: everything the caller sees, and the stats of this solve."""
    ls.reset_stats()
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    its, res, rc = ls.solve_resident(S.FGMRES, tol, K)
    xu, xp = ls.download_solution()
    return [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])], ls.stats()


def _pair(fn):
    """fn(skip) for both settings, the switch on first (so that a stale-state bug cannot hide behind the run order)."""
    on = fn(ON)
    off = fn(OFF)
    return on, off


KS = [1, 5, 29, 30, 31, 58, 65]   # ends inside a cycle, exactly at a cycle's end, and just behind one


@functools.lru_cache(maxsize=2)
def _mesh(nx, ny):
    return P.generate(nx, ny, nu=1.0 / 90.0)


def _asimple_case(mesh, K, gs):
    from navier_stokes_solver_amd import solver as S
    pr = _mesh(*mesh)

    def run(skip):
        ls = _handle(S, pr, skip, S.ASIMPLE, S.STATIONARY, gs)
        try:
            return _solve(S, ls, pr, 0.0, K)
        finally:
            ls.close()

    (on, st1), (off, st0) = _pair(run)
    print(f"\n{mesh} K={K} gs={gs}: applies {st0['prec_applies']} -> {st1['prec_applies']}, inner F its {st0['inner_u_its']} -> "
          f"{st1['inner_u_its']}, SpMVs {st0['spmv_calls']} -> {st1['spmv_calls']}, triangular applies {st0['tri_applies']} -> "
          f"{st1['tri_applies']}, columns skipped {st1['columns_skipped']}")
    assert_same(on, off, f"{mesh} K={K} gs={gs}")
    assert tuple(on[3]) == (K, 1) and len(on[2]) == K + 1 + (K - 1) // 29    # (every cycle starts with a check of its own)
    assert st0["prec_applies"] == K + math.ceil(K / 29)
    assert st1["prec_applies"] == st0["prec_applies"] - 1
    assert st0["columns_skipped"] == 0 and st1["columns_skipped"] > 0
    # work done: nothing may grow, and the surplus application's work is gone (its inner solves may have stopped at
    # their first check, but each of them forms a residual first)
    for key in ("inner_u_its", "inner_p_its", "tri_applies"):
        assert st1[key] <= st0[key], key
    assert st1["spmv_calls"] < st0["spmv_calls"]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("gs", [0, 1, 2], ids=["mgs", "cgs", "one_red"])
def test_asimple_at_60x20_is_the_same_bytes(gs, K):
    _asimple_case((60, 20), K, gs)


@pytest.mark.parametrize("K", KS)
def test_asimple_at_300x100_is_the_same_bytes(K):
    _asimple_case((300, 100), K, None)


@pytest.mark.parametrize("case", [("ns16", 0, 0), ("stokes16", 0, 0), ("ns16", 1, 0), ("unsteady16", 2, 1), ("unsteady16", 0, 1)],
                         ids=["blockDiagonal_ns", "blockDiagonal_stokes", "blockTriangular_amg", "aSIMPLE_unsteady",
                              "blockDiagonal_unsteady"])
def test_converged_solves_are_the_same_bytes(case):
    """The `success` exit: the solve ends at a check that is met, inside a cycle, with the column behind it not built.
    blockTriangular (stationary) preconditions F with the AMG V-cycle, unsteady aSIMPLE is two triangular applies."""
    from navier_stokes_solver_amd import solver as S
    name, prec, variant = case
    pr = problem(name)
    tol = 1e-10

    def run(skip):
        ls = _handle(S, pr, skip, prec, variant)
        try:
            return _solve(S, ls, pr, tol, 20000)
        finally:
            ls.close()

    (on, st1), (off, st0) = _pair(run)
    print(f"\n{case}: {on[3][0]} iterations, applies {st0['prec_applies']} -> {st1['prec_applies']}, columns skipped "
          f"{st1['columns_skipped']}")
    assert_same(on, off, str(case))
    assert on[3][1] == 0 and on[4][0] <= tol and on[3][0] >= 2
    assert st0["columns_skipped"] == 0 and st1["columns_skipped"] > 0
    cycles = math.ceil(on[3][0] / 29)
    assert st0["prec_applies"] == on[3][0] + cycles
    if (prec, variant) == (2, 1):
        # two triangular applies that overwrite dst: no application for any column that is not built, and every
        # cycle builds as many columns as it counts iterations
        assert st1["prec_applies"] == on[3][0]
    else:
        assert st1["prec_applies"] == st0["prec_applies"] - 1


@pytest.mark.parametrize("name", ["ns60", "stokes60"])
def test_block_diagonal_application_loses_one_apply_and_one_spmv_per_skipped_column(name):
    from navier_stokes_solver_amd import solver as S
    pr = problem(name)
    su, sp_ = rng_vec(pr.n_u, 11), rng_vec(pr.n_p, 12)

    def run(skip):
        ls = _handle(S, pr, skip, S.BLOCK_DIAGONAL, S.STATIONARY)
        try:
            du, dp, rc = ls.precond_vmult(su, sp_)
            return [du, dp, np.array([rc])], ls.stats()
        finally:
            ls.close()

    (on, st1), (off, st0) = _pair(run)
    print(f"\n{name}: inner F its {st1['inner_u_its']}, triangular applies {st0['tri_applies']} -> {st1['tri_applies']}, SpMVs "
          f"{st0['spmv_calls']} -> {st1['spmv_calls']}, columns skipped {st1['columns_skipped']}")
    assert_same(on, off, name)
    assert on[2][0] == 0
    assert st1["inner_u_its"] == st0["inner_u_its"] > 0 and st1["inner_p_its"] == st0["inner_p_its"]
    skipped = st1["columns_skipped"]
    assert st0["columns_skipped"] == 0
    # the F solve ends at a check (one column) after inner_u_its iterations, with one more per full cycle before it
    assert skipped == 1 + (st1["inner_u_its"] - 1) // 29
    assert st0["tri_applies"] - st1["tri_applies"] == skipped
    assert st0["spmv_calls"] - st1["spmv_calls"] == skipped


# ------------------------------------------------------------------ the application a solve leaves behind
def _two_calls(second, K1=7):
    """Stationary aSIMPLE on one set-up: a solve of K1 iterations, then `second(ls)` without a set-up in between."""
    from navier_stokes_solver_amd import solver as S
    pr = problem("ns60")

    def run(skip):
        ls = _handle(S, pr, skip, S.ASIMPLE, S.STATIONARY)
        try:
            first, st_first = _solve(S, ls, pr, 0.0, K1)
            ls.reset_stats()
            out = second(S, ls, pr)
            return first + out, (st_first, ls.stats())
        finally:
            ls.close()

    return _pair(run)


def test_a_second_solve_on_the_same_setup_is_the_same_bytes():
    """delta_p and the CG's starting guess live on from one application to the next: the second solve starts from the
    state the first one's last application leaves, so with the switch on that application runs in front of it."""
    def second(S, ls, pr):
        ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
        its, res, rc = ls.solve_resident(S.FGMRES, 0.0, 9)
        xu, xp = ls.download_solution()
        return [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])]

    (on, (f1, s1)), (off, (f0, s0)) = _two_calls(second)
    assert_same(on, off)
    assert (f0["prec_applies"], f1["prec_applies"]) == (8, 7)
    # second solve: 9 iterations = 10 applications in deal.II's order; with the switch on the first solve's left-over
    # application and 9 of its own
    assert (s0["prec_applies"], s1["prec_applies"]) == (10, 10)
    assert f1["columns_skipped"] > 0 and s1["columns_skipped"] > 0 and s0["columns_skipped"] == 0


def test_a_solve_followed_by_one_application_is_the_same_bytes():
    def second(S, ls, pr):
        du, dp, rc = ls.precond_vmult(rng_vec(pr.n_u, 21), rng_vec(pr.n_p, 22))
        return [du, dp, np.array([rc])]

    (on, (f1, s1)), (off, (f0, s0)) = _two_calls(second)
    assert_same(on, off)
    assert (s0["prec_applies"], s1["prec_applies"]) == (1, 2)   # the left-over application ran first
    assert s0["columns_skipped"] == 0 and f1["columns_skipped"] > 0


def test_a_new_setup_drops_the_left_over_application():
    """The Newton loop, the benchmark and every driver: set-up, solve, set-up, solve.  delta_p starts from zero again, so
    nothing of the first solve is replayed: the second solve runs K applications where deal.II's order runs K + 1."""
    def second(S, ls, pr):
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        ls.reset_stats()
        ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
        its, res, rc = ls.solve_resident(S.FGMRES, 0.0, 7)
        xu, xp = ls.download_solution()
        return [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])]

    (on, (f1, s1)), (off, (f0, s0)) = _two_calls(second)
    assert_same(on, off)
    assert (s0["prec_applies"], s1["prec_applies"]) == (8, 7)
    assert (f0["prec_applies"], f1["prec_applies"]) == (8, 7)
