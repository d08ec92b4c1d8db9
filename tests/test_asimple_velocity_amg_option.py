"""NSK_OPT_ASIMPLE_VELOCITY_AMG, the host side: the public surface, the rule that sends the level-0 residuals
of that hierarchy to F's 2 x 2 node blocks, and the evidence the option rests on — one V-cycle of the smoothed-aggregation
hierarchy of F is a preconditioner the inner FGMRES of stationary aSIMPLE can take in ILU(F)'s place.  No GPU: F is the
host producer's, the cycle the CPU restatement's (oracle.Amg), the solver a plain right-preconditioned FGMRES(30) from
zero on rhs_u to the 1e-1 aSIMPLE asks for.

Bound: at most 14 iterations — twice the 7 measured at 60x20 (Newton) when the option was proposed (6 / 6 / 6 for the
other three cases); natural-order ILU(0) took 4 / 5 / 6 / 10.  At these sizes the cycle buys nothing and nothing here
says it does: its count stays near 10 up to 480x160 where ILU(0)'s reaches 22 and 29."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSR_VECTOR, STREAM, STREAM_F32, BLK, BLK_F32 = range(5)


def test_header_and_python_declare_the_option():
    text = open(os.path.join(ROOT, "include", "nsk.h")).read()
    assert re.search(r"\bNSK_OPT_ASIMPLE_VELOCITY_AMG\s*=\s*22\b", text)
    assert S.OPT_ASIMPLE_VELOCITY_AMG == 22
    internal = open(os.path.join(ROOT, "navier_stokes_solver_amd", "csrc", "nsk_internal.h")).read()
    assert re.search(r"\bNSK_IOPT_AMG_FUSED_CHEBY\s*=\s*113\b", internal) and S.IOPT_AMG_FUSED_CHEBY == 113
    assert callable(S.LinearSolver.asimple_velocity_amg)
    L = S.lib()          # (no GPU call)
    for name in ("nsk_debug_amg_spmv_form2", "nsk_debug_amg_fused", "nsk_debug_cheby_fused"):
        getattr(L, name)


def test_the_rule_is_the_old_one_without_the_flag_and_blocked_exactly_under_its_conditions():
    L = S.lib()
    L.nsk_debug_amg_spmv_form.argtypes = [C.c_int] * 6
    L.nsk_debug_amg_spmv_form2.argtypes = [C.c_int] * 7
    n = 0
    for blk_ok, stream_ok, amg32, use_bsr, aligned16 in itertools.product((0, 1), repeat=5):
        for mode in (0, 1, 2):
            old = L.nsk_debug_amg_spmv_form(blk_ok, stream_ok, amg32, use_bsr, mode, aligned16)
            assert L.nsk_debug_amg_spmv_form2(blk_ok, stream_ok, amg32, use_bsr, mode, aligned16, 0) == old
            new = L.nsk_debug_amg_spmv_form2(blk_ok, stream_ok, amg32, use_bsr, mode, aligned16, 1)
            if not amg32 and mode == 2 and blk_ok and use_bsr and aligned16:
                assert new == BLK and old in (STREAM, CSR_VECTOR)
                n += 1
            else:
                assert new == old, (blk_ok, stream_ok, amg32, use_bsr, mode, aligned16)
    assert n == 2            # (with and without a stream plan)


def fgmres(A, b, M, rel_tol, restart=30, max_it=400):
    """Right-preconditioned FGMRES(restart) from zero; iterations until the Arnoldi residual is <= rel_tol |b|."""
    x = np.zeros_like(b)
    stop = rel_tol * np.linalg.norm(b)
    its = 0
    while its < max_it:
        r = b - A @ x
        beta = np.linalg.norm(r)
        if beta <= stop:
            return its
        V, Z = [r / beta], []
        H = np.zeros((restart + 1, restart))
        for j in range(restart):
            Z.append(M(V[j]))
            w = A @ Z[j]
            for i in range(j + 1):
                H[i, j] = float(w @ V[i])
                w = w - H[i, j] * V[i]
            H[j + 1, j] = np.linalg.norm(w)
            V.append(w / H[j + 1, j])
            its += 1
            e1 = np.zeros(j + 2)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)
            if np.linalg.norm(e1 - H[:j + 2, :j + 1] @ y) <= stop or its >= max_it:
                break
        x = x + sum(yk * zk for yk, zk in zip(y, Z))
        if np.linalg.norm(b - A @ x) <= 1.0000001 * stop:
            return its
    return its


CASES = [("newton", dict(mode=1, state=1)), ("stokes", dict(mode=0, state=0, inlet_bc=1))]


@pytest.mark.parametrize("phase,kw", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("nx,ny", [(16, 10), (60, 20)])
def test_the_v_cycle_on_f_is_a_preconditioner_the_inner_fgmres_can_take(nx, ny, phase, kw):
    from oracle import oracle as O
    pr = P.generate(nx, ny, nu=0.01, **kw)
    F = pr.F.to_scipy().tocsr()
    F.sort_indices()
    holder = O.CsrHolder.from_scipy(F)
    amg, ilu = O.Amg(holder), O.Tri(holder, 0)
    lv = amg.levels()
    assert len(lv) >= 2 and lv[0][:2] == (pr.n_u, F.nnz)
    its = fgmres(F, pr.rhs_u, amg.apply, 1e-1)
    its_ilu = fgmres(F, pr.rhs_u, ilu.apply, 1e-1)
    print(f"{nx}x{ny} {phase}: n_u {pr.n_u}, levels {[(r, z) for r, z, _ in lv]}; FGMRES(30) to 1e-1: {its} iterations with the "
          f"V-cycle, {its_ilu} with natural-order ILU(0)")
    assert 0 < its <= 14
