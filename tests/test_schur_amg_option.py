"""NSK_OPT_SCHUR_AMG, the host side: the public surface, and the evidence the option rests on — one V-cycle of
the smoothed-aggregation hierarchy of aSIMPLE's S = B~ diag(F)^-1 B~^T is a preconditioner the inner CG can take
(symmetric, of S's sign) and a much better one than ILU(0).  No GPU: S is formed with SciPy from the host producer's
blocks, the cycle is the CPU restatement's (oracle.Amg), the CG a plain PCG from a zero start on aSIMPLE's right-hand side
rhs_p - B F^-1 rhs_u.

Bounds: symmetry to 1e-12 relative (the cycle is R = P^T, Galerkin, the same Chebyshev polynomial before and after:
symmetric in exact arithmetic; measured 1e-14), and at most 12 PCG iterations to 1e-1 — twice the 6 and 6 measured at
16x10 and 60x20 when the option was proposed, against 15 and 33 with multicolour ILU(0)."""
import os
import re

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import solver as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_option_and_both_entry_points():
    text = open(os.path.join(ROOT, "include", "nsk.h")).read()
    assert re.search(r"\bNSK_OPT_SCHUR_AMG\s*=\s*21\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("nsk_schur_amg_info", "nsk_schur_amg_apply"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*nsk_handle\b", code), name
        assert name in S.EXPORTS
    assert S.OPT_SCHUR_AMG == 21
    assert callable(S.LinearSolver.schur_amg_info) and callable(S.LinearSolver.schur_amg_apply)
    L = S.lib()          # (no GPU call)
    for name in ("nsk_schur_amg_info", "nsk_schur_amg_apply"):
        getattr(L, name)


def schur_of(pr):
    """S as the set-up forms it, and aSIMPLE's right-hand side for the CG on it."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    F, B, Bt = pr.F.to_scipy().tocsr(), pr.B.to_scipy().tocsr(), pr.Bt.to_scipy().tocsr()
    Sm = (B @ sp.diags(1.0 / F.diagonal()) @ Bt).tocsr()
    Sm.sort_indices()
    rhs = pr.rhs_p - B @ spla.splu(F.tocsc()).solve(pr.rhs_u)
    return Sm, rhs


def pcg(A, b, M, rel_tol, max_it=200):
    """Preconditioned CG from zero; iterations until |r| <= rel_tol |b| (the 2-norm SolverCG checks)."""
    x, r = np.zeros_like(b), b.copy()
    z = M(r)
    p, rz = z.copy(), float(r @ z)
    stop = rel_tol * np.linalg.norm(b)
    for it in range(1, max_it + 1):
        Ap = A @ p
        a = rz / float(p @ Ap)
        x += a * p
        r -= a * Ap
        if np.linalg.norm(r) <= stop:
            return it
        z = M(r)
        rz, old = float(r @ z), rz
        p = z + (rz / old) * p
    return max_it + 1


CASES = [("newton", dict(mode=1, state=1)), ("stokes", dict(mode=0, state=0, inlet_bc=1))]


@pytest.mark.parametrize("phase,kw", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("nx,ny", [(16, 10), (60, 20)])
def test_the_v_cycle_on_s_is_a_preconditioner_cg_can_take(nx, ny, phase, kw):
    from oracle import oracle as O
    pr = P.generate(nx, ny, nu=0.01, **kw)
    Sm, rhs = schur_of(pr)
    d = Sm.diagonal()
    sign = 1.0 if d[0] > 0 else -1.0
    assert np.all(sign * d > 0)                                        # one sign, no zero
    assert abs(Sm - Sm.T).max() <= 1e-14 * abs(Sm).max()
    amg = O.Amg(O.CsrHolder.from_scipy(Sm))
    lv = amg.levels()
    assert len(lv) >= 2 and lv[0][:2] == (pr.n_p, Sm.nnz)
    rng = np.random.default_rng(21)
    x, y = rng.standard_normal(pr.n_p), rng.standard_normal(pr.n_p)
    Mx, My = amg.apply(x), amg.apply(y)
    a, b = float(Mx @ y), float(x @ My)
    print(f"{nx}x{ny} {phase}: n_p {pr.n_p}, levels {[(r, z) for r, z, _ in lv]}, lambda {[round(l, 4) for _, _, l in lv]}, "
          f"symmetry {abs(a - b) / abs(a):.1e}, sign {sign:+.0f}")
    assert abs(a - b) <= 1e-12 * abs(a)
    assert sign * float(x @ Mx) > 0 and sign * float(y @ My) > 0        # the cycle has the sign of S
    its = pcg(Sm, rhs, amg.apply, 1e-1)
    print(f"{nx}x{ny} {phase}: PCG with the V-cycle reaches 1e-1 in {its} iterations, 1e-2 in {pcg(Sm, rhs, amg.apply, 1e-2)}")
    assert its <= 12
