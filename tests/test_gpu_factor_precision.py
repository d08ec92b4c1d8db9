"""NSK_OPT_FACTOR_PRECISION = 32: the off-diagonal values of the split ILU(0) / SGS halves stored in fp32 (include/nsk.h).

The reference for an fp32 apply is the oracle's factor under the library's permutation with exactly the entries the GPU
stores in fp32 rounded to fp32 (every off-diagonal entry of a scalar factor; every entry outside a node's own 2x2 block
of the blocked velocity factor — node m is permuted rows 2m, 2m+1), solved on the host in fp64.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests.util import problem, rel_err, rng_vec

pytestmark = pytest.mark.gpu


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


def _O():
    from oracle import oracle as O
    return O


def _solve_factor(rp, col, val, kind, perm, b, round_f32, block2):
    """x = M^-1 b for the oracle's exported factor (permuted numbering, perm[new] = old), optionally with the entries the GPU
    keeps in fp32 rounded to fp32."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = val.copy()
    if round_f32:
        off = (rows // 2 != col // 2) if block2 else (rows != col)
        v[off] = v[off].astype(np.float32).astype(np.float64)
    A = sp.csr_matrix((v, col, rp), shape=(n, n))
    Lo, Up, d = sp.tril(A, -1, format="csr"), sp.triu(A, 1, format="csr"), A.diagonal()
    I = sp.identity(n, format="csr")
    bp = b[perm]
    if kind == 0:   # unit lower L, U with the diagonal
        y = spl.spsolve_triangular(Lo + I, bp, lower=True)
        xp = spl.spsolve_triangular((Up + sp.diags(d)).tocsr(), y, lower=False)
    else:           # one symmetric Gauss-Seidel sweep from zero: (D + L) y = b ; (D + U) x = D y
        y = spl.spsolve_triangular((Lo + sp.diags(d)).tocsr(), bp, lower=True)
        xp = spl.spsolve_triangular((Up + sp.diags(d)).tocsr(), d * y, lower=False)
    x = np.empty(n)
    x[perm] = xp
    return x


def _schur(ls, pr):
    S = _S()
    rp, col, val = ls.get_block(S.BLK_S)
    return sp.csr_matrix((val, col, rp), shape=(pr.n_p, pr.n_p))


def _check_f32(ls, which, A, kind, seed, label):
    """fp32 apply of one factor against the exactly-rounded host reference"""
    S, O = _S(), _O()
    perm = ls.tri_perm(which)
    H = O.CsrHolder.from_scipy(A) if sp.issparse(A) else O.CsrHolder.from_block(A)
    rp, col, val = O.Tri(H, kind=kind, perm=perm).export()
    b = rng_vec(len(perm), seed)
    block2 = which == S.TRI_VELOCITY
    ref32 = _solve_factor(rp, col, val, kind, perm, b, True, block2)
    ref64 = _solve_factor(rp, col, val, kind, perm, b, False, block2)
    x = ls.tri_apply(which, b)
    assert ls.tri_value_bytes(which) == 4, label
    e, gap = rel_err(x, ref32), rel_err(ref64, ref32)
    print(f"FP32 {label}: |gpu - ref32| {e:.2e}, |ref64 - ref32| {gap:.2e}")
    assert e <= 0.01 * gap and e <= 1e-9, (label, e, gap)
    return x


@pytest.mark.parametrize("name", ["ns16", "ns60"])
@pytest.mark.parametrize("groups", [0, 1])
@pytest.mark.parametrize("sync_free", [0, 2])
def test_fp32_applies_match_the_rounded_factor(name, groups, sync_free):
    """ILU(0) of F and S (aSIMPLE), of F and Mp (unsteady blockDiagonal, multicolour Mp), SGS of F and Mp (stationary
    blockDiagonal): single-launch and per-colour kernels, with and without line groups."""
    S = _S()
    pr = problem(name)
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_option(S.OPT_TRI_LINE_GROUPS, groups)
        ls.set_option(S.OPT_TRI_SYNC_FREE, sync_free)
        ls.set_option(S.OPT_MASS_ORDERING, 1)
        ls.set_option(S.IOPT_TINY_BYTES, 0)
        ls.set_option(S.OPT_FACTOR_PRECISION, 32)
        ls.set_problem(pr)
        tag = f"{name} groups {groups} sync_free {sync_free}"
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        _check_f32(ls, S.TRI_VELOCITY, pr.F, 0, 1, "ILU(F) " + tag)
        _check_f32(ls, S.TRI_PRESSURE, _schur(ls, pr), 0, 2, "ILU(S) " + tag)
        ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.UNSTEADY)
        _check_f32(ls, S.TRI_PRESSURE, pr.Mp, 0, 3, "ILU(Mp) " + tag)
        ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.STATIONARY)
        _check_f32(ls, S.TRI_VELOCITY, pr.F, 1, 4, "SGS(F) " + tag)
        _check_f32(ls, S.TRI_PRESSURE, pr.Mp, 1, 5, "SGS(Mp) " + tag)
        assert ls.stats()["sync_free_fallbacks"] == 0
    finally:
        ls.close()


def test_default_and_switch_back_are_bit_identical():
    """Unset and 64 give the same bits; 64 -> 32 -> 64 on one handle ends where it started, and the middle apply is the
    rounded factor's."""
    S = _S()
    pr = problem("ns60")
    hs = []
    try:
        for opt in (None, 64):
            ls = S.LinearSolver()
            hs.append(ls)
            ls.set_option(S.OPT_TRI_ORDERING, 1)
            ls.set_option(S.IOPT_TINY_BYTES, 0)
            if opt is not None:
                ls.set_option(S.OPT_FACTOR_PRECISION, opt)
            ls.set_problem(pr)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        bu, bp = rng_vec(pr.n_u, 41), rng_vec(pr.n_p, 42)
        a, b = hs
        for which, v in ((S.TRI_VELOCITY, bu), (S.TRI_PRESSURE, bp)):
            assert a.tri_value_bytes(which) == 8 and b.tri_value_bytes(which) == 8
            assert np.array_equal(a.tri_apply(which, v), b.tri_apply(which, v))
        first = {w: b.tri_apply(w, v) for w, v in ((S.TRI_VELOCITY, bu), (S.TRI_PRESSURE, bp))}
        b.set_option(S.OPT_FACTOR_PRECISION, 32)
        b.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        _check_f32(b, S.TRI_VELOCITY, pr.F, 0, 41, "ILU(F) switched to 32")
        _check_f32(b, S.TRI_PRESSURE, _schur(b, pr), 0, 42, "ILU(S) switched to 32")
        b.set_option(S.OPT_FACTOR_PRECISION, 64)
        b.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        for which, v in ((S.TRI_VELOCITY, bu), (S.TRI_PRESSURE, bp)):
            assert b.tri_value_bytes(which) == 8
            assert np.array_equal(b.tri_apply(which, v), first[which])
        with pytest.raises(RuntimeError):
            b.set_option(S.OPT_FACTOR_PRECISION, 16)
    finally:
        for ls in hs:
            ls.close()


def test_factors_off_the_split_kernels_stay_fp64():
    """With 32 set: the natural-order (LDS ring) mass factor, tiny factors and the AMG slot report 8 / 8 / 0 and still
    apply as the fp64 oracle does."""
    S, O = _S(), _O()
    pr = problem("ns60")
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_option(S.IOPT_TINY_BYTES, 0)
        ls.set_option(S.OPT_FACTOR_PRECISION, 32)
        ls.set_problem(pr)
        # unsteady blockDiagonal: Mp in the caller's order (ring), F multicolour (fp32)
        ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.UNSTEADY)
        assert np.array_equal(ls.tri_perm(S.TRI_PRESSURE), np.arange(pr.n_p))
        assert ls.tri_value_bytes(S.TRI_PRESSURE) == 8 and ls.tri_value_bytes(S.TRI_VELOCITY) == 4
        before = ls.stats()["ring_applies"]
        b = rng_vec(pr.n_p, 51)
        assert rel_err(ls.tri_apply(S.TRI_PRESSURE, b), O.Tri(O.CsrHolder.from_block(pr.Mp), kind=0).apply(b)) <= 1e-11
        assert ls.stats()["ring_applies"] == before + 1
        # stationary blockTriangular: the velocity slot is the AMG V-cycle, bit-equal to an fp64 handle's
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.tri_value_bytes(S.TRI_VELOCITY) == 0 and ls.tri_value_bytes(S.TRI_PRESSURE) == 4
        ref = S.LinearSolver()
        try:
            ref.set_option(S.OPT_TRI_ORDERING, 1)
            ref.set_option(S.IOPT_TINY_BYTES, 0)
            ref.set_problem(pr)
            ref.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
            bu = rng_vec(pr.n_u, 52)
            assert np.array_equal(ls.tri_apply(S.TRI_VELOCITY, bu), ref.tri_apply(S.TRI_VELOCITY, bu))
        finally:
            ref.close()
    finally:
        ls.close()
    # tiny factors (default threshold): the single-workgroup walker on the fp64 factor
    pr = problem("ns16")
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_option(S.OPT_FACTOR_PRECISION, 32)
        ls.set_problem(pr)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        for which, A in ((S.TRI_VELOCITY, pr.F), (S.TRI_PRESSURE, None)):
            assert ls.tri_value_bytes(which) == 8
            H = O.CsrHolder.from_block(A) if A is not None else O.CsrHolder.from_scipy(_schur(ls, pr))
            tri = O.Tri(H, kind=0, perm=ls.tri_perm(which))
            b = rng_vec(H.n_rows, 53 + which)
            assert rel_err(ls.tri_apply(which, b), tri.apply(b)) <= 1e-11
    finally:
        ls.close()


@pytest.mark.parametrize("name,prec,variant", [("ns16", 0, 0), ("ns16", 2, 0), ("unsteady16", 0, 1), ("unsteady16", 2, 1)])
def test_fgmres_with_fp32_factors_converges_to_the_same_solution(name, prec, variant):
    """The outer FGMRES stays fp64 and checks the true residual: same solution, about the same iteration count."""
    S = _S()
    pr = problem(name)
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    xs = spl.splu(J).solve(b)
    tol = 1e-12
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_option(S.IOPT_TINY_BYTES, 0)
        ls.set_problem(pr)
        its = {}
        for bits in (64, 32):
            ls.set_option(S.OPT_FACTOR_PRECISION, bits)
            ls.setup_preconditioner(prec, variant, 0.5)
            assert ls.tri_value_bytes(S.TRI_VELOCITY) == bits // 8
            xu, xp, it, res, rc = ls.solve(1, tol, 20000 if variant == 0 else 100000, pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
            x = np.concatenate([xu, xp])
            assert rc == 0, (bits, rc)
            assert np.linalg.norm(b - J @ x) <= 1.05 * tol, bits
            assert rel_err(x, xs) <= 2e-8, bits
            its[bits] = it
        print(f"ITERATIONS {name} prec {prec} variant {variant}: fp64 {its[64]}, fp32 {its[32]}")
        assert abs(its[32] - its[64]) <= max(3, 0.1 * its[64]), its
    finally:
        ls.close()


def _newton_run(env_extra):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navier_stokes_solver_amd", "bin",
                       "StationaryNSSolver")
    env = dict(os.environ)
    env.pop("NSK_FACTOR_PRECISION", None)
    env.update(env_extra)
    out = subprocess.run([exe, "-m", "60,20", "-r", "10", "-p", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = [float(v) for v in re.findall(r"Newton iteration \d+/\d+ - \|\|r\|\| = ([-+.0-9eE]+)", out.stdout)]
    return out.stdout, res


def test_driver_with_fp32_factors():
    """NSK_FACTOR_PRECISION=32 StationaryNSSolver -m 60,20 -r 10 -p 2: the [nsk] line, the same Newton steps, the same end
    (final Newton residual within 1e-8 of the run's first one).  One continuation level (Re 10, the whole inlet ramp): -r 50
    takes 47 s per run, more than the GPU suite can spare."""
    # the Q3 velocity factor at 60x20 is far above the 4 MB single-workgroup threshold (12 bytes per entry)
    assert problem("ns60").F.nnz * 12 > 4e6
    out64, r64 = _newton_run({})
    out32, r32 = _newton_run({"NSK_FACTOR_PRECISION": "32"})
    line = "[nsk] NSK_FACTOR_PRECISION=32: ILU/SGS factors stored in fp32 (deviation from the reference)"
    assert line in out32 and line not in out64
    print(f"NEWTON fp64 {len(r64)} steps, last ||r|| {r64[-1]:.6e}; fp32 {len(r32)} steps, last ||r|| {r32[-1]:.6e}")
    assert len(r32) == len(r64)
    assert abs(r32[-1] - r64[-1]) <= 1e-8 * max(r64), (r64[-1], r32[-1])
