"""NSK_OPT_ASIMPLE_VELOCITY_AMG (include/nsk.h): in the stationary aSIMPLE set-up one V-cycle of the velocity
hierarchy preconditions the inner FGMRES on F, in place of ILU(F); with one sub-domain level 0 is F itself, its residual
products run on F's 2 x 2 node blocks and the Chebyshev steps behind them in those products' epilogues.

1. The public surface: option values, what nsk_amg_info and the velocity slot of the triangular getters report after
   each kind of set-up.
2. 0 is the code path and the bits of a handle that never touched the option, whatever the internal fused switch says.
3. The cycle alone against the CPU restatement (oracle.Amg on F): level rows, non-zeros, lambda to 1e-12, one cycle to
   1e-11 relative — the bound tests/test_gpu_parity.py::test_amg_vcycle_matches_oracle holds under blockTriangular — and
   the forms it launched: with one sub-domain the four level-0 products of a cycle in the blocked double form, three of
   them fused steps; with three sub-domains (level 0 a copy without node blocks) none.  The fused switch at 0: same bits.
4. The fused kernel alone (nsk_debug_cheby_fused) on every 2 x 2 pattern of tests/spmv_reference.py and on F of a 1x1, a
   2x1 and a 3x2 mesh: w and x_out bit for bit those of spmv_blk22_residual followed by vec_cheby_step on the same device
   data, in double and on the fp32 copy, with c1 != 0 and with c1 = 0 over a w full of NaN; the residual of the two-launch
   path within the counted bound of the blocked residual form (tests/test_gpu_amg_precision.py: gamma(roundings("blk_c2"))
   |A||x| + u |s| + 2 u |z - s|); no guard word written; an in-place call refused.
5. fp32 operators (NSK_OPT_AMG_PRECISION = 32 governs this use of the hierarchy too) against the double cycle, within the
   first-order bound derived in the docstring of tests/test_gpu_schur_amg.py, item 4, with F in S's place and nothing
   re-fitted:   max |x32 - x64| <= 3.23 N g 2^-24 max |x64|,   N = 6 products with rounded operators per level that has
   a coarser one, 3.23 / lambda the largest Chebyshev coefficient, g = max(1, ||D^-1 |F|||_inf / lambda).
6. Whole solves to 1e-10 against the sparse-direct solution, option off, on, and on together with NSK_OPT_SCHUR_AMG.
7. Inner work is bounded, not "better": at 60x20 the cycle needs at most 14 inner iterations per F-solve over the first 8
   outer iterations — twice the 7 the CPU restatement measured (tests/test_asimple_velocity_amg_option.py; the oracle's
   aSIMPLE has no velocity AMG to count with).  NO SPEED-UP IS EXPECTED AT THIS SIZE: ILU(0) needs about as few.
8. One Newton iteration of the driver with NSK_ASIMPLE_VELOCITY_AMG=1 in a child's environment.
9. The fallback: an F whose product A P has a row of 801 distinct columns (two weakly coupled hub rows; the set-up's
   hash-set kernels count at most 512 and say so in their error word: -81, no fault) keeps ILU(F), one warning per handle.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from navier_stokes_solver_amd import problem as P
from tests import spmv_reference as M
from tests.util import problem, rel_err, rng_vec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = M.U
U32 = 2.0 ** -24
CSR_VECTOR, STREAM, STREAM_F32, BLK, BLK_F32 = range(5)


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


def _O():
    from oracle import oracle as O
    return O


def _handle(pr, on=None, subdomains=1, amg_bits=None, schur=None, fused=None):
    S = _S()
    ls = S.LinearSolver()
    if on is not None:
        ls.set_option(S.OPT_ASIMPLE_VELOCITY_AMG, on)
    if subdomains > 1:
        ls.set_option(S.OPT_SUBDOMAINS, subdomains)
    if amg_bits is not None:
        ls.set_option(S.OPT_AMG_PRECISION, amg_bits)
    if schur is not None:
        ls.set_option(S.OPT_SCHUR_AMG, schur)
    if fused is not None:
        ls.set_option(S.IOPT_AMG_FUSED_CHEBY, fused)
    ls.set_problem(pr)
    return ls


def _forms(ls):
    out, fused = np.zeros(5, np.int64), np.zeros(1, np.int64)
    ls.L.nsk_debug_amg_forms.argtypes = [C.c_void_p, C.c_void_p]
    ls.L.nsk_debug_amg_fused.argtypes = [C.c_void_p, C.c_void_p]
    assert ls.L.nsk_debug_amg_forms(ls.h, out.ctypes.data) == 0
    assert ls.L.nsk_debug_amg_fused(ls.h, fused.ctypes.data) == 0
    return out.tolist(), int(fused[0])


def _u_offsets(n_u, subdomains):
    if subdomains <= 1:
        return None
    return np.array([(n_u * k // subdomains) & ~1 for k in range(subdomains)] + [n_u], np.int32)


# ------------------------------------------------------------------------------------------------ 1. the surface
def test_option_values_and_what_the_getters_report():
    S = _S()
    pr = problem("ns16")
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_ASIMPLE_VELOCITY_AMG, 1)
        with pytest.raises(RuntimeError, match="nsk error -61"):
            ls.set_option(S.OPT_ASIMPLE_VELOCITY_AMG, 2)
        with pytest.raises(RuntimeError, match="nsk error -61"):
            ls.set_option(S.IOPT_AMG_FUSED_CHEBY, 2)
        ls.set_option(S.OPT_VELOCITY_AMG, 0)            # (blockTriangular's own switch: it keeps meaning that set-up only)
        ls.set_problem(pr)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        lv = ls.amg_levels()
        assert len(lv) >= 2 and lv[0][:2] == (pr.n_u, ls.L.nsk_block_nnz(ls.h, S.BLK_F)) and lv[0][2] > 0
        assert ls.asimple_velocity_amg() and ls.amg_value_bytes() == 8
        # the velocity slot holds no triangular factor: as under blockTriangular's velocity AMG
        assert ls.tri_value_bytes(S.TRI_VELOCITY) == 0 and ls.tri_value_bytes(S.TRI_PRESSURE) == 8
        assert np.array_equal(ls.tri_perm(S.TRI_VELOCITY), np.arange(pr.n_u))
        assert ls.schur_amg_info() == []
        for prec, variant in ((S.BLOCK_DIAGONAL, S.STATIONARY), (S.BLOCK_TRIANGULAR, S.STATIONARY), (S.ASIMPLE, S.UNSTEADY)):
            ls.setup_preconditioner(prec, variant, 0.5)
            assert ls.amg_levels() == [] and not ls.asimple_velocity_amg(), (prec, variant)
            assert ls.tri_value_bytes(S.TRI_VELOCITY) == 8, (prec, variant)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert [a[:2] for a in ls.amg_levels()] == [a[:2] for a in lv]
        ls.set_option(S.OPT_ASIMPLE_VELOCITY_AMG, 0)    # takes effect at the next set-up
        assert ls.amg_levels() != []
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.amg_levels() == [] and ls.tri_value_bytes(S.TRI_VELOCITY) == 8 and not ls.asimple_velocity_amg()
    finally:
        ls.close()


# ------------------------------------------------------------------------------------------------ 2. default bits
def _solve(ls, pr, tol=0.0, steps=8):
    S = _S()
    ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
    ls.reset_stats()
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    its, res, rc = ls.solve_resident(S.FGMRES, tol, steps)
    xu, xp = ls.download_solution()
    st = ls.stats()
    return dict(its=its, rc=rc, x=np.concatenate([xu, xp]), hist=ls.history(), inner_u=st["inner_u_its"],
                inner_p=st["inner_p_its"], applies=st["prec_applies"])


def test_option_at_0_has_the_bits_of_a_handle_that_never_touched_it():
    S = _S()
    pr = problem("ns16")
    hs = [_handle(pr), _handle(pr, 0), _handle(pr, 0, fused=0), _handle(pr, 0, fused=1)]
    try:
        hs[1].set_option(S.OPT_ASIMPLE_VELOCITY_AMG, 1)
        hs[1].set_option(S.OPT_ASIMPLE_VELOCITY_AMG, 0)
        runs = [_solve(ls, pr, 0.0, 40) for ls in hs]          # (40 outer iterations: past one restart of FGMRES(30))
        assert runs[0]["its"] == 40 and len(runs[0]["hist"]) > 40
        for ls, r in zip(hs[1:], runs[1:]):
            assert ls.amg_levels() == [] and ls.tri_value_bytes(S.TRI_VELOCITY) == 8
            assert np.array_equal(runs[0]["hist"], r["hist"]) and np.array_equal(runs[0]["x"], r["x"])
            assert (runs[0]["inner_u"], runs[0]["inner_p"]) == (r["inner_u"], r["inner_p"])
    finally:
        [ls.close() for ls in hs]


# ------------------------------------------------------------------------------------------------ 3. the cycle alone
@functools.lru_cache(maxsize=8)
def _oracle_cycle(name, subdomains):
    """Levels per shard and one cycle on the seeded b, computed once per case."""
    O = _O()
    pr = problem(name)
    ref = O.Amg(O.CsrHolder.from_block(pr.F), _u_offsets(pr.n_u, subdomains))
    b = rng_vec(pr.n_u, 77)
    return [ref.levels(s) for s in range(subdomains)], b, ref.apply(b)


@pytest.mark.parametrize("name,subdomains", [("ns16", 1), ("ns16", 3), ("ns60", 1), ("ns60", 3)])
def test_the_cycle_on_f_matches_the_cpu_restatement_and_runs_on_the_node_blocks(name, subdomains):
    S = _S()
    pr = problem(name)
    levels, b, xo = _oracle_cycle(name, subdomains)
    out = {}
    for fused in (None, 0):
        ls = _handle(pr, 1, subdomains, fused=fused)
        try:
            ls.set_option(S.IOPT_TINY_BYTES, 0)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            n_prod = 0
            for shard in range(subdomains):
                lv, ov = ls.amg_levels(shard), levels[shard]
                if fused is None:
                    print(f"{name} x{subdomains} shard {shard}: levels {[(r, z, round(lam, 6)) for r, z, lam in lv]}")
                assert len(lv) == len(ov) >= 2
                for (r, z, lam), (orows, onnz, olam) in zip(lv, ov):
                    assert (r, z) == (orows, onnz) and abs(lam - olam) <= 1e-12 * olam
                n_prod += 6 * (len(lv) - 1)            # per cycle; the last level is solved by its dense inverse
            assert ls.amg_levels(subdomains) == []
            assert _forms(ls) == ([0] * 5, 0)
            x = ls.tri_apply(S.TRI_VELOCITY, b)
            assert np.array_equal(ls.tri_apply(S.TRI_VELOCITY, b), x)          # two applies, the same bits
            out[fused] = x
            forms, n_fused = _forms(ls)
            if subdomains == 1:
                # level 0 is F itself: its four products per cycle on the 2 x 2 node blocks in double, three of them fused
                assert forms == [0, 2 * (n_prod - 4), 0, 2 * 4, 0], forms
                assert n_fused == (2 * 3 if fused is None else 0)
            else:
                assert forms == [0, 2 * n_prod, 0, 0, 0] and n_fused == 0, (forms, n_fused)
        finally:
            ls.close()
    err = rel_err(out[None], xo)
    print(f"{name} x{subdomains}: one cycle against the CPU restatement {err:.2e}")
    assert err <= 1e-11
    assert np.array_equal(out[None], out[0])             # fused steps or two launches: the same bits
    if subdomains == 1:
        assert np.linalg.norm(b - pr.F.to_scipy() @ out[None]) < 0.8 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------------------ 4. the fused kernel alone
class Mat(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_own_cols", C.c_int32), ("pad_", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("x_own", C.c_void_p),
                ("x_ghost", C.c_void_p)]


class Hook:
    """nsk_debug_cheby_fused (nsk_internal.h): one fused step and the two launches it replaces, between guard words."""

    def __init__(self):
        S = _S()
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_cheby_fused.argtypes = ([C.c_void_p] * 5 + [C.c_double, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 6)

    def run(self, A, x, b, dinv, w, c1, c2, fp32=0, in_place=0):
        xo, xg = (np.ascontiguousarray(v, dtype=np.float64) for v in x)
        ma = Mat(A.n_rows, A.n_cols, A.n_own, 0, A.rowptr.ctypes.data, A.col.ctypes.data, A.val.ctypes.data,
                 xo.ctypes.data, xg.ctypes.data)
        vec = [np.ascontiguousarray(v, dtype=np.float64) for v in (b, dinv, w)]
        outs = [np.full(A.n_rows, 7.0) for _ in range(5)]
        info = np.zeros(4, dtype=np.int32)
        rc = self.L.nsk_debug_cheby_fused(self.ls.h, C.byref(ma), *[v.ctypes.data for v in vec], c1, c2, fp32, in_place,
                                          *[o.ctypes.data for o in outs], info.ctypes.data)
        return rc, dict(zip(("w", "x", "r_ref", "w_ref", "x_ref"), outs)), info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()


@functools.lru_cache(maxsize=1)
def fused_patterns():
    """Every 2 x 2 pattern of tests/spmv_reference.py (rows at and above the run cap, empty block rows, ghost columns, a
    broken node structure) and F of three tiny meshes."""
    pats = {name: A for name, (Rr, Cc, A) in M.block_patterns().items() if (Rr, Cc) == (2, 2)}
    for nx, ny in ((1, 1), (2, 1), (3, 2)):
        F = P.generate(nx, ny, nu=1.0 / 90.0, mode=1, state=1, inlet_bc=0).F
        pats[f"F_{nx}x{ny}"] = M.Csr(F.rows, F.cols, F.rowptr, F.col, F.val, F.cols, f"F_{nx}x{ny}")
    return pats


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", sorted(fused_patterns()))
def test_fused_step_has_the_bits_of_the_two_launches(hook, name):
    A0 = fused_patterns()[name]
    p = M.blocked_plan(A0, 2, 2)
    A = A0 if name.startswith("F_") else M.real_values(A0, 7)
    x = M.real_x(A, 8)
    rng = np.random.default_rng(A.n_rows + 1)
    b, dinv, w = rng.uniform(-1, 1, A.n_rows), rng.uniform(0.5, 1.5, A.n_rows), rng.uniform(-1, 1, A.n_rows)
    if not p["ok"]:              # broken node structure, a block row above the run cap: reported, never forced
        rc, _, info = hook.run(A, x, b, dinv, w, 0.37, 1.21)
        assert rc == 1 and info[2] == 2
        return
    s, a = M.exact_row_sums(A, *x)
    Lb = np.repeat(np.diff(p["brp"]), 2)
    tol = M.gamma(M.roundings("blk_c2", Lb)) * a + U * np.abs(s) + 2 * U * np.abs(b - s)
    for fp32 in (0, 1):
        for c1, c2, wv in ((0.37, 1.21, w), (0.0, 0.83, np.full(A.n_rows, np.nan))):
            rc, o, info = hook.run(A, x, b, dinv, wv, c1, c2, fp32=fp32)
            assert rc == 0, (rc, hook.ls.last_error())
            assert info[0] == 0, f"{name}: {info[0]} guard words were written"
            assert info[1] == len(p["rb"]) - 1
            what = f"{name} fp32 {fp32} c1 {c1}"
            assert np.all(np.isfinite(o["w"])) and np.all(np.isfinite(o["x"])), what      # (c1 = 0: the NaN in w is not read)
            assert np.array_equal(_bits(o["w"]), _bits(o["w_ref"])), what
            assert np.array_equal(_bits(o["x"]), _bits(o["x_ref"])), what
            if not fp32:
                err = np.abs(o["r_ref"] - (b - s))
                assert np.all(err <= tol), (what, float(np.max(err / np.maximum(tol, 1e-300))))
            # and it is the update: w = c1 w + c2 dinv r, x_out = x_in + w (two roundings apart from the kernel's contraction)
            wn = (c1 * wv if c1 else 0.0) + c2 * dinv * o["r_ref"]
            assert np.all(np.abs(o["w"] - wn) <= 4 * U * (np.abs(wn) + np.abs(c2 * dinv * o["r_ref"]))), what
            assert np.array_equal(o["x"], x[0][:A.n_rows] + o["w"]), what
    # in place: refused by the launcher, nothing launched
    rc, o, info = hook.run(A, x, b, dinv, w, 0.37, 1.21, in_place=1)
    assert rc == -61 and "x_out must not be x_in" in hook.ls.last_error()
    assert all(np.all(v == 7.0) for v in o.values()) and info[1] == 0


# ------------------------------------------------------------------------------------------------ 5. fp32 operators
@pytest.mark.parametrize("name", ["ns16", "ns60"])
def test_the_fp32_cycle_stays_within_the_first_order_bound_of_the_double_one(name):
    S = _S()
    pr = problem(name)
    b = rng_vec(pr.n_u, 79)
    out = {}
    for bits in (64, 32):
        ls = _handle(pr, 1, amg_bits=bits)
        try:
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            assert ls.amg_value_bytes() == bits // 8
            x = ls.tri_apply(S.TRI_VELOCITY, b)
            assert np.array_equal(ls.tri_apply(S.TRI_VELOCITY, b), x)
            out[bits] = dict(x=x, lv=ls.amg_levels(), forms=_forms(ls))
        finally:
            ls.close()
    a, c = out[64], out[32]
    assert a["lv"] == c["lv"]                                             # the set-up is the double one
    n_prod = 6 * (len(a["lv"]) - 1)
    assert a["forms"] == ([0, 2 * (n_prod - 4), 0, 8, 0], 6), a["forms"]
    # every product of the fp32 cycle reads fp32 values, level 0's on the node blocks, three of four fused
    assert c["forms"] == ([0, 0, 2 * (n_prod - 4), 0, 8], 6), c["forms"]
    F = pr.F.to_scipy().tocsr()
    g = max(1.0, float((abs(F).sum(axis=1).A1 / np.abs(F.diagonal())).max()) / a["lv"][0][2])
    bound = 3.23 * n_prod * g * U32
    dev = rel_err(c["x"], a["x"])
    print(f"{name}: fp32 cycle against the double cycle {dev:.2e}, bound {bound:.2e} (N {n_prod}, g {g:.2f})")
    assert 0 < dev <= bound


# ------------------------------------------------------------------------------------------------ 6, 7. whole solves
@functools.lru_cache(maxsize=2)
def _direct(name):
    pr = problem(name)
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    return J, b, spl.splu(J).solve(b)


@pytest.mark.parametrize("on,schur", [(0, 0), (1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("name", ["ns16", "stokes16"])
def test_whole_solves_reach_the_sparse_direct_solution_with_the_option_on_and_off(name, on, schur):
    pr = problem(name)
    J, b, xs = _direct(name)
    ls = _handle(pr, on, schur=schur)
    try:
        r = _solve(ls, pr, 1e-10, 20000)
        assert bool(ls.amg_levels()) == bool(on) and bool(ls.schur_amg_info()) == bool(schur)
    finally:
        ls.close()
    print(f"{name} velocity AMG {on} Schur AMG {schur}: outer {r['its']}, inner on F {r['inner_u']} in {r['applies']} "
          f"F-solves, inner on S {r['inner_p']}, |x - x_direct| {rel_err(r['x'], xs):.2e}, "
          f"true residual {np.linalg.norm(b - J @ r['x']):.2e}")
    assert r["rc"] == 0 and np.linalg.norm(b - J @ r["x"]) <= 1.05e-10
    assert rel_err(r["x"], xs) <= 1e-8


def test_inner_iterations_on_f_at_60x20_are_bounded():
    """At most 14 inner iterations per F-solve with the cycle — twice the CPU restatement's 7 (the oracle's aSIMPLE offers
    no velocity AMG, so the figure is the evidence test's).  No speed-up is expected at this size: ILU(F) needs about as
    few iterations here, and the test does not compare the two."""
    pr = problem("ns60")
    res = {}
    for on in (0, 1):
        ls = _handle(pr, on)
        try:
            res[on] = _solve(ls, pr)
        finally:
            ls.close()
    per = {on: res[on]["inner_u"] / res[on]["applies"] for on in (0, 1)}
    print(f"60x20, 8 outer iterations: inner iterations on F per F-solve {per[0]:.2f} with ILU(F) ({res[0]['inner_u']} in "
          f"{res[0]['applies']}), {per[1]:.2f} with the V-cycle ({res[1]['inner_u']} in {res[1]['applies']}); residual after "
          f"8: {res[0]['hist'][-1]:.3e} / {res[1]['hist'][-1]:.3e}")
    assert res[0]["its"] == res[1]["its"] == 8 and res[1]["applies"] > 0
    assert 0 < per[1] <= 14


# ------------------------------------------------------------------------------------------------ 8. the driver
_CHILD = r"""
import json, sys
import numpy as np
from navier_stokes_solver_amd import newton as N, problem as P, solver as S
first = P.generate(16, 10, nu=0.1, mode=0, state=0, inlet_bc=1)
ls = S.LinearSolver()
dev = N.DeviceBackend(ls, first, S.FGMRES, S.ASIMPLE, 1e-12)
r0 = dev.assemble(True, True, 0.1)
its = dev.solve()
dev.save()
dev.update(1.0)
r1 = dev.assemble(False, True, 0.1)
u, p = dev.solution()
np.save(sys.argv[1], np.concatenate([u, p]))
print("RESULT " + json.dumps(dict(r0=r0, r1=r1, its=its, levels=len(ls.amg_levels()), inner_u=ls.stats()["inner_u_its"])))
ls.close()
"""


def test_one_newton_iteration_with_the_switch_in_a_childs_environment(tmp_path):
    """NSK_ASIMPLE_VELOCITY_AMG is read once per process: a child process each, with and without it."""
    out = {}
    for key, val in (("off", None), ("on", "1")):
        env = dict(os.environ)
        env.pop("NSK_ASIMPLE_VELOCITY_AMG", None)
        if val is not None:
            env["NSK_ASIMPLE_VELOCITY_AMG"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        path = str(tmp_path / f"state_{key}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out[key] = dict(json.loads(line[7:]), x=np.load(path), said="[nsk] NSK_ASIMPLE_VELOCITY_AMG=1" in r.stdout)
    off, on = out["off"], out["on"]
    print(f"Newton iteration: |r| {off['r0']:.3e} -> {off['r1']:.3e} (ILU(F), {off['its']} outer, {off['inner_u']} inner on F) / "
          f"{on['r1']:.3e} (V-cycle, {on['its']} outer, {on['inner_u']} inner on F)")
    assert off["levels"] == 0 and on["levels"] >= 2 and on["said"] and not off["said"]
    assert abs(on["r0"] - off["r0"]) <= 1e-12 * off["r0"]
    assert off["r1"] < off["r0"] and abs(on["r1"] - off["r1"]) <= 1e-8 * off["r1"]


# ------------------------------------------------------------------------------------------------ 9. the fallback
def two_hub_system(pairs=800):
    """F: `pairs` strongly coupled pairs of unknowns (each its own aggregate) and one more pair, the hubs; hub 1 is coupled
    to one member of each pair of the first half by 1e-6 — far below the strength threshold, so the aggregates stay, and
    still an entry of F, so they are columns of the hub's row of the smoothed prolongator — hub 2 to the second half.
    Rows of P hold at most pairs / 2 + 1 columns; the hub rows of A P pairs + 1 = 801: over the 512 the set-up's product
    kernels count.  Every row of F has at most 402 entries (ILU(F) takes 448).  B~: one 1 x 2 block per row."""
    rng = np.random.default_rng(9)
    n = 2 * pairs + 2
    m = n // 2
    h1, h2 = n - 2, n - 1
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [rng.uniform(1.0, 2.0, n)]
    even = np.arange(0, n, 2)
    for a, b in ((even, even + 1), (even + 1, even)):
        rows.append(a), cols.append(b), vals.append(np.full(m, -0.3))
    for hub, members in ((h1, even[:pairs // 2]), (h2, even[pairs // 2:pairs])):
        for a, b in ((np.full(len(members), hub), members), (members, np.full(len(members), hub))):
            rows.append(a), cols.append(b), vals.append(np.full(len(members), 1e-6))
    F = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    B = sp.csr_matrix((rng.uniform(0.5, 1.5, n), np.arange(n), 2 * np.arange(m + 1)), shape=(m, n))

    def blk(A):
        A = A.tocsr()
        A.sort_indices()
        return SimpleNamespace(rows=A.shape[0], cols=A.shape[1], rowptr=A.indptr.astype(np.int32),
                               col=A.indices.astype(np.int32), val=A.data.astype(np.float64))
    return blk(F), blk(B.T), blk(B), sp.bmat([[F, B.T], [B, None]]).tocsc(), n, m


def test_an_f_the_set_up_cannot_coarsen_keeps_ilu_and_says_so_once(capfd):
    S = _S()
    F, Bt, B, J, n, m = two_hub_system()
    assert np.diff(F.rowptr).max() == 402
    rhs = rng_vec(n + m, 91)
    b = rng_vec(n, 92)
    got = {}
    capfd.readouterr()
    for on in (1, 0):
        ls = S.LinearSolver()
        try:
            ls.n_u, ls.n_p = n, m
            ls.set_option(S.OPT_ASIMPLE_VELOCITY_AMG, on)
            ls.set_partition(S.SPACE_U, 0, n, [])
            ls.set_partition(S.SPACE_P, 0, m, [])
            for k, A in ((S.BLK_F, F), (S.BLK_BT, Bt), (S.BLK_B, B)):
                ls.set_block(k, A)
            xs = []
            for _ in range(2):                       # two set-ups: still one warning
                ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
                assert ls.amg_levels() == [] and ls.tri_value_bytes(S.TRI_VELOCITY) == 8 and not ls.asimple_velocity_amg()
                xu, xp, its, res, rc = ls.solve(S.FGMRES, 1e-10, 400, rhs[:n], rhs[n:], np.zeros(n), np.zeros(m))
                assert rc == 0
                xs.append(np.concatenate([xu, xp]))
            got[on] = dict(x=xs[0], x2=xs[1], tri=ls.tri_apply(S.TRI_VELOCITY, b), its=its)
        finally:
            ls.close()
        err = capfd.readouterr().err
        warnings = [ln for ln in err.splitlines() if ln.startswith("[nsk] warning:") and "NSK_OPT_ASIMPLE_VELOCITY_AMG" in ln]
        assert len(warnings) == on, err
        if on:
            assert "ILU(F)" in warnings[0] and "512" in warnings[0]
    print(f"fallback: {got[1]['its']} outer iterations with ILU(F) in charge")
    assert rel_err(got[1]["x"], spl.splu(J).solve(rhs)) <= 1e-8
    for k in ("x", "x2", "tri"):                                                          # and the bits of the option at 0
        assert np.array_equal(got[1][k], got[0][k]), k
