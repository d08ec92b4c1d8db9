"""NSK_OPT_SCHUR_AMG (include/nsk.h): in the stationary aSIMPLE set-up one V-cycle of a smoothed-aggregation
hierarchy of S preconditions the inner CG on S, in place of ILU(S).

1. The public surface: option values, what nsk_schur_amg_info reports after each kind of set-up, the pressure slot of the
   triangular getters under the option.
2. 0 is the code path and the bits of a handle that never touched the option.
3. The cycle alone against the CPU restatement (oracle.Amg) on the S the handle formed: level rows, non-zeros, lambda to
   1e-12, one cycle to 1e-11 relative — the bound tests/test_gpu_parity.py::test_amg_vcycle_matches_oracle holds for F.
4. fp32 operators (NSK_OPT_AMG_PRECISION = 32 governs this hierarchy too).  Level 0 is S itself, which carries 16-bit
   column offsets: the residual products take spmv_stream_kernel<float, VEC, 2, unsigned short>, the form this change adds.
   That form alone (nsk_debug_spmv) on the irregular patterns of tests/spmv_reference.py: integer data exactly, random
   doubles within the counted bound of tests/test_gpu_spmv_kernels.py for the fp32 stream form (+ 2 u |result| for the
   subtraction and the reference's own), and the bytes of the int32-column form.
   The fp32 cycle against the double cycle.  Every product of the cycle with a rounded operator returns (A o (1 + d)) x,
   |d| <= u32 = 2^-24, so it differs from the double product by at most u32 |A| |x| entry by entry (double roundings,
   1e-16, left out).  A cycle holds N = 6 such products per level that has a coarser one (four with A — three residuals of
   the two Chebyshev smoothers and the one that is restricted — one with R, one with P) and none on a level solved by its
   dense inverse.  A perturbed residual enters x through a Chebyshev update x += c D^-1 r whose largest coefficient is
   c = 2 rho_1 / delta = 3.23 / lambda (degree 2 on [lambda / 20, lambda]), so one product moves x by at most
   3.23 u32 g |x|, g = max(1, ||D^-1 |S|||_inf / lambda), formed from the downloaded S and its lambda and taken for the
   Galerkin level too; in first order the N contributions add and the rest of the cycle (a contraction in the energy
   norm) does not amplify them:   max |x32 - x64| <= 3.23 N g u32 max |x64|.   First-order reasoning, not a theorem;
   no measured figure enters it.
5. Whole solves: to 1e-10 against the sparse-direct solution at 16x10, the inner pressure iterations of 8 outer steps at
   60x20 (less than half of ILU(S)'s), one Newton iteration through DeviceBackend with NSK_SCHUR_AMG=1 in a child's
   environment.
6. The fallback: an S whose diagonal carries both signs cannot take the cycle; ILU(S) stands, one warning per handle.
"""
import ctypes as C
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
STREAM_F32, STREAM_I16_F32 = 2, 12


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


def _O():
    from oracle import oracle as O
    return O


def _handle(pr, schur_amg=None, subdomains=1, amg_bits=None):
    S = _S()
    ls = S.LinearSolver()
    if schur_amg is not None:
        ls.set_option(S.OPT_SCHUR_AMG, schur_amg)
    if subdomains > 1:
        ls.set_option(S.OPT_SUBDOMAINS, subdomains)
    if amg_bits is not None:
        ls.set_option(S.OPT_AMG_PRECISION, amg_bits)
    ls.set_problem(pr)
    return ls


def _forms(ls):
    out = np.zeros(5, np.int64)
    ls.L.nsk_debug_schur_amg_forms.argtypes = [C.c_void_p, C.c_void_p]
    assert ls.L.nsk_debug_schur_amg_forms(ls.h, out.ctypes.data) == 0
    return out.tolist()


def _schur(ls, n_p):
    rp, col, val = ls.get_block(_S().BLK_S)
    return sp.csr_matrix((val, col, rp), shape=(n_p, n_p))


def _p_offsets(n_p, subdomains):
    return None if subdomains <= 1 else np.array([n_p * k // subdomains for k in range(subdomains + 1)], np.int32)


# ------------------------------------------------------------------------------------------------ 1. the surface
def test_option_values_and_what_the_info_reports():
    S = _S()
    pr = problem("ns16")
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_SCHUR_AMG, 1)
        with pytest.raises(RuntimeError, match="nsk error -61"):
            ls.set_option(S.OPT_SCHUR_AMG, 2)
        ls.set_problem(pr)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        lv = ls.schur_amg_info()
        assert len(lv) >= 2 and lv[0][:2] == (pr.n_p, ls.L.nsk_block_nnz(ls.h, S.BLK_S)) and lv[0][2] > 0
        # the pressure slot holds no triangular factor: as the velocity slot under the velocity AMG
        assert ls.tri_value_bytes(S.TRI_PRESSURE) == 0
        assert np.array_equal(ls.tri_perm(S.TRI_PRESSURE), np.arange(pr.n_p))
        b = rng_vec(pr.n_p, 3)
        assert np.array_equal(ls.tri_apply(S.TRI_PRESSURE, b), ls.schur_amg_apply(b))
        assert ls.index_width(S.BLK_S) == (16, 0, 0)          # S's SpMV on 16-bit offsets, no halves in this set-up
        assert ls.amg_value_bytes() == 0 and ls.amg_levels() == []      # (these keep reporting the velocity hierarchy)
        for prec, variant in ((S.BLOCK_DIAGONAL, S.STATIONARY), (S.BLOCK_TRIANGULAR, S.STATIONARY), (S.ASIMPLE, S.UNSTEADY)):
            ls.setup_preconditioner(prec, variant, 0.5)
            assert ls.schur_amg_info() == [], (prec, variant)
            with pytest.raises(RuntimeError, match="nsk error -62"):
                ls.schur_amg_apply(b)
        assert ls.tri_value_bytes(S.TRI_PRESSURE) == 8          # unsteady aSIMPLE: ILU(S) again
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert [a[:2] for a in ls.schur_amg_info()] == [a[:2] for a in lv]
        ls.set_option(S.OPT_SCHUR_AMG, 0)                       # takes effect at the next set-up
        assert ls.schur_amg_info() != []
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.schur_amg_info() == [] and ls.tri_value_bytes(S.TRI_PRESSURE) == 8
    finally:
        ls.close()


# ------------------------------------------------------------------------------------------------ 2. default bits
def _solve8(ls, pr, tol=0.0, steps=8):
    S = _S()
    ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
    ls.reset_stats()
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    its, res, rc = ls.solve_resident(S.FGMRES, tol, steps)
    xu, xp = ls.download_solution()
    return dict(its=its, rc=rc, x=np.concatenate([xu, xp]), hist=ls.history(), inner_p=ls.stats()["inner_p_its"])


def test_option_at_0_has_the_bits_of_a_handle_that_never_touched_it():
    pr = problem("ns16")
    hs = [_handle(pr), _handle(pr, 0)]
    try:
        hs[1].set_option(_S().OPT_SCHUR_AMG, 1)
        hs[1].set_option(_S().OPT_SCHUR_AMG, 0)
        runs = [_solve8(ls, pr, 0.0, 40) for ls in hs]          # (40 outer iterations: past one restart of FGMRES(30))
        assert runs[0]["its"] == 40 and hs[1].schur_amg_info() == []
        assert len(runs[0]["hist"]) > 40 and np.array_equal(runs[0]["hist"], runs[1]["hist"])
        assert np.array_equal(runs[0]["x"], runs[1]["x"]) and runs[0]["inner_p"] == runs[1]["inner_p"]
    finally:
        [ls.close() for ls in hs]


# ------------------------------------------------------------------------------------------------ 3. the cycle alone
@pytest.mark.parametrize("name,subdomains", [("ns16", 1), ("ns16", 3), ("ns60", 1), ("ns60", 3)])
def test_the_cycle_on_s_matches_the_cpu_restatement(name, subdomains):
    S, O = _S(), _O()
    pr = problem(name)
    ls = _handle(pr, 1, subdomains)
    try:
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        Sm = _schur(ls, pr.n_p)
        ref = O.Amg(O.CsrHolder.from_scipy(Sm), _p_offsets(pr.n_p, subdomains))
        for shard in range(subdomains):
            lv, ov = ls.schur_amg_info(shard), ref.levels(shard)
            print(f"{name} x{subdomains} shard {shard}: levels {[(r, z, round(lam, 6)) for r, z, lam in lv]}")
            assert len(lv) == len(ov) >= 2
            for (r, z, lam), (orows, onnz, olam) in zip(lv, ov):
                assert (r, z) == (orows, onnz) and abs(lam - olam) <= 1e-12 * olam
        assert ls.schur_amg_info(subdomains) == []
        b = rng_vec(pr.n_p, 78)
        x, xo = ls.schur_amg_apply(b), ref.apply(b)
        print(f"{name} x{subdomains}: one cycle against the CPU restatement {rel_err(x, xo):.2e}")
        assert rel_err(x, xo) <= 1e-11
        assert np.array_equal(ls.schur_amg_apply(b), x)                 # two applies, the same bits
        # of S's sign (negative here: the Newton system) and a contraction: what the CG needs of it
        assert float(b @ x) * Sm.diagonal()[0] > 0
        if subdomains == 1:
            assert np.linalg.norm(b - Sm @ x) < 0.8 * np.linalg.norm(b)
    finally:
        ls.close()


# ------------------------------------------------------------------------------------------------ 4. fp32 operators
class Mat(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_own_cols", C.c_int32), ("pad_", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("x_own", C.c_void_p),
                ("x_ghost", C.c_void_p)]


class Hook:
    """nsk_debug_spmv (nsk_internal.h): one launch of one form on copies of the operands, between guard words."""

    def __init__(self):
        S = _S()
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_spmv.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]

    def call(self, form, A, x, y, mode, z):
        xo, xg = (np.ascontiguousarray(v, dtype=np.float64) for v in x)
        ma = Mat(A.n_rows, A.n_cols, A.n_own, 0, A.rowptr.ctypes.data, A.col.ctypes.data, A.val.ctypes.data,
                 xo.ctypes.data, xg.ctypes.data)
        zz = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
        yy = np.array(y, dtype=np.float64, copy=True)
        info = np.zeros(16, dtype=np.int32)
        rc = self.L.nsk_debug_spmv(self.ls.h, form, 0, mode, 0, -1, -1, C.byref(ma), None, yy.ctypes.data,
                                   None if zz is None else zz.ctypes.data, None, None, None, 0, info.ctypes.data)
        return rc, yy, info

    def run(self, form, A, x, y, mode=2, z=None):
        """y after, or None when the plan refuses the form (a row above the run cap); no guard word may have changed."""
        rc, yy, info = self.call(form, A, x, y, mode, z)
        assert rc in (0, 1), (rc, self.ls.last_error(), A.name)
        if rc == 1:
            assert info[0] == -1 and info[15] != 0
            return None, info
        assert info[0] == form and info[15] == 0
        assert info[13] == 0, f"form {form} mode {mode} on {A.name}: {info[13]} guard words were written"
        return yy, info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()


PATTERNS = M.scalar_patterns()
# the patterns the exact (Python) row sums are formed for: empty rows, rows at and above the run cap, odd and even row
# pointers, runs ending on either residue, a coarse-operator-like pattern
EXACT = ["empty_start", "empty_65_last", "nnz0", "row_2048", "row_2049", "len_1_2", "geom_12", "even", "odd_after_0",
         "ends_alternate", "ends_alternate_plus_1", "amg_like"]


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_residual_form_on_16_bit_offsets_integer_exact_and_the_bytes_of_the_int32_form(hook, name):
    A = M.int_values(PATTERNS[name], 1)
    x, y, z = M.int_x(A), M.int_vec(A.n_rows, 13, 6), M.int_vec(A.n_rows, 7, 3)
    got, info = hook.run(STREAM_I16_F32, A, x, y, z=z)
    if not M.stream_plan(A)["ok"]:
        assert got is None and info[15] == 1
        return
    assert info[1] == M.stream_plan(A)["vec"]
    want = z - M.int_row_sums(A, *x).astype(np.float64)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
    # values that are no floats: the same lanes sum the same entries as on int32 columns, so the same bytes
    Ar = M.real_values(PATTERNS[name], 3)
    xr = M.real_x(Ar, 4)
    zr = rng_vec(Ar.n_rows, 5)
    a, ia = hook.run(STREAM_I16_F32, Ar, xr, y, z=zr)
    b, ib = hook.run(STREAM_F32, Ar, xr, y, z=zr)
    assert ia[1] == ib[1] and list(ia[5:13]) == list(ib[5:13])
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    assert np.array_equal(hook.run(STREAM_I16_F32, Ar, xr, y, z=zr)[0], a)        # twice, the same bits


@pytest.mark.parametrize("name", EXACT)
def test_residual_form_on_16_bit_offsets_within_the_counted_bound(hook, name):
    A = M.real_values(PATTERNS[name], 7)
    x = M.real_x(A, 8)
    z = rng_vec(A.n_rows, 9)
    got, info = hook.run(STREAM_I16_F32, A, x, np.zeros(A.n_rows), z=z)
    if not M.stream_plan(A)["ok"]:
        assert got is None and info[15] == 1
        return
    s32, a32 = M.exact_row_sums(A, *x, fp32=True)
    want = z - s32
    tol = M.gamma(M.roundings("stream", A.row_len)) * a32 + U * np.abs(s32) + 2 * U * np.abs(want)
    err = np.abs(got - want)
    print(f"{name}: VEC {info[1]}, largest error / bound {float(np.max(err / np.maximum(tol, 1e-300))) if A.n_rows else 0:.3f}")
    assert np.all(err <= tol), (name, np.nonzero(err > tol)[0][:8])
    if A.nnz:
        s64, _ = M.exact_row_sums(A, *x)
        assert not np.array_equal(got, z - s64)                                    # (it did read the rounded values)


def test_mode_1_has_no_fp32_kernel_on_16_bit_offsets_and_says_so(hook):
    A = M.int_values(PATTERNS["even"], 1)
    y = M.int_vec(A.n_rows, 13, 6)
    rc, yy, info = hook.call(STREAM_I16_F32, A, M.int_x(A), y, 1, None)
    assert rc == -1 and "mode 1" in hook.ls.last_error()
    assert info[0] == -1


@pytest.mark.parametrize("name,subdomains", [("ns16", 1), ("ns60", 1), ("ns60", 3)])
def test_the_fp32_cycle_runs_on_s_and_stays_within_the_counted_bound_of_the_double_one(name, subdomains):
    S = _S()
    pr = problem(name)
    b = rng_vec(pr.n_p, 79)
    out = {}
    for bits in (64, 32):
        ls = _handle(pr, 1, subdomains, bits)
        try:
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            lv = ls.schur_amg_info()
            Sm = _schur(ls, pr.n_p)
            x = ls.schur_amg_apply(b)           # (today: error -1, no mode-2 kernel on 16-bit offsets)
            assert np.array_equal(ls.schur_amg_apply(b), x)
            f = _forms(ls)
            out[bits] = dict(x=x, lv=lv, f=f, S=Sm, width=ls.index_width(S.BLK_S)[0])
        finally:
            ls.close()
    a, c = out[64], out[32]
    assert a["lv"] == c["lv"] and np.array_equal(a["S"].data, c["S"].data)       # the set-up is the double one
    n_prod = 6 * (len(a["lv"]) - 1)             # per shard and cycle; the last level is solved by its dense inverse
    assert a["width"] == c["width"] == 16
    assert a["f"] == [0, 2 * n_prod * subdomains, 0, 0, 0], a["f"]
    # every product of the fp32 cycle reads fp32 values — level 0's four residuals among them, on S's 16-bit offsets
    # with one shard (a shard of several is a block of its own on int32 columns)
    assert c["f"] == [0, 0, 2 * n_prod * subdomains, 0, 0], c["f"]
    d = np.abs(a["S"].diagonal())
    g = max(1.0, float((abs(a["S"]).sum(axis=1).A1 / d).max()) / a["lv"][0][2])
    bound = 3.23 * n_prod * g * U32
    dev = rel_err(c["x"], a["x"])
    print(f"{name} x{subdomains}: fp32 cycle against the double cycle {dev:.2e}, bound {bound:.2e} (N {n_prod}, g {g:.2f})")
    assert 0 < dev <= bound


# ------------------------------------------------------------------------------------------------ 5. whole solves
@pytest.mark.parametrize("name", ["ns16", "stokes16"])
def test_whole_solves_reach_the_sparse_direct_solution_with_the_option_on_and_off(name):
    S = _S()
    pr = problem(name)
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    xs = spl.splu(J).solve(b)
    res = {}
    for on in (0, 1):
        ls = _handle(pr, on)
        try:
            res[on] = _solve8(ls, pr, 1e-10, 20000)
            assert bool(ls.schur_amg_info()) == bool(on)
        finally:
            ls.close()
    for on in (0, 1):
        r = res[on]
        print(f"{name} option {on}: outer {r['its']}, inner pressure iterations {r['inner_p']}, "
              f"|x - x_direct| {rel_err(r['x'], xs):.2e}, true residual {np.linalg.norm(b - J @ r['x']):.2e}")
        assert r["rc"] == 0 and np.linalg.norm(b - J @ r["x"]) <= 1.05e-10
        assert rel_err(r["x"], xs) <= 1e-8


def test_inner_pressure_iterations_at_60x20_are_less_than_half():
    pr = problem("ns60")
    res = {}
    for on in (0, 1):
        ls = _handle(pr, on)
        try:
            res[on] = _solve8(ls, pr)
        finally:
            ls.close()
    print(f"60x20, 8 outer iterations: inner pressure iterations {res[0]['inner_p']} with ILU(S), {res[1]['inner_p']} with "
          f"the V-cycle; residual after 8: {res[0]['hist'][-1]:.3e} / {res[1]['hist'][-1]:.3e}")
    assert res[0]["its"] == res[1]["its"] == 8
    assert 0 < res[1]["inner_p"] < 0.5 * res[0]["inner_p"], (res[1]["inner_p"], res[0]["inner_p"])


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
print("RESULT " + json.dumps(dict(r0=r0, r1=r1, its=its, levels=len(ls.schur_amg_info()), inner_p=ls.stats()["inner_p_its"])))
ls.close()
"""


def test_one_newton_iteration_with_the_switch_in_a_childs_environment(tmp_path):
    """NSK_SCHUR_AMG is read once per process: a child process each, with and without it."""
    out = {}
    for key, val in (("off", None), ("on", "1")):
        env = dict(os.environ)
        env.pop("NSK_SCHUR_AMG", None)
        if val is not None:
            env["NSK_SCHUR_AMG"] = val
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        path = str(tmp_path / f"state_{key}.npy")
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        out[key] = dict(json.loads(line[7:]), x=np.load(path), said="NSK_SCHUR_AMG=1" in r.stdout)
    off, on = out["off"], out["on"]
    print(f"Newton iteration: |r| {off['r0']:.3e} -> {off['r1']:.3e} (ILU(S), {off['its']} outer, {off['inner_p']} inner on S) / "
          f"{on['r1']:.3e} (V-cycle, {on['its']} outer, {on['inner_p']} inner on S)")
    assert off["levels"] == 0 and on["levels"] >= 2 and on["said"] and not off["said"]
    assert abs(on["r0"] - off["r0"]) <= 1e-12 * off["r0"]
    # (the first pass of the driver: the inlet data enter with this step and the ramp goes on, so |r| falls, not to zero)
    assert off["r1"] < off["r0"] and abs(on["r1"] - off["r1"]) <= 1e-8 * off["r1"]
    assert rel_err(on["x"], off["x"]) <= 1e-8


# ------------------------------------------------------------------------------------------------ 6. the fallback
def _two_sign_system(m=96):
    """F diagonal with both signs, B~ with one 1 x 2 block per row: S = B~ F^-1 B~^T is diagonal, positive on the first
    half of the rows and negative on the second.  The device set-up refuses it where it forms dinv (-85)."""
    rng = np.random.default_rng(6)
    d = rng.uniform(1.0, 2.0, 2 * m) * np.where(np.arange(2 * m) < m, 1.0, -1.0)
    bv = rng.uniform(0.5, 1.5, 2 * m)
    F = sp.diags(d).tocsr()
    B = sp.csr_matrix((bv, np.arange(2 * m), 2 * np.arange(m + 1)), shape=(m, 2 * m))

    def blk(A):
        A = A.tocsr()
        A.sort_indices()
        return SimpleNamespace(rows=A.shape[0], cols=A.shape[1], rowptr=A.indptr.astype(np.int32),
                               col=A.indices.astype(np.int32), val=A.data.astype(np.float64))
    J = sp.bmat([[F, B.T], [B, None]]).tocsc()
    return blk(F), blk(B.T), blk(B), J, (B @ sp.diags(1.0 / d) @ B.T).diagonal()


def test_an_s_with_a_two_signed_diagonal_keeps_ilu_and_says_so_once(capfd):
    S = _S()
    m = 96
    F, Bt, B, J, s_diag = _two_sign_system(m)
    assert s_diag.min() < 0 < s_diag.max()
    rhs = rng_vec(3 * m, 61)
    b = rng_vec(m, 62)
    got = {}
    capfd.readouterr()
    for on in (1, 0):
        ls = S.LinearSolver()
        try:
            ls.n_u, ls.n_p = 2 * m, m
            ls.set_option(S.OPT_SCHUR_AMG, on)
            ls.set_partition(S.SPACE_U, 0, 2 * m, [])
            ls.set_partition(S.SPACE_P, 0, m, [])
            for k, A in ((S.BLK_F, F), (S.BLK_BT, Bt), (S.BLK_B, B)):
                ls.set_block(k, A)
            xs = []
            for _ in range(2):                       # two set-ups: still one warning
                ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
                assert ls.schur_amg_info() == [] and ls.tri_value_bytes(S.TRI_PRESSURE) == 8
                xu, xp, its, res, rc = ls.solve(S.FGMRES, 1e-10, 200, rhs[:2 * m], rhs[2 * m:], np.zeros(2 * m), np.zeros(m))
                assert rc == 0
                xs.append(np.concatenate([xu, xp]))
            got[on] = dict(x=xs[0], x2=xs[1], tri=ls.tri_apply(S.TRI_PRESSURE, b), its=its)
        finally:
            ls.close()
        err = capfd.readouterr().err
        warnings = [ln for ln in err.splitlines() if ln.startswith("[nsk] warning:") and "NSK_OPT_SCHUR_AMG" in ln]
        assert len(warnings) == on, err
        if on:
            assert "ILU(S)" in warnings[0] and "both signs" in warnings[0]
    assert rel_err(got[1]["x"], spl.splu(J).solve(rhs)) <= 1e-8
    assert np.abs(got[1]["tri"] - b / s_diag).max() <= 4 * U * np.abs(b / s_diag).max()     # ILU(0) of a diagonal S
    for k in ("x", "x2", "tri"):                                                          # and the bits of the option at 0
        assert np.array_equal(got[1][k], got[0][k]), k
