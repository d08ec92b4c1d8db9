"""NSK_OPT_AMG_PRECISION = 32: the velocity AMG's V-cycle multiplies by fp32 copies of every level's A, P and R
(include/nsk.h).

1. The new kernels alone (nsk_debug_spmv) on the irregular patterns of tests/spmv_reference.py: the 2 x 2 node-block
   residual y = z - A x in fp64 against exact row sums (integer data: equality; random doubles: the blocked form's counted
   bound of tests/test_gpu_spmv_kernels.py plus one rounding for the subtraction, and one for the reference's own), and
   every fp32 form — the block residual, the scalar stream kernel in modes 1 and 2 — bit for bit against the fp64 kernel
   of the same form on the values rounded to float.  Guard words around every vector.
2. The V-cycle on 60x20 (three levels: a coarse operator of the hierarchy's own smooths in fp32), one shard, three
   sub-domains and one shard without node blocks: the device's hierarchy is downloaded (nsk_debug_amg_level) and the device
   cycle held to 1e-11 against the NumPy cycle of tests/amg_cycle_reference.py on it — in double with 64, on the operators
   rounded through np.float32 with 32.
3. 64 is the code path and the bits of a handle that never touched the option.
4. Whole FGMRES + blockTriangular solves to 1e-12 at 64 and 32, alone and together with NSK_OPT_INNER_MATRIX_PRECISION.
5. Refusals: another value, a set-up without AMG, a value outside fp32's range — in F itself (level 0's A, converted
   last), in a Galerkin coarse operator and in a shard's diagonal block (converted inside the build) — and the handle
   after the refusal.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from tests import amg_cycle_reference as V
from tests import spmv_reference as M
from tests.util import problem, rel_err, rng_vec

pytestmark = pytest.mark.gpu

U = M.U
STREAM, STREAM_F32, BLK22, BLK22_RES, BLK22_RES_F32 = 1, 2, 3, 13, 14
G, YO = 1, 4    # misalign bits: ghost tails, y / z


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


class Mat(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_own_cols", C.c_int32), ("pad_", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("x_own", C.c_void_p),
                ("x_ghost", C.c_void_p)]


def _ptr(a):
    return None if a is None else a.ctypes.data


class Hook:
    def __init__(self):
        S = _S()
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_spmv.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]

    def run(self, form, A, x, y, mode=0, z=None, misalign=0):
        """y after one launch (None when the plan refuses the form), info."""
        xo, xg = (np.ascontiguousarray(v, dtype=np.float64) for v in x)
        ma = Mat(A.n_rows, A.n_cols, A.n_own, 0, _ptr(A.rowptr), _ptr(A.col), _ptr(A.val), _ptr(xo), _ptr(xg))
        zz = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
        yy = np.array(y, dtype=np.float64, copy=True)
        info = np.zeros(16, dtype=np.int32)
        rc = self.L.nsk_debug_spmv(self.ls.h, form, 0, mode, misalign, -1, -1, C.byref(ma), None, _ptr(yy), _ptr(zz), None, None,
                                   None, 0, _ptr(info))
        assert rc in (0, 1), (rc, self.ls.last_error(), form, A.name)
        if rc == 1:
            assert info[0] == -1 and info[15] != 0
            return None, info
        assert info[0] == form and info[13] == 0, f"form {form} mode {mode} on {A.name}: {info[13]} guard words were written"
        return yy, info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()


@functools.lru_cache(maxsize=1)
def blocks22():
    return {name: A for name, (Rr, Cc, A) in M.block_patterns().items() if (Rr, Cc) == (2, 2)}


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} wrong rows, first {bad[:8].tolist()}, got - want {(got[bad[:8]] - want[bad[:8]]).tolist()}"


# ------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("name", sorted(blocks22()))
def test_block_residual_integer_exact(hook, name):
    A = M.int_values(blocks22()[name], 2)
    x, y, z = M.int_x(A), M.int_vec(A.n_rows, 13, 6), M.int_vec(A.n_rows, 7, 3)
    p = M.blocked_plan(A, 2, 2)
    want = z - M.int_row_sums(A, *x).astype(np.float64)
    for form in (BLK22_RES, BLK22_RES_F32):
        for mis in (0, G):
            got, info = hook.run(form, A, x, y, mode=2, z=z, misalign=mis)
            if not p["ok"]:      # broken node structure: reported, never forced
                assert got is None and info[15] == 2
                continue
            assert (info[3], info[4], info[7]) == (2, 2, 1) and info[14] == len(p["rb"]) - 1
            same(got, want, f"form {form} misalign {mis} on {name}")


@pytest.mark.parametrize("name", sorted(blocks22()))
def test_block_residual_random_and_fp32_bits(hook, name):
    A0 = blocks22()[name]
    p = M.blocked_plan(A0, 2, 2)
    if not p["ok"]:
        return
    A = M.real_values(A0, 7)
    x = M.real_x(A, 8)
    rng = np.random.default_rng(A.n_rows)
    y, z = rng.uniform(-1, 1, A.n_rows), rng.uniform(-1, 1, A.n_rows)
    s, a = M.exact_row_sums(A, *x)
    Lb = np.repeat(np.diff(p["brp"]), 2)
    E = M.gamma(M.roundings("blk_c2", Lb)) * a + U * np.abs(s)
    want = z - s
    A32 = A.with_values(A.val.astype(np.float32).astype(np.float64))
    for mis in (0, G):
        got, _ = hook.run(BLK22_RES, A, x, y, mode=2, z=z, misalign=mis)
        err = np.abs(got - want)
        tol = E + 2 * U * np.abs(want)
        assert np.all(err <= tol), (name, mis, float(np.max(err / np.maximum(tol, 1e-300))))
        got32, _ = hook.run(BLK22_RES_F32, A, x, y, mode=2, z=z, misalign=mis)
        same(got32, hook.run(BLK22_RES, A32, x, y, mode=2, z=z, misalign=mis)[0], f"block residual fp32, misalign {mis}, on {name}")
        # the same lanes and sums as y = A x: the residual of the fp64 kernel is z minus its product, rounded once
        same(got, z - hook.run(BLK22, A, x, y, misalign=mis)[0], f"block residual against z - (A x), misalign {mis}, on {name}")
        if A.nnz:
            assert not np.array_equal(got32, got), name


def _scalar_cases():
    out = dict(M.scalar_patterns())
    out.update({name: A for name, (_, _, A) in M.block_patterns().items()})
    return out


@pytest.mark.parametrize("name", sorted(_scalar_cases()))
def test_stream_fp32_modes_have_the_bits_of_fp64_on_rounded_values(hook, name):
    A = M.real_values(_scalar_cases()[name], 7)
    p = M.stream_plan(A)
    x = M.real_x(A, 8)
    rng = np.random.default_rng(A.n_rows + 1)
    y, z = rng.uniform(-1, 1, A.n_rows), rng.uniform(-1, 1, A.n_rows)
    A32 = A.with_values(A.val.astype(np.float32).astype(np.float64))
    for mis in (0, G | YO):
        for mode, zz in ((1, None), (1, z), (2, z)):
            got32, i32 = hook.run(STREAM_F32, A, x, y, mode=mode, z=zz, misalign=mis)
            if not p["ok"]:      # a row above the run cap: the level keeps the CSR-vector kernel on double values
                assert got32 is None and i32[15] == 1
                continue
            got64, i64 = hook.run(STREAM, A32, x, y, mode=mode, z=zz, misalign=mis)
            assert i32[1] == i64[1] == p["vec"] and i32[14] == len(p["rb"]) - 1
            same(got32, got64, f"stream fp32 mode {mode} z {zz is not None} misalign {mis} on {name}")
            if A.nnz and mis == 0:
                assert not np.array_equal(got32, hook.run(STREAM, A, x, y, mode=mode, z=zz)[0]), name


def test_both_pair_forms_of_the_stream_kernel_were_covered():
    vecs = {M.stream_plan(A)["vec"] for A in _scalar_cases().values() if M.stream_plan(A)["ok"]}
    assert vecs == {2, 3}


# ------------------------------------------------------------------ 2. the V-cycle on the device's own hierarchy
def _level_hook(ls):
    L = ls.L
    L.nsk_debug_amg_level.restype = C.c_int64
    L.nsk_debug_amg_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    return L.nsk_debug_amg_level


def download(ls, shard=0):
    """The hierarchy of one shard as tests/amg_cycle_reference.py takes it."""
    f = _level_hook(ls)
    info = ls.amg_levels(shard)
    levels = []
    for l, (rows, nnz, lam) in enumerate(info):
        last = l == len(info) - 1
        ops = []
        for which in ((0,) if last else (0, 1, 2)):
            n_r = info[l + 1][0] if which == 2 else rows
            n_c = info[l + 1][0] if which == 1 else rows
            z = f(ls.h, shard, l, which, None, None, None, None)
            assert z >= 0 and (which != 0 or z == nnz), (l, which, z, ls.last_error())
            rp, col, val = np.zeros(n_r + 1, np.int32), np.zeros(z, np.int32), np.zeros(z)
            has_inv = which == 0 and f(ls.h, shard, l, 3, None, None, None, None) == 1
            d = np.zeros(rows * rows if has_inv else rows) if which == 0 else None
            assert f(ls.h, shard, l, which, _ptr(rp), _ptr(col), _ptr(val), _ptr(d)) == z
            assert rp[0] == 0 and rp[-1] == z
            ops.append(sp.csr_matrix((val, col, rp), shape=(n_r, n_c)))
            if which == 0:
                dinv, inv = (None, d.reshape(rows, rows)) if has_inv else (d, None)
        if last:
            assert f(ls.h, shard, l, 1, None, None, None, None) == -61     # no P on the last level
            levels.append(V.Level(ops[0], dinv if dinv is not None else np.ones(rows), lam, inv=inv))
        else:
            levels.append(V.Level(ops[0], dinv, lam, ops[1], ops[2]))
    return levels


def forms(ls):
    """Products of the cycles since the hierarchy was built, by kernel form (csr_vector, stream, stream_f32, blk, blk_f32)."""
    out = np.zeros(5, np.int64)
    ls.L.nsk_debug_amg_forms.argtypes = [C.c_void_p, C.c_void_p]
    assert ls.L.nsk_debug_amg_forms(ls.h, _ptr(out)) == 0
    return out.tolist()


def _same_operators(a, b):
    for La, Lb in zip(a, b):
        for Ma, Mb in ((La.A, Lb.A), (La.P, Lb.P), (La.R, Lb.R)):
            if Ma is not None and not (np.array_equal(Ma.indptr, Mb.indptr) and np.array_equal(Ma.indices, Mb.indices) and
                                       np.array_equal(Ma.data, Mb.data)):
                return False
    return len(a) == len(b)


CYCLE_CASES = {"one_shard": dict(sub=1, bsr=1), "three_subdomains": dict(sub=3, bsr=1), "no_node_blocks": dict(sub=1, bsr=0)}


@pytest.mark.parametrize("case", sorted(CYCLE_CASES))
def test_v_cycle_against_the_numpy_cycle_on_the_device_hierarchy(case):
    S = _S()
    sub, bsr = CYCLE_CASES[case]["sub"], CYCLE_CASES[case]["bsr"]
    pr = problem("ns60")
    off = [(pr.n_u * k // sub) & ~1 for k in range(sub)] + [pr.n_u]
    b = rng_vec(pr.n_u, 77)
    F = pr.F.to_scipy()
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        ls.set_option(S.OPT_SUBDOMAINS, sub)
        ls.set_option(S.OPT_BSR_VELOCITY, bsr)
        out, hier = {}, {}
        for bits in (64, 32):
            ls.set_option(S.OPT_AMG_PRECISION, bits)
            ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
            assert ls.amg_value_bytes() == bits // 8
            assert ls.inner_value_bytes(S.BLK_F) == 8
            assert forms(ls) == [0] * 5
            out[bits] = ls.tri_apply(S.TRI_VELOCITY, b)
            hier[bits] = [download(ls, k) for k in range(sub)]
            # which kernels the cycle took: three levels, the last one a dense inverse — per shard four residual products
            # with the level's A, one with R and one with P on each of the two upper levels
            fl = forms(ls)
            print(f"FORMS {case} {bits}: {fl}")
            if bits == 64:
                assert fl == [0, 12 * sub, 0, 0, 0]
            elif sub == 1 and bsr:
                assert fl == [0, 0, 8, 0, 4]      # F itself through its 2 x 2 fp32 copy, the rest scalar fp32
            else:
                assert fl == [0, 0, 12 * sub, 0, 0]
            assert np.array_equal(out[bits], ls.tri_apply(S.TRI_VELOCITY, b)), "two cycles, two results"
        for k in range(sub):
            sizes = [L.n for L in hier[64][k]]
            print(f"LEVELS {case} shard {k}: {sizes}")
            assert len(sizes) >= 3 and sizes[0] == off[k + 1] - off[k], sizes
            assert hier[64][k][1].inv is None, "level 1 is smoothed: its operator is one of the hierarchy's own"
            # the set-up is the same in double whatever the cycle reads
            assert _same_operators(hier[64][k], hier[32][k])
        ref64 = V.apply_shards(hier[64], off, b)
        ref32 = V.apply_shards([V.rounded(h) for h in hier[64]], off, b)
        e64, e32 = rel_err(out[64], ref64), rel_err(out[32], ref32)
        d = rel_err(out[32], out[64])
        print(f"CYCLE {case}: device 64 against NumPy {e64:.3e}, device 32 against NumPy on rounded operators {e32:.3e}, "
              f"32 against 64 {d:.3e}")
        assert e64 <= 1e-11
        assert e32 <= 1e-11
        assert not np.array_equal(out[32], out[64])
        assert rel_err(ref32, ref64) > 1e-9, "the rounded hierarchy is another operator: the two references tell the arms apart"
        if sub == 1:
            for bits in (64, 32):
                assert np.linalg.norm(b - F @ out[bits]) < 0.8 * np.linalg.norm(b), bits
    finally:
        ls.close()


def test_values_changed_without_a_new_setup_reach_level_0():
    """Level 0 is F itself: after nsk_scale_values without a set-up the fp64 cycle reads the new F on level 0 (and the old
    hierarchy below), and so does the fp32 cycle — its copy is converted again before the next product."""
    S = _S()
    pr = problem("ns16")
    b = rng_vec(pr.n_u, 78)
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        x0 = ls.tri_apply(S.TRI_VELOCITY, b)
        levels = download(ls)
        ls.scale_values(S.BLK_F, 0.75)
        x1 = ls.tri_apply(S.TRI_VELOCITY, b)
        assert ls.amg_value_bytes() == 4
        changed = [V.Level(levels[0].A * 0.75, levels[0].dinv, levels[0].lam, levels[0].P, levels[0].R)] + levels[1:]
        assert rel_err(x0, V.vcycle(V.rounded(levels), b)) <= 1e-11
        assert rel_err(x1, V.vcycle(V.rounded(changed), b)) <= 1e-11
        assert rel_err(x1, x0) > 1e-3
    finally:
        ls.close()


# ------------------------------------------------------------------ 3. 64 is today's path and bits
def test_64_is_the_untouched_handle_bit_for_bit():
    S = _S()
    pr = problem("ns16")
    b = rng_vec(pr.n_u, 79)
    hs = []
    try:
        res = []
        for opt in (None, 64):
            ls = S.LinearSolver()
            hs.append(ls)
            if opt is not None:
                ls.set_option(S.OPT_AMG_PRECISION, opt)
            ls.set_problem(pr)
            ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
            assert ls.amg_value_bytes() == 8
            x = ls.tri_apply(S.TRI_VELOCITY, b)
            xu, xp, it, r, rc = ls.solve(1, 1e-12, 20000, pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
            assert rc == 0
            res.append((x, xu, xp, it, ls.history()))
        a, c = res
        assert np.array_equal(a[0], c[0])
        assert a[3] == c[3] and np.array_equal(a[4], c[4]) and len(a[4]) > 1
        assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
        # and back from 32: the same bits again
        ls = hs[1]
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 4 and not np.array_equal(ls.tri_apply(S.TRI_VELOCITY, b), a[0])
        ls.set_option(S.OPT_AMG_PRECISION, 64)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 8 and np.array_equal(ls.tri_apply(S.TRI_VELOCITY, b), a[0])
    finally:
        for ls in hs:
            ls.close()


# ------------------------------------------------------------------ 4. whole solves
@pytest.mark.parametrize("name", ["ns16", "ns60"])
def test_fgmres_block_triangular_with_an_fp32_v_cycle(name):
    """The outer FGMRES stays double and checks the true residual: the same solution; outer iterations at 32 no more than
    1.10 x those of the 64 arm beside it (the margin of the inner-matrix option's test), with the inner matrices in double
    and in fp32 (F's 2 x 2 fp32 copy shared by both readers)."""
    S = _S()
    pr = problem(name)
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    xs = spl.splu(J).solve(b)
    tol = 1e-12
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        its = {}
        for inner in (64, 32):
            for amg in (64, 32):
                ls.set_option(S.OPT_INNER_MATRIX_PRECISION, inner)
                ls.set_option(S.OPT_AMG_PRECISION, amg)
                ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
                xu, xp, it, res, rc = ls.solve(1, tol, 20000, pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
                assert ls.amg_value_bytes() == amg // 8 and ls.inner_value_bytes(S.BLK_F) == inner // 8, (inner, amg)
                x = np.concatenate([xu, xp])
                assert rc == 0, (inner, amg, rc)
                assert np.linalg.norm(b - J @ x) <= 1.05 * tol, (inner, amg)
                assert rel_err(x, xs) <= 2e-8, (inner, amg)
                its[(inner, amg)] = it
        print(f"ITERATIONS {name} FGMRES + blockTriangular to 1e-12 (inner matrices, AMG) -> outer iterations: {its}")
        for inner in (64, 32):
            assert its[(inner, 32)] <= 1.10 * its[(inner, 64)], its
    finally:
        ls.close()


# ------------------------------------------------------------------ 5. other cases
def test_other_values_and_set_ups_without_amg():
    S = _S()
    pr = problem("ns16")
    ls = S.LinearSolver()
    try:
        with pytest.raises(RuntimeError, match="-61"):
            ls.set_option(S.OPT_AMG_PRECISION, 16)
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.set_problem(pr)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        assert ls.amg_value_bytes() == 0
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.UNSTEADY)
        assert ls.amg_value_bytes() == 0
        ls.set_option(S.OPT_VELOCITY_AMG, 0)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 0 and ls.amg_levels() == []
        ls.set_option(S.OPT_VELOCITY_AMG, 1)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 4
        t32, by32 = ls.time_op(57, 2)
        t20, by20 = ls.time_op(20, 2)
        assert 0 < by32 < by20, "op 57 counts the stored formats, op 20 the algorithmic CSR bytes"
        ls.set_option(S.OPT_AMG_PRECISION, 64)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.time_op(57, 2)[1] == ls.time_op(20, 2)[1] == by20
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY)
        with pytest.raises(RuntimeError, match="-62"):
            ls.time_op(57, 2)
    finally:
        ls.close()


@pytest.mark.parametrize("scale", [1e200, 1e60])
def test_a_value_outside_the_range_of_fp32_is_refused(scale):
    """1e200: the squares of the strength test overflow too (no aggregates, one smoothed level); 1e60: the full hierarchy
    is built in double and its first operator does not fit fp32.  Either way -48 names the level and the operator."""
    S = _S()
    pr = problem("ns16")
    b = rng_vec(pr.n_u, 80)
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        ls.scale_values(S.BLK_F, scale)
        ls.set_option(S.OPT_AMG_PRECISION, 64)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 8
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)    # (the hierarchy is built on first use)
        for call in (ls.amg_value_bytes, lambda: ls.tri_apply(S.TRI_VELOCITY, b)):
            with pytest.raises(RuntimeError, match=r"nsk error -48: NSK_OPT_AMG_PRECISION = 32: .* level 0's A "):
                call()
        ls.scale_values(S.BLK_F, 1.0 / scale)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 4 and ls.inner_value_bytes(S.BLK_F) == 8
        assert np.all(np.isfinite(ls.tri_apply(S.TRI_VELOCITY, b)))
    finally:
        ls.close()


@pytest.mark.parametrize("sub, where", [(1, "level 1's A"), (3, "level 0's A")])
def test_an_operator_of_the_hierarchy_outside_the_range_of_fp32_is_refused(sub, where):
    """The conversion of the hierarchy's OWN operators, thrown from inside the build.  60x20 has three levels, and F times
    2^200 (1.6e60) is fine in double.  One shard: level 0 is F itself (checked last), P and R of level 0 do not scale with F
    (I - omega / lambda D^-1 F is scale-free) and convert, so the first value that does not fit is one of the Galerkin
    coarse operator R F P, level 1's A.  Three sub-domains: level 0 is the first shard's diagonal block, an operator of its
    own, converted when level 0 is finished.  The scale is a power of two, so scaling back restores F bit for bit: the
    handle must then give the cycle it gave before, to the bit."""
    S = _S()
    pr = problem("ns60")
    b = rng_vec(pr.n_u, 81)
    scale = 2.0 ** 200
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        ls.set_option(S.OPT_SUBDOMAINS, sub)
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        before = ls.tri_apply(S.TRI_VELOCITY, b)
        assert ls.amg_value_bytes() == 4 and len(ls.amg_levels()) >= 3
        ls.scale_values(S.BLK_F, scale)
        ls.set_option(S.OPT_AMG_PRECISION, 64)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 8 and len(ls.amg_levels()) >= 3    # (the double hierarchy stands on these values)
        ls.set_option(S.OPT_AMG_PRECISION, 32)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        msg = r"nsk error -48: NSK_OPT_AMG_PRECISION = 32: \d+ value\(s\) of " + re.escape(where) + " are finite in fp64"
        for call in (ls.amg_value_bytes, lambda: ls.tri_apply(S.TRI_VELOCITY, b), ls.amg_levels):
            with pytest.raises(RuntimeError, match=msg):
                call()
        assert ls.inner_value_bytes(S.BLK_F) == 8
        # the handle recovers from the throw in the middle of the build
        ls.scale_values(S.BLK_F, 1.0 / scale)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 4 and ls.inner_value_bytes(S.BLK_F) == 8
        assert np.array_equal(ls.tri_apply(S.TRI_VELOCITY, b), before)
        # and with the values still out of range, 64 stands where 32 was refused
        ls.scale_values(S.BLK_F, scale)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        with pytest.raises(RuntimeError, match=msg):
            ls.amg_value_bytes()
        ls.set_option(S.OPT_AMG_PRECISION, 64)
        ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY)
        assert ls.amg_value_bytes() == 8 and np.all(np.isfinite(ls.tri_apply(S.TRI_VELOCITY, b)))
    finally:
        ls.close()
