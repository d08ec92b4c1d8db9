"""NSK_OPT_INNER_BASIS_PRECISION = 32: the inner FGMRES on F keeps its Krylov basis in fp32 (include/nsk.h).

Each new kernel runs alone through the test hook nsk_debug_krylov, i.e. through the launchers the solver calls
(Ctx::multi_dot_all_f32, Ctx::multi_axpy_all_f32, vec_equ_f32, arnoldi_column on an fp32 basis):
  * integer-valued data: every coefficient, the updated w and the norm EQUAL the integer sums;
  * random fp32 bases with a double w: within the bounds tests/krylov_f32_reference.py counts from the kernel source
    (1.01 D u sum |w_i v_i| for a sum, D = 4 trips + 48 <= 84; (1.01 m + 1) u (|w| + sum |h_k v_k|) per updated entry);
  * m = 1 .. 30 (a 31st output with the w.w rider), n tiny / odd / even / at the 256-workgroup cap / 8 575 417;
  * no guard word changes (Hook.run asserts it for every call), one launch per sweep in the one-launch setting;
  * the three NSK_IOPT_GS_ONE_LAUNCH settings and a repetition give the same bytes.
Then the option as a whole: the default is untouched bit for bit, the getter and the fallbacks, whole solves held to the
cases and bounds of tests/test_gpu_inner_matrix_precision.py, two ranks on one GPU, one driver run.

The whole solves, the two-rank run and the driver run print their iteration counts (fp64 basis / fp32 basis).  Only
the kernel-alone tests have run on a GPU so far (DESIGN 5l says so): no measured figure is recorded here."""
import ctypes as C
import math
import os
import re
import subprocess
import threading

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from navier_stokes_solver_amd import partition as PT
from navier_stokes_solver_amd import problem as P
from tests import krylov_f32_reference as F
from tests import krylov_reference as R
from tests.util import CASES, problem, rel_err

pytestmark = pytest.mark.gpu

U = R.U
DOT32, AXPY32, COLUMN32, EQU, EQU32 = 16, 17, 18, 19, 20
PAIRS = 2
ONE, CAP16, CHUNKS = 1, 2, 0      # NSK_IOPT_GS_ONE_LAUNCH

SMALL = [1, 2, 3, 5, 1000, 1001, 20_001]       # below one quad, odd, even, three trips with a tail
AT_CAP = 4_194_304                              # 256 workgroups x 1024 threads x 4 trips of one quad: exactly at the cap
PAST_CAP = 4_194_304 + 4099                     # past it, odd, a tail of three
HEADLINE = 8_575_417                            # velocity unknowns at 1200 x 400 (+ 1: odd)


def _S():
    from navier_stokes_solver_amd import solver as S
    return S


class Hook:
    def __init__(self):
        S = _S()
        self.S = S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_krylov.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(self, mode, op, vecs, n, m, par=(), offset=0, pairs=1, rc_want=0):
        """The op on copies of vecs with NSK_IOPT_GS_ONE_LAUNCH = mode; (vectors after, 64 slots, info)."""
        self.ls.set_option(self.S.OPT_BLAS1_PAIRS, pairs)
        self.ls.set_option(self.S.IOPT_GS_ONE_LAUNCH, mode)
        arrs = [np.array(v, dtype=np.float64, copy=True).ravel() for v in vecs]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.int64)
        p = np.zeros(64)
        p[:len(par)] = par
        slots = np.empty(64)
        info = np.zeros(8, dtype=np.int32)
        rc = self.L.nsk_debug_krylov(self.ls.h, op, n, m, offset, p.ctypes.data, len(arrs), ptrs, lens.ctypes.data,
                                     slots.ctypes.data, info.ctypes.data)
        assert rc == rc_want, (rc, self.ls.last_error())
        if rc == 0:
            assert info[3] == 0, f"op {op}, n {n}, m {m}: {info[3]} guard words were written"
        return arrs, slots, info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


_CACHE = {}


def vectors(n, kind, count=30):
    """w (double) and `count` fp32 basis vectors; kind "int": small integers, "rand": normal deviates.  Cached per size."""
    key = (n, kind)
    if key not in _CACHE:
        _CACHE.clear()
        rng = np.random.default_rng(2000 + n % 977)
        if kind == "int":
            w = rng.integers(-50, 51, n).astype(np.float64)
            V = [rng.integers(-20, 21, n).astype(np.float32).astype(np.float64) for _ in range(count)]
        else:
            w = rng.standard_normal(n)
            V = [rng.standard_normal(n).astype(np.float32).astype(np.float64) for _ in range(count)]
        _CACHE[key] = (w, V)
    return _CACHE[key]


def int_coefs(m):
    return [float((k % 7) - 3) for k in range(m)]


def coefs(m):
    return [0.5 - 0.03 * k for k in range(m)]


# ------------------------------------------------------------------ each kernel alone
def _int_case(hook, n, m, mode=ONE, quick=False):
    w, V = vectors(n, "int")
    for rider in ((1,) if quick else (0, 1)):
        _, s, i = hook.run(mode, DOT32, [w] + V[:m], n, m, par=[rider])
        assert i[0] == PAIRS and i[4] == F.launches(mode, m, bool(rider)), (n, m, rider, i[4])
        want = [float(F.int_dot(w, v)) for v in V[:m]] + ([float(F.int_dot(w, w))] if rider else [])
        assert np.array_equal(s[:m + rider], np.array(want)), (n, m, rider, s[:m + rider] - np.array(want))
        assert np.all(np.isnan(s[m + rider:]))          # nothing written past the outputs
    h = int_coefs(m)
    want_w = w - sum(hk * v for hk, v in zip(h, V[:m]))     # integers: exact in any order
    for norm in ((1,) if quick else (1, 0)):
        (w1, *rest), s, i = hook.run(mode, AXPY32, [w] + V[:m], n, m, par=h + [norm])
        assert i[4] == F.launches(mode, m) and (not norm or i[0] == PAIRS)
        assert np.array_equal(w1, want_w), (n, m, norm)
        assert all(same_bytes(a, b) for a, b in zip(rest, V[:m]))      # the basis is only read
        if norm:
            ww = float(F.int_dot(want_w, want_w))
            assert s[m] == ww and abs(s[m + 1] - math.sqrt(ww)) <= 2 * U * math.sqrt(ww), (n, m, s[m], ww)
        else:
            assert np.isnan(s[m])


@pytest.mark.parametrize("n", SMALL)
def test_integer_data_gives_exactly_the_integer_sums_for_every_m(hook, n):
    for m in range(1, 31):
        _int_case(hook, n, m)


def _rand_case(hook, n, m):
    w, V = vectors(n, "rand")
    _, s, i = hook.run(ONE, DOT32, [w] + V[:m], n, m, par=[1])
    assert i[0] == PAIRS and i[4] == 1
    want = F.dots(w, V[:m], rider=True)
    for k, v in enumerate(V[:m] + [w]):
        err, bound = abs(s[k] - want[k]), F.dot_bound(n, w, v)
        assert err <= bound, (n, m, k, s[k], want[k], err / bound)
    h = coefs(m)
    (w1, *_), s, i = hook.run(ONE, AXPY32, [w] + V[:m], n, m, par=h + [1])
    assert i[4] == 1
    ref, scale = F.axpy(w, V[:m], h)
    assert np.all(np.abs(w1 - ref) <= F.axpy_bound(m, scale)), (n, m, np.max(np.abs(w1 - ref) / scale) / U)
    ww = R.exact_dot(w1, w1)
    assert abs(s[m] - ww) <= F.dot_bound(n, w1, w1), (n, m, s[m], ww)
    assert abs(s[m + 1] - math.sqrt(abs(s[m]))) <= 2 * U * math.sqrt(abs(s[m]))


@pytest.mark.parametrize("n", [3, 1001, 20_001])
def test_random_fp32_bases_meet_the_correctly_rounded_sums_within_the_counted_bounds(hook, n):
    for m in (1, 2, 7, 8, 9, 16, 17, 24, 30):
        _rand_case(hook, n, m)


def test_random_data_at_four_trips_per_thread(hook):
    _rand_case(hook, (1 << 20) + 3, 30)


@pytest.mark.parametrize("n", [AT_CAP, PAST_CAP, HEADLINE])
def test_at_the_grid_cap_and_the_headline_size(hook, n):
    """Integer data: exact whatever the number of trips; m = 30 with the rider; at the headline size the three settings
    give the same bytes of a whole column."""
    _int_case(hook, n, 30, quick=True)
    if n != HEADLINE:
        return
    w, V = vectors(n, "int")
    outs = []
    for mode in (ONE, CAP16, CHUNKS):
        (w1, *_), s, i = hook.run(mode, COLUMN32, [w] + V, n, 30, par=[2])
        assert i[4] == F.launches(mode, 30, True) + F.launches(mode, 30)
        outs.append((w1, s[:32]))
    assert all(same_bytes(o[0], outs[0][0]) and same_bytes(o[1], outs[0][1]) for o in outs[1:])


def test_unaligned_w_and_the_8_byte_forms_have_no_fp32_form(hook):
    """The solver never gets here (its vectors are allocations of their own, and it keeps the double basis with the 8-byte
    forms); the launchers refuse instead of reading 16 bytes from an address that is not a multiple of 16."""
    w, V = vectors(1001, "rand")
    hook.run(ONE, DOT32, [w] + V[:9], 1001, 9, par=[0], offset=1, rc_want=-61)
    hook.run(ONE, AXPY32, [w] + V[:9], 1001, 9, par=coefs(9) + [1], offset=1, rc_want=-61)
    hook.run(ONE, COLUMN32, [w] + V[:9], 1001, 9, par=[1], pairs=0, rc_want=-61)
    bad = [v + 1e-9 for v in V[:2]]                           # not fp32 values
    hook.run(ONE, DOT32, [w] + bad, 1001, 2, par=[0], rc_want=-61)


# ------------------------------------------------------------------ normalise-and-store
@pytest.mark.parametrize("n", [1, 5, 1001, 20_001])
def test_normalise_stores_the_rounded_vector_and_the_same_value_widened(hook, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    a = float(np.linalg.norm(x))
    nan = np.full(n, np.nan)
    (_, y), _, _ = hook.run(ONE, EQU, [x, nan], n, 0, par=[a])
    (x1, v, vw), _, _ = hook.run(ONE, EQU32, [x, np.zeros(n), nan], n, 0, par=[a])
    y_ref, v_ref, vw_ref = F.normalise(x, a)
    assert same_bytes(y, y_ref)                               # what the fp64 path stores for this input
    assert same_bytes(v.astype(np.float32), y.astype(np.float32)), n     # fl32 of it, to nearest even, bit for bit
    assert same_bytes(vw, v) and same_bytes(vw, vw_ref) and same_bytes(x1, x)
    assert n == 1 or np.any(vw != y)                          # (it did round; n = 1: x / |x| is +-1, an fp32 value)


# ------------------------------------------------------------------ same bits between the settings, and on repetition
@pytest.mark.parametrize("n", [1001, 20_000, (1 << 20) + 1])
def test_the_three_launch_settings_and_a_repetition_give_the_same_bytes(hook, n):
    w, V = vectors(n, "rand")
    for m in ((1, 7, 8, 9, 16, 17, 30) if n < (1 << 20) else (9, 30)):
        h = coefs(m)
        runs = []
        for mode in (ONE, ONE, CAP16, CHUNKS):
            out = []
            for rider in (0, 1):
                _, s, i = hook.run(mode, DOT32, [w] + V[:m], n, m, par=[rider])
                assert i[4] == F.launches(mode, m, bool(rider)), (n, m, mode, rider, i[4])
                out.append(s[:m + rider])
            for norm in (1, 0):
                (w1, *_), s, i = hook.run(mode, AXPY32, [w] + V[:m], n, m, par=h + [norm])
                assert i[4] == F.launches(mode, m)
                out += [w1, s[:m + 2]]
            for gs in (1, 2):
                (w1, *_), s, i = hook.run(mode, COLUMN32, [w] + V[:m], n, m, par=[gs])
                assert i[4] == F.launches(mode, m, gs == 2) + F.launches(mode, m), (n, m, mode, gs, i[4])
                out += [w1, s[:m + 2]]
            runs.append(out)
        for k, other in enumerate(runs[1:]):
            assert all(same_bytes(a, b) for a, b in zip(other, runs[0])), (n, m, k)


@pytest.mark.parametrize("gs", [1, 2], ids=["cgs", "one_red"])
def test_the_arnoldi_column_on_an_fp32_basis_meets_its_reference(hook, gs):
    n, m = 20_001, 12
    V = [F.round_f32(v) for v in R.orthonormal_basis(n, m)]
    w = np.random.default_rng(3).standard_normal(n)
    (w1, *_), s, i = hook.run(ONE, COLUMN32, [w] + V, n, m, par=[gs])
    assert i[4] == 2 and i[0] == PAIRS
    want = F.dots(w, V)
    for k in range(m):
        assert abs(s[k] - want[k]) <= F.dot_bound(n, w, V[k]), (k, s[k], want[k])
    ref, scale = F.axpy(w, V, s[:m])                          # the update with the coefficients the sweep produced
    assert np.all(np.abs(w1 - ref) <= F.axpy_bound(m, scale))
    if gs == 1:
        ww = R.exact_dot(w1, w1)
        assert abs(s[m] - ww) <= F.dot_bound(n, w1, w1)
    else:
        ww0 = R.exact_dot(w, w)
        q, _ = R.pythagoras(s[:m], ww0)
        assert abs(s[m] - q) <= F.dot_bound(n, w, w) + (m + 2) * U * ww0
    assert abs(s[m + 1] - math.sqrt(s[m])) <= 2 * U * math.sqrt(s[m])


# ------------------------------------------------------------------ the option
def _resident(S, pr, opts, outer=8):
    """FGMRES + stationary aSIMPLE, `outer` outer steps; opts: values of the option set before each of the set-ups."""
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_problem(pr)
        for o in opts:
            if o is not None:
                ls.set_option(S.OPT_INNER_BASIS_PRECISION, o)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        width = ls.inner_basis_bytes()
        ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
        its, res, rc = ls.solve_resident(S.FGMRES, 0.0, outer)
        xu, xp = ls.download_solution()
        return [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])], width, ls.stats()
    finally:
        ls.close()


def test_the_default_is_untouched_bit_for_bit():
    """Never set, set to 64, and 32 -> set-up -> 64 -> set-up: residual history and solution of FGMRES + aSIMPLE at 60 x 20
    are the same bytes; with 32 they are not (the option does something)."""
    S = _S()
    pr = P.generate(60, 20, nu=1.0 / 90.0)
    unset, w0, _ = _resident(S, pr, [None])
    at64, w1, _ = _resident(S, pr, [64])
    back, w2, _ = _resident(S, pr, [32, 64])
    on, w3, st = _resident(S, pr, [32])
    assert (w0, w1, w2, w3) == (8, 8, 8, 4)
    for other in (at64, back):
        for k, (a, b) in enumerate(zip(other, unset)):
            assert same_bytes(a, b), f"item {k}"
    assert not same_bytes(on[2], unset[2])


def test_the_getter_and_the_fallbacks():
    S = _S()
    pr = problem("ns16")
    ls = S.LinearSolver()
    try:
        ls.set_problem(pr)
        with pytest.raises(RuntimeError, match="-46"):
            ls.inner_basis_bytes()                            # no set-up yet
        for v in (16, 0, 33, 128):
            with pytest.raises(RuntimeError, match="-61"):
                ls.set_option(S.OPT_INNER_BASIS_PRECISION, v)
        ls.set_option(S.OPT_INNER_BASIS_PRECISION, 32)
        for prec in (S.BLOCK_DIAGONAL, S.BLOCK_TRIANGULAR, S.ASIMPLE):
            ls.setup_preconditioner(prec, S.STATIONARY, 0.5)
            assert ls.inner_basis_bytes() == 4, prec
        ls.setup_preconditioner(S.ASIMPLE, S.UNSTEADY, 0.5)
        assert ls.inner_basis_bytes() == 0                    # ILU applies only: no inner FGMRES on F
        ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.UNSTEADY, 0.5)
        assert ls.inner_basis_bytes() == 8                    # the unsteady variant's 8-byte reduction forms
        ls.set_option(S.OPT_BLAS1_PAIRS, 1)
        ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.UNSTEADY, 0.5)
        assert ls.inner_basis_bytes() == 4
        ls.set_option(S.OPT_BLAS1_PAIRS, 0)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.inner_basis_bytes() == 8
        ls.set_option(S.OPT_BLAS1_PAIRS, -1)
        ls.set_option(S.OPT_INNER_FUSED_GS, 0)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.inner_basis_bytes() == 8                    # modified Gram-Schmidt keeps the double basis
        for gs in (1, 2):
            ls.set_option(S.OPT_INNER_FUSED_GS, gs)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            assert ls.inner_basis_bytes() == 4
        ls.set_option(S.OPT_INNER_BASIS_PRECISION, 64)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.inner_basis_bytes() == 8
    finally:
        ls.close()


def test_the_fallbacks_solve_with_the_bits_of_the_double_basis():
    """NSK_OPT_INNER_FUSED_GS = 0 and NSK_OPT_BLAS1_PAIRS = 0 with the option at 32: the solve is the option-64 solve."""
    S = _S()
    pr = P.generate(60, 20, nu=1.0 / 90.0)
    for opt, val in ((S.OPT_INNER_FUSED_GS, 0), (S.OPT_BLAS1_PAIRS, 0)):
        outs = []
        for bits in (64, 32):
            ls = S.LinearSolver()
            try:
                ls.set_option(opt, val)
                ls.set_option(S.OPT_INNER_BASIS_PRECISION, bits)
                ls.set_problem(pr)
                ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
                assert ls.inner_basis_bytes() == 8
                ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
                ls.solve_resident(S.FGMRES, 0.0, 5)
                outs.append(list(ls.download_solution()) + [ls.history()])
            finally:
                ls.close()
        assert all(same_bytes(a, b) for a, b in zip(*outs)), opt


@pytest.mark.parametrize("gs", [1, 2], ids=["cgs", "one_red"])
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_fgmres_with_an_fp32_inner_basis_converges_to_the_same_solution(prec, gs):
    """ns16, stationary, tol 1e-12, the bounds tests/test_gpu_inner_matrix_precision.py holds its option to: rc 0, true
    residual <= 1.05 tol, solution within 2e-8 of the sparse-direct one, outer iterations within max(3, 10 %) of the fp64
    run on the same handle."""
    S = _S()
    pr = problem("ns16")
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    xs = spl.splu(J).solve(b)
    tol = 1e-12
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_INNER_FUSED_GS, gs)
        ls.set_problem(pr)
        its, inner = {}, {}
        for bits in (64, 32):
            ls.set_option(S.OPT_INNER_BASIS_PRECISION, bits)
            ls.setup_preconditioner(prec, S.STATIONARY, 0.5)
            assert ls.inner_basis_bytes() == bits // 8
            ls.reset_stats()
            xu, xp, it, res, rc = ls.solve(1, tol, 20000, pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
            x = np.concatenate([xu, xp])
            its[bits], inner[bits] = it, ls.stats()["inner_u_its"]
            print(f"ITERATIONS ns16 prec {prec} gs {gs} basis fp{bits}: outer {it}, inner on F {inner[bits]}, "
                  f"true residual {np.linalg.norm(b - J @ x):.3e}, error {rel_err(x, xs):.3e}")
            assert rc == 0, (bits, rc)
            assert np.linalg.norm(b - J @ x) <= 1.05 * tol, bits
            assert rel_err(x, xs) <= 2e-8, bits
        assert abs(its[32] - its[64]) <= max(3, 0.1 * its[64]), its
    finally:
        ls.close()


def test_two_ranks_on_one_gpu():
    """Two local-group rank threads: the coefficients go through the all-reduce, every rank reads its own fp32 basis; the
    same solution as the one-rank run, to the tolerance of the whole solves."""
    S = _S()
    world = 2
    case = CASES["ns16"]
    pr = problem("ns16")
    parts = [P.generate(**case, nranks=world, rank=r) for r in range(world)]
    plans = [{S.SPACE_U: PT.build_halo_plan(r, parts[0].u_ranges, [p.ghost_u for p in parts]),
              S.SPACE_P: PT.build_halo_plan(r, parts[0].p_ranges, [p.ghost_p for p in parts])} for r in range(world)]
    uid = S.local_group_id(world, True)
    res, errs = [None] * world, []
    done = threading.Barrier(world, timeout=300)

    def run(r):
        try:
            p = parts[r]
            ls = S.LinearSolver(r, world, 0, uid)
            ls.set_option(S.OPT_INNER_BASIS_PRECISION, 32)
            ls.set_problem(p, plans[r])
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            width = ls.inner_basis_bytes()
            su, sp_, its, fres, rc = ls.solve(S.FGMRES, 1e-12, 20000, p.rhs_u, p.rhs_p, p.x0_u, p.x0_p)
            res[r] = dict(su=su, sp=sp_, its=its, rc=rc, width=width)
            done.wait()   # (a destroyed handle takes its group down: no rank leaves while a peer is still inside)
            ls.close()
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(300) for t in th]
    assert not errs, errs
    assert all(o is not None and o["rc"] == 0 and o["width"] == 4 for o in res), res
    assert len({o["its"] for o in res}) == 1
    x2 = np.concatenate([o["su"] for o in res] + [o["sp"] for o in res])
    one = S.LinearSolver()
    try:
        one.set_option(S.OPT_INNER_BASIS_PRECISION, 32)
        one.set_problem(pr)
        one.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        xu, xp, it1, _, rc = one.solve(S.FGMRES, 1e-12, 20000, pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    finally:
        one.close()
    x1 = np.concatenate([xu, xp])
    J = pr.jacobian_scipy().tocsc()
    b = np.concatenate([pr.rhs_u, pr.rhs_p])
    print(f"TWO RANKS ns16 aSIMPLE fp32 basis: outer {res[0]['its']} (two ranks) / {it1} (one rank)")
    assert rc == 0 and np.linalg.norm(b - J @ x2) <= 1.05e-12
    assert rel_err(x2, x1) <= 2e-8 and rel_err(x2, spl.splu(J).solve(b)) <= 2e-8


def _newton_run(env_extra):
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navier_stokes_solver_amd", "bin",
                       "StationaryNSSolver")
    env = dict(os.environ)
    for k in ("NSK_INNER_BASIS_PRECISION", "NSK_INNER_MATRIX_PRECISION", "NSK_FACTOR_PRECISION"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([exe, "-m", "16,10", "-r", "10", "-p", "2"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    res = [float(v) for v in re.findall(r"Newton iteration \d+/\d+ - \|\|r\|\| = ([-+.0-9eE]+)", out.stdout)]
    return out.stdout, res


def test_driver_with_an_fp32_inner_basis():
    """NSK_INNER_BASIS_PRECISION=32 StationaryNSSolver -m 16,10 -r 10 -p 2: the [nsk] line, the same Newton steps, the
    same end; a value the switch does not know is ignored."""
    out64, r64 = _newton_run({})
    out32, r32 = _newton_run({"NSK_INNER_BASIS_PRECISION": "32"})
    outxx, rxx = _newton_run({"NSK_INNER_BASIS_PRECISION": "16"})
    line = "[nsk] NSK_INNER_BASIS_PRECISION=32: inner FGMRES basis on F stored in fp32 (deviation from the reference)"
    assert line in out32 and line not in out64 and line not in outxx
    assert r64 and r32 and len(rxx) == len(r64) and abs(rxx[-1] - r64[-1]) <= 1e-8 * max(r64)
    print(f"NEWTON fp64 {len(r64)} steps, last ||r|| {r64[-1]:.6e}; fp32 basis {len(r32)} steps, last ||r|| {r32[-1]:.6e}")
    assert len(r32) == len(r64)
    assert abs(r32[-1] - r64[-1]) <= 1e-8 * max(r64), (r64[-1], r32[-1])
