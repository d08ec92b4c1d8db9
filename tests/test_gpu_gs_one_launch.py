"""The fused Gram-Schmidt sweeps and FGMRES' cycle-end update in ONE launch each over the whole basis (DESIGN 5j;
NSK_IOPT_GS_ONE_LAUNCH): multi_dot2_all_kernel, multi_axpy2_all_kernel and multi_add2_kernel against the chunked launches
they replace (eight basis vectors per launch; one vec_axpy per term).  The one-launch forms keep the grid, the trips and
the order of the operations per accumulator and per entry, so everything here compares BYTES between the option on (1),
capped at 16 vectors per launch (2) and off (0): every coefficient, the norm and its root, the updated w and x — for
every m = 1 .. 30 (31 for the coefficient sweep: w.w rides along as one more "basis vector" when NSK_OPT_INNER_FUSED_GS = 2),
for n tiny (less than one trip of one workgroup), even and odd, with paired trips and single trailing trips, at the
256-workgroup cap and at the headline velocity size; then whole FGMRES + aSIMPLE solves.  Each case asserts which kernels
ran (the hook reports the reduction forms and the number of launches): an unaligned vector and the 8-byte forms must
take the chunked fallback.

The one-launch results are also held to the exact references and the bounds of tests/test_gpu_krylov_kernels.py (see
its docstring for where they come from): |s - exact| <= 64 u sum |w_i v_i| for a coefficient and the norm at n <= 2^20
(the per-thread chain is multi_dot2_kernel's, 8 products at 2^20), and (m + 2) u (|w| + sum_k |h_k| |v_k|) per entry of
an update of m terms (each of the m + 1 operations rounds once, or fuses)."""
import ctypes as C
import math

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from tests import krylov_reference as R

pytestmark = pytest.mark.gpu

U = R.U
GS_COLUMN, MULTI_DOT_ALL, MULTI_AXPY_ALL, MULTI_ADD = 7, 13, 14, 15
SCALAR, PAIRS = 1, 2
ONE, CAP16, CHUNKS = 1, 2, 0      # NSK_IOPT_GS_ONE_LAUNCH

# tiny: below one workgroup's trip (1024 pairs); 20 000 / 20 001: 3 workgroups, paired trips and a single trailing trip
SIZES = [2, 3, 1000, 1001, 20_000, 20_001]
BIG = [(1 << 20) - 1, 1 << 20]                # 128 workgroups, 4 trips: the largest size the 64 u bound covers
CAP = 2_097_153 + 4096                        # past the 256-workgroup cap, odd
HEADLINE = 8_575_417                          # velocity unknowns at 1200 x 400 (+ 1: odd)


class Hook:
    def __init__(self):
        from navier_stokes_solver_amd import solver as S
        self.S = S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_krylov.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(self, mode, op, vecs, n, m, offset=0, par=(), pairs=1):
        """Runs the op on copies of vecs with NSK_IOPT_GS_ONE_LAUNCH = mode; (vectors after, 64 slots, info)."""
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
        assert rc == 0, (rc, self.ls.last_error())
        assert info[3] == 0, f"op {op}, n {n}, m {m}, offset {offset}: {info[3]} guard words were written"
        return arrs, slots, info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def chunks(m, per):
    return (m + per - 1) // per


def launches(mode, m, one_launch_applies, chunk=8):
    """Launches Ctx::multi_dot_all / multi_axpy_all must have made (chunk = 1: multi_add, one vec_axpy per term)."""
    if mode == CHUNKS or not one_launch_applies:
        return chunks(m, chunk)
    if chunk == 1:
        return chunks(m, 32 if mode == ONE else 16)
    # a piece of <= 8 vectors is one launch of the chunked kernel either way
    return 1 if mode == ONE else chunks(m, 16)


_CACHE = {}


def vectors(n, count=32):
    """w and `count` basis vectors, random; cached per n (the largest sizes are built once)."""
    if n not in _CACHE:
        _CACHE.clear()
        rng = np.random.default_rng(1000 + n % 977)
        _CACHE[n] = (rng.standard_normal(n), [rng.standard_normal(n) for _ in range(count)])
    return _CACHE[n]


def coefs(m):
    return [0.5 - 0.03 * k for k in range(m)]


# ------------------------------------------------------------------ the three kernels alone
def _dot(hook, n, m, exact):
    w, V = vectors(n)
    vv = V[:m - 1] + [w] if m == 31 else V[:m]      # 31: the w.w rider of NSK_OPT_INNER_FUSED_GS = 2 behind 30 vectors
    _, s0, i0 = hook.run(CHUNKS, MULTI_DOT_ALL, [w] + vv, n, m)
    assert i0[0] == PAIRS and i0[4] == chunks(m, 8)
    for mode in (ONE, CAP16):
        _, s1, i1 = hook.run(mode, MULTI_DOT_ALL, [w] + vv, n, m)
        assert i1[0] == PAIRS and i1[4] == launches(mode, m, True), (n, m, mode, i1[4])
        assert same_bytes(s1[:m], s0[:m]), (n, m, mode, s1[:m] - s0[:m])
        assert np.all(np.isnan(s1[m:]))             # nothing written past the m outputs
    if exact:
        for k in range(m):
            want, scale = R.exact_dot(w, vv[k]), R.abs_dot(w, vv[k])
            assert abs(s1[k] - want) <= 64 * U * scale, (n, m, k, s1[k], want)


def _axpy(hook, n, m, exact):
    w, V = vectors(n)
    h = coefs(m)
    for norm in (1, 0):
        (w0, *_), s0, i0 = hook.run(CHUNKS, MULTI_AXPY_ALL, [w] + V[:m], n, m, par=h + [norm])
        assert i0[0] == PAIRS and i0[4] == chunks(m, 8)
        for mode in (ONE, CAP16):
            (w1, *rest), s1, i1 = hook.run(mode, MULTI_AXPY_ALL, [w] + V[:m], n, m, par=h + [norm])
            assert i1[0] == PAIRS and i1[4] == launches(mode, m, True), (n, m, mode, i1[4])
            assert same_bytes(w1, w0), (n, m, norm, mode, np.flatnonzero(w1 != w0)[:5])
            assert all(same_bytes(a, b) for a, b in zip(rest, V[:m]))          # the basis is only read
            assert same_bytes(s1[:m + 2], s0[:m + 2]), (n, m, norm, mode)      # h as given; the norm and its root, or NaN
            assert np.isnan(s1[m]) == (norm == 0)
    if exact:
        ref, scale = w.copy(), np.abs(w)
        for hk, v in zip(h, V[:m]):
            ref = ref - hk * v
            scale = scale + abs(hk) * np.abs(v)
        assert np.all(np.abs(w1 - ref) <= (m + 2) * U * scale), (n, m)
        (wn, *_), s, _ = hook.run(ONE, MULTI_AXPY_ALL, [w] + V[:m], n, m, par=h + [1])
        ww = R.exact_dot(wn, wn)
        assert abs(s[m] - ww) <= 64 * U * ww, (n, m, s[m], ww)
        assert abs(s[m + 1] - math.sqrt(abs(s[m]))) <= 2 * U * math.sqrt(abs(s[m]))


def _add(hook, n, m, exact):
    x, Z = vectors(n)
    y = coefs(m)
    (x0, *_), _, i0 = hook.run(CHUNKS, MULTI_ADD, [x] + Z[:m], n, m, par=y)
    assert i0[4] == m
    for mode in (ONE, CAP16):
        (x1, *rest), _, i1 = hook.run(mode, MULTI_ADD, [x] + Z[:m], n, m, par=y)
        assert i1[4] == launches(mode, m, True, chunk=1), (n, m, mode, i1[4])
        assert same_bytes(x1, x0), (n, m, mode, np.flatnonzero(x1 != x0)[:5])
        assert all(same_bytes(a, b) for a, b in zip(rest, Z[:m]))
    if exact:
        ref, scale = x.copy(), np.abs(x)
        for yj, z in zip(y, Z[:m]):
            ref = ref + yj * z
            scale = scale + abs(yj) * np.abs(z)
        assert np.all(np.abs(x1 - ref) <= (m + 2) * U * scale), (n, m)


@pytest.mark.parametrize("n", SIZES)
def test_every_m_has_the_bytes_of_the_chunked_launches_and_meets_the_exact_references(hook, n):
    for m in range(1, 32):
        _dot(hook, n, m, exact=True)
        if m <= 30:
            _axpy(hook, n, m, exact=True)
            _add(hook, n, m, exact=True)


@pytest.mark.parametrize("n", BIG)
def test_four_trips_per_thread_same_bytes_and_exact_references(hook, n):
    for m in (9, 16, 17, 24, 30, 31):
        _dot(hook, n, m, exact=(m == 30))
        if m <= 30:
            _axpy(hook, n, m, exact=(m == 30))
            _add(hook, n, m, exact=(m == 30))


@pytest.mark.parametrize("n", [CAP, HEADLINE])
def test_at_the_grid_cap_and_the_headline_size_same_bytes(hook, n):
    for m in ((12, 23, 31) if n == CAP else (30,)):
        _dot(hook, n, m, exact=False)
        _axpy(hook, n, min(m, 30), exact=False)
        _add(hook, n, min(m, 30), exact=False)


@pytest.mark.parametrize("n", [3, 1001, 20_000])
@pytest.mark.parametrize("offset,pairs", [(1, 1), (0, 0)], ids=["unaligned", "8-byte-forms"])
def test_unaligned_vectors_and_the_8_byte_forms_take_the_chunked_fallback(hook, n, offset, pairs):
    """Vectors 8 bytes off a 16-byte boundary, or NSK_OPT_BLAS1_PAIRS = 0: no one-launch form; the chunked launches run
    (the scalar reductions; the update without a norm still in pairs where aligned) and give the bytes of option 0."""
    w, V = vectors(n)
    for m in (9, 17, 30):
        h = coefs(m)
        for mode in (ONE, CAP16):
            _, s0, _ = hook.run(CHUNKS, MULTI_DOT_ALL, [w] + V[:m], n, m, offset=offset, pairs=pairs)
            _, s1, i1 = hook.run(mode, MULTI_DOT_ALL, [w] + V[:m], n, m, offset=offset, pairs=pairs)
            assert i1[0] == SCALAR and i1[4] == chunks(m, 8) and same_bytes(s1[:m], s0[:m])
            for k in range(m):
                assert abs(s1[k] - R.exact_dot(w, V[k])) <= 64 * U * R.abs_dot(w, V[k])
            (w0, *_), s0, _ = hook.run(CHUNKS, MULTI_AXPY_ALL, [w] + V[:m], n, m, offset=offset, par=h + [1], pairs=pairs)
            (w1, *_), s1, i1 = hook.run(mode, MULTI_AXPY_ALL, [w] + V[:m], n, m, offset=offset, par=h + [1], pairs=pairs)
            # (pairs = 0, aligned: the chunks without the norm are entry-by-entry updates and run in pairs; the one with the norm is scalar)
            assert i1[0] & SCALAR and i1[4] == chunks(m, 8)
            assert same_bytes(w1, w0) and same_bytes(s1[:m + 2], s0[:m + 2])
            (x0, *_), _, _ = hook.run(CHUNKS, MULTI_ADD, [w] + V[:m], n, m, offset=offset, par=h, pairs=pairs)
            (x1, *_), _, i1 = hook.run(mode, MULTI_ADD, [w] + V[:m], n, m, offset=offset, par=h, pairs=pairs)
            # (the cycle-end update has no reduction: aligned vectors take the one launch whatever the reductions' form)
            assert i1[4] == (m if offset else launches(mode, m, True, chunk=1)) and same_bytes(x1, x0)


@pytest.mark.parametrize("gs", [1, 2], ids=["cgs", "one_red"])
def test_the_arnoldi_column_is_the_same_bytes_and_one_launch_per_sweep(hook, gs):
    for n in (1001, 20_000, (1 << 20) + 1):
        w, V = vectors(n)
        for m in (1, 8, 9, 16, 17, 30):
            (w0, *_), s0, i0 = hook.run(CHUNKS, GS_COLUMN, [w] + V[:m], n, m, par=[gs])
            (w1, *_), s1, i1 = hook.run(ONE, GS_COLUMN, [w] + V[:m], n, m, par=[gs])
            mm = m + (gs == 2)
            assert i0[4] == chunks(mm, 8) + chunks(m, 8)
            assert i1[4] == 2, (n, m, i1[4])
            assert same_bytes(w1, w0) and same_bytes(s1[:m + 2], s0[:m + 2]), (n, m, gs)


# ------------------------------------------------------------------ whole solves
def _solve(S, pr, mode, gs, outer=6):
    ls = S.LinearSolver()
    try:
        ls.set_option(S.OPT_TRI_ORDERING, 1)
        ls.set_option(S.OPT_INNER_FUSED_GS, gs)
        ls.set_option(S.IOPT_GS_ONE_LAUNCH, mode)
        ls.set_problem(pr)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
        its, res, rc = ls.solve_resident(S.FGMRES, 0.0, outer)
        xu, xp = ls.download_solution()
        st = ls.stats()
        return [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])], st
    finally:
        ls.close()


@pytest.mark.parametrize("gs", [1, 2], ids=["cgs", "one_red"])
@pytest.mark.parametrize("mesh", [(60, 20), (300, 100)], ids=["60x20", "300x100"])
def test_a_whole_solve_is_the_same_bytes_with_the_option_on_and_off(mesh, gs):
    """FGMRES + aSIMPLE on one rank: residual history, solution, iteration counts.  The counted BLAS-1 bytes must drop
    (the inner solves on F pass 8 basis vectors, so the one-launch sweeps ran, and every cycle ends in one update)."""
    from navier_stokes_solver_amd import solver as S
    pr = P.generate(*mesh, nu=1.0 / 90.0)
    on, st1 = _solve(S, pr, ONE, gs)
    off, st0 = _solve(S, pr, CHUNKS, gs)
    for k, (a, b) in enumerate(zip(on, off)):
        assert same_bytes(a, b), f"item {k}"
    assert len(on[2]) >= 6 + 1
    assert st1["inner_u_its"] == st0["inner_u_its"] and st1["inner_p_its"] == st0["inner_p_its"]
    print(f"\n{mesh} gs={gs}: inner F its {st1['inner_u_its']}, applies {st1['prec_applies']}, "
          f"BLAS-1 bytes {st1['blas1_bytes']:.4e} (one launch) / {st0['blas1_bytes']:.4e} (chunks)")
    assert st1["blas1_bytes"] < st0["blas1_bytes"]
