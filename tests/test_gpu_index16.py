"""16-bit column offsets in the scalar stream kernels of S and M_p (NSK_IOPT_INDEX16): the SpMV and both
halves of the triangular factor read `base of the run + uint16 offset` instead of an int32 column id.  The arithmetic is
untouched, so everything here compares BYTES: the new SpMV form against NSK_DBG_SPMV_STREAM on the irregular patterns of
tests/spmv_reference.py, the ILU(S) apply and whole FGMRES + aSIMPLE solves with the option on against the option off,
and the qualification rule at its edge (a run spanning 65 535 columns is taken, 65 536 refused).  The one bound in this
file is that rule's 65 535 = 2^16 - 1, the largest offset a uint16 holds."""
import ctypes as C

import numpy as np
import pytest

from navier_stokes_solver_amd import problem as P
from tests import spmv_reference as M

pytestmark = pytest.mark.gpu

STREAM, STREAM_F32, STREAM_I16, STREAM_I16_F32 = 1, 2, 11, 12
REFUSED_WIDE = 5


class Mat(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_own_cols", C.c_int32), ("pad_", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("x_own", C.c_void_p),
                ("x_ghost", C.c_void_p)]


class Hook:
    """nsk_debug_spmv (nsk_internal.h): one launch of one form on copies of the operands."""

    def __init__(self):
        from navier_stokes_solver_amd import solver as S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_spmv.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]

    def run(self, form, A, x, y, mode=0, z=None, runs=None):
        """(y after, info) or (None, info) when the plan refuses the form; no guard word may have changed."""
        xo, xg = (np.ascontiguousarray(v, dtype=np.float64) for v in x)
        ma = Mat(A.n_rows, A.n_cols, A.n_own, 0, A.rowptr.ctypes.data, A.col.ctypes.data, A.val.ctypes.data,
                 xo.ctypes.data, xg.ctypes.data)
        zz = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
        yy = np.array(y, dtype=np.float64, copy=True)
        info = np.zeros(16, dtype=np.int32)
        c0, c1 = runs if runs is not None else (-1, -1)
        rc = self.L.nsk_debug_spmv(self.ls.h, form, 0, mode, 0, c0, c1, C.byref(ma), None, yy.ctypes.data,
                                   None if zz is None else zz.ctypes.data, None, None, None, 0, info.ctypes.data)
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


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


PATTERNS = M.scalar_patterns()


def run_spans(A):
    """max column - min column of every run of the stream plan (runs without entries: 0)."""
    rb = M.stream_plan(A)["rb"]
    out = []
    for b in range(len(rb) - 1):
        c = A.col[A.rowptr[rb[b]]:A.rowptr[rb[b + 1]]]
        out.append(int(c.max()) - int(c.min()) if len(c) else 0)
    return out


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_spmv_on_16_bit_offsets_has_the_bits_of_the_int32_form(hook, name):
    """Empty rows, rows at the run cap, odd and even row pointers (a run that starts on an odd entry reads its pairs of
    offsets 2-byte aligned), ghost columns inside a run's span; every mode; sub-ranges of the plan; the fp32 values."""
    A = M.real_values(PATTERNS[name], 3)
    x = M.real_x(A, 4)
    rng = np.random.default_rng(5)
    y, z = rng.uniform(-1, 1, A.n_rows), rng.uniform(-1, 1, A.n_rows)
    want, info = hook.run(STREAM, A, x, y)
    if want is None:     # a row above the run cap: no stream plan at all, for either index width
        got, info16 = hook.run(STREAM_I16, A, x, y)
        assert got is None and info16[15] == info[15] == 1
        return
    assert max(run_spans(A)) <= 65535      # every pattern of the generator qualifies (at most 20 000 columns)
    for mode, zz in ((0, None), (1, None), (1, z), (2, z)):
        want, info = hook.run(STREAM, A, x, y, mode=mode, z=zz)
        got, info16 = hook.run(STREAM_I16, A, x, y, mode=mode, z=zz)
        assert got is not None, f"{name}: refused with reason {info16[15]}"
        assert info16[1] == info[1] and list(info16[5:13]) == list(info[5:13])      # same VEC, same plan
        assert same_bytes(got, want), f"{name} mode {mode}"
    nb = int(info[8])
    for c0, c1 in ((0, nb // 2), (nb // 2, nb), (1, max(1, nb - 1))):
        if c0 <= c1 <= nb:
            want, _ = hook.run(STREAM, A, x, y, runs=(c0, c1))
            got, _ = hook.run(STREAM_I16, A, x, y, runs=(c0, c1))
            assert same_bytes(got, want), f"{name} runs [{c0}, {c1})"
    want, _ = hook.run(STREAM_F32, A, x, y)
    got, _ = hook.run(STREAM_I16_F32, A, x, y)
    assert same_bytes(got, want), f"{name} fp32 values"


def _two_rows(span, odd_start):
    """One run of two or three rows whose columns span exactly `span`; odd_start: a one-entry row in front, so that the
    wide rows start on an odd entry."""
    n_cols = 70000
    lo = 1234
    rows = ([[lo + 7]] if odd_start else []) + [[lo, lo + 1, lo + 5], [lo + 2, lo + span]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    A = M.Csr(len(rows), n_cols, rp, np.concatenate(rows), None, n_cols, name=f"span_{span}_{int(odd_start)}")
    return M.real_values(A, 6)


@pytest.mark.parametrize("odd_start", [False, True])
def test_a_run_spanning_65535_columns_is_taken_and_65536_is_refused(hook, odd_start):
    for span, taken in ((65535, True), (65536, False)):
        A = _two_rows(span, odd_start)
        assert run_spans(A) == [span]
        x = M.real_x(A, 7)
        y = np.zeros(A.n_rows)
        want, _ = hook.run(STREAM, A, x, y)
        assert want is not None
        exact, mag = M.exact_row_sums(A, *x)      # the int32 form runs correctly: at most 3 roundings per row of <= 3 terms
        assert np.all(np.abs(want - exact) <= 3 * M.U * mag)
        got, info = hook.run(STREAM_I16, A, x, y)
        if taken:
            assert same_bytes(got, want)
        else:
            assert got is None and info[15] == REFUSED_WIDE


# ------------------------------------------------------------------ on a handle: ILU(S) applies and whole solves
def _handle(S, pr, index16, sync_free, fault=0, factor_bits=64, inner_bits=64):
    ls = S.LinearSolver()
    ls.set_option(S.OPT_TRI_ORDERING, 1)
    ls.set_option(S.IOPT_TINY_BYTES, 0)       # the streamed kernels on small meshes too
    ls.set_option(S.IOPT_INDEX16, index16)
    ls.set_option(S.OPT_TRI_SYNC_FREE, sync_free)
    ls.set_option(S.IOPT_FAULT_INJECT, fault)
    ls.set_option(S.OPT_FACTOR_PRECISION, factor_bits)
    ls.set_option(S.OPT_INNER_MATRIX_PRECISION, inner_bits)
    ls.set_problem(pr)
    ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
    return ls


def _results(S, pr, index16, sync_free, fault=0, factor_bits=64, inner_bits=64, outer=8):
    ls = _handle(S, pr, index16, sync_free, fault, factor_bits, inner_bits)
    try:
        widths = ls.index_width(S.BLK_S)
        out = []
        if not fault:      # (a single apply has no fallback: the injected fault is met inside the solve below)
            out += [ls.tri_apply(S.TRI_PRESSURE, np.random.default_rng(60 + k).uniform(-1, 1, pr.n_p)) for k in range(2)]
            out.append(ls.inner_spmv(S.BLK_S, np.random.default_rng(70).uniform(-1, 1, pr.n_p)))
        before = ls.stats()["sync_free_fallbacks"]
        ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
        its, res, rc = ls.solve_resident(S.FGMRES, 0.0, outer)
        xu, xp = ls.download_solution()
        out += [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])]
        return widths, out, ls.stats()["sync_free_fallbacks"] - before
    finally:
        ls.close()


@pytest.fixture(scope="module", params=[(100, 70), (300, 100)], ids=["100x70", "300x100"])
def mesh(request):
    return P.generate(*request.param, nu=1.0 / 90.0)


# single launch per half; one launch per colour; the single launch with its upper half walking backwards
# (NSK_IOPT_FAULT_INJECT bit 0, as the existing suite uses it).  On meshes this small every workgroup of the backwards
# walk is resident at once, the waits end and NO fallback is taken: the third case covers the kernel's polling path on
# 16-bit offsets; the fallback itself is compared where it happens, at 1200 x 400 (last test of this file).
@pytest.mark.parametrize("sync_free,fault", [(1, 0), (0, 0), (1, 1)], ids=["single-launch", "per-level", "backwards-walk"])
def test_ilu_s_applies_and_a_whole_solve_are_the_same_bytes_with_the_option_on_and_off(mesh, sync_free, fault):
    from navier_stokes_solver_amd import solver as S
    w1, on, fb1 = _results(S, mesh, 1, sync_free, fault)
    w0, off, fb0 = _results(S, mesh, 0, sync_free, fault)
    assert w1 == (16, 16, 16) and w0 == (32, 32, 32), (w1, w0)
    assert fb1 == fb0 and (fault or fb1 == 0)
    assert len(on) == len(off)
    for k, (a, b) in enumerate(zip(on, off)):
        assert same_bytes(a, b), f"item {k}"
    assert len(on[-3]) >= 8 + 1       # the history of 8 outer iterations


@pytest.mark.parametrize("factor_bits,inner_bits", [(32, 64), (64, 32)], ids=["fp32-factors", "fp32-inner-matrices"])
def test_same_bytes_with_fp32_values(factor_bits, inner_bits):
    from navier_stokes_solver_amd import solver as S
    pr = P.generate(100, 70, nu=1.0 / 90.0)
    w1, on, _ = _results(S, pr, 1, 1, 0, factor_bits, inner_bits)
    w0, off, _ = _results(S, pr, 0, 1, 0, factor_bits, inner_bits)
    assert w1 == (16, 16, 16) and w0 == (32, 32, 32), (w1, w0)
    for k, (a, b) in enumerate(zip(on, off)):
        assert same_bytes(a, b), f"item {k}"


def test_option_flipped_on_a_live_handle(mesh):
    """The option set after the hand-off rebuilds (or drops) the offsets of S and M_p and the next set-up those of the
    factors: the same bytes again, and the getter follows."""
    from navier_stokes_solver_amd import solver as S
    ls = _handle(S, mesh, 1, 1)
    try:
        b = np.random.default_rng(80).uniform(-1, 1, mesh.n_p)
        assert ls.index_width(S.BLK_S) == (16, 16, 16)
        a16, s16 = ls.tri_apply(S.TRI_PRESSURE, b), ls.inner_spmv(S.BLK_S, b)
        ls.set_option(S.IOPT_INDEX16, 0)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.index_width(S.BLK_S) == (32, 32, 32)
        assert same_bytes(ls.tri_apply(S.TRI_PRESSURE, b), a16) and same_bytes(ls.inner_spmv(S.BLK_S, b), s16)
        ls.set_option(S.IOPT_INDEX16, 1)
        ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
        assert ls.index_width(S.BLK_S) == (16, 16, 16)
        assert same_bytes(ls.tri_apply(S.TRI_PRESSURE, b), a16) and same_bytes(ls.inner_spmv(S.BLK_S, b), s16)
    finally:
        ls.close()


@pytest.mark.slow
def test_the_headline_mesh_runs_the_16_bit_form_everywhere_and_its_fallback_keeps_the_bytes():
    """1200 x 400.  With the defaults of bench.py S's SpMV and both halves of ILU(S) must report 16-bit offsets (no silent
    fall-back to int32), and profile_read's format bytes of the SpMV count 10 bytes per entry.  Then the fault-injected
    fallback where it really happens: the upper half of the single-launch ILU(S) solve walks backwards, the bounded spins
    give up, nsk_solve_resident redoes the solve with one launch per colour (tri_stream_kernel on the same halves, over a
    partly written vector).  Both index widths must take the same, nonzero number of fallbacks and return the same bytes."""
    from navier_stokes_solver_amd import solver as S
    pr = P.generate(1200, 400, nu=1.0 / 90.0)
    got = {}
    for index16 in (1, 0):
        ls = S.LinearSolver()
        try:
            ls.set_option(S.OPT_TRI_ORDERING, 1)
            ls.set_option(S.IOPT_INDEX16, index16)
            ls.set_problem(pr)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            assert ls.index_width(S.BLK_S) == ((16, 16, 16) if index16 else (32, 32, 32))
            if index16:
                nnz_s = ls.stats()["nnz_s"]
                ls.profile_begin(S.BLK_S, 4)
                fmt = ls.profile_read(S.BLK_S)[4]
                ls.profile_end()
                assert 10.0 * nnz_s <= fmt <= 10.0 * nnz_s + 64.0 * pr.n_p      # (+ row pointers, run plan, x and y)
            ls.set_option(S.IOPT_FAULT_INJECT, 1)
            ls.set_option(S.OPT_TRI_SYNC_FREE, 1)
            ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
            assert ls.index_width(S.BLK_S) == ((16, 16, 16) if index16 else (32, 32, 32))
            ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
            before = ls.stats()["sync_free_fallbacks"]
            its, res, rc = ls.solve_resident(S.FGMRES, 0.0, 1)
            xu, xp = ls.download_solution()
            got[index16] = (ls.stats()["sync_free_fallbacks"] - before,
                            [xu, xp, ls.history(), np.array([its, rc], dtype=np.int64), np.array([res])])
        finally:
            ls.close()
    assert got[1][0] == got[0][0] and got[1][0] >= 1, (got[1][0], got[0][0])
    for k, (a, b) in enumerate(zip(got[1][1], got[0][1])):
        assert same_bytes(a, b), f"item {k}"
