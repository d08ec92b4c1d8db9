"""Every SpMV kernel form alone, on irregular patterns, against exact row sums (nsk_internal.h: nsk_debug_spmv).

The solvers check their true residual with the same products they iterate with, so a kernel that drops or double-counts
an entry is self-consistent: the solve converges to the solution of another matrix.  Here each form — CSR-vector at every
lanes-per-row instantiation, the staged stream kernels in fp64 and fp32, the R x C blocked kernels, the 2 x 1 kernel with
aSIMPLE's epilogue, the two two-matrix kernels — runs alone on the caller's matrix, through the plan builders and
launchers the handle uses, and the hook reports which kernel ran on which plan: every case asserts its own coverage, the
plan is compared with the Python model of tests/spmv_reference.py, and the module's tally must hold every instantiation
at the end.  Every device vector sits between guard words; the ghost tail (and the operands the call sites align no
better: the second matrix's x, the y of the scalar forms) can start 8 bytes off a 16-byte boundary.

Two kinds of input:

* Integer-exact: |a| <= 8, |x| <= 16, small integers in y, z, d: every product and every partial sum is an integer far
  below 2^53 (and exact in fp32), any order gives the same bits, and the result must EQUAL the int64 row sums, row by row.
  x_j differs from column to column (period 31; the ghost tail follows another law), so a wrong column, the wrong half
  of a pair, or x_own where x_ghost belongs changes a sum.  These carry the large cases.

* Random doubles against the correctly rounded row sum s_i, per row:
      |y_i - s_i| <= d u / (1 - d u) * sum_j |a_ij x_j| + u |s_i|,   u = 2^-53
  (u |s_i|: the reference itself is rounded once), where d is the largest number of roundings a product can pass.  Counted
  from nsk_kernels.hip for a row of L stored entries (Lb blocks), RG = 4 lanes per row in the staged kernels:
    - stream (spmv_stream_kernel, any VEC, fp64 or fp32 values): the product is rounded into LDS (1); lane l of the row
      adds its ceil(L / 4) products to 0.0 in one chain, the first addition is exact: ceil(L / 4) - 1; the 4-lane
      shuffle tree: 2.  d = 1 + (ceil(L / 4) - 1) + 2.
    - CSR-vector (spmv_kernel<LPR>): s += a x per entry, fused or not: the product (1, none if fused) and a chain of
      ceil(L / LPR) additions of which the first is exact, then the LPR-lane tree log2 LPR:  d = ceil(L / LPR) + log2 LPR.
    - blocked (spmv_blk_kernel): C = 2: a00 x0 + a01 x1 — each product rounded, then their sum: 2 (C = 1: 1); then the
      stream kernel's chain and tree over blocks: d = C + (ceil(Lb / 4) - 1) + 2.
    - two-matrix (spmv2_stream_kernel, spmv_blk_fused_kernel): ONE accumulator per lane runs over the first matrix's
      products and then the second's: d = p + (ceil(La / 4) + ceil(Lb / 4) - 1) + 2, p = 1 (stream) or 2 (A's 2 x 2 blocks).
  Modes 1 and 2 add z (or y) once, and so does the reference, each with a rounding of its own: + 2 u |result|.  The
  epilogue ((y d) - s) dinv rounds three times more, each operation once, in the kernel and in the reference: with
  t = y d - s the bound is |dinv| (E_s + 2 u |t|) + 2 u |result|, E_s the bound on s.  No measured constant enters any
  of these.

fp32 forms: bits equal to the fp64 form of the same kernel on the values rounded to float (the promise of nsk_kernels.h),
on every pattern.  Determinism: the same call twice gives the same bits.  Sub-ranges of a plan, as spmv_halo launches
them: y holds NaN beforehand and the rows outside the range must keep it.

The tally's kernel names: VEC of the stream kernels and the lanes per row of the CSR-vector kernel are what the
launchers return for the instantiation they chose, R, C, the value type and the epilogue are the hook's arguments to
launchers that map them one to one; a launch over an empty run range is not counted.

spmv_kernel<2, *> is reachable only through the hook (pick_lpr never returns 2); it is tested here by forcing lpr = 2.
"""
import ctypes as C
import functools
import time
from collections import Counter

import numpy as np
import pytest

from tests import spmv_reference as M

pytestmark = pytest.mark.gpu

U = M.U
CSRV, STREAM, STREAM_F32, BLK22, BLK21, BLK12, BLK11, BLK22_F32, BLK21_EPI, STREAM2, BLK_FUSED = range(11)
BLK_FORM = {(2, 2): BLK22, (2, 1): BLK21, (1, 2): BLK12, (1, 1): BLK11}
FORM_NAME = ["csrv", "stream", "stream_f32", "blk22", "blk21", "blk12", "blk11", "blk22_f32", "blk21_epi", "stream2",
             "blk_fused"]
LPRS = [2, 4, 8, 16, 32, 64]
G, XB, YO = 1, 2, 4    # misalign bits: ghost tails, the second matrix's x_own, y / z

TALLY = Counter()      # kernel instantiations launched over the module: printed at teardown (pytest -s)
T0 = time.time()


class Mat(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("n_cols", C.c_int32), ("n_own_cols", C.c_int32), ("pad_", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("x_own", C.c_void_p),
                ("x_ghost", C.c_void_p)]


def _ptr(a):
    return None if a is None else a.ctypes.data


def kernel_name(form, info, mode):
    if form == CSRV:
        return f"spmv_kernel<{info[2]}, {mode}>"
    if form in (STREAM, STREAM_F32):
        return f"spmv_stream_kernel<{'float' if form == STREAM_F32 else 'double'}, {info[1]}, {mode}>"
    if form == STREAM2:
        return f"spmv2_stream_kernel<{info[1]}>"
    if form == BLK_FUSED:
        return "spmv_blk_fused_kernel"
    return f"spmv_blk_kernel<{'float' if form == BLK22_F32 else 'double'}, {info[3]}, {info[4]}, {int(form == BLK21_EPI)}>"


class Hook:
    def __init__(self):
        from navier_stokes_solver_amd import solver as S
        self.S = S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_spmv.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]

    def run(self, form, A, x, y, mode=0, z=None, B=None, xb=None, d=None, dinv=None, lpr=0, misalign=0, runs=None,
            twice=True):
        """One launch on copies of the operands: (y after, info, row runs of the plan) or (None, info, None) when the plan
        refuses the form.  twice: launched again, the bits must be the same."""
        keep = []

        def mat(Am, xs):
            xo, xg = (np.ascontiguousarray(v, dtype=np.float64) for v in xs)
            assert len(xo) == Am.n_own and len(xg) == Am.n_cols - Am.n_own
            keep.extend([xo, xg])
            return Mat(Am.n_rows, Am.n_cols, Am.n_own, 0, _ptr(Am.rowptr), _ptr(Am.col), _ptr(Am.val), _ptr(xo), _ptr(xg))

        ma = mat(A, x)
        mb = mat(B, xb) if B is not None else None
        vec = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (z, d, dinv)]
        c0, c1 = runs if runs is not None else (-1, -1)
        out = []
        for _ in range(2 if twice else 1):
            yy = np.array(y, dtype=np.float64, copy=True)
            info = np.zeros(16, dtype=np.int32)
            rb = np.full(A.n_rows + 2, -1, dtype=np.int32)
            rc = self.L.nsk_debug_spmv(self.ls.h, form, lpr, mode, misalign, c0, c1, C.byref(ma),
                                       C.byref(mb) if mb is not None else None, _ptr(yy), _ptr(vec[0]), _ptr(vec[1]),
                                       _ptr(vec[2]), _ptr(rb), len(rb), _ptr(info))
            assert rc in (0, 1), (rc, self.ls.last_error(), FORM_NAME[form], A.name)
            if rc == 1:
                assert info[0] == -1 and info[15] != 0
                return None, info, None
            assert info[0] == form and info[15] == 0
            assert info[13] == 0, f"{FORM_NAME[form]} mode {mode} on {A.name}: {info[13]} guard words were written"
            out.append(yy)
        if twice:
            assert np.array_equal(out[0], out[1], equal_nan=True), f"{FORM_NAME[form]} on {A.name}: two runs differ"
        if form == CSRV or info[14] > 0:      # (an empty run range launches nothing)
            TALLY[kernel_name(form, info, mode)] += 1
        return out[0], info, rb[:info[8] + 1].tolist() if form != CSRV else None


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()
    print("\nSpMV kernel instantiations launched:", dict(sorted(TALLY.items())))
    print(f"module wall time {time.time() - T0:.1f} s")


@functools.lru_cache(maxsize=1)
def scalar_patterns():
    return M.scalar_patterns()


@functools.lru_cache(maxsize=1)
def block_patterns():
    return M.block_patterns()


@functools.lru_cache(maxsize=1)
def pair_patterns():
    return M.pair_patterns()


def same(got, want, what):
    """Equality row by row; the message names the first wrong rows and got - want."""
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} wrong rows, first {bad[:8].tolist()}, got - want "
                           f"{(got[bad[:8]] - want[bad[:8]]).tolist()}")


def within(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    bad = np.nonzero(~(err <= tol))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows outside the bound, first {bad[:8].tolist()}, error / bound "
                           f"{(err[bad[:8]] / np.maximum(tol[bad[:8]], 1e-300)).tolist()}")


def int_operands(A):
    n = A.n_rows
    return M.int_x(A), M.int_vec(n, 13, 6), M.int_vec(n, 7, 3)     # x, y, z


def check_stream_plan(A, info, rb):
    p = M.stream_plan(A)
    assert p["ok"] and info[5] == 1 and info[6] == int(p["even"]) and info[1] == p["vec"], A.name
    assert rb == p["rb"] and (info[9], info[10]) == (p["int_b0"], p["int_b1"]), A.name
    assert (info[8], info[11], info[12]) == (len(p["rb"]) - 1, p["rows"], p["entries"]), A.name
    return p


def sub_ranges(p):
    nb = len(p["rb"]) - 1
    return [(p["int_b0"], p["int_b1"]), (0, p["int_b0"]), (p["int_b1"], nb)]


def nan_outside(want, rb, c0, c1, Rr=1):
    """The expected y of a sub-range launch on a y full of NaN: only the rows of runs [c0, c1) are written."""
    out = np.full(len(want), np.nan)
    a, b = Rr * rb[c0], Rr * rb[c1]
    out[a:b] = want[a:b]
    return out


# ------------------------------------------------------------------ integer-exact: scalar forms on every scalar pattern
def _scalar_forms_int(hook, A, big=False):
    (x, y, z) = int_operands(A)
    s = M.int_row_sums(A, *x).astype(np.float64)
    name = A.name
    p = M.stream_plan(A)
    cases = [(0, None), (1, None), (1, z), (2, z)]
    for lpr in ([0] if big else LPRS + [0]):
        for mis in (0, G | YO):
            for mode, zz in (cases[:1] + cases[3:] if big else cases):
                got, info, _ = hook.run(CSRV, A, x, y, mode=mode, z=zz, lpr=lpr, misalign=mis, twice=not big)
                assert info[2] == (lpr or M.pick_lpr(A)) and info[5] == int(p["ok"])
                same(got, M.apply_mode(s, mode, y, zz),
                     f"csrv lpr {info[2]} mode {mode} z {zz is not None} misalign {mis} on {name}")
    got, info, rb = hook.run(STREAM, A, x, y)
    if not p["ok"]:      # a row above kStreamNnz: reported, not forced (the handle falls back to CSR-vector)
        assert got is None and info[15] == 1 and info[5] == 0
        assert hook.run(STREAM_F32, A, x, y)[1][15] == 1
        return
    check_stream_plan(A, info, rb)
    for mis in (0, G | YO):
        for mode, zz in cases:
            got, info, _ = hook.run(STREAM, A, x, y, mode=mode, z=zz, misalign=mis, twice=not big)
            same(got, M.apply_mode(s, mode, y, zz), f"stream VEC {info[1]} mode {mode} z {zz is not None} misalign {mis} on {name}")
        got, info, rb = hook.run(STREAM_F32, A, x, y, misalign=mis, twice=not big)
        check_stream_plan(A, info, rb)
        same(got, s, f"stream fp32 VEC {info[1]} misalign {mis} on {name}")
        for form in (STREAM, STREAM_F32):
            for c0, c1 in sub_ranges(p):
                got, info, _ = hook.run(form, A, x, np.full(A.n_rows, np.nan), misalign=mis, runs=(c0, c1), twice=False)
                assert info[14] == c1 - c0
                same(got, nan_outside(s, p["rb"], c0, c1), f"{FORM_NAME[form]} runs [{c0}, {c1}) misalign {mis} on {name}")


@pytest.mark.parametrize("name", sorted(M.scalar_patterns()))
def test_scalar_forms_integer_exact(hook, name):
    _scalar_forms_int(hook, M.int_values(scalar_patterns()[name], 1))


def test_stream_refuses_a_row_above_the_cap_and_takes_one_at_it(hook):
    P = scalar_patterns()
    for name, ok in (("row_2048", True), ("row_2049", False), ("row_6144", False)):
        A = M.int_values(P[name])
        x, y, _ = int_operands(A)
        got, info, _ = hook.run(STREAM, A, x, y)
        assert (got is not None) == ok and info[5] == int(ok) and info[15] == (0 if ok else 1)
        if ok:
            assert info[12] == M.K_STREAM_NNZ


# ------------------------------------------------------------------ integer-exact: blocked forms
def _blocked_forms_int(hook, Rr, Cc, A, big=False):
    (x, y, z) = int_operands(A)
    s = M.int_row_sums(A, *x).astype(np.float64)
    p = M.blocked_plan(A, Rr, Cc)
    form = BLK_FORM[(Rr, Cc)]
    forms = [form] + ([BLK22_F32] if (Rr, Cc) == (2, 2) else [])
    got, info, rb = hook.run(form, A, x, y)
    if not p["ok"]:
        assert got is None and info[15] == 2 and info[7] == 0, A.name
        for f in forms[1:] + ([BLK21_EPI] if (Rr, Cc) == (2, 1) else []):
            assert hook.run(f, A, x, y, d=y, dinv=y)[1][15] == 2
        return
    assert info[7] == 1 and (info[3], info[4]) == (Rr, Cc) and rb == p["rb"], A.name
    assert (info[8], info[9], info[10], info[11], info[12]) == (len(rb) - 1, p["int_b0"], p["int_b1"], p["rows"], p["entries"])
    for mis in (0, G | (YO if Rr == 1 else 0)):
        for f in forms:
            got, info, _ = hook.run(f, A, x, y, misalign=mis, twice=not big)
            same(got, s, f"{FORM_NAME[f]} misalign {mis} on {A.name}")
            for c0, c1 in sub_ranges(p):
                got, info, _ = hook.run(f, A, x, np.full(A.n_rows, np.nan), misalign=mis, runs=(c0, c1), twice=False)
                same(got, nan_outside(s, p["rb"], c0, c1, Rr), f"{FORM_NAME[f]} runs [{c0}, {c1}) misalign {mis} on {A.name}")
        if (Rr, Cc) == (2, 1):
            d = M.int_vec(A.n_rows, 5, 2) + 3.0                    # 1 .. 5
            dinv = 2.0 ** -(np.arange(A.n_rows) % 3)               # powers of two: the last product is exact too
            got, info, _ = hook.run(BLK21_EPI, A, x, y, d=d, dinv=dinv, misalign=mis & G, twice=not big)
            same(got, M.epilogue(s, y, d, dinv), f"blk21 epilogue misalign {mis & G} on {A.name}")


@pytest.mark.parametrize("name", sorted(M.block_patterns()))
def test_blocked_forms_integer_exact(hook, name):
    Rr, Cc, A = block_patterns()[name]
    A = M.int_values(A, 2)
    _blocked_forms_int(hook, Rr, Cc, A)
    if name.endswith("_mixed") or name.endswith("_ghost_edges") or name.endswith("_broken"):
        _scalar_forms_int(hook, A)          # the same matrix through the scalar forms: what the handle falls back to


def test_a_block_shape_the_pattern_does_not_have_is_refused(hook):
    P = block_patterns()
    for name, form in (("blk2x1_mixed", BLK22), ("blk1x2_mixed", BLK22), ("blk1x1_mixed", BLK12), ("blk1x1_mixed", BLK21)):
        A = M.int_values(P[name][2])
        x, y, _ = int_operands(A)
        got, info, _ = hook.run(form, A, x, y)
        assert got is None and info[15] == 2 and info[7] == 0, name


# ------------------------------------------------------------------ integer-exact: two-matrix forms
def _pair_forms_int(hook, A, B, name, big=False):
    xa, y, _ = int_operands(A)
    xb = tuple(-v for v in M.int_x(B))
    s = (M.int_row_sums(A, *xa) + M.int_row_sums(B, *xb)).astype(np.float64)
    for form, blocked in ((STREAM2, False), (BLK_FUSED, True)):
        p = M.fused_plan(A, B, blocked)
        got, info, rb = hook.run(form, A, xa, y, B=B, xb=xb)
        if not p["ok"]:
            assert got is None and info[15] == p["reason"], (name, FORM_NAME[form])
            continue
        assert rb == p["rb"] and (info[11], info[12]) == (p["rows"], p["entries"]), (name, FORM_NAME[form])
        for mis in (0, G | XB):
            got, info, _ = hook.run(form, A, xa, y, B=B, xb=xb, misalign=mis, twice=not big)
            same(got, s, f"{FORM_NAME[form]} misalign {mis} on {name}")


@pytest.mark.parametrize("name", sorted(M.pair_patterns()))
def test_two_matrix_forms_integer_exact(hook, name):
    A, B = pair_patterns()[name]
    _pair_forms_int(hook, M.int_values(A, 3), M.int_values(B, 4), name)


def test_two_matrix_refusals(hook):
    A, B = pair_patterns()["pair_over_cap"]
    A, B = M.int_values(A), M.int_values(B)
    xa, y, _ = int_operands(A)
    assert hook.run(BLK_FUSED, A, xa, y, B=B, xb=M.int_x(B))[1][15] == 4
    # an odd row pointer in the first matrix: the scalar two-matrix kernel reads it in aligned pairs and is not chosen
    A1 = M.int_values(M.add_entry_to_first_row(A))
    B1 = M.int_values(M.from_lengths(np.ones(A1.n_rows, dtype=np.int64), 50, 5))
    got, info, _ = hook.run(STREAM2, A1, M.int_x(A1), y, B=B1, xb=M.int_x(B1))
    assert got is None and info[15] == 3
    # a scalar pair without node structure: the scalar kernel runs, the blocked one is refused
    A2 = M.int_values(scalar_patterns()["even"])
    B2 = M.int_values(M.from_lengths(M.geometric_lengths(A2.n_rows, 3, 6, cap=30), 500, 7))
    s = (M.int_row_sums(A2, *M.int_x(A2)) + M.int_row_sums(B2, *M.int_x(B2))).astype(np.float64)
    got, info, _ = hook.run(STREAM2, A2, M.int_x(A2), np.zeros(A2.n_rows), B=B2, xb=M.int_x(B2))
    same(got, s, "stream2 on a pair without node structure")
    assert hook.run(BLK_FUSED, A2, M.int_x(A2), np.zeros(A2.n_rows), B=B2, xb=M.int_x(B2))[1][15] == 2


# ------------------------------------------------------------------ integer-exact: the large cases
def test_one_million_rows_of_mixed_lengths(hook):
    A = M.int_values(M.big_mixed())
    assert A.n_rows == 1 << 20 and A.nnz > 7e6
    _scalar_forms_int(hook, A, big=True)


def test_generator_blocks_600x200_integer_exact(hook):
    blocks = {name: (Rr, Cc, M.int_values(A, 5)) for name, Rr, Cc, A in M.generator_blocks(600, 200)}
    for name, (Rr, Cc, A) in blocks.items():
        _blocked_forms_int(hook, Rr, Cc, A, big=True)
        x, y, z = int_operands(A)
        s = M.int_row_sums(A, *x).astype(np.float64)
        for form, kw in ((STREAM, dict(mode=2, z=z)), (STREAM_F32, {}), (CSRV, dict(mode=1))):
            got, info, _ = hook.run(form, A, x, y, twice=False, **kw)
            same(got, M.apply_mode(s, kw.get("mode", 0), y, kw.get("z")), f"{FORM_NAME[form]} on {A.name}")
    _pair_forms_int(hook, blocks["F"][2], blocks["Bt"][2], "F, Bt 600x200", big=True)


# ------------------------------------------------------------------ random doubles against the correctly rounded row sums
@functools.lru_cache(maxsize=None)
def real_case(kind, name):
    if kind == "scalar":
        A = scalar_patterns()[name]
    elif kind == "block":
        A = block_patterns()[name][2]
    elif kind == "gen":
        A = {n: a for n, _, _, a in M.generator_blocks(60, 20)}[name]
    else:
        A = pair_patterns()[name][0 if kind == "pairA" else 1]
    if kind != "gen":
        A = M.real_values(A, 7)
    x = M.real_x(A, 8)
    s, a = M.exact_row_sums(A, *x)
    return A, x, s, a


@functools.lru_cache(maxsize=None)
def real_case32(kind, name):
    """The fp32 forms' reference: exact row sums over float32(a_ij) widened back."""
    A, x, _, _ = real_case(kind, name)
    return M.exact_row_sums(A, *x, fp32=True)


def real_vecs(n):
    rng = np.random.default_rng(n)
    return rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


def _scalar_forms_real(hook, kind, name):
    A, x, s, a = real_case(kind, name)
    y, z = real_vecs(A.n_rows)
    L = A.row_len
    p = M.stream_plan(A)
    A32 = A.with_values(A.val.astype(np.float32).astype(np.float64))
    for lpr in LPRS:
        E = M.gamma(M.roundings("csrv", L, lpr=lpr)) * a + U * np.abs(s)
        for mis in (0, G | YO):
            for mode, zz in ((0, None), (1, None), (1, z), (2, z)):
                want = M.apply_mode(s, mode, y, zz)
                got, _, _ = hook.run(CSRV, A, x, y, mode=mode, z=zz, lpr=lpr, misalign=mis)
                within(got, want, E + (2 * U * np.abs(want) if mode else 0),
                       f"csrv lpr {lpr} mode {mode} misalign {mis} on {name}")
    if not p["ok"]:
        return
    E = M.gamma(M.roundings("stream", L)) * a + U * np.abs(s)
    for mis in (0, G | YO):
        for mode, zz in ((0, None), (1, None), (1, z), (2, z)):
            want = M.apply_mode(s, mode, y, zz)
            got, _, _ = hook.run(STREAM, A, x, y, mode=mode, z=zz, misalign=mis)
            within(got, want, E + (2 * U * np.abs(want) if mode else 0), f"stream mode {mode} misalign {mis} on {name}")
        got32, i32, _ = hook.run(STREAM_F32, A, x, y, misalign=mis)
        got64, i64, _ = hook.run(STREAM, A32, x, y, misalign=mis)
        assert i32[1] == i64[1]
        same(got32, got64, f"stream fp32 against fp64 on the rounded values, misalign {mis}, on {name}")
        s32, a32 = real_case32(kind, name)
        within(got32, s32, M.gamma(M.roundings("stream", L)) * a32 + U * np.abs(s32),
               f"stream fp32 against the exact sums over the rounded values, misalign {mis}, on {name}")
        if mis == 0 and A.nnz:
            assert not np.array_equal(got32, hook.run(STREAM, A, x, y)[0]), name   # (the values are not floats)


@pytest.mark.parametrize("name", sorted(M.scalar_patterns()))
def test_scalar_forms_random(hook, name):
    _scalar_forms_real(hook, "scalar", name)


@pytest.mark.parametrize("name", ["F", "B", "Bt", "Mp"])
def test_scalar_forms_random_generator_blocks(hook, name):
    _scalar_forms_real(hook, "gen", name)


def _blocked_forms_real(hook, kind, name, Rr, Cc):
    A, x, s, a = real_case(kind, name)
    p = M.blocked_plan(A, Rr, Cc)
    if not p["ok"]:
        return
    y, _ = real_vecs(A.n_rows)
    Lb = np.repeat(np.diff(p["brp"]), Rr)
    E = M.gamma(M.roundings(f"blk_c{Cc}", Lb)) * a + U * np.abs(s)
    form = BLK_FORM[(Rr, Cc)]
    for mis in (0, G):
        got, _, _ = hook.run(form, A, x, y, misalign=mis)
        within(got, s, E, f"{FORM_NAME[form]} misalign {mis} on {name}")
        if (Rr, Cc) == (2, 2):
            A32 = A.with_values(A.val.astype(np.float32).astype(np.float64))
            got32 = hook.run(BLK22_F32, A, x, y, misalign=mis)[0]
            same(got32, hook.run(BLK22, A32, x, y, misalign=mis)[0],
                 f"blk22 fp32 against fp64 on the rounded values, misalign {mis}, on {name}")
            s32, a32 = real_case32(kind, name)
            within(got32, s32, M.gamma(M.roundings("blk_c2", Lb)) * a32 + U * np.abs(s32),
                   f"blk22 fp32 against the exact sums over the rounded values, misalign {mis}, on {name}")
            if A.nnz:
                assert not np.array_equal(hook.run(BLK22_F32, A, x, y)[0], got), name
        if (Rr, Cc) == (2, 1):
            rng = np.random.default_rng(5)
            d = rng.uniform(0.5, 2.0, A.n_rows)
            dinv = 1.0 / d
            t = y * d - s
            want = M.epilogue(s, y, d, dinv)
            tol = (np.abs(dinv) * (E + 2 * U * np.abs(t)) + 2 * U * np.abs(want)) * (1 + 8 * U)
            got, _, _ = hook.run(BLK21_EPI, A, x, y, d=d, dinv=dinv, misalign=mis)
            within(got, want, tol, f"blk21 epilogue misalign {mis} on {name}")


@pytest.mark.parametrize("name", sorted(M.block_patterns()))
def test_blocked_forms_random(hook, name):
    Rr, Cc, _ = block_patterns()[name]
    _blocked_forms_real(hook, "block", name, Rr, Cc)


@pytest.mark.parametrize("name,Rr,Cc", [("F", 2, 2), ("Bt", 2, 1), ("B", 1, 2), ("Mp", 1, 1)])
def test_blocked_forms_random_generator_blocks(hook, name, Rr, Cc):
    _blocked_forms_real(hook, "gen", name, Rr, Cc)


def _pair_forms_real(hook, name, ca, cb):
    (A, xa, sa, aa), (B, xb, sb, ab) = ca, cb
    y, _ = real_vecs(A.n_rows)
    want = sa + sb
    ref = 2 * U * (np.abs(sa) + np.abs(sb) + np.abs(want))      # the reference: two rounded sums and their rounded sum
    for form, blocked in ((STREAM2, False), (BLK_FUSED, True)):
        p = M.fused_plan(A, B, blocked)
        if not p["ok"]:
            continue
        if blocked:
            d = M.roundings("blk_fused", np.repeat(np.diff(p["ra"]), 2), np.repeat(np.diff(p["rb2"]), 2))
        else:
            d = M.roundings("stream2", A.row_len, B.row_len)
        for mis in (0, G | XB):
            got, _, _ = hook.run(form, A, xa, y, B=B, xb=xb, misalign=mis)
            within(got, want, M.gamma(d) * (aa + ab) + ref, f"{FORM_NAME[form]} misalign {mis} on {name}")


@pytest.mark.parametrize("name", sorted(M.pair_patterns()))
def test_two_matrix_forms_random(hook, name):
    _pair_forms_real(hook, name, real_case("pairA", name), real_case("pairB", name))


def test_two_matrix_forms_random_generator_blocks(hook):
    _pair_forms_real(hook, "F, Bt 60x20", real_case("gen", "F"), real_case("gen", "Bt"))


# ------------------------------------------------------------------ the public entry points launch these forms
@functools.lru_cache(maxsize=1)
def irregular_system():
    """An irregular node-structured system: F 2 x 2 blocks, B~^T 2 x 1, B~ 1 x 2, M_p scalar, random values.  F (in
    blocks) and M_p are structurally symmetric with a full diagonal, so that a preconditioner can be set up on them."""
    nn, n_p = 900, 500
    lf = np.maximum(M.geometric_lengths(nn, 8, 41, cap=80), 1)
    F = M.real_values(M.expand_blocks(M.symmetric_with_diagonal(M.from_lengths(lf, nn, 42)), 2, 2, name="F_irregular"), 1)
    Bt = M.real_values(M.expand_blocks(M.from_lengths(M.geometric_lengths(nn, 3, 43, cap=30) - 1, n_p, 44), 2, 1, name="Bt_irregular"), 2)
    B = M.real_values(M.expand_blocks(M.from_lengths(M.geometric_lengths(n_p, 5, 45, cap=50), nn, 46), 1, 2, name="B_irregular"), 3)
    Mp = M.real_values(M.symmetric_with_diagonal(M.from_lengths(M.geometric_lengths(n_p, 4, 47, cap=40), n_p, 48),
                                                 name="Mp_irregular"), 4)
    return F, Bt, B, Mp


def test_public_entry_points_launch_the_forms_the_options_select(hook):
    S = hook.S
    F, Bt, B, Mp = irregular_system()
    n_u, n_p = F.n_rows, Mp.n_rows
    from types import SimpleNamespace
    ls = S.LinearSolver()
    try:
        ls.n_u, ls.n_p = n_u, n_p
        ls.set_partition(S.SPACE_U, 0, n_u, [])
        ls.set_partition(S.SPACE_P, 0, n_p, [])
        for b, A in ((S.BLK_F, F), (S.BLK_BT, Bt), (S.BLK_B, B), (S.BLK_MP, Mp)):
            ls.set_block(b, SimpleNamespace(rowptr=A.rowptr, col=A.col, val=A.val, rows=A.n_rows, cols=A.n_cols))
        rng = np.random.default_rng(9)
        xu, xp = rng.uniform(-1, 1, n_u), rng.uniform(-1, 1, n_p)
        yu, yp = rng.uniform(-1, 1, n_u), rng.uniform(-1, 1, n_p)
        e = np.zeros(0)
        ops = [(S.BLK_F, F, xu, yu, BLK22), (S.BLK_BT, Bt, xp, yu, BLK21), (S.BLK_B, B, xu, yp, BLK12),
               (S.BLK_MP, Mp, xp, yp, None)]
        assert M.stream_plan(Mp)["vec"] == 3 and M.stream_plan(F)["vec"] == 2
        for stream, bsr, fuse in ((1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 1, 1)):
            ls.set_option(S.OPT_STREAM_KERNELS, stream)
            ls.set_option(S.OPT_BSR_VELOCITY, bsr)
            ls.set_option(S.OPT_FUSE_BLOCK_ROW, fuse)
            what = f"stream {stream} bsr {bsr} fuse {fuse}"
            for b, A, x, y, blk_form in ops:
                plain = blk_form if (stream and bsr and blk_form is not None) else STREAM if stream else CSRV
                added = STREAM if stream else CSRV          # y += A x never takes the blocked kernels
                same(ls.spmv(b, x), hook.run(plain, A, (x, e), y)[0], f"nsk_spmv {A.name} {what}")
                same(ls.spmv(b, x, y=y, add=True), hook.run(added, A, (x, e), y, mode=1)[0], f"nsk_spmv add {A.name} {what}")
            gu, gp = ls.jacobian_vmult(xu, xp)
            if stream and bsr and fuse:
                want_u = hook.run(BLK_FUSED, F, (xu, e), yu, B=Bt, xb=(xp, e))[0]
            elif stream and fuse:
                want_u = hook.run(STREAM2, F, (xu, e), yu, B=Bt, xb=(xp, e))[0]
            else:
                t = hook.run(BLK22 if stream and bsr else STREAM if stream else CSRV, F, (xu, e), yu)[0]
                want_u = hook.run(STREAM if stream else CSRV, Bt, (xp, e), t, mode=1)[0]
            same(gu, want_u, f"nsk_jacobian_vmult, velocity rows, {what}")
            same(gp, hook.run(BLK12 if stream and bsr else STREAM if stream else CSRV, B, (xu, e), yp)[0],
                 f"nsk_jacobian_vmult, pressure rows, {what}")
        # the forms differ in their bits on this system, so the equalities above do tell them apart
        assert not np.array_equal(hook.run(BLK22, F, (xu, e), yu)[0], hook.run(CSRV, F, (xu, e), yu)[0])
    finally:
        ls.close()


def test_inner_spmv_launches_the_form_the_options_and_the_precision_select(hook):
    """nsk_inner_spmv is the SpMV of the preconditioner's inner solves (spmv_halo): with NSK_OPT_INNER_MATRIX_PRECISION = 32
    it reads the fp32 copies the set-up made — F's 2 x 2 blocks, M_p's scalar values — wherever a stream kernel runs."""
    S = hook.S
    F, Bt, B, Mp = irregular_system()
    n_u, n_p = F.n_rows, Mp.n_rows
    from types import SimpleNamespace
    assert M.stream_plan(Mp)["vec"] == 3 and M.blocked_plan(F, 2, 2)["ok"]
    ls = S.LinearSolver()
    try:
        ls.n_u, ls.n_p = n_u, n_p
        ls.set_partition(S.SPACE_U, 0, n_u, [])
        ls.set_partition(S.SPACE_P, 0, n_p, [])
        for b, A in ((S.BLK_F, F), (S.BLK_BT, Bt), (S.BLK_B, B), (S.BLK_MP, Mp)):
            ls.set_block(b, SimpleNamespace(rowptr=A.rowptr, col=A.col, val=A.val, rows=A.n_rows, cols=A.n_cols))
        rng = np.random.default_rng(10)
        xu, xp = rng.uniform(-1, 1, n_u), rng.uniform(-1, 1, n_p)
        e = np.zeros(0)
        for bits in (64, 32):
            for stream, bsr in ((1, 1), (1, 0), (0, 1)):
                ls.set_option(S.OPT_STREAM_KERNELS, stream)
                ls.set_option(S.OPT_BSR_VELOCITY, bsr)
                ls.set_option(S.OPT_INNER_MATRIX_PRECISION, bits)
                ls.setup_preconditioner(S.BLOCK_DIAGONAL, S.STATIONARY)      # (symmetric Gauss-Seidel: no factorisation)
                what = f"precision {bits} stream {stream} bsr {bsr}"
                f32 = bits == 32
                form_f = (BLK22_F32 if f32 else BLK22) if stream and bsr else STREAM if stream else CSRV
                form_m = (STREAM_F32 if f32 else STREAM) if stream else CSRV
                assert ls.inner_value_bytes(S.BLK_F) == (4 if form_f == BLK22_F32 else 8), what
                assert ls.inner_value_bytes(S.BLK_MP) == (4 if form_m == STREAM_F32 else 8), what
                want_f, _, _ = hook.run(form_f, F, (xu, e), np.zeros(n_u))
                want_m, info, _ = hook.run(form_m, Mp, (xp, e), np.zeros(n_p))
                assert form_m == CSRV or info[1] == 3
                same(ls.inner_spmv(S.BLK_F, xu), want_f, f"nsk_inner_spmv F, {what}")
                same(ls.inner_spmv(S.BLK_MP, xp), want_m, f"nsk_inner_spmv M_p, {what}")
        # the fp32 and fp64 forms differ in their bits here, so the equalities above tell them apart
        assert not np.array_equal(hook.run(BLK22_F32, F, (xu, e), np.zeros(n_u))[0], hook.run(BLK22, F, (xu, e), np.zeros(n_u))[0])
        assert not np.array_equal(hook.run(STREAM_F32, Mp, (xp, e), np.zeros(n_p))[0], hook.run(STREAM, Mp, (xp, e), np.zeros(n_p))[0])
    finally:
        ls.close()


# ------------------------------------------------------------------ coverage: must stay the last test of the module
def test_every_instantiation_ran(hook):
    want = [f"spmv_kernel<{lpr}, {m}>" for lpr in LPRS for m in range(3)]
    want += [f"spmv_stream_kernel<double, {v}, {m}>" for v in (2, 3) for m in range(3)]
    want += [f"spmv_stream_kernel<float, {v}, 0>" for v in (2, 3)]
    want += ["spmv2_stream_kernel<2>", "spmv_blk_fused_kernel", "spmv_blk_kernel<float, 2, 2, 0>",
             "spmv_blk_kernel<double, 2, 1, 1>"]
    want += [f"spmv_blk_kernel<double, {r}, {c}, 0>" for r in (1, 2) for c in (1, 2)]
    missing = [k for k in want if TALLY[k] == 0]
    assert not missing, f"never launched: {missing}"
