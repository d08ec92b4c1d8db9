"""Every triangular-solve kernel alone, against exact substitution (nsk_internal.h: nsk_debug_tri).

The solvers check residuals of the OUTER system: an ILU(0) or SGS kernel that drops an entry gives a slightly worse
preconditioner, a few more iterations, and no failing test; and the parity tests compare a whole apply with the oracle's
in one norm, where the factorisation and the two solves cannot be told apart.  Here ONE TriSolve runs on the caller's
matrix — analyze, numeric, three applies — through the plan builders and launchers the handle uses.  The hook reports the
branch of TriSolve::apply that ran, the value type and index width in use, the line-group size, the run plan and the
walker's schedule: every case asserts the path and the instantiation it MEANT to run, and the module's tally must hold
every instantiation apply() can reach at the end (test_zz_tally_is_complete).  The tally's names are composed from
what the hook reports of the TriSolve (branch, f32, the offsets' presence, lanes per row, the schedule's steps) — the
state the launchers switch on — not returned by the launchers: a launcher that chose its instantiation on another
condition than that state would not show here, only in the results.  b and x sit between guard words, the intermediate
vector and the colour-ordered working vector in front of some.  tests/tri_reference.py has the exact statements, the bounds and their rounding counts.

Checked on every call (Hook.solve): no guard word changed, sf_err not raised, the handle's sync_free_fallbacks unchanged,
ring_applies moved exactly when the ring was the reported path; the returned perm is a permutation, the factor carries
NaN exactly at the entries the sub-domains drop; for SGS the factor is the matrix, for ILU(0) every position meets its
exact-defect bound; and every x:
  * integer-exact inputs (SGS, unit diagonal, integer off-diagonals |a| <= 3, integer b built from a small integer
    solution; tri_reference.int_solve proves every sum below 2^53): bit equality with the integer solve, row by row;
  * random doubles (off-diagonals of mixed sign over 10^-7 .. 1, the diagonal dominant): the derived residual bound, row
    by row, against the returned factor (fp32 halves: with its off-diagonals rounded to float).
Three applies on one factor, right-hand sides b0, b1, b0; the call is repeated with b1, b0, b1: first applies on a fresh
factor equal second and third ones on a used one (the sentinel the single-launch kernels leave behind is state), and —
small cases — the same call twice gives the same bits.

Shapes are the smallest at which the kernels can go wrong.  tri_reference.stair gives patterns whose colouring is known
(colours = layers of consecutive rows, identity permutation): runs of exactly 64 rows and of exactly 2048 entries (1024
blocks) and one more, a colour of one row, whole colours of rows without a lower / upper half — every single-launch grid
starts with runs WITHOUT entries (the first colour of the lower half, the last of the upper one: the stand-in loads of
tri_stream_sf_kernel, any == false) behind and in front of padding runs, which info[9] / info[11] count.  Nothing here
sets NSK_IOPT_FAULT_INJECT, provokes a time-out or feeds a non-finite value to a kernel (DESIGN.md 5o has the answer on
those from the code).
"""
import ctypes as C
import functools
import time
from collections import Counter

import numpy as np
import pytest

from tests import spmv_reference as M
from tests import tri_reference as T

pytestmark = pytest.mark.gpu

ILU, SGS = 0, 1
NATURAL, MULTI = 0, 1
SF_SCALAR, COL_SCALAR, SF_BLK, COL_BLK, RING, WALKER = 1, 2, 3, 4, 5, 6
KIND = {ILU: "ilu", SGS: "sgs"}

TALLY = Counter()      # kernel instantiations launched over the module: printed at teardown (pytest -s)


class Args(C.Structure):
    _fields_ = [("n", C.c_int32), ("kind", C.c_int32), ("ordering", C.c_int32), ("n_sub", C.c_int32),
                ("rowptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("sub_off", C.c_void_p),
                ("xy", C.c_void_p), ("group", C.c_int32), ("want_block2", C.c_int32), ("use_stream", C.c_int32),
                ("sync_free", C.c_int32), ("tiny_bytes", C.c_double), ("host_analysis", C.c_int32),
                ("want_index16", C.c_int32), ("want_f32", C.c_int32), ("x_layout", C.c_int32), ("n_apply", C.c_int32),
                ("pad_", C.c_int32), ("b", C.c_void_p), ("x", C.c_void_p), ("perm_out", C.c_void_p),
                ("factor_out", C.c_void_p)]


def _ptr(a):
    return None if a is None else a.ctypes.data


def kernel_names(kind, info):
    """The instantiations one apply launched, from the hook's report."""
    path, vt, g = int(info[0]), "float" if info[1] == 32 else "double", int(info[4])
    k = KIND[kind]
    halves = (("lower", info[2], info[19], info[20]), ("upper", info[3], info[28], info[29]))
    out = []
    for half, width, level_steps, serial_steps in halves:
        if path == SF_SCALAR:
            out.append(f"tri_stream_sf_kernel<{vt}, {half}, {k}, GMAX {g}, {'I16' if width == 16 else 'int32'}>")
        elif path == COL_SCALAR:
            out.append(f"tri_stream_kernel<{vt}, {half}, {k}, {'I16' if width == 16 else 'int32'}>")
        elif path == SF_BLK:
            out.append(f"tri_blk_sf_kernel<{vt}, {half}, {k}, PERMX {int(info[32])}, GMAX {g}>")
        elif path == COL_BLK:
            out.append(f"tri_blk_kernel<{vt}, {half}, {k}>")
        elif path == RING:
            out.append(f"tri_ring_kernel<{k}, {half}>")
        elif path == WALKER:
            if level_steps:
                out.append(f"tri_level_kernel<{int(info[18])}, {k}, {half}>")
            if serial_steps:
                out.append(f"tri_serial_kernel<{k}, {half}>")
    if path == WALKER and info[21]:
        out.append("tiny: one workgroup walks all levels")
    if kind == ILU:
        out += ["ilu0_level_kernel"] * bool(info[23]) + ["ilu0_serial_kernel"] * bool(info[24])
    return out


class Run:
    def __init__(self, x, perm, factor, info):
        self.x, self.perm, self.factor, self.info = x, perm, factor, info

    @property
    def path(self):
        return int(self.info[0])


class Hook:
    def __init__(self):
        from navier_stokes_solver_amd import solver as S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_tri.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.ring_applies = 0

    def call(self, A, kind, ordering, bs, sub_off=None, xy=None, group=1, block2=False, use_stream=True, sync_free=False,
             tiny_bytes=0.0, host=False, index16=False, f32=False, x_layout=0):
        """One call of the hook: (return code, Run)."""
        n = A.n_rows
        bs = np.ascontiguousarray(np.stack(bs), dtype=np.float64)
        x = np.full_like(bs, np.nan)
        x[:] = -777.0           # what the kernels find in x: nothing they may use
        perm = np.full(n, -1, dtype=np.int32)
        factor = np.zeros(A.nnz)
        info = np.zeros(40, dtype=np.int32)
        so = None if sub_off is None else np.ascontiguousarray(sub_off, dtype=np.int32)
        xyc = None if xy is None else np.ascontiguousarray(xy, dtype=np.float64)
        a = Args(n, kind, ordering, 0 if so is None else len(so) - 1, _ptr(A.rowptr), _ptr(A.col), _ptr(A.val), _ptr(so),
                 _ptr(xyc), group, int(block2), int(use_stream), int(sync_free), float(tiny_bytes), int(host), int(index16),
                 int(f32), x_layout, len(bs), 0, _ptr(bs), _ptr(x), _ptr(perm), _ptr(factor))
        rc = self.L.nsk_debug_tri(self.ls.h, C.byref(a), _ptr(info))
        return rc, Run(x, perm.astype(np.int64), factor, info)

    def solve(self, A, kind, ordering, bs, what, **opts):
        """A call that must run: the checks every case shares, and the tally."""
        rc, r = self.call(A, kind, ordering, bs, **opts)
        assert rc == 0, (what, rc, self.ls.last_error())
        info = r.info
        assert info[15] == 0, f"{what}: {info[15]} guard words were written"
        assert info[14] == 0, f"{what}: sf_err was raised"
        st = self.ls.stats()
        assert st["sync_free_fallbacks"] == 0, what
        self.ring_applies += len(bs) if r.path == RING else 0
        assert st["ring_applies"] == self.ring_applies, (what, "ring_applies and the reported path disagree")
        assert 1 <= r.path <= 6, what
        for name in kernel_names(kind, info):
            TALLY[name] += 1
        return r


@pytest.fixture(scope="module")
def hook():
    t0 = time.time()
    h = Hook()
    yield h
    h.ls.close()
    print("\ntriangular-solve kernel instantiations launched:")
    for k, v in sorted(TALLY.items()):
        print(f"  {v:5d}  {k}")
    print(f"module wall time {time.time() - t0:.1f} s")


# ------------------------------------------------------------------ verification
_FACTOR_OK = {}     # (pattern, kind, perm, sub-domains) -> the factor whose defect was checked
_X_OK = {}          # (pattern, kind, perm, halves in fp32, b) -> x already verified, by bits


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} wrong rows, first {bad[:8].tolist()}, got {got[bad[:8]].tolist()}, "
                           f"want {want[bad[:8]].tolist()}")


def verify(A, kind, r, bs, what, sub_off=None, exact=False):
    """The factor and every x of a run against the reference; returns the permuted matrix."""
    keep = T.keep_mask(A, sub_off)
    P = T.Permuted(A, r.perm, keep)            # (asserts that perm is a permutation and every row kept its diagonal)
    assert r.info[31] == P.nnz, what
    assert np.array_equal(np.isnan(r.factor), ~keep), f"{what}: the dropped entries are not the cross-sub-domain ones"
    f = P.values(r.factor)
    a = P.values(A.val)
    key = (A.name, id(A), kind, r.perm.tobytes(), None if sub_off is None else tuple(sub_off))
    if kind == SGS:
        same(f, a, f"{what}: the SGS factor is not the matrix")
    elif key in _FACTOR_OK:
        same(f, _FACTOR_OK[key], f"{what}: the factor differs from the one of another run on this pattern and ordering")
    else:
        E, B, m = T.ilu0_defect(P, a, f)
        bad = np.nonzero(~(E <= B))[0]
        assert len(bad) == 0, (f"{what}: ILU(0) defect outside its bound at (row, column) of P "
                               f"{[(int(P.row[k]), int(P.col[k])) for k in bad[:6]]} = caller rows "
                               f"{r.perm[P.row[bad[:6]]].tolist()}, defect / bound {(E[bad[:6]] / np.maximum(B[bad[:6]], 1e-300)).tolist()}")
        _FACTOR_OK[key] = f.copy()
    path = T.PATH_NAME[r.path]
    f32 = r.info[1] == 32
    fh = T.round_halves_f32(P, f, block2=r.path in (SF_BLK, COL_BLK)) if f32 else f
    for k, b in enumerate(bs):
        xk = r.x[k]
        assert np.all(np.isfinite(xk)), f"{what}: apply {k}: non-finite entries in x at rows {np.nonzero(~np.isfinite(xk))[0][:8].tolist()}"
        done = _X_OK.setdefault(key + (bool(f32), b.tobytes(), path if not exact else "exact"), set())
        if xk.tobytes() in done:
            continue
        if exact:
            want, _ = T.int_solve(P, fh, b)
            if not np.array_equal(xk, want):      # name the rows where the relations break, not all the rows they spoil
                res, _ = T.residual_composed(P, fh, kind, b, xk, path)
                rows = np.nonzero(res != 0.0)[0]
                what = (f"{what}: rows of P whose exact residual is not zero {rows[:8].tolist()} = caller rows "
                        f"{r.perm[rows[:8]].tolist()}")
            same(xk, want, f"{what}: apply {k} ({path})")
        else:
            bad = T.check_solution(P, fh, kind, b, xk, path)
            assert not bad, (f"{what}: apply {k} ({path}): {len(bad)} rows outside the residual bound; (row of P, caller row, "
                             f"residual, bound) {bad[:6]}")
        done.add(xk.tobytes())
    return P


def run_case(hook, A, kind, ordering, what, path, exact=False, twice=True, b_seed=0, **opts):
    """Three applies (b0, b1, b0), the same with the right-hand sides swapped, and — twice — the first call again."""
    sub_off = opts.get("sub_off")
    if exact:
        perm = np.arange(A.n_rows) if ordering == NATURAL else T.multicolour_perm(
            A, sub_off, opts.get("block2", False), opts.get("xy"), opts.get("group", 1))[0]
        Pp = T.Permuted(A, perm, T.keep_mask(A, sub_off))
        b0, b1 = (T.integer_problem(Pp, Pp.values(A.val), law) for law in (0, 1))
    else:
        rng = np.random.default_rng(500 + b_seed)
        b0, b1 = rng.uniform(-1.0, 1.0, A.n_rows), rng.uniform(-1.0, 1.0, A.n_rows) * 10.0 ** rng.integers(-3, 3, A.n_rows)
    what = f"{what} [{A.name}, {KIND[kind]}, {'multicolour' if ordering else 'natural'}, {opts}]".replace("array", "")
    ra = hook.solve(A, kind, ordering, [b0, b1, b0], what, **opts)
    assert ra.path == path, f"{what}: took path {T.PATH_NAME[ra.path]}, meant {T.PATH_NAME[path]}; info {ra.info.tolist()}"
    verify(A, kind, ra, [b0, b1, b0], what, sub_off, exact)
    same(ra.x[2], ra.x[0], f"{what}: the third apply differs from the first (same right-hand side)")
    rb = hook.solve(A, kind, ordering, [b1, b0, b1], what, **opts)
    assert np.array_equal(rb.info, ra.info) and np.array_equal(rb.perm, ra.perm), what
    same(rb.factor[~np.isnan(rb.factor)], ra.factor[~np.isnan(ra.factor)], f"{what}: factor of the second call")
    same(rb.x[0], ra.x[1], f"{what}: a first apply on a fresh factor differs from a second apply on a used one")
    same(rb.x[1], ra.x[0], f"{what}: a second apply differs from a first apply on a fresh factor")
    same(rb.x[2], ra.x[1], f"{what}: third apply of the swapped call")
    if twice:
        rc = hook.solve(A, kind, ordering, [b0, b1, b0], what, **opts)
        same(rc.x.ravel(), ra.x.ravel(), f"{what}: the same call twice")
        same(rc.factor[~np.isnan(rc.factor)], ra.factor[~np.isnan(ra.factor)], f"{what}: the factor of the same call twice")
    return ra


def equal_runs(ra, rb, what, factor=True, x=True):
    """perm, factor and x of two runs bit for bit.  x = False: two branches whose rows sum in different orders (single-
    launch against per-colour kernels, the colour-ordered working vector against the caller's order, whose block columns
    sort differently): the project promises no equal bits there — each x met its own bound or the integer solve."""
    assert np.array_equal(ra.perm, rb.perm), f"{what}: perm differs"
    if factor:
        m = ~np.isnan(ra.factor)
        assert np.array_equal(m, ~np.isnan(rb.factor)), what
        same(ra.factor[m], rb.factor[m], f"{what}: factor")
    if x:
        same(ra.x.ravel(), rb.x.ravel(), f"{what}: x")


# ------------------------------------------------------------------ patterns (built once, never modified)
values, pattern = T.values, T.pattern


def pat(name):
    p = pattern(name)
    return p if isinstance(p, tuple) else (p, None)


@functools.lru_cache(maxsize=None)
def matrix(name, vals, seed=1):
    A, xy = pat(name)
    Av = values(A, vals, seed)
    Av.name = f"{name}:{vals}"
    if hasattr(A, "layers"):
        Av.layers = A.layers
    return Av, xy


# ------------------------------------------------------------------ sizes n = 1 .. 129, every path that takes them
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_small_sizes(hook, n, kind):
    for vals in ("int", "real") if kind == SGS else ("real",):
        A, _ = matrix(f"n{n}", vals)
        ex = vals == "int"
        run_case(hook, A, kind, MULTI, "sf scalar", SF_SCALAR, ex, sync_free=True)
        run_case(hook, A, kind, MULTI, "sf scalar i16 f32", SF_SCALAR, ex, sync_free=True, index16=True, f32=True)
        run_case(hook, A, kind, MULTI, "per-colour", COL_SCALAR, ex)
        run_case(hook, A, kind, MULTI, "walker, multicolour", WALKER, ex, use_stream=False)
        run_case(hook, A, kind, NATURAL, "walker, natural", WALKER, ex)
        r = run_case(hook, A, kind, MULTI, "tiny", WALKER, ex, sync_free=True, tiny_bytes=4.0e6)
        assert r.info[21] == 1 and r.info[19] == 0 and r.info[20] >= 1
        if n % 2 == 0:
            B = T.expand_nodes(pattern(f"n{n}"), f"n{n}:nodes")
            Bv = values(B, vals)
            Bv.name = f"n{n}:nodes:{vals}"
            run_case(hook, Bv, kind, MULTI, "sf blocked", SF_BLK, ex, block2=True, sync_free=True, x_layout=2)
            run_case(hook, Bv, kind, MULTI, "per-colour blocked", COL_BLK, ex, block2=True)


# ------------------------------------------------------------------ scalar single-launch: GMAX x value type x index width
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_scalar_single_launch_line_groups(hook, kind, group, f32):
    """The lattice with entries removed at random: chains of 1, 2 and 3 members in one factor, groups end at run
    boundaries.  Both index widths; 16-bit against int32 columns: the same bits."""
    for vals in ("int", "real") if kind == SGS else ("real",):
        A, xy = matrix("lattice", vals)
        runs = []
        for i16 in (False, True):
            r = run_case(hook, A, kind, MULTI, f"group {group}", SF_SCALAR, vals == "int", twice=not i16, xy=xy, group=group,
                         sync_free=True, index16=i16, f32=f32)
            assert r.info[4] == group and r.info[1] == (32 if f32 else 64), r.info.tolist()
            assert (r.info[2], r.info[3]) == ((16, 16) if i16 else (32, 32)), r.info.tolist()
            assert r.info[27] == (1 if group == 1 else 0)       # line groups: the symbolic set-up stays on the host
            assert r.info[9] > 0 and r.info[11] > 0             # padding runs in both grids
            runs.append(r)
        equal_runs(runs[0], runs[1], f"16-bit against int32 columns, group {group}, {KIND[kind]}, {vals}")


def test_line_groups_without_single_launch_take_the_walker(hook):
    A, xy = matrix("lattice", "real")
    r = run_case(hook, A, ILU, MULTI, "grouped, per-colour asked", WALKER, xy=xy, group=3, f32=True, index16=True)
    assert r.info[4] == 3 and r.info[1] == 64 and r.info[17] & 6 == 6      # fp32 and 16-bit asked for, not in use
    assert r.info[6] == r.info[5] * 3                                        # levels = colours x gmax


# ------------------------------------------------------------------ blocked single-launch: x_layout x GMAX x value type
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("group", [1, 2, 3])
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_blocked_single_launch(hook, kind, group, f32):
    for vals in ("int", "real") if kind == SGS else ("real",):
        A, xy = matrix("nodes_lattice", vals)
        runs = []
        for layout in (0, 2):
            r = run_case(hook, A, kind, MULTI, f"blocked group {group} layout {layout}", SF_BLK, vals == "int",
                         twice=layout == 0, xy=xy, group=group, block2=True, sync_free=True, x_layout=layout, f32=f32)
            assert r.info[4] == group and r.info[26] == 1 and r.info[1] == (32 if f32 else 64), r.info.tolist()
            assert r.info[2] == 0 and r.info[17] == 0
            runs.append(r)
        equal_runs(runs[0], runs[1], f"working vector in colour order against the caller's, group {group}", x=False)


def test_blocked_on_irregular_nodes_and_at_the_block_cap(hook):
    """Node rows of mixed length with empty halves; and node runs of exactly kBlkMax blocks, and one more."""
    for kind, vals in ((SGS, "int"), (ILU, "real"), (SGS, "real")):
        A, _ = matrix("nodes", vals)
        ra = run_case(hook, A, kind, MULTI, "irregular nodes", SF_BLK, vals == "int", block2=True, sync_free=True, x_layout=2)
        rb = run_case(hook, A, kind, MULTI, "irregular nodes", COL_BLK, vals == "int", block2=True)
        rh = run_case(hook, A, kind, MULTI, "irregular nodes, host", SF_BLK, vals == "int", twice=False, block2=True,
                      sync_free=True, x_layout=2, host=True)
        assert ra.info[27] == 1 and rh.info[27] == 0
        equal_runs(ra, rh, "blocked: device against host analysis")
        equal_runs(ra, rb, "blocked: single-launch against per-colour", x=False)
        A, _ = matrix("nodes_stair", vals)
        r = run_case(hook, A, kind, MULTI, "node runs at the cap", SF_BLK, vals == "int", block2=True, sync_free=True)
        first = A.layers
        assert np.array_equal(r.perm, np.arange(A.n_rows)) and r.info[5] == len(first) - 1
        Pn = T.Permuted(A, r.perm)
        lower_blocks = Pn.n_lower[0::2] // 2          # blocks towards earlier nodes: the own node's l10 is not one
        nl, rows, ent = T.run_plan(lower_blocks, first[1:-1], M.K_BLK_MAX)
        assert ent == M.K_BLK_MAX and r.info[8] == nl and r.info[13] == M.K_BLK_MAX, (r.info.tolist(), nl, rows, ent)
        # layer 4: 16 node rows x 64 blocks = one run of exactly the cap; layer 5: 17 x 61 = 1037 blocks: two runs
        assert lower_blocks[first[4]:first[5]].sum() == M.K_BLK_MAX and lower_blocks[first[5]:first[6]].sum() == 17 * 61


def test_block2_is_refused_on_odd_n_and_the_scalar_path_reported(hook):
    A, _ = matrix("odd_nodes", "real")
    r = run_case(hook, A, ILU, MULTI, "odd n", SF_SCALAR, block2=True, sync_free=True)
    assert r.info[26] == 0 and r.info[25] == 1 and r.info[17] & 1
    r = run_case(hook, A, ILU, MULTI, "odd n", COL_SCALAR, block2=True)
    assert r.info[17] & 1
    # even n without node structure
    A, _ = matrix("n64", "real")
    r = run_case(hook, A, SGS, MULTI, "no node structure", SF_SCALAR, block2=True, sync_free=True)
    assert r.info[17] & 1


def test_colour_ordered_vector_without_the_blocked_single_launch_is_refused(hook):
    A, _ = matrix("n64", "real")
    b = np.ones(A.n_rows)
    for opts in (dict(x_layout=2), dict(x_layout=2, block2=True), dict(x_layout=2, sync_free=True)):
        rc, r = hook.call(A, ILU, MULTI, [b], **opts)
        assert rc == 1 and r.info[16] == 1 and r.info[0] == 0, (opts, rc, r.info.tolist())
        assert np.all(r.x == -777.0)


# ------------------------------------------------------------------ per-colour kernels
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_per_colour_kernels(hook, kind, f32):
    for name in ("irregular", "nonsymmetric"):
        for vals in ("int", "real") if kind == SGS else ("real",):
            A, _ = matrix(name, vals)
            runs = []
            for i16 in (False, True):
                r = run_case(hook, A, kind, MULTI, "per-colour", COL_SCALAR, vals == "int", twice=not i16, index16=i16, f32=f32)
                assert (r.info[2], r.info[3]) == ((16, 16) if i16 else (32, 32)) and r.info[1] == (32 if f32 else 64)
                runs.append(r)
            equal_runs(runs[0], runs[1], f"per-colour: 16-bit against int32 columns on {name}")
            rs = run_case(hook, A, kind, MULTI, "single-launch", SF_SCALAR, vals == "int", twice=False, sync_free=True, f32=f32)
            equal_runs(runs[0], rs, f"per-colour against single-launch on {name}", x=False)
            if name == "nonsymmetric":
                rh = run_case(hook, A, kind, MULTI, "host analysis", COL_SCALAR, vals == "int", twice=False, host=True, f32=f32)
                assert runs[0].info[27] == 1 and rh.info[27] == 0
                equal_runs(runs[0], rh, "device against host analysis")
    A, _ = matrix("nodes", "real")
    r = run_case(hook, A, kind, MULTI, "per-colour blocked", COL_BLK, block2=True, f32=f32)
    assert r.info[1] == (32 if f32 else 64)


# ------------------------------------------------------------------ run boundaries, empty halves, a colour of one row
def odd_runs_with_a_successor(counts, cuts):
    """Runs of the half's plan (build_rowblocks as TriSolve::analyze calls it) that hold an odd number of entries and
    end in front of a later run with entries: the array position behind their last entry is another run's."""
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rb = M.build_rowblocks(rp, None, len(counts), M.K_STREAM_NNZ, [int(c) for c in cuts])
    ent = [int(rp[rb[k + 1]] - rp[rb[k]]) for k in range(len(rb) - 1)]
    return sum(1 for k, e in enumerate(ent) if e % 2 == 1 and any(ent[k + 1:]))


@pytest.mark.parametrize("kind", [ILU, SGS])
def test_runs_at_the_caps_and_colours_of_one_row(hook, kind):
    """stair: colours are the layers {300, 1, 70, 1, 64, 65, 32, 33, 129}; layer 6 holds 32 rows x 64 lower entries =
    exactly kStreamNnz in one run, layer 7 33 x 63 = 2079: two runs; layers 4 / 5 runs of exactly 64 rows and 64 + 1."""
    for vals in ("int", "real") if kind == SGS else ("real",):
        A, _ = matrix("stair", vals)
        first = A.layers
        runs = []
        for opts in (dict(sync_free=True), dict(sync_free=True, index16=True), dict(), dict(index16=True),
                     dict(sync_free=True, host=True)):
            path = SF_SCALAR if opts.get("sync_free") else COL_SCALAR
            r = run_case(hook, A, kind, MULTI, "stair", path, vals == "int", twice=False, **opts)
            assert np.array_equal(r.perm, np.arange(A.n_rows)) and r.info[5] == len(first) - 1, r.info.tolist()
            P = T.Permuted(A, r.perm)
            nl, rl, el = T.run_plan(P.n_lower, first[1:-1], M.K_STREAM_NNZ)
            nu, ru, eu = T.run_plan(P.n_upper, first[1:-1], M.K_STREAM_NNZ)
            assert (r.info[8], r.info[10], r.info[12], r.info[13]) == (nl, nu, max(rl, ru), max(el, eu)), (r.info.tolist(), nl, nu)
            assert r.info[12] == M.K_STREAM_ROWS and r.info[13] == M.K_STREAM_NNZ
            assert P.n_lower[first[6]:first[7]].sum() == M.K_STREAM_NNZ and P.n_lower[first[7]:first[8]].sum() == 33 * 63
            # the single-launch grids pad every colour to a multiple of eight runs
            per_colour = lambda cnt: sum(-(-T.run_plan(cnt[first[q]:first[q + 1]], [], M.K_STREAM_NNZ)[0] // 8) * 8   # noqa: E731
                                         for q in range(len(first) - 1))
            assert r.info[8] + r.info[9] == per_colour(P.n_lower) and r.info[10] + r.info[11] == per_colour(P.n_upper)
            if opts.get("index16"):
                # the pair load of 16-bit offsets: a run that ends on an ODD entry has another run's first offset in the
                # high half-word of its last load, which the kernel must drop — in both halves, on 16-bit offsets
                assert (r.info[2], r.info[3]) == (16, 16), r.info.tolist()
                for half, cnt in (("lower", P.n_lower), ("upper", P.n_upper)):
                    assert odd_runs_with_a_successor(cnt, first[1:-1]) >= 1, half
            runs.append(r)
        equal_runs(runs[0], runs[1], "stair: single-launch, 16-bit against int32 columns")
        equal_runs(runs[0], runs[4], "stair: single-launch, host against device analysis")
        equal_runs(runs[2], runs[3], "stair: per-colour, 16-bit against int32 columns")
        equal_runs(runs[0], runs[2], "stair: single-launch against per-colour", x=False)


@pytest.mark.parametrize("kind", [ILU, SGS])
@pytest.mark.parametrize("name", ["stair_lower", "stair_upper", "diagonal", "stair_nonsymmetric"])
def test_empty_halves_and_nonsymmetric_patterns(hook, kind, name):
    """One half empty in EVERY row: the other half alone, row by row (tri_reference.residual_alone); the diagonal alone;
    and a nonsymmetric staircase.  Every path that takes the pattern."""
    for vals in ("int", "real") if kind == SGS else ("real",):
        A, _ = matrix(name, vals)
        ex = vals == "int"
        ref = None
        for what, path, ordering, opts in (
                ("sf", SF_SCALAR, MULTI, dict(sync_free=True)), ("sf i16 f32", SF_SCALAR, MULTI, dict(sync_free=True, index16=True, f32=True)),
                ("per-colour", COL_SCALAR, MULTI, dict()), ("per-colour i16", COL_SCALAR, MULTI, dict(index16=True)),
                ("walker", WALKER, MULTI, dict(use_stream=False)), ("walker natural", WALKER, NATURAL, dict())):
            r = run_case(hook, A, kind, ordering, what, path, ex, twice=False, **opts)
            P = T.Permuted(A, r.perm)
            if name == "stair_lower":
                assert not P.n_upper.any()
            if name == "stair_upper":
                assert not P.n_lower.any()
            if ex:      # integers: every path gives the same bits
                ref = ref or r
                same(r.x.ravel(), ref.x.ravel(), f"{name} {what}")


# ------------------------------------------------------------------ sub-domains
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_emulated_sub_domains_with_an_empty_one(hook, kind):
    for name, block2, offs in (("irregular", False, [0, 700, 700, 1501, 2300]), ("nodes", True, [0, 600, 600, 1800])):
        for vals in ("int", "real") if kind == SGS else ("real",):
            A, _ = matrix(name, vals)
            keep = T.keep_mask(A, offs)
            assert 0 < (~keep).sum() < A.nnz
            sf, col = (SF_BLK, COL_BLK) if block2 else (SF_SCALAR, COL_SCALAR)
            ra = run_case(hook, A, kind, MULTI, "sub-domains", sf, vals == "int", twice=False, sub_off=offs, block2=block2,
                          sync_free=True, index16=not block2)
            assert ra.info[27] == 0
            rb = run_case(hook, A, kind, MULTI, "sub-domains", col, vals == "int", twice=False, sub_off=offs, block2=block2)
            equal_runs(ra, rb, f"sub-domains on {name}", x=False)
            rw = run_case(hook, A, kind, NATURAL, "sub-domains, natural", WALKER, vals == "int", twice=False, sub_off=offs)
            assert np.array_equal(np.isnan(rw.factor), ~keep)


# ------------------------------------------------------------------ the caller's order: ring, walker, tiny
@functools.lru_cache(maxsize=None)
def ring_matrix(which, vals):
    """Layers in the caller's order (levels = layers): 4 200 rows, levels of 300 .. 600 rows (more than the 256 of one
    pass), 0 .. 16 entries per half and row, many rows with exactly 16; 'ring17': one row with 17 strict-lower entries,
    'ring17u': one with 17 strict-upper ones."""
    sizes = [600, 330, 400, 500, 350, 420, 300, 450, 380, 470]
    rng = np.random.default_rng(60)
    n = sum(sizes)
    nl, nu = rng.integers(0, T.K_RING_HALF + 1, n), rng.integers(0, T.K_RING_HALF + 1, n)
    nl[2000], nu[2001] = T.K_RING_HALF, T.K_RING_HALF
    if which == "ring17":
        nl[3000] = T.K_RING_HALF + 1
    if which == "ring17u":
        nu[1000] = T.K_RING_HALF + 1
    A = T.banded(sizes, 61, nl, nu, name=which)
    Av = values(A, vals, 3)
    Av.name, Av.layers = f"{which}:{vals}", A.layers
    return Av


@pytest.mark.parametrize("kind", [ILU, SGS])
def test_ring_against_walker(hook, kind):
    for vals in ("int", "real") if kind == SGS else ("real",):
        for which in ("ring",):
            A = ring_matrix(which, vals)
            P = T.Permuted(A, np.arange(A.n_rows))
            assert P.n_lower.max() == T.K_RING_HALF and P.n_upper.max() == T.K_RING_HALF
            rr = run_case(hook, A, kind, NATURAL, "ring", RING, vals == "int", twice=False)
            assert rr.info[22] > 0 and rr.info[17] == 0
            rw = run_case(hook, A, kind, NATURAL, "walker", WALKER, vals == "int", twice=False, use_stream=False)
            # levels below 1024 rows: serial steps, 8 lanes per row — the ring promises THEIR bits
            assert rw.info[19] == 0 and rw.info[20] >= 1 and rw.info[6] == len(A.layers) - 1
            equal_runs(rr, rw, f"ring against walker on {which}")
        for which in ("ring17", "ring17u"):
            A = ring_matrix(which, vals)
            r = run_case(hook, A, kind, NATURAL, "17 entries in a half", WALKER, vals == "int", twice=False)
            assert r.info[22] == 0 and r.info[17] & 8


@functools.lru_cache(maxsize=None)
def long_ring_matrix():
    """60 000 rows in 30 layers of 2 000, the caller's order; every row holds 1 .. 8 entries in the layer before its own
    and 1 .. 8 in the one after it, so a row's level is its layer in both halves, whichever way the ring's planner moves
    rows between levels, and no dependency is more than 4 000 positions long: 8 passes a level, 60 000 positions — more
    than three times round the ring of 16 384 slots.  Integer-exact."""
    rng = np.random.default_rng(62)
    A = T.banded([2000] * 30, 62, rng.integers(1, 9, 60000), rng.integers(1, 9, 60000), name="ring_long", reach=2000)
    Av = T.integer_values(A, 5, p_zero=0.1, amax=3)
    Av.name, Av.layers = "ring_long:int", A.layers
    return Av


def test_ring_several_times_round(hook):
    A = long_ring_matrix()
    r = run_case(hook, A, SGS, NATURAL, "ring, 60 000 rows", RING, True, twice=False)
    assert r.info[22] >= 30 * 8 and A.n_rows > 3 * 16384
    rw = run_case(hook, A, SGS, NATURAL, "walker, 60 000 rows", WALKER, True, twice=False, use_stream=False)
    assert rw.info[19] == 30 and rw.info[28] == 30 and rw.info[18] == 4    # levels of 2 000 rows: level steps, 4 lanes
    same(rw.x.ravel(), r.x.ravel(), "ring against walker, integers")


@functools.lru_cache(maxsize=None)
def wide_matrix(per_row, long_half, vals):
    """Two levels of 1 100 rows (level steps of the walker): the rows of the second hold per_row strict-lower entries and
    those of the first 2 strict-upper ones (long_half 'lower'), or the other way round."""
    cnt = [np.r_[np.zeros(1100), np.full(1100, per_row)], np.r_[np.full(1100, 2), np.zeros(1100)]]
    if long_half == "upper":
        cnt = [np.r_[np.zeros(1100), np.full(1100, 2)], np.r_[np.full(1100, per_row), np.zeros(1100)]]
    A = T.banded([1100, 1100], 70 + per_row, cnt[0], cnt[1], name=f"wide{per_row}{long_half}")
    Av = values(A, vals, 4)
    Av.name, Av.layers = f"wide{per_row}{long_half}:{vals}", A.layers
    return Av


@pytest.mark.parametrize("long_half", ["lower", "upper"])
@pytest.mark.parametrize("per_row,lpr", [(16, 4), (40, 8), (120, 16), (200, 32)])
def test_walker_level_steps_at_every_lanes_per_row(hook, per_row, lpr, long_half):
    for kind, vals in ((SGS, "int"), (ILU, "real"), (SGS, "real")):
        A = wide_matrix(per_row, long_half, vals)
        mean_half = 0.5 * A.nnz / A.n_rows          # TriSolve::analyze: <= 6: 4 lanes, <= 14: 8, <= 48: 16, else 32
        assert lpr == (4 if mean_half <= 6 else 8 if mean_half <= 14 else 16 if mean_half <= 48 else 32), mean_half
        r = run_case(hook, A, kind, NATURAL, f"walker lpr {lpr}", WALKER, vals == "int", twice=False)
        assert r.info[18] == lpr and r.info[19] == 2 and r.info[28] == 2 and r.info[20] == 0, r.info.tolist()
        if kind == ILU:
            assert r.info[23] == 2 and r.info[24] == 0       # one factorisation launch per level of 1 100 rows
    A = wide_matrix(per_row, long_half, "real")
    r = run_case(hook, A, SGS, MULTI, f"walker lpr {lpr}, multicolour", WALKER, twice=False, use_stream=False)
    assert r.info[18] == lpr


def test_tiny_factors_take_one_workgroup(hook):
    for kind, vals in ((SGS, "int"), (ILU, "real")):
        A, _ = matrix("irregular", vals)
        r = run_case(hook, A, kind, MULTI, "tiny", WALKER, vals == "int", sync_free=True, index16=True, f32=True,
                     tiny_bytes=4.0e6)
        assert r.info[21] == 1 and r.info[25] == 1 and r.info[1] == 64 and r.info[17] & 6 == 6
        assert r.info[19] == 0 and r.info[20] == 1 and r.info[29] == 1      # all levels in ONE serial step per half
        if kind == ILU:
            assert r.info[24] >= 1                                           # levels below 48 rows: the serial factorisation
        A, _ = matrix("nodes", vals)
        r = run_case(hook, A, kind, MULTI, "tiny, node structure", WALKER, vals == "int", block2=True, sync_free=True,
                     tiny_bytes=4.0e6)
        assert r.info[21] == 1 and r.info[26] == 1


# ------------------------------------------------------------------ rows at the length cap
@functools.lru_cache(maxsize=None)
def long_row_matrix(width):
    """800 rows of three entries, row 500 with `width` stored entries, 224 of them behind the diagonal."""
    rows = [sorted({i, (i * 7 + 3) % 800, (i * 13 + 5) % 800}) for i in range(800)]
    rows[500] = sorted(set(range(500 - (width - 225), 500)) | {500} | set(range(501, 501 + 224)))
    A = T.csr(800, [np.array(r) for r in rows], f"row{width}")
    assert A.row_len[500] == width
    return A


def test_a_row_of_448_entries_runs_and_449_is_an_error(hook):
    A = T.dominant_values(long_row_matrix(448), 6)
    A.name = "row448:real"
    for path, opts in ((SF_SCALAR, dict(sync_free=True)), (COL_SCALAR, dict(index16=True)), (WALKER, dict(use_stream=False))):
        r = run_case(hook, A, ILU, MULTI, "448 entries", path, twice=False, **opts)
        assert r.info[30] == T.K_ROW_MAX
    run_case(hook, A, ILU, NATURAL, "448 entries", WALKER, twice=False)
    Ai = T.integer_values(long_row_matrix(448), 6, p_zero=0.1, amax=3)
    Ai.name = "row448:int"
    run_case(hook, Ai, SGS, MULTI, "448 entries", SF_SCALAR, True, twice=False, sync_free=True, f32=True)
    B = T.dominant_values(long_row_matrix(449), 6)
    for ordering in (MULTI, NATURAL):
        rc, r = hook.call(B, ILU, ordering, [np.ones(800)], sync_free=True)
        assert rc == -32 and r.info[0] == 0, (rc, hook.ls.last_error())


def test_a_row_without_diagonal_is_an_error(hook):
    A = T.csr(3, [np.array([0, 1]), np.array([0, 2]), np.array([2])]).with_values(np.ones(5))
    rc, _ = hook.call(A, SGS, MULTI, [np.ones(3)])
    assert rc == -31


# ------------------------------------------------------------------ above 65 536 columns
@functools.lru_cache(maxsize=None)
def big_matrix():
    """80 000 rows in 8 layers, about 13 entries per row; a row of the last layer holds a column in every earlier one — the
    first 10 000 and the 60 000s among them — so its run spans more than 65 536 columns.  Integer-exact."""
    A = T.stair([10000] * 8, 63, extra=3, name="big")
    Av = T.integer_values(A, 7, p_zero=0.1, amax=3)
    Av.name, Av.layers = "big:int", A.layers
    return Av


def test_a_run_spanning_65536_columns_keeps_int32_columns(hook):
    A = big_matrix()
    assert A.n_rows > 65536 + 4096
    for path, opts in ((SF_SCALAR, dict(sync_free=True)), (COL_SCALAR, dict())):
        r = run_case(hook, A, SGS, MULTI, "80 000 rows, 16-bit asked", path, True, twice=False, index16=True, f32=True, **opts)
        assert (r.info[2], r.info[3]) == (32, 32) and r.info[17] & 2 and r.info[1] == 32, r.info.tolist()
        assert r.info[27] == 1 and np.array_equal(r.perm, np.arange(A.n_rows))


# ------------------------------------------------------------------ promised equalities on one irregular pattern
@pytest.mark.parametrize("kind", [ILU, SGS])
def test_promised_equalities(hook, kind):
    """fp32 against fp64 halves on off-diagonals that are exact in float (SGS: the halves then hold the same numbers);
    16-bit against int32 columns; device against host analysis; single-launch against per-colour."""
    A, _ = matrix("irregular", "real32")
    base = run_case(hook, A, kind, MULTI, "base", SF_SCALAR, sync_free=True)
    for what, path, opts in (("16-bit", SF_SCALAR, dict(sync_free=True, index16=True)),
                             ("host analysis", SF_SCALAR, dict(sync_free=True, host=True)),
                             ("host analysis, 16-bit", SF_SCALAR, dict(sync_free=True, host=True, index16=True)),
                             ("per-colour", COL_SCALAR, dict()), ("per-colour, host", COL_SCALAR, dict(host=True))):
        r = run_case(hook, A, kind, MULTI, what, path, twice=False, **opts)
        assert r.info[27] == (0 if opts.get("host") else 1)
        if what == "per-colour":
            base_colour = r
        equal_runs(base_colour if what == "per-colour, host" else base, r,
                   f"{what} against the device-analysed int32 solve of the same branch", x=what != "per-colour")
    if kind == SGS:
        for opts in (dict(sync_free=True, f32=True), dict(sync_free=True, f32=True, index16=True), dict(f32=True)):
            r = run_case(hook, A, kind, MULTI, "fp32 halves", SF_SCALAR if opts.get("sync_free") else COL_SCALAR, twice=False, **opts)
            assert r.info[1] == 32
            equal_runs(base if opts.get("sync_free") else base_colour, r, "fp32 against fp64 halves on float-exact off-diagonals")
        B, _ = matrix("nodes", "real32")
        rb = run_case(hook, B, kind, MULTI, "blocked", SF_BLK, block2=True, sync_free=True, x_layout=2)
        r32 = run_case(hook, B, kind, MULTI, "blocked fp32", SF_BLK, twice=False, block2=True, sync_free=True, x_layout=2, f32=True)
        equal_runs(rb, r32, "blocked: fp32 against fp64 halves on float-exact off-diagonals")


# ------------------------------------------------------------------ the tally
def expected_instantiations():
    out = set()
    for half in ("lower", "upper"):
        for k in KIND.values():
            for vt in ("double", "float"):
                for g in (1, 2, 3):
                    for w in ("int32", "I16"):
                        out.add(f"tri_stream_sf_kernel<{vt}, {half}, {k}, GMAX {g}, {w}>")
                    for px in (0, 1):
                        out.add(f"tri_blk_sf_kernel<{vt}, {half}, {k}, PERMX {px}, GMAX {g}>")
                for w in ("int32", "I16"):
                    out.add(f"tri_stream_kernel<{vt}, {half}, {k}, {w}>")
                out.add(f"tri_blk_kernel<{vt}, {half}, {k}>")
            out.add(f"tri_ring_kernel<{k}, {half}>")
            out.add(f"tri_serial_kernel<{k}, {half}>")
            for lpr in (4, 8, 16, 32):
                out.add(f"tri_level_kernel<{lpr}, {k}, {half}>")
    out |= {"tiny: one workgroup walks all levels", "ilu0_level_kernel", "ilu0_serial_kernel"}
    return out


def test_zz_tally_is_complete(hook):
    """Runs last in the module: every instantiation TriSolve::apply and numeric() can reach was launched by a case that
    asserted it.  (Run the whole module: a subset leaves names missing.)"""
    missing = sorted(expected_instantiations() - set(TALLY))
    assert not missing, f"{len(missing)} instantiations never ran: {missing}"
    unknown = sorted(set(TALLY) - expected_instantiations())
    assert not unknown, f"instantiations the list does not know: {unknown}"
