"""The Krylov vector kernels one by one against exact references (nsk_internal.h: nsk_debug_krylov).

Every Krylov iteration runs grid-wide reductions, fused Gram-Schmidt passes, the one-launch modified Gram-Schmidt sweep,
the single-reduction CG steps and the AMG smoother's vector step.  A whole solve is a poor detector for them: the outer
FGMRES checks its true residual, so a kernel that drops or double-counts one entry, or takes the wrong h_k, only costs
iterations.  Here each one runs alone, through the entry points the solvers call, on the handle's own reduction
workspace, slots and sweep tables, with the pair kernels on and off (NSK_OPT_BLAS1_PAIRS) and with the vectors 16-byte
aligned or not (offset 0 / 1: the pair launchers fall back to the 8-byte kernels), and the hook reports which kernel
ran, so every case asserts its own coverage.  Every vector sits between guard words; a write outside it fails the case.

Two kinds of input:

* Integer-exact: every product and every partial sum is an integer below 2^53, so any summation order gives the exact
  value and the GPU must return it bit for bit.  A dropped or duplicated entry is an exact integer difference (with
  x = 1, y_i = i + 1 it names the index).  These carry the large sizes: the grid caps (512 workgroups for the 8-byte
  reductions, 128 for the pair dot, 256 for the pair multi_* kernels: 2 * 128 * 4096 = 1 048 576 and 2 097 152 = 512 *
  4096, +-1), the headline velocity size 8 575 416 / 8 575 417, and the sweep's tiers G * 1024 * {4, 8, 12} +- 1.

* Random, against the correctly rounded sum (tests/krylov_reference.py), at n <= 2^20, with
      |s_gpu - s| <= 64 u sum_i |x_i y_i|,   u = 2^-53.
  Why 64: a sum formed by a tree in which no term passes more than d roundings is within d u / (1 - d u) * sum |terms|
  of the exact one.  Counting the roundings a product can pass at n <= 2^20 (RBLK = 1024 threads, 16 waves of 64):
  the product (or the pair f2 = x0 y0 + x1 y1: 2), the thread's chain (reduce1 / reduce2 / dot3: <= 4 trips in four
  chains, 0 adds after the first, then (a0 + a1) + (a2 + a3): 2; multi_dot2: 8 products in ONE chain, 7; the sweep: E <=
  12 entries per thread, 11), the 64-lane shuffle tree (6), the 16-wave sum of the workgroup (15), and the cross-
  workgroup pass (<= 512 partials over 1024 threads: at most one per thread, exact; shuffle tree 6; 16-wave sum 15 —
  the sweep: G <= 1024 partials, tree 6, <= 16 serial).  The longest is multi_dot2's 1 + 7 + 6 + 15 + 6 + 15 = 50, the
  sweep's 1 + 11 + 6 + 15 + 6 + 16 = 55: all below 64.  (At n = 2^24 the pair dot's 128-workgroup grid gives 16 trips
  per chain: 2 + 15 + 2 + 42 = 61, still inside, but the single-chain multi_dot forms reach 75-106: the large sizes are
  therefore integer-exact only.)  Element-wise results (multi_axpy, the CG updates, the Chebyshev step) are held to
  (m + 2) u (|w| + sum_k |h_k| |v_k|) per entry: each of the m + 1 operations of an entry rounds once (or fuses).
"""
import ctypes as C
import functools
import math
from collections import Counter

import numpy as np
import pytest

from tests import krylov_reference as R

pytestmark = pytest.mark.gpu

U = R.U
DOT, NORM2, AXPY_DOT, AXPY_NORM2, CG_UPDATE, MULTI_DOT, MULTI_AXPY, GS_COLUMN, DOT3, CG_SCALARS, CG_FUSED_UPDATE, \
    CHEBY, DENSE_MV = range(13)
SCALAR, PAIRS = 1, 2          # info[0] bits: the 8-byte-per-lane and the 16-byte pair reduction kernels
GS_MGS, GS_CGS, GS_ONE_RED = 0, 1, 2   # NSK_OPT_INNER_FUSED_GS of the column routine

SMALL = [1, 2, 3, 63, 64, 65, 1023, 1025, 4095, 4096, 4097]
CAPS = [1_048_575, 1_048_576, 1_048_577, 2_097_151, 2_097_152, 2_097_153]
HEADLINE = [8_575_416, 8_575_417]

PATHS = Counter()   # (op, what ran) over the module: printed at teardown (pytest -s)


class Hook:
    def __init__(self):
        from navier_stokes_solver_amd import solver as S
        self.S = S
        self.ls = S.LinearSolver()
        self.L = S.lib()
        self.L.nsk_debug_krylov.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.pairs = None
        self.fused_mgs = 1

    def set_pairs(self, p):
        self.ls.set_option(self.S.OPT_BLAS1_PAIRS, p)
        self.pairs = p

    def set_fused_mgs(self, f):
        self.ls.set_option(self.S.IOPT_FUSED_MGS, f)
        self.fused_mgs = f

    def run(self, op, vecs, n, m=0, offset=0, par=()):
        """Runs the op on copies of vecs; returns (vectors after the op, 64 slots, info)."""
        arrs = [np.array(v, dtype=np.float64, copy=True).ravel() for v in vecs]
        ptrs = (C.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
        lens = np.array([a.size for a in arrs] or [0], dtype=np.int64)
        p = np.zeros(64)
        p[:len(par)] = par
        slots = np.empty(64)
        info = np.zeros(8, dtype=np.int32)
        rc = self.L.nsk_debug_krylov(self.ls.h, op, n, m, offset, p.ctypes.data, len(arrs), ptrs, lens.ctypes.data,
                                     slots.ctypes.data, info.ctypes.data)
        assert rc == 0, (rc, self.ls.last_error())
        assert info[3] == 0, f"op {op}, n {n}, offset {offset}: {info[3]} guard words around the vectors were written"
        PATHS[(op, int(info[0]), int(info[1]))] += 1
        return arrs, slots, info


@pytest.fixture(scope="module")
def hook():
    h = Hook()
    yield h
    h.ls.close()
    print("\nkernel paths (op, reduction bits, sweep tier):", dict(sorted(PATHS.items())))


def red_kind(pairs, offset, n):
    return PAIRS if (pairs and offset == 0 and n >= 2) else SCALAR


def axpy_kind(offset, n):   # multi_axpy without the norm: pairs whenever aligned (entry by entry: the same bits)
    return PAIRS if (offset == 0 and n >= 2) else SCALAR


# ------------------------------------------------------------------ integer-exact inputs (cached per size)
@functools.lru_cache(maxsize=4)
def ints(n):
    i = np.arange(n, dtype=np.int64)
    return {
        "one": np.ones(n), "ramp": (i + 1).astype(np.float64), "i": i,
        "m7": (i % 7 - 3).astype(np.float64), "m5": (i % 5 - 2).astype(np.float64),
        "m3": (i % 3 - 1).astype(np.float64), "m11": (i % 11).astype(np.float64),
    }


def root_ok(root, sq):
    """The kernels' sqrt(|s|): correctly rounded or within one ulp."""
    want = math.sqrt(abs(sq))
    return abs(root - want) <= 2 * U * want


def exact_int_dot(a, b):
    return float(np.dot(a.astype(np.int64), b.astype(np.int64)))


def check_ramp_dot(got, n, what):
    want = n * (n + 1) // 2
    assert math.isfinite(got), f"{what}: {got}"
    d = int(got) - want
    assert got == want, f"{what}: off by {d} (an entry {'counted twice' if d > 0 else 'dropped'}: index {abs(d) - 1})"


@functools.lru_cache(maxsize=2)
def multi_vecs(n):
    """Integer-exact inputs of the multi_* kernels: dot basis v_k[i] = (i + 1) + k (i % 7), axpy basis
    (i % (k + 3)) - 1, both distinct for every k."""
    I = ints(n)
    return ([I["ramp"] + k * (I["i"] % 7) for k in range(8)],
            [(I["i"] % (k + 3) - 1).astype(np.float64) for k in range(8)])


# ------------------------------------------------------------------ reductions, integer-exact, all sizes
def _reduction_ops(hook, n, pairs, offset):
    I = ints(n)
    k = red_kind(pairs, offset, n)
    _, s, info = hook.run(DOT, [I["one"], I["ramp"]], n, offset=offset)
    check_ramp_dot(s[0], n, f"dot n={n} pairs={pairs} offset={offset}")
    assert info[0] == k
    _, s, info = hook.run(NORM2, [I["m7"]], n, offset=offset)
    ww = exact_int_dot(I["m7"], I["m7"])
    assert s[0] == ww and root_ok(s[1], ww) and info[0] == k, n
    (x, y, w), s, info = hook.run(AXPY_DOT, [I["one"], I["i"].astype(float), I["one"]], n, offset=offset, par=[2.0])
    assert np.array_equal(y, I["i"] + 2.0) and info[0] == k
    assert s[0] == float((I["i"] + 2).sum()), n
    (x, y), s, info = hook.run(AXPY_NORM2, [I["one"], I["m5"]], n, offset=offset, par=[-1.0])
    assert np.array_equal(y, I["m5"] - 1.0) and info[0] == k
    assert s[0] == exact_int_dot(y, y) and root_ok(s[1], s[0]), n
    (d, hh, x, g), s, info = hook.run(CG_UPDATE, [I["one"], I["m3"], I["m11"], I["m5"]], n, offset=offset, par=[2.0])
    assert np.array_equal(x, I["m11"] + 2.0) and np.array_equal(g, I["m5"] + 2.0 * I["m3"]) and info[0] == k
    assert s[0] == exact_int_dot(g, g) and root_ok(s[1], s[0]), n
    (r, u, w), s, info = hook.run(DOT3, [I["m7"], I["ramp"], I["m3"]], n, offset=offset)
    assert list(s[:3]) == [exact_int_dot(I["m7"], I["ramp"]), exact_int_dot(I["m3"], I["ramp"]),
                           exact_int_dot(I["m7"], I["m7"])], n
    assert info[0] == SCALAR


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("offset", [0, 1])
def test_reductions_integer_exact_small_and_caps(hook, pairs, offset):
    hook.set_pairs(pairs)
    for n in SMALL + CAPS:
        _reduction_ops(hook, n, pairs, offset)


@pytest.mark.parametrize("n", HEADLINE)
def test_reductions_integer_exact_headline(hook, n):
    for pairs, offset in ((1, 0), (0, 0)):   # (offset 1 runs the kernel of pairs 0)
        hook.set_pairs(pairs)
        _reduction_ops(hook, n, pairs, offset)


def _multi(hook, n, m, pairs, offset):
    I = ints(n)
    V, Vs = multi_vecs(n)
    V, Vs = V[:m], Vs[:m]
    w = 1.0 + (I["i"] & 1)
    _, s, info = hook.run(MULTI_DOT, [w] + V, n, m=m, offset=offset)
    want = [exact_int_dot(w, v) for v in V]
    assert list(s[:m]) == want, (n, m, pairs, offset, np.array(s[:m]) - want)
    assert info[0] == red_kind(pairs, offset, n)
    # multi_axpy: small integers everywhere
    hk = [float(k + 1) for k in range(m)]
    want_w = I["m11"].copy()
    for h_, v in zip(hk, Vs):
        want_w = want_w - h_ * v
    for norm in (1, 0):
        (wn, *_), s, info = hook.run(MULTI_AXPY, [I["m11"]] + Vs, n, m=m, offset=offset, par=hk + [norm])
        assert np.array_equal(wn, want_w), (n, m, norm, np.flatnonzero(wn != want_w)[:5])
        assert list(s[:m]) == hk
        if norm:
            assert s[m] == exact_int_dot(want_w, want_w) and root_ok(s[m + 1], s[m]), (n, m)
            assert info[0] == red_kind(pairs, offset, n)
        else:
            assert np.isnan(s[m]) and info[0] == axpy_kind(offset, n)


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("offset", [0, 1])
def test_multi_dot_axpy_every_m_integer_exact(hook, pairs, offset):
    hook.set_pairs(pairs)
    for n in (1, 2, 3, 65, 4097) + ((1_048_577, 2_097_153) if offset == 0 else (1_048_575,)):
        for m in range(1, 9):
            _multi(hook, n, m, pairs, offset)


def test_multi_dot_axpy_headline(hook):
    for n, m, pairs, offset in ((HEADLINE[1], 8, 1, 0), (HEADLINE[1], 3, 0, 0), (HEADLINE[0], 2, 1, 1)):
        hook.set_pairs(pairs)
        _multi(hook, n, m, pairs, offset)


# ------------------------------------------------------------------ reductions, random, against the exact sum
def _rand(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _near(got, want, bound, what):
    assert abs(got - want) <= bound, f"{what}: |{got!r} - {want!r}| = {abs(got - want):.3e} > {bound:.3e}"


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("offset", [0, 1])
def test_reductions_random_against_exact_sum(hook, pairs, offset):
    hook.set_pairs(pairs)
    for n in (1, 3, 64, 65, 4097, 100_003, 1 << 20):
        x, y, z, g = _rand(n, 1), _rand(n, 2), _rand(n, 3), _rand(n, 4)
        _, s, info = hook.run(DOT, [x, y], n, offset=offset)
        _near(s[0], R.exact_dot(x, y), 64 * U * R.abs_dot(x, y), f"dot {n}")
        _, s, _ = hook.run(NORM2, [x], n, offset=offset)
        _near(s[0], R.exact_dot(x, x), 64 * U * R.abs_dot(x, x), f"norm2 {n}")
        assert root_ok(s[1], s[0])
        a = 0.37
        (_, yn, _), s, _ = hook.run(AXPY_DOT, [x, y, z], n, offset=offset, par=[a])
        assert np.all(np.abs(yn - (y + a * x)) <= 2 * U * (np.abs(y) + np.abs(a * x)))
        _near(s[0], R.exact_dot(yn, z), 64 * U * R.abs_dot(yn, z), f"axpy_dot {n}")
        (_, yn), s, _ = hook.run(AXPY_NORM2, [x, y], n, offset=offset, par=[a])
        _near(s[0], R.exact_dot(yn, yn), 64 * U * R.abs_dot(yn, yn), f"axpy_norm2 {n}")
        (_, _, xn, gn), s, _ = hook.run(CG_UPDATE, [x, y, z, g], n, offset=offset, par=[a])
        assert np.all(np.abs(xn - (z + a * x)) <= 2 * U * (np.abs(z) + np.abs(a * x)))
        assert np.all(np.abs(gn - (g + a * y)) <= 2 * U * (np.abs(g) + np.abs(a * y)))
        _near(s[0], R.exact_dot(gn, gn), 64 * U * R.abs_dot(gn, gn), f"cg_update {n}")
        _, s, _ = hook.run(DOT3, [x, y, z], n, offset=offset)
        for got, (p, q) in zip(s[:3], ((x, y), (z, y), (x, x))):
            _near(got, R.exact_dot(p, q), 64 * U * R.abs_dot(p, q), f"dot3 {n}")


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("offset", [0, 1])
def test_multi_random_against_exact_sum(hook, pairs, offset):
    hook.set_pairs(pairs)
    for n in (3, 4097, 1 << 20):
        w = _rand(n, 10)
        V = [_rand(n, 11 + k) for k in range(8)]
        for m in ((1, 3, 8) if n < 1 << 20 else (2, 8)):
            _, s, _ = hook.run(MULTI_DOT, [w] + V[:m], n, m=m, offset=offset)
            for k in range(m):
                _near(s[k], R.exact_dot(w, V[k]), 64 * U * R.abs_dot(w, V[k]), f"multi_dot {n} {m} {k}")
            h = [0.5 - 0.1 * k for k in range(m)]
            (wn, *_), s, _ = hook.run(MULTI_AXPY, [w] + V[:m], n, m=m, offset=offset, par=h + [1])
            ref = w.copy()
            scale = np.abs(w)
            for hk, v in zip(h, V[:m]):
                ref = ref - hk * v
                scale = scale + abs(hk) * np.abs(v)
            assert np.all(np.abs(wn - ref) <= (m + 2) * U * scale), (n, m)
            _near(s[m], R.exact_dot(wn, wn), 64 * U * R.abs_dot(wn, wn), f"multi_axpy norm {n} {m}")


# ------------------------------------------------------------------ the Arnoldi column (arnoldi_column)
def gs_bits(mode, m, pairs, offset, n, tier):
    """Reduction kernels a column must have run."""
    k, a = red_kind(pairs, offset, n), axpy_kind(offset, n)
    if mode == GS_MGS:
        return 0 if tier else k
    if mode == GS_CGS:
        return k | (a if m > 8 else 0) | k
    return k | a


def mgs_bounded(w, V):
    """MGS reference (float64 steps, exact dots) and, per link, a bound on what the GPU's h_k may differ by: the dot's
    own 64 u sum |w v| plus what the earlier links' differences carried into w (per entry: |dh_j| |v_j| + 2 u (|w| +
    |h_j v_j|))."""
    w = np.array(w, dtype=np.float64)
    bw = np.zeros_like(w)
    h, bh = [], []
    for v in V:
        hk = R.exact_dot(w, v)
        b = 64 * U * R.abs_dot(w, v) + float(np.dot(bw, np.abs(v)))
        wn = w - hk * v
        bw = bw + b * np.abs(v) + 2 * U * (np.abs(w) + np.abs(hk * v))
        w = wn
        h.append(hk)
        bh.append(b)
    nn = R.exact_dot(w, w)
    bn = 64 * U * nn + 2 * float(np.dot(np.abs(w), bw)) + float(np.dot(bw, bw))
    return np.array(h), np.array(bh), w, bw, nn, bn


def cgs_bounded(w, V):
    h, wn, nn = R.cgs(w, V)
    bh = np.array([64 * U * R.abs_dot(w, v) for v in V])
    bw = np.zeros_like(wn)
    acc = np.abs(np.asarray(w, dtype=np.float64))
    for hk, b, v in zip(h, bh, V):
        acc = acc + np.abs(hk * v)
        bw = bw + b * np.abs(v)
    bw = bw + (len(V) + 2) * U * acc
    bn = 64 * U * nn + 2 * float(np.dot(np.abs(wn), bw)) + float(np.dot(bw, bw))
    return h, bh, wn, bw, nn, bn


GS_MODES = [("sweep", GS_MGS, 1), ("chain", GS_MGS, 0), ("cgs", GS_CGS, 1), ("one_red", GS_ONE_RED, 1)]


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("offset", [0, 1])
def test_gram_schmidt_column_nearly_parallel_basis(hook, pairs, offset):
    """On a nearly parallel, non-orthonormal basis MGS and CGS give h_k that differ at O(1): the sweep and the chain
    must give the MGS reference, the fused modes the CGS one (and never the other).  Column sizes cross the passes of
    8 (m = 1, 7, 8, 9, 16, 17, 30, 31)."""
    hook.set_pairs(pairs)
    n = 4097
    for m in (1, 7, 8, 9, 16, 17, 30, 31):
        w, V = R.nearly_parallel_case(n, m, seed=m)
        ref_m = mgs_bounded(w, V)
        ref_c = cgs_bounded(w, V)
        for name, mode, fused in GS_MODES:
            hook.set_fused_mgs(fused)
            (wn, *_), s, info = hook.run(GS_COLUMN, [w] + V, n, m=m, offset=offset, par=[mode])
            h, bh, wref, bw, nn, bn = ref_m if mode == GS_MGS else ref_c
            other = ref_c if mode == GS_MGS else ref_m
            tier = int(info[1]) if mode == GS_MGS else 0
            if mode == GS_MGS:
                assert tier == (4 if fused else 0), (name, info)
            assert info[0] == gs_bits(mode, m, pairs, offset, n, tier), (name, m, info)
            bad = np.flatnonzero(np.abs(s[:m] - h) > bh)
            assert bad.size == 0, f"{name} m={m}: h_k off the reference at k = {bad[:6]}: {s[bad[:3]]} vs {h[bad[:3]]}"
            if m > 1:
                assert np.abs(s[1:m] - other[0][1:]).min() > 0.5, f"{name} m={m}: matches the other Gram-Schmidt"
            assert np.all(np.abs(wn - wref) <= bw), (name, m)
            if mode == GS_ONE_RED:
                q, r = R.pythagoras(s[:m], R.exact_dot(w, w))
                if m > 1:
                    assert q == 0.0   # sum h_k^2 > |w|^2 on this basis: the difference is negative and clamps to 0
                _near(s[m], q, 64 * U * R.exact_dot(w, w) + 4 * m * U * float(np.dot(s[:m], s[:m])), name)
                assert s[m] >= 0.0 and root_ok(s[m + 1], s[m])
            else:
                _near(s[m], nn, bn, f"{name} m={m} |w|^2")
                assert root_ok(s[m + 1], s[m])
    hook.set_fused_mgs(1)


@pytest.mark.parametrize("m", [1, 9, 30])
def test_gram_schmidt_one_reduction_norm_on_an_orthonormal_basis(hook, m):
    """|w|^2 - sum h_k^2 (one reduction) agrees with the two-pass norm when the basis is orthonormal."""
    hook.set_pairs(1)
    n = 4097
    V = R.orthonormal_basis(n, m, seed=m)
    G = np.array([[np.dot(a, b) for b in V] for a in V])
    orth = float(np.abs(G - np.eye(m)).max())
    w = _rand(n, 40 + m)
    ww = R.exact_dot(w, w)
    _, s1, _ = hook.run(GS_COLUMN, [w] + V, n, m=m, par=[GS_CGS])
    _, s2, _ = hook.run(GS_COLUMN, [w] + V, n, m=m, par=[GS_ONE_RED])
    assert np.array_equal(s1[:m], s2[:m])   # the same coefficient pass
    _near(s2[m], s1[m], (64 + 4 * m) * U * ww + 4 * m * orth * ww, f"one-reduction norm m={m}")
    assert root_ok(s2[m + 1], s2[m])


def int_case(n):
    """Integer-exact non-orthonormal column of three vectors that overlap at entries 0, n / 2 and n - 1: MGS and CGS
    differ, and a dropped or repeated entry anywhere changes |w|^2."""
    I = ints(n)
    w = I["m7"].copy()
    w[0], w[n // 2], w[n - 1] = 5.0, -2.0, 3.0
    V = [np.zeros(n) for _ in range(3)]
    V[0][[0, n // 2, n - 1]] += 1.0
    V[1][[n // 2, n - 1]] += [2.0, 1.0]
    V[2][[0, n - 1]] += [3.0, 1.0]
    return w, V


def int_gs(w, V, modified):
    w = w.astype(np.int64)
    Vi = [v.astype(np.int64) for v in V]
    h = []
    w0 = w.copy()
    for v in Vi:
        hk = int(np.dot(w if modified else w0, v))
        h.append(hk)
        w = w - hk * v
    return np.array(h, dtype=np.float64), w.astype(np.float64), float(np.dot(w, w)), float(np.dot(w0, w0))


def test_mgs_sweep_tiers_integer_exact(hook):
    """The sweep at the sizes where its tier changes (G * 1024 * {4, 8, 12} +- 1, G from the hook) and the chain beyond
    the last one, against the integer MGS reference (exact); the fused modes against the integer CGS one."""
    hook.set_pairs(1)
    hook.set_fused_mgs(1)
    _, _, info = hook.run(NORM2, [np.ones(4)], 4)
    G = int(info[2])
    tiers = {}
    for e in (4, 8, 12):
        for dn in (-1, 0, 1):
            n = G * 1024 * e + dn
            want_tier = {(4, -1): 4, (4, 0): 4, (4, 1): 8, (8, -1): 8, (8, 0): 8, (8, 1): 12, (12, -1): 12, (12, 0): 12,
                         (12, 1): 0}[(e, dn)]
            w, V = int_case(n)
            h, wref, nn, _ = int_gs(w, V, True)
            hc = int_gs(w, V, False)[0]
            assert not np.array_equal(h, hc)
            (wn, *_), s, info = hook.run(GS_COLUMN, [w] + V, n, m=3, par=[GS_MGS])
            assert info[1] == want_tier, (n, info)
            tiers[want_tier] = tiers.get(want_tier, 0) + 1
            assert np.array_equal(s[:3], h), (n, s[:3], h, "CGS" if np.array_equal(s[:3], hc) else "")
            assert np.array_equal(wn, wref), (n, np.flatnonzero(wn != wref)[:5])
            assert s[3] == nn and root_ok(s[4], nn), (n, s[3], nn)
    assert sorted(tiers) == [0, 4, 8, 12]
    # the fused classical modes at the largest tier (and the integer one-reduction formula, clamp included)
    n = G * 1024 * 12 + 1
    w, V = int_case(n)
    hc, wc, nc, ww = int_gs(w, V, False)
    for mode in (GS_CGS, GS_ONE_RED):
        (wn, *_), s, info = hook.run(GS_COLUMN, [w] + V, n, m=3, par=[mode])
        assert np.array_equal(s[:3], hc) and np.array_equal(wn, wc), mode
        if mode == GS_CGS:
            assert s[3] == nc
        else:
            assert s[3] == R.pythagoras(hc, ww)[0]


# ------------------------------------------------------------------ single-reduction CG
@pytest.mark.parametrize("first", [1, 0])
def test_cg_fused_scalars(hook, first):
    rng = np.random.default_rng(50 + first)
    for _ in range(20):
        sc = list(rng.uniform(0.5, 2.0, 7) * rng.choice([-1.0, 1.0], 7))
        sc[1] = abs(sc[1]) + 3.0   # delta - beta gamma / alpha away from 0
        sc[2] = abs(sc[2])
        _, s, _ = hook.run(CG_SCALARS, [], 1, par=sc + [first])
        ref = R.cg_fused_scalars(sc, first)
        assert np.array_equal(s[:3], sc[:3])
        assert np.all(np.abs(s[3:7] - ref[3:]) <= 4 * U * np.abs(ref[3:])), (s[:7], ref)


def test_cg_fused_sequence_on_an_spd_matrix(hook):
    """dot3 -> scalars -> update, six steps of single-reduction CG (identity preconditioner) on a host-held SPD matrix,
    the matrix-vector products on the host and fed back through the hook, against the same recurrence in NumPy."""
    hook.set_pairs(0)
    n = 301
    rng = np.random.default_rng(60)
    A = np.diag(2.5 + rng.uniform(0, 1, n)) - np.eye(n, k=1) - np.eye(n, k=-1)
    b = rng.standard_normal(n)
    g = {"x": np.zeros(n), "r": b.copy(), "p": np.zeros(n), "s": np.zeros(n)}
    c = {k: v.copy() for k, v in g.items()}
    sc_g, sc_c = np.zeros(7), np.zeros(7)
    for it in range(6):
        first = 1 if it == 0 else 0
        for st, sc, gpu in ((g, sc_g, True), (c, sc_c, False)):
            u = st["r"].copy()
            w = A @ u
            if gpu:
                _, s, _ = hook.run(DOT3, [st["r"], u, w], n)
                sc[:3] = s[:3]
                _, s, _ = hook.run(CG_SCALARS, [], 1, par=list(sc) + [first])
                sc[:] = s[:7]
                (_, _, st["p"], st["s"], st["x"], st["r"]), _, _ = hook.run(
                    CG_FUSED_UPDATE, [u, w, st["p"], st["s"], st["x"], st["r"]], n, par=list(sc))
            else:
                sc[:3] = [R.exact_dot(st["r"], u), R.exact_dot(w, u), R.exact_dot(st["r"], st["r"])]
                sc[:] = R.cg_fused_scalars(sc, first)
                st["p"], st["s"], st["x"], st["r"] = R.cg_fused_update(sc[4], sc[5], u, w, st["p"], st["s"], st["x"],
                                                                       st["r"])
        assert abs(sc_g[4] - sc_c[4]) <= 1e-13 * abs(sc_c[4]) and abs(sc_g[5] - sc_c[5]) <= 1e-12 * max(abs(sc_c[5]), 1e-3)
        for k in ("x", "r"):
            assert np.abs(g[k] - c[k]).max() <= 1e-13 * np.abs(c[k]).max() * (it + 1), (it, k)
    assert np.linalg.norm(b - A @ g["x"]) < 0.1 * np.linalg.norm(b)   # and it is CG: the residual went down


# ------------------------------------------------------------------ AMG smoother step, coarse solve
@pytest.mark.parametrize("c1,set_x", [(0.0, 0), (0.0, 1), (0.7, 0), (-1.3, 1)])
def test_cheby_step(hook, c1, set_x):
    for n in (1, 65, 4097):
        rng = np.random.default_rng(70 + n)
        dinv, r, w, x = rng.uniform(0.5, 2, n), rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        if c1 == 0.0:
            w[::3] = np.nan   # w is not read when c1 == 0 (the first step of the smoother)
        c2 = 0.61
        (_, _, wn, xn), _, _ = hook.run(CHEBY, [dinv, r, w, x], n, par=[c1, c2, set_x])
        rw, rx = R.cheby_step(c1, c2, dinv, r, w, x, set_x)
        assert np.all(np.isfinite(wn)) and np.all(np.isfinite(xn))
        sw = (np.abs(c1 * w) if c1 != 0.0 else 0.0) + np.abs(c2 * dinv * r)
        assert np.all(np.abs(wn - rw) <= 4 * U * sw), n
        assert np.all(np.abs(xn - rx) <= 4 * U * sw + (0 if set_x else 2 * U * (np.abs(x) + np.abs(rw)))), n


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 700])
def test_dense_mv(hook, n):
    rng = np.random.default_rng(80 + n)
    M, b = rng.standard_normal((n, n)), rng.standard_normal(n)
    (_, _, x), _, _ = hook.run(DENSE_MV, [M, b, np.full(n, np.nan)], n)
    for i in range(n):
        _near(x[i], R.exact_dot(M[i], b), 64 * U * R.abs_dot(M[i], b), f"dense_mv n={n} row {i}")


# ------------------------------------------------------------------ state between launches, determinism
@pytest.mark.parametrize("pairs", [1, 0])
def test_no_stale_state_between_grids(hook, pairs):
    """Reductions of alternating sizes back to back on one handle (grids of 1 up to 512 workgroups): each is exact, so
    no partial sum or ticket of one grid survives into the next."""
    hook.set_pairs(pairs)
    for n in (3, 8_575_417, 5, 1_048_577, 1, 2_097_152, 64, 8_575_416, 2):
        I = ints(n)
        _, s, _ = hook.run(DOT, [I["one"], I["ramp"]], n)
        check_ramp_dot(s[0], n, f"dot n={n} after another size")
        _, s, _ = hook.run(MULTI_DOT, [I["one"]] + [I["ramp"]] * 3, n, m=3)
        check_ramp_dot(s[2], n, f"multi_dot n={n} after another size")


def test_determinism(hook):
    """The same call twice gives the same bits, for every op."""
    n = 100_003
    x, y, z, g, e = (_rand(n, 90 + k) for k in range(5))
    V = [_rand(n, 100 + k) for k in range(9)]
    cases = [(DOT, [x, y], 0, ()), (NORM2, [x], 0, ()), (AXPY_DOT, [x, y, z], 0, (0.3,)), (AXPY_NORM2, [x, y], 0, (0.3,)),
             (CG_UPDATE, [x, y, z, g], 0, (0.3,)), (MULTI_DOT, [x] + V[:8], 8, ()),
             (MULTI_AXPY, [x] + V[:8], 8, [0.1] * 8 + [1]), (DOT3, [x, y, z], 0, ()),
             (CG_FUSED_UPDATE, [x, y, z, g, e, V[0]], 0, (1, 2, 3, 4, 0.5, 0.25, 1)),
             (CHEBY, [np.abs(x) + 1, y, z, g], 0, (0.5, 0.7, 0)), (DENSE_MV, [V[0][:129 * 129], y[:129], z[:129]], 0, ())]
    for pairs in (1, 0):
        hook.set_pairs(pairs)
        for op, vecs, m, par in cases:
            nn = 129 if op == DENSE_MV else n
            a = hook.run(op, vecs, nn, m=m, par=par)
            b = hook.run(op, vecs, nn, m=m, par=par)
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[0], b[0])), op
            assert np.array_equal(a[1], b[1], equal_nan=True), op
        for mode, fused in ((GS_MGS, 1), (GS_MGS, 0), (GS_CGS, 1), (GS_ONE_RED, 1)):
            hook.set_fused_mgs(fused)
            a = hook.run(GS_COLUMN, [x] + V, n, m=9, par=[mode])
            b = hook.run(GS_COLUMN, [x] + V, n, m=9, par=[mode])
            assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[1], b[1], equal_nan=True), mode
        hook.set_fused_mgs(1)
