"""Host reference for the triangular-solve kernel tests (tests/test_gpu_tri_kernels.py, nsk_internal.h: nsk_debug_tri).

Everything is stated on the PERMUTED, RESTRICTED matrix  P = Q A~ Q^T :  A~ is the caller's square matrix without the
entries whose column lies in another emulated sub-domain than the row, Q the ordering the analysis chose (perm[new] =
old).  Row i of P has strict-lower entries L_i = {j < i}, the diagonal d_i and strict-upper entries U_i = {j > i}.  A
returned factor F has P's pattern: ILU(0) stores l_ij below the diagonal (unit diagonal implied) and u_ij on and above
it; for SGS F is P itself.  b~ = Q b, x~ = Q x.

What the kernels define (comments of nsk_kernels.h; the 2 x 2 node-block formulas are the same relations with the node's
own l10 / u01 counted as ordinary entries of rows 2r + 1 / 2r, and a line group's couplings as ordinary entries too):
    ILU(0)   lower  y_i + sum_{L_i} l_ij y_j = b~_i           upper  u_ii x_i + sum_{U_i} u_ij x_j = y_i
    SGS      lower  d_i y_i + sum_{L_i} a_ij y_j = b~_i       upper  d_i x_i + sum_{U_i} a_ij x_j = d_i y_i

EXACT ARITHMETIC.  Doubles are dyadic rationals: every value becomes a Python integer on one common power of two
(to_ints), products and sums are then exact; the one division (SGS: y = z / d) goes through fractions.Fraction.

ILU(0) DEFECT.  For every position (i, j) of the pattern, on the returned factor,
    E_ij = a_ij - sum_{k < min(i,j), (i,k) and (k,j) in the pattern} l_ik u_kj - (i > j ? l_ij u_jj : u_ij)
    |E_ij| <= gamma_m (sum_k |l_ik||u_kj| + |last term|),     gamma_m = m u / (1 - m u), u = 2^-53.
m counted from ilu0_row (nsk_kernels.hip; ilu0_level_kernel and ilu0_serial_kernel both call it): the value starts as
a_ij (no rounding), every k subtracts l * u_kj from it in one statement, `w -= l * val` — two roundings, one if the
compiler fuses it — and a lower entry is finally divided by u_jj, one more: with t terms  m = 2 t + (i > j).  An upper
entry of a row without eliminations is a copy: m = 0, E = 0 exactly.  (Higham, Accuracy and Stability, Lemma 8.4.)

SUBSTITUTION RESIDUALS.  A row with c off-diagonal entries in the half forms c products, adds them in some tree (at most
c - 1 additions that are not additions of an exact zero), subtracts the sum from its own value and scales: by a division
(level walker tri_row, ring: 2 roundings after the sum) or by the product with a rounded reciprocal (stream, blocked and
single-launch kernels: dinv = 1 / d rounded once in numeric(), 3 after the sum).  A term passes at most
    d = c + 2  (walker, ring)      d = c + 3  (per-colour and single-launch kernels, scalar and 2 x 2)
roundings (ROUNDINGS_AFTER_SUM), whatever the summation order (Higham, Theorem 8.5 row by row).  fp32 halves add none:
the values are rounded once when stored, and the bound is taken against the factor with THOSE off-diagonals
(round_halves_f32; the diagonal, and a node's own l10 / u01, stay double).
  * A half that is empty in every row leaves the other one alone.  Upper empty: x = y up to the scaling; with T = D + L
    (SGS) or T = (I + L) diag(u_ii) (ILU)   |b~_i - (T x^)_i| <= gamma_{d + e} (|T||x^|)_i ,  e = the empty half's 2 or 3
    roundings (its subtraction of an exact 0 is exact).  Lower empty: T = D + U (SGS) or U (ILU), the same bound.
  * Full patterns: the hook returns x only.  With y* the EXACT result of the upper relation applied to x^
    (ILU: y* = U x^; SGS: y* = x^ + D^-1 U_strict x^), the computed y^ satisfies |y^ - y*| <= e_y,
        e_y = gamma_d (|U||x^|)  (ILU, diagonal included)      e_y = gamma_d (|x^| + |D^-1||U_strict||x^|)  (SGS)
    and the lower relation holds for y^ with its own gamma_d, so with T_L = I + |L| (ILU) or |D| + |L| (SGS)
        |b~ - T_L y*| <= gamma_d T_L (|y*| + e_y) + T_L e_y            (row by row, d per row and half).
The bounds are evaluated in double on non-negative numbers (at most a few hundred operations a row: relative error below
2^-40) and multiplied by 1 + 2^-40 (EVAL_SLACK).  No measured constant enters.

INTEGER-EXACT INPUTS (SGS): unit diagonal, small integer off-diagonals, integer b: every y_i, x_i is an integer; int_solve
computes them with Python integers and proves that every sum_j |a_ij||v_j| + |own| stays below 2^53 — then every product,
partial sum and result of ANY kernel is an exact double, dinv = 1 exactly, and the bits must equal the integer solve.

multicolour_perm asks the library's host-only hook nsk_debug_tri_ordering for the ordering the analysis chooses: it (and
with it tests/test_tri_reference.py) needs the built libnsk_hip.so, though no GPU.

model_apply is a plain double model of the kernels (row after row, one accumulator); its `mutate` argument breaks one
entry the way a wrong kernel would — the CPU tests show that the checks above catch each of them on the row concerned.
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

from tests import spmv_reference as M

U = 2.0 ** -53
EVAL_SLACK = 1.0 + 2.0 ** -40
PATH_NAME = {1: "sf_scalar", 2: "colour_scalar", 3: "sf_blocked", 4: "colour_blocked", 5: "ring", 6: "walker"}
ROUNDINGS_AFTER_SUM = {"walker": 2, "ring": 2, "sf_scalar": 3, "colour_scalar": 3, "sf_blocked": 3, "colour_blocked": 3}
K_ROW_MAX = 448        # nsk_tri.cpp: the LDS-staged ILU kernel's longest row
K_RING_HALF = 16       # kRingLpr * kRingRegs: entries per half and row the ring takes


def gamma(d):
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


# ------------------------------------------------------------------ patterns
def csr(n, rows, name=""):
    lens = [len(r) for r in rows]
    col = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if sum(lens) else np.zeros(0, dtype=np.int64)
    return M.Csr(n, n, np.concatenate([[0], np.cumsum(lens)]), col, None, n, name)


def with_diagonal(A, name=None):
    """A + I on the pattern (rows stay sorted); unlike symmetric_with_diagonal the pattern stays nonsymmetric."""
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(A.nnz), A.col, A.rowptr), shape=(A.n_rows, A.n_cols))
    P = (P + sp.identity(A.n_rows, format="csr")).tocsr()
    P.sort_indices()
    return M.Csr(A.n_rows, A.n_cols, P.indptr, P.indices, None, A.n_own, A.name if name is None else name)


def square(lens, seed, symmetric=True, name=""):
    """A square pattern with the diagonal from rows of the given lengths (spmv_reference.from_lengths)."""
    A = M.from_lengths(np.asarray(lens, dtype=np.int64), len(lens), seed, name=name)
    return M.symmetric_with_diagonal(A, name) if symmetric else with_diagonal(A, name)


def rows_of(A):
    return [A.col[A.rowptr[i]:A.rowptr[i + 1]].astype(np.int64) for i in range(A.n_rows)]


def banded(sizes, seed, n_lower, n_upper, name="", reach=None):
    """Rows in layers (sizes[q] consecutive rows each) for the CALLER'S order: row i holds the diagonal, n_lower[i] columns
    in earlier layers and n_upper[i] in later ones (as many as there are; none for the first / last layer), none in its
    own: both dependency graphs have at most len(sizes) levels, and the entries per half and row are exactly what the
    caller asks for.  A half's columns: start + k * step inside the earlier (later) rows — the nearest `reach` of them,
    all without it — start and step random."""
    rng = np.random.default_rng(seed)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(first[-1])
    layer = np.repeat(np.arange(len(sizes)), sizes)
    i = np.arange(n, dtype=np.int64)

    def half(cnt, lo, width):
        cnt = np.minimum(np.asarray(cnt, dtype=np.int64), width)
        step = np.maximum(np.minimum(rng.integers(1, 60, n), (width - 1) // np.maximum(cnt - 1, 1)), 1)
        start = (rng.random(n) * (width - (cnt - 1) * step)).astype(np.int64)
        start = np.clip(start, 0, np.maximum(width - 1 - (cnt - 1) * step, 0))
        k = np.arange(cnt.sum(), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return np.repeat(i, cnt), np.repeat(lo + start, cnt) + k * np.repeat(step, cnt)

    wl, wu = first[layer], n - first[layer + 1]
    if reach is not None:
        wl, wu = np.minimum(wl, reach), np.minimum(wu, reach)
    rl, cl = half(n_lower, first[layer] - wl, wl)
    ru, cu = half(n_upper, first[layer + 1], wu)
    import scipy.sparse as sp
    r, c = np.concatenate([rl, ru, i]), np.concatenate([cl, cu, i])
    assert c.min() >= 0 and c.max() < n
    Pm = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    assert Pm.nnz == len(r)
    Pm.sort_indices()
    A = M.Csr(n, n, Pm.indptr, Pm.indices, None, n, name)
    A.layers = first
    return A


def stair(sizes, seed, extra=2, p_lower=1.0, p_upper=1.0, lower_exact=None, name=""):
    """A pattern whose greedy colouring is KNOWN: rows in layers of sizes[q] consecutive rows; every row of layer q is a
    graph neighbour of one random row of EVERY earlier layer (plus `extra` more random earlier rows) and of no row of its
    own layer.  The analysis visits the rows in order, so a row of layer q finds the colours 0 .. q - 1 taken and gets
    colour q: the colours are the layers, the multicolour permutation is the identity, and in the caller's order both
    dependency graphs have len(sizes) levels.  An edge {i > j} is stored as (i, j) with probability p_lower and as (j, i)
    with probability p_upper (at least one of them): p_upper = 0 gives rows without a strict upper half.
    lower_exact = {q: c}: the rows of layer q get exactly c strict-lower entries (one in each of the layers 1 .. q - 1, the
    rest a window of consecutive columns of layer 0), always stored."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    sizes = [int(v) for v in sizes]
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(first[-1])
    ei, ej, forced = [], [], []
    for q in range(1, len(sizes)):
        rows = np.arange(first[q], first[q + 1], dtype=np.int64)
        m = len(rows)
        if lower_exact and q in lower_exact:
            k = lower_exact[q] - (q - 1)
            assert 1 <= k <= sizes[0], (q, lower_exact[q], sizes[0])
            for p in range(1, q):
                ei.append(rows); ej.append(first[p] + rng.integers(0, sizes[p], m)); forced.append(np.ones(m, dtype=bool))
            start = rng.integers(0, sizes[0], m)
            ei.append(np.repeat(rows, k))
            ej.append(((start[:, None] + np.arange(k)[None, :]) % sizes[0]).ravel())
            forced.append(np.ones(m * k, dtype=bool))
            continue
        for p in range(q):
            ei.append(rows); ej.append(first[p] + rng.integers(0, sizes[p], m)); forced.append(np.zeros(m, dtype=bool))
        for _ in range(extra):
            p = rng.integers(0, q, m)
            ei.append(rows)
            ej.append(first[p] + (rng.random(m) * np.asarray(sizes)[p]).astype(np.int64))
            forced.append(np.zeros(m, dtype=bool))
    if ei:
        ei, ej, forced = np.concatenate(ei), np.concatenate(ej), np.concatenate(forced)
        order = np.argsort(~forced, kind="stable")           # forced copies of an edge first: unique keeps them
        ei, ej, forced = ei[order], ej[order], forced[order]
        _, keep = np.unique(ei * n + ej, return_index=True)
        ei, ej, forced = ei[keep], ej[keep], forced[keep]
        low = (rng.random(len(ei)) < p_lower) | forced
        up = (rng.random(len(ei)) < p_upper) & ~forced
        neither = ~(low | up)
        if p_lower > 0:
            low |= neither
        else:
            up |= neither
        r = np.concatenate([ei[low], ej[up], np.arange(n)])
        c = np.concatenate([ej[low], ei[up], np.arange(n)])
    else:
        r = c = np.arange(n)
    Pm = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    Pm.sort_indices()
    A = M.Csr(n, n, Pm.indptr, Pm.indices, None, n, name)
    A.layers = first
    return A


def lattice(nx, ny, drop, seed, name=""):
    """(pattern, xy): the 9-point stencil on an nx x ny lattice, row = ix + nx * iy, support point (ix, iy); every
    off-diagonal entry is removed with probability `drop`, each direction on its own — a line group needs both (a, b)
    and (b, a), so chains of 1, 2 and 3 members occur side by side."""
    rng = np.random.default_rng(seed)
    rows = []
    for iy in range(ny):
        for ix in range(nx):
            c = []
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    jx, jy = ix + dx, iy + dy
                    if 0 <= jx < nx and 0 <= jy < ny and ((dx == 0 and dy == 0) or rng.random() >= drop):
                        c.append(jx + nx * jy)
            rows.append(np.array(sorted(c), dtype=np.int64))
    xy = np.stack([np.tile(np.arange(nx, dtype=np.float64), ny), np.repeat(np.arange(ny, dtype=np.float64), nx)], axis=1)
    return csr(nx * ny, rows, name), np.ascontiguousarray(xy)


def expand_nodes(B, name=None):
    """The scalar pattern of a node pattern B with 2 x 2 blocks (spmv_reference.expand_blocks)."""
    return M.expand_blocks(B, 2, 2, name=name)


# ------------------------------------------------------------------ values
def dominant_values(A, seed, lo=-7, hi=0):
    """Random doubles: off-diagonals of mixed sign over the decades 10^lo .. 10^hi, the diagonal strictly dominant over
    its row AND its column (1.5 times the larger absolute sum, at least 1), so that ILU(0) exists in any ordering."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 1.0, A.nnz) * 10.0 ** rng.uniform(lo, hi, A.nnz) * rng.choice([-1.0, 1.0], A.nnz)
    r = A.row_ids
    off = A.col != r
    rs = np.bincount(r[off], np.abs(v[off]), A.n_rows)
    cs = np.bincount(A.col[off], np.abs(v[off]), A.n_rows)
    v[~off] = (1.5 * np.maximum(rs, cs) + 1.0)[r[~off]] * rng.choice([-1.0, 1.0], A.n_rows)[r[~off]]
    return A.with_values(v)


def float_exact(A):
    """The same matrix with off-diagonals rounded to float (exact in fp32); the diagonal keeps its double."""
    v = A.val.copy()
    off = A.col != A.row_ids
    v[off] = v[off].astype(np.float32).astype(np.float64)
    return A.with_values(v)


def integer_values(A, seed, p_zero=0.3, amax=1):
    """Unit diagonal, off-diagonals drawn from {-amax .. amax} (zero with probability p_zero: a stored zero is an entry
    like any other)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, amax + 1, A.nnz) * rng.choice([-1.0, 1.0], A.nnz)
    v[rng.random(A.nnz) < p_zero] = 0.0
    v[A.col == A.row_ids] = 1.0
    return A.with_values(v)


def integer_rhs(n, seed=0):
    """Integers -4 .. 4, never 0, different laws in neighbouring rows (a row that reads its neighbour's b shows)."""
    i = np.arange(n, dtype=np.int64)
    b = ((i * 7 + seed) % 9 - 4).astype(np.float64)
    b[b == 0] = 3.0
    return b


# ------------------------------------------------------------------ the named patterns
def values(A, kind_of_values, seed=1):
    if kind_of_values == "int":
        return integer_values(A, seed, p_zero=0.1, amax=3)
    if kind_of_values == "real32":
        return float_exact(dominant_values(A, seed))
    return dominant_values(A, seed)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """The named patterns of the kernel tests (GPU module and the CPU checks of this reference): a Csr, or (Csr, xy)."""
    g = M.geometric_lengths
    if name[1:].isdigit():                         # n1, n2, n63, ...: small symmetric patterns
        n = int(name[1:])
        return square(np.minimum(g(n, 3, n, cap=max(1, n - 1)), n), 100 + n, True, name)
    if name == "irregular":                        # mixed row lengths, rows with the diagonal alone
        L = M.with_empty_rows(g(2300, 5, 7, cap=150), [(0, 3), (700, 760), (2299, 2300)])
        return square(L, 11, True, name)
    if name == "nonsymmetric":
        return square(M.with_empty_rows(g(1500, 6, 8, cap=120), [(40, 45)]), 12, False, name)
    if name == "stair":                            # colours = layers: one row, 64, 65, 2048 entries in 32 rows, 2049 in 33
        A = stair([300, 1, 70, 1, 64, 65, 32, 33, 129], 21, extra=2, lower_exact={6: 64, 7: 63}, name=name)
        return A
    if name == "stair_nonsymmetric":
        return stair([200, 1, 64, 65, 130, 7], 22, extra=3, p_lower=0.6, p_upper=0.6, name=name)
    if name == "stair_lower":                      # no strict upper half anywhere
        return stair([150, 1, 64, 65, 90], 23, extra=3, p_upper=0.0, name=name)
    if name == "stair_upper":                      # no strict lower half anywhere
        return stair([150, 1, 64, 65, 90], 24, extra=3, p_lower=0.0, name=name)
    if name == "diagonal":
        return csr(130, [[i] for i in range(130)], name)
    if name == "lattice":                          # line groups: chains of 1, 2 and 3 members
        return lattice(37, 23, 0.12, 31, name)
    if name == "nodes":                            # 2 x 2 node blocks on an irregular node pattern
        return expand_nodes(square(M.with_empty_rows(g(900, 5, 9, cap=100), [(5, 9)]), 41, True), name)
    if name == "nodes_stair":                      # node runs of exactly kBlkMax blocks (16 rows x 64) and one more
        B = stair([200, 1, 64, 65, 16, 17], 42, extra=2, lower_exact={4: 64, 5: 61})
        A = expand_nodes(B, name)
        A.layers = B.layers
        return A
    if name == "nodes_lattice":
        B, xy = lattice(29, 17, 0.12, 43)
        return expand_nodes(B, name), np.repeat(xy, 2, axis=0)
    if name == "odd_nodes":                        # odd n: no node structure
        return square(g(301, 4, 5, cap=50), 44, True, name)
    raise KeyError(name)



# ------------------------------------------------------------------ the permuted, restricted matrix
def keep_mask(A, sub_off=None):
    """Entries the analysis keeps: the column lies in the row's own sub-domain (all, without sub-domains)."""
    if sub_off is None or len(sub_off) <= 2:
        return np.ones(A.nnz, dtype=bool)
    shard = np.zeros(A.n_rows, dtype=np.int64)
    for s in range(len(sub_off) - 1):
        shard[sub_off[s]:sub_off[s + 1]] = s
    return shard[A.row_ids] == shard[A.col]


class Permuted:
    """P = Q A~ Q^T as sorted CSR: rp, col, src (position of the entry in the caller's arrays), diag (position of the
    diagonal in P's arrays), row (row of every entry)."""

    def __init__(self, A, perm, keep=None):
        n = A.n_rows
        perm = np.asarray(perm, dtype=np.int64)
        assert sorted(perm.tolist()) == list(range(n)), "perm is not a permutation"
        keep = np.ones(A.nnz, dtype=bool) if keep is None else keep
        iperm = np.empty(n, dtype=np.int64)
        iperm[perm] = np.arange(n)
        pos = np.nonzero(keep)[0]
        r = iperm[A.row_ids[pos]]
        c = iperm[A.col[pos].astype(np.int64)]
        order = np.lexsort((c, r))
        self.n, self.perm, self.iperm = n, perm, iperm
        self.row, self.col, self.src = r[order], c[order], pos[order]
        self.rp = np.concatenate([[0], np.cumsum(np.bincount(self.row, minlength=n))]).astype(np.int64)
        d = np.nonzero(self.row == self.col)[0]
        assert len(d) == n and np.array_equal(self.row[d], np.arange(n)), "a row has no diagonal entry"
        self.diag = d
        self.nnz = len(self.col)
        self.n_lower = self.diag - self.rp[:-1]
        self.n_upper = self.rp[1:] - self.diag - 1

    def values(self, caller_vals):
        return np.asarray(caller_vals, dtype=np.float64)[self.src]

    def to_caller(self, vals, nnz):
        out = np.full(nnz, np.nan)
        out[self.src] = vals
        return out

    def abs_half(self, vals, which):
        """scipy CSR of |vals| on the strict lower ('L') or strict upper ('U') entries."""
        import scipy.sparse as sp
        m = self.col < self.row if which == "L" else self.col > self.row
        return sp.csr_matrix((np.abs(vals[m]), (self.row[m], self.col[m])), shape=(self.n, self.n))


def round_halves_f32(P, vals, block2=False):
    """The factor as fp32 halves hold it: off-diagonals rounded to float — except, for the 2 x 2 node-block factor, the
    node's own l10 / u01 (rows 2r, 2r + 1 against each other), which stay double in `intra`."""
    v = np.array(vals, dtype=np.float64, copy=True)
    m = P.col != P.row
    if block2:
        m &= P.col != (P.row ^ 1)
    v[m] = v[m].astype(np.float32).astype(np.float64)
    return v


# ------------------------------------------------------------------ exact arithmetic on doubles
def to_ints(*arrays):
    """(lists of Python integers, S): value = integer / 2^S, one S for all arrays."""
    S = 0
    parts = []
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        assert np.all(np.isfinite(a)), "exact arithmetic on finite values only"
        m, e = np.frexp(a)
        mant = (m * 2.0 ** 53).astype(np.int64)          # exact: |m| < 1 has 53 bits
        e = e.astype(np.int64) - 53
        nz = mant != 0
        if nz.any():
            S = max(S, int(-(e[nz].min())))
        parts.append((mant, e))
    out = []
    for mant, e in parts:
        out.append([int(q) << int(s + S) if q else 0 for q, s in zip(mant.tolist(), e.tolist())])
    return out, S


def _to_float(num, shift):
    """num / 2^shift, correctly rounded."""
    return float(Fraction(num, 1 << shift)) if num else 0.0


# ------------------------------------------------------------------ ILU(0)
def ilu0_float(P, a_vals, skip=None):
    """ILU(0) of P in double, rows in order (what ilu0_row does for a row, sequentially).  skip = (k, t): the update of
    entry t by the lower entry k of its row is left out (a model of a wrong kernel)."""
    f = np.array(a_vals, dtype=np.float64, copy=True)
    rp, col, dg = P.rp, P.col, P.diag
    for i in range(P.n):
        rs, re = int(rp[i]), int(rp[i + 1])
        where = {int(col[k]): k for k in range(rs, re)}
        for k in range(rs, int(dg[i])):
            c = int(col[k])
            l = f[k] / f[dg[c]]
            f[k] = l
            for m in range(int(dg[c]) + 1, int(rp[c + 1])):
                t = where.get(int(col[m]))
                if t is not None and t > k and skip != (k, t):
                    f[t] -= l * f[m]
    return f


def ilu0_defect(P, a_vals, f_vals):
    """(E, bound, m) per entry of P: the exact defect |E_ij| of the factor, its bound and the rounding count."""
    (a, f), S = to_ints(a_vals, f_vals)
    rp, col, dg = P.rp, P.col, P.diag
    E = np.zeros(P.nnz)
    B = np.zeros(P.nnz)
    cnt = np.zeros(P.nnz, dtype=np.int64)
    for i in range(P.n):
        rs, re, di = int(rp[i]), int(rp[i + 1]), int(dg[i])
        where = {int(col[k]): k for k in range(rs, re)}
        acc = [0] * (re - rs)
        ab = [0] * (re - rs)
        tt = [0] * (re - rs)
        for k in range(rs, di):
            c = int(col[k])
            l = f[k]
            for m in range(int(dg[c]) + 1, int(rp[c + 1])):
                t = where.get(int(col[m]))
                if t is not None and t > k:
                    p = l * f[m]
                    acc[t - rs] += p
                    ab[t - rs] += abs(p)
                    tt[t - rs] += 1
        for k in range(rs, re):
            last = f[k] * f[dg[int(col[k])]] if k < di else f[k] << S
            e = (a[k] << S) - acc[k - rs] - last
            E[k] = abs(_to_float(e, 2 * S))
            cnt[k] = 2 * tt[k - rs] + (1 if k < di else 0)
            B[k] = float(gamma(cnt[k])) * _to_float(ab[k - rs] + abs(last), 2 * S) * EVAL_SLACK
    return E, B, cnt


# ------------------------------------------------------------------ substitutions
def model_apply(P, f_vals, kind, b, mutate=None):
    """x = M^-1 b in plain double, rows of P in order, one accumulator per row (a model of a correct kernel).
    mutate = (what, k): 'drop' skips entry k of P; 'swap' reads the vector at the column of the row's next entry of the
    same half (or the previous one); 'other_half' uses the value of the transposed position (j, i) where the pattern
    holds it, else the row's diagonal."""
    n, rp, col, dg = P.n, P.rp, P.col, P.diag
    f = np.asarray(f_vals, dtype=np.float64)
    bp = np.asarray(b, dtype=np.float64)[P.perm]

    def term(k, vec, lo, hi):
        v, c = f[k], int(col[k])
        if mutate is not None and mutate[1] == k:
            if mutate[0] == "drop":
                return 0.0
            if mutate[0] == "swap":
                c = int(col[k + 1]) if k + 1 < hi else int(col[k - 1]) if k - 1 >= lo else c + (1 if c + 1 < n else -1)
            if mutate[0] == "other_half":
                i = int(P.row[k])
                t = [q for q in range(int(rp[c]), int(rp[c + 1])) if int(col[q]) == i]
                v = f[t[0]] if t else f[dg[i]]
        return v * vec[c]

    y = np.zeros(n)
    for i in range(n):
        s = 0.0
        for k in range(int(rp[i]), int(dg[i])):
            s += term(k, y, int(rp[i]), int(dg[i]))
        y[i] = bp[i] - s if kind == 0 else (bp[i] - s) / f[dg[i]]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = 0.0
        for k in range(int(dg[i]) + 1, int(rp[i + 1])):
            s += term(k, x, int(dg[i]) + 1, int(rp[i + 1]))
        x[i] = (y[i] - s) / f[dg[i]] if kind == 0 else y[i] - s / f[dg[i]]
    out = np.empty(n)
    out[P.perm] = x
    return out


def int_solve(P, vals, b):
    """SGS with unit diagonal on integers: (x in the caller's order as doubles, the largest sum_j |a_ij||v_j| + |own|
    met in either half).  Asserts the unit diagonal, integer data and that the largest sum stays below 2^53: every
    intermediate of any summation order is then an exact double."""
    v = np.asarray(vals, dtype=np.float64)
    assert np.all(v == np.rint(v)) and np.all(v[P.diag] == 1.0) and np.all(np.asarray(b) == np.rint(b))
    a = [int(t) for t in v.tolist()]
    bp = [int(t) for t in np.asarray(b, dtype=np.float64)[P.perm].tolist()]
    rp, col, dg = P.rp.tolist(), P.col.tolist(), P.diag.tolist()
    n = P.n
    y, x, big = [0] * n, [0] * n, 0
    for i in range(n):
        s = m = 0
        for k in range(rp[i], dg[i]):
            t = a[k] * y[col[k]]
            s += t
            m += abs(t)
        y[i] = bp[i] - s
        big = max(big, m + abs(bp[i]))
    for i in range(n - 1, -1, -1):
        s = m = 0
        for k in range(dg[i] + 1, rp[i + 1]):
            t = a[k] * x[col[k]]
            s += t
            m += abs(t)
        x[i] = y[i] - s
        big = max(big, m + abs(y[i]))
    assert big < 2 ** 53, f"integer-exact input: a sum reaches 2^{big.bit_length()} — not exact in double"
    out = np.empty(n)
    out[P.perm] = np.array(x, dtype=np.float64)
    return out, big


def integer_problem(P, vals, law=0):
    """Integer b (caller's order) for SGS with unit diagonal whose solve stays small: a small integer x* is chosen (|x*|
    <= 4, a different law per `law`), y* = x* + U x*, b = y* + L y*.  Forward and backward substitution then meet exactly
    these y* and x*, whatever the number of levels."""
    v = np.rint(np.asarray(vals, dtype=np.float64)).astype(np.int64)
    i = P.perm.astype(np.int64)
    xs = (i * (7 + 4 * law) + 3 * law) % 9 - 4
    xs[xs == 0] = 3 - law
    up, lo = P.col > P.row, P.col < P.row
    y = xs + np.bincount(P.row[up], v[up] * xs[P.col[up]], P.n).astype(np.int64)
    bb = y + np.bincount(P.row[lo], v[lo] * y[P.col[lo]], P.n).astype(np.int64)
    b = np.empty(P.n)
    b[P.perm] = bb.astype(np.float64)
    return b


def run_plan(counts, cuts, cap, glue=None):
    """Model of build_rowblocks as TriSolve::analyze calls it for one half: (runs, longest in rows, longest in entries)."""
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rb = M.build_rowblocks(rp, None, len(counts), cap, [int(c) for c in cuts])
    assert rb is not None and glue is None
    rows = max(rb[k + 1] - rb[k] for k in range(len(rb) - 1))
    ent = max(int(rp[rb[k + 1]] - rp[rb[k]]) for k in range(len(rb) - 1))
    return len(rb) - 1, rows, ent


def _half_counts(P, path):
    c = ROUNDINGS_AFTER_SUM[path]
    return P.n_lower + c, P.n_upper + c, c


def residual_alone(P, f_vals, kind, b, x, path):
    """One half empty in every row: (|residual|, bound) per row of P for the other half alone, or None when both halves
    hold entries.  Rows in P's order."""
    lower_empty, upper_empty = not P.n_lower.any(), not P.n_upper.any()
    if not (lower_empty or upper_empty):
        return None
    (f, bp, xp), S = to_ints(f_vals, np.asarray(b, dtype=np.float64)[P.perm], np.asarray(x, dtype=np.float64)[P.perm])
    rp, col, dg = P.rp.tolist(), P.col.tolist(), P.diag.tolist()
    dl, du, c = _half_counts(P, path)
    res, bound = np.zeros(P.n), np.zeros(P.n)
    for i in range(P.n):
        if upper_empty:       # T = D + L (SGS), (I + L) diag(u) (ILU): the lower row, y_j = x_j (SGS) or u_jj x_j (ILU)
            if kind == 1:
                terms = [(f[k] * xp[col[k]]) << S for k in range(rp[i], dg[i] + 1)]
            else:
                terms = [f[k] * f[dg[col[k]]] * xp[col[k]] for k in range(rp[i], dg[i])] + [(f[dg[i]] * xp[i]) << S]
            d = dl[i] + c
        else:                 # T = D + U (SGS), U (ILU)
            terms = [(f[k] * xp[col[k]]) << S for k in range(dg[i], rp[i + 1])]
            d = du[i] + c
        r = (bp[i] << (2 * S)) - sum(terms)
        res[i] = abs(_to_float(r, 3 * S))
        bound[i] = float(gamma(d)) * _to_float(sum(abs(t) for t in terms), 3 * S) * EVAL_SLACK
    return res, bound


def residual_composed(P, f_vals, kind, b, x, path):
    """(|b~ - T_L y'|, bound) per row of P.  ILU: y' = y*, the exact upper relation applied to x.  SGS: y' = y* rounded
    to double once (y* = z / d is no dyadic number; everything else then stays in integers), and e_y grows by that
    rounding, u |y'| (1 + 2u) (module docstring)."""
    fv = np.asarray(f_vals, dtype=np.float64)
    bpf = np.asarray(b, dtype=np.float64)[P.perm]
    xpf = np.asarray(x, dtype=np.float64)[P.perm]
    (f, xp), S = to_ints(fv, xpf)
    rp, col, dg = P.rp.tolist(), P.col.tolist(), P.diag.tolist()
    n = P.n
    dl, du, _ = _half_counts(P, path)
    # z_i = u_ii x_i + sum_U u_ij x_j at scale 2 S: y* (ILU), d_i y* (SGS)
    z = [sum(f[k] * xp[col[k]] for k in range(dg[i], rp[i + 1])) for i in range(n)]
    dabs = np.abs(fv[P.diag])
    Ux = P.abs_half(fv, "U") @ np.abs(xpf)
    if kind == 0:
        yq = np.array([_to_float(t, 2 * S) for t in z])            # |y*| for the bound (rounded once: the 1 + U below)
        e_y = gamma(du) * (dabs * np.abs(xpf) + Ux)
        (bp,), Sb = to_ints(bpf)
        sh = max(3 * S, Sb)
        res = np.zeros(n)
        for i in range(n):
            r = (bp[i] << (sh - Sb)) - (((z[i] << S) + sum(f[k] * z[col[k]] for k in range(rp[i], dg[i]))) << (sh - 3 * S))
            res[i] = abs(_to_float(r, sh))
        TL = lambda v: v + P.abs_half(fv, "L") @ v   # noqa: E731
    else:
        yq = np.array([float(Fraction(z[i], f[dg[i]] << S)) for i in range(n)])     # y' = fl(z / d)
        e_y = gamma(du) * (np.abs(xpf) + Ux / dabs) + U * np.abs(yq) * (1.0 + 2.0 * U)
        (f2, bp, yp), S2 = to_ints(fv, bpf, yq)
        res = np.zeros(n)
        for i in range(n):
            r = (bp[i] << S2) - sum(f2[k] * yp[col[k]] for k in range(rp[i], dg[i] + 1))
            res[i] = abs(_to_float(r, 2 * S2))
        TL = lambda v: dabs * v + P.abs_half(fv, "L") @ v   # noqa: E731
    bound = (gamma(dl) * TL(np.abs(yq) * (1.0 + U) + e_y) + TL(e_y)) * EVAL_SLACK
    return res, bound


def check_solution(P, f_vals, kind, b, x, path):
    """Rows of P (and their caller rows) outside the bound: [(row of P, caller row, residual, bound)], empty when x is a
    solution to working precision.  Uses the half-alone form where a half is empty, the composed one otherwise."""
    r = residual_alone(P, f_vals, kind, b, x, path)
    if r is None:
        r = residual_composed(P, f_vals, kind, b, x, path)
    res, bound = r
    bad = np.nonzero(~(res <= bound))[0]
    return [(int(i), int(P.perm[i]), float(res[i]), float(bound[i])) for i in bad]


def multicolour_perm(A, sub_off=None, want_block2=False, xy=None, group=1):
    """The ordering the analysis chooses (host-only hook nsk_debug_tri_ordering): perm, (colours, gmax, block2, items)."""
    import ctypes as C
    from navier_stokes_solver_amd import solver as S
    L = S.lib()
    L.nsk_debug_tri_ordering.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    perm = np.zeros(A.n_rows, dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    so = None if sub_off is None else np.ascontiguousarray(sub_off, dtype=np.int32)
    xyc = None if xy is None else np.ascontiguousarray(xy, dtype=np.float64)
    rc = L.nsk_debug_tri_ordering(A.n_rows, A.rowptr.ctypes.data, A.col.ctypes.data, 0 if so is None else len(so) - 1,
                                  None if so is None else so.ctypes.data, int(want_block2),
                                  None if xyc is None else xyc.ctypes.data, group, perm.ctypes.data, info.ctypes.data, None)
    assert rc == 0
    return perm, info
