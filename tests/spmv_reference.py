"""Host references and sparsity patterns for the SpMV kernel tests (tests/test_gpu_spmv_kernels.py).

* Exact row sums: the correctly rounded sum_j a_ij x_j and sum_j |a_ij x_j| of every row, on the exact dot product of
  tests/krylov_reference.py; for the fp32 forms the same on float32(a_ij) widened back.  The int64 row sums serve the
  integer-exact inputs.
* roundings(): the largest number of roundings one product can pass in a kernel form for a row of a given length,
  counted from nsk_kernels.hip (the count is written out in the docstring of the GPU test module).
* A plain-Python model of the plan builders (build_rowblocks, Csr::find_interior, Csr::build_stream_plan,
  Csr::build_blocked in nsk_core.cpp), so that what the test hook reports can be told apart from a wrong expectation.
* Seeded pattern generators; every one returns a Csr with sorted, distinct columns per row.
"""
from __future__ import annotations

import math

import numpy as np

from tests import krylov_reference as R

U = R.U
K_STREAM_NNZ = 2048   # nsk_kernels.h: kStreamNnz
K_STREAM_ROWS = 64    # kStreamRows
K_BLK_MAX = 1024      # kBlkMax
RG = 4                # nsk_kernels.hip: lanes per row in the reduce phase of the staged kernels


class Csr:
    def __init__(self, n_rows, n_cols, rowptr, col, val=None, n_own=None, name=""):
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.n_own = self.n_cols if n_own is None else int(n_own)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.zeros(len(self.col)) if val is None else np.ascontiguousarray(val, dtype=np.float64)
        self.name = name
        assert len(self.rowptr) == self.n_rows + 1 and self.rowptr[0] == 0 and self.rowptr[-1] == len(self.col)

    @property
    def nnz(self):
        return int(self.rowptr[-1])

    @property
    def row_len(self):
        return np.diff(self.rowptr.astype(np.int64))

    @property
    def row_ids(self):
        return np.repeat(np.arange(self.n_rows, dtype=np.int64), self.row_len)

    def with_values(self, val, name=None):
        return Csr(self.n_rows, self.n_cols, self.rowptr, self.col, val, self.n_own, self.name if name is None else name)

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val, self.col, self.rowptr), shape=(self.n_rows, self.n_cols))

    def columns_sorted(self):
        if self.nnz < 2:
            return True
        up = np.diff(self.col.astype(np.int64)) > 0
        starts = self.rowptr[1:-1].astype(np.int64)   # position k = first entry of a later row: col[k - 1] -> col[k] is free
        starts = starts[(starts > 0) & (starts < self.nnz)]
        up[starts - 1] = True
        return bool(up.all())


# ------------------------------------------------------------------ references
def gather_x(A, x_own, x_ghost):
    """x as the kernels see it: owned entries, then the ghost tail."""
    x = np.concatenate([np.asarray(x_own, dtype=np.float64), np.asarray(x_ghost, dtype=np.float64)])
    assert len(x) == A.n_cols
    return x[A.col] if A.nnz else np.zeros(0)


def int_row_sums(A, x_own, x_ghost):
    """Row sums of integer-valued data in int64: exact, whatever the order."""
    p = np.rint(A.val).astype(np.int64) * np.rint(gather_x(A, x_own, x_ghost)).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(p, dtype=np.int64)])
    rp = A.rowptr.astype(np.int64)
    return cs[rp[1:]] - cs[rp[:-1]]


def exact_row_sums(A, x_own, x_ghost, fp32=False):
    """(s, a): per row the correctly rounded sum_j a_ij x_j and sum_j |a_ij x_j|; fp32: on float32(a_ij) widened back."""
    v = A.val.astype(np.float32).astype(np.float64) if fp32 else A.val
    xv = gather_x(A, x_own, x_ghost)
    s, a = np.zeros(A.n_rows), np.zeros(A.n_rows)
    rp = A.rowptr
    for i in range(A.n_rows):
        b, e = rp[i], rp[i + 1]
        if e > b:
            s[i] = R.exact_dot(v[b:e], xv[b:e])
            a[i] = R.abs_dot(v[b:e], xv[b:e])
    return s, a


def apply_mode(s, mode, y, z):
    """mode 0: s ; 1: (z or y) + s ; 2: z - s, one rounding."""
    if mode == 0:
        return s.copy()
    base = y if z is None else z
    return base + s if mode == 1 else base - s


def epilogue(s, y, d, dinv):
    """((y .* d) - s) .* dinv, every operation rounded once."""
    return ((y * d) - s) * dinv


def ceil_div(a, b):
    return -(-a // b)


def roundings(form, la, lb=0, lpr=0):
    """Largest number of roundings a product passes before it is part of y_i, for a row with la (and lb) stored
    entries — BLOCKS for the blocked forms.  See the docstring of tests/test_gpu_spmv_kernels.py for the count."""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    if form == "csrv":
        return ceil_div(la, lpr) + int(math.log2(lpr))
    chain = np.maximum(ceil_div(la, RG) + ceil_div(lb, RG) - 1, 0)
    prod = {"stream": 1, "stream2": 1, "blk_c1": 1, "blk_c2": 2, "blk_fused": 2}[form]
    return prod + chain + 2


def gamma(d):
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


# ------------------------------------------------------------------ model of the plan builders (nsk_core.cpp)
def build_rowblocks(ra, rb, n_rows, max_nnz, cuts=None, row_cap=K_STREAM_ROWS):
    """Greedy runs of whole rows: at most row_cap rows and max_nnz entries (of ra and rb together), never across a cut.
    None when a single row is above max_nnz."""
    ra = [int(v) for v in ra]
    rb = None if rb is None else [int(v) for v in rb]
    cuts = sorted(cuts or [])

    def nnz_of(a, b):
        return ra[b] - ra[a] + (rb[b] - rb[a] if rb is not None else 0)

    out, r0, ci = [0], 0, 0
    while r0 < n_rows:
        while ci < len(cuts) and cuts[ci] <= r0:
            ci += 1
        limit = min(n_rows, cuts[ci]) if ci < len(cuts) else n_rows
        r1 = r0 + 1
        if nnz_of(r0, r1) > max_nnz:
            return None
        while r1 < limit and r1 - r0 < row_cap and nnz_of(r0, r1 + 1) <= max_nnz:
            r1 += 1
        out.append(r1)
        r0 = r1
    return out


def find_interior(A):
    """The longest run of rows without ghost columns (the first of equally long ones)."""
    if A.n_cols == A.n_own:
        return 0, A.n_rows
    ghost = np.zeros(A.n_rows, dtype=bool)
    ghost[A.row_ids[A.col >= A.n_own]] = True
    best0 = best1 = start = 0
    for i in range(A.n_rows + 1):
        if i == A.n_rows or ghost[i]:
            if i - start > best1 - best0:
                best0, best1 = start, i
            start = i + 1
    return best0, best1


def interior_runs(rb, r0, r1):
    b0 = b1 = 0
    for b in range(len(rb) - 1):
        if rb[b] >= r0 and rb[b + 1] <= r1:
            if b1 == b0:
                b0 = b
            b1 = b + 1
    return b0, b1


def _run_stats(rb, *rowptrs):
    rows = max((rb[b + 1] - rb[b] for b in range(len(rb) - 1)), default=0)
    ent = max((sum(int(rp[rb[b + 1]]) - int(rp[rb[b]]) for rp in rowptrs) for b in range(len(rb) - 1)), default=0)
    return rows, ent


def stream_plan(A):
    """What Csr::build_stream_plan decides: stream_ok, the runs, the interior run range, even_rows."""
    i0, i1 = find_interior(A)
    cuts = ([i0] if i0 > 0 else []) + ([i1] if i1 < A.n_rows and i1 > i0 else [])
    rb = build_rowblocks(A.rowptr, None, A.n_rows, K_STREAM_NNZ, cuts)
    if rb is None:
        return dict(ok=False)
    b0, b1 = interior_runs(rb, i0, i1)
    rows, ent = _run_stats(rb, A.rowptr)
    return dict(ok=True, rb=rb, int_b0=b0, int_b1=b1, even=bool(np.all(A.rowptr % 2 == 0)), rows=rows, entries=ent,
                vec=2 if np.all(A.rowptr % 2 == 0) else 3)


def blocked_rowptr(A, Rr, Cc):
    """Block row pointers when the pattern is made of aligned Rr x Cc blocks, else None (Csr::build_blocked's check)."""
    if A.n_rows <= 0 or A.n_rows % Rr or A.n_own % Cc or A.n_cols % Cc:
        return None
    nr = A.n_rows // Rr
    rp = A.rowptr.astype(np.int64)
    lens = np.diff(rp).reshape(nr, Rr)
    if np.any(lens % Cc) or np.any(lens != lens[:, :1]):
        return None
    col = A.col.astype(np.int64)
    first = col.reshape(-1, Cc) if A.nnz else np.zeros((0, Cc), dtype=np.int64)
    if np.any(first[:, 0] % Cc) or np.any(first != first[:, :1] + np.arange(Cc)):
        return None
    for q in range(1, Rr):     # the rows of a block row share their columns
        for r in np.nonzero(lens[:, 0])[0]:
            a, b = rp[Rr * r], rp[Rr * r + q]
            if not np.array_equal(col[a:a + lens[r, 0]], col[b:b + lens[r, 0]]):
                return None
    return np.concatenate([[0], np.cumsum(lens[:, 0] // Cc)]).astype(np.int64)


def blocked_plan(A, Rr, Cc):
    """What Csr::build_blocked decides: blk_ok, the block row pointers, the runs of block rows, the interior run range."""
    brp = blocked_rowptr(A, Rr, Cc)
    if brp is None:
        return dict(ok=False)
    nr = A.n_rows // Rr
    i0, i1 = find_interior(A)
    ib0, ib1 = (i0 + Rr - 1) // Rr, i1 // Rr
    cuts = ([ib0] if 0 < ib0 < nr else []) + ([ib1] if ib1 < nr and ib1 > ib0 else [])
    rb = build_rowblocks(brp, None, nr, K_BLK_MAX, cuts)
    if rb is None:
        return dict(ok=False)
    b0, b1 = interior_runs(rb, ib0, ib1)
    rows, ent = _run_stats(rb, brp)
    return dict(ok=True, brp=brp, rb=rb, int_b0=b0, int_b1=b1, rows=rows, entries=ent)


def fused_plan(A, B, blocked):
    """The combined runs of jacobian_vmult's fused block row (no cuts): reason 0 and the plan, or why it is refused
    (the codes of nsk_debug_spmv: 2 no node structure, 3 A has an odd row pointer, 4 a row above the combined cap)."""
    if blocked:
        pa, pb = blocked_plan(A, 2, 2), blocked_plan(B, 2, 1)
        if not (pa["ok"] and pb["ok"]):
            return dict(ok=False, reason=2)
        ra, rbp, n, cap = pa["brp"], pb["brp"], A.n_rows // 2, K_BLK_MAX
    else:
        if not stream_plan(A).get("even", False):
            return dict(ok=False, reason=3)
        ra, rbp, n, cap = A.rowptr, B.rowptr, A.n_rows, K_STREAM_NNZ
    rb = build_rowblocks(ra, rbp, n, cap)
    if rb is None:
        return dict(ok=False, reason=4)
    rows, ent = _run_stats(rb, ra, rbp)
    return dict(ok=True, reason=0, rb=rb, rows=rows, entries=ent, ra=np.asarray(ra), rb2=np.asarray(rbp))


def pick_lpr(A):
    mean = A.nnz / A.n_rows if A.n_rows else 0.0
    return 4 if mean <= 6 else 8 if mean <= 20 else 16 if mean <= 80 else 32 if mean <= 200 else 64


# ------------------------------------------------------------------ values and operands
def int_values(A, seed=0):
    """Integer values 1 <= |a| <= 8 (no zero: every stored entry counts)."""
    rng = np.random.default_rng(1000 + seed)
    return A.with_values(rng.integers(1, 9, A.nnz) * rng.choice([-1.0, 1.0], A.nnz))


def real_values(A, seed=0):
    """Values of mixed sign over six decades (not representable in fp32)."""
    rng = np.random.default_rng(2000 + seed)
    return A.with_values(rng.uniform(-1.0, 1.0, A.nnz) * 10.0 ** rng.integers(-3, 3, A.nnz))


def int_x(A):
    """x_j distinct per column over a period of 31, never 0, |x| <= 16; the ghost tail on another law (period 29), so
    that x_own read where x_ghost belongs, or a neighbouring column, changes the sum."""
    j = np.arange(A.n_own, dtype=np.int64)
    xo = (j % 31 - 15).astype(np.float64)
    xo[xo == 0] = 16.0
    g = np.arange(A.n_cols - A.n_own, dtype=np.int64)
    xg = -((g + 7) % 29 - 14).astype(np.float64)
    xg[xg == 0] = -16.0
    return xo, xg


def real_x(A, seed=0):
    rng = np.random.default_rng(3000 + seed)
    return rng.uniform(-1.0, 1.0, A.n_own), rng.uniform(-1.0, 1.0, A.n_cols - A.n_own)


def int_vec(n, period, shift):
    v = (np.arange(n, dtype=np.int64) % period - shift).astype(np.float64)
    return v


# ------------------------------------------------------------------ pattern generators
def from_lengths(lens, n_cols, seed, n_own=None, ghost_lens=None, name=""):
    """Rows of the given lengths over the owned columns [0, n_own): row i holds base_i + j * step_i, j < len_i (sorted,
    distinct; base and step 1..3 random), followed by ghost_lens[i] ghost columns from [n_own, n_cols) built the same
    way."""
    rng = np.random.default_rng(seed)
    n_own = n_cols if n_own is None else n_own
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    glens = np.zeros(n, dtype=np.int64) if ghost_lens is None else np.asarray(ghost_lens, dtype=np.int64)

    def part(L, lo, width):
        if L.sum() == 0:
            return np.zeros(0, dtype=np.int64)
        assert width >= L.max(), (width, L.max())
        step = np.minimum(rng.integers(1, 4, n), np.maximum((width - 1) // np.maximum(L - 1, 1), 1))
        span = (L - 1) * step
        base = (rng.random(n) * (width - span)).astype(np.int64)
        base = np.minimum(base, width - 1 - span)
        base[L == 0] = 0
        j = np.arange(L.sum(), dtype=np.int64) - np.repeat(np.cumsum(L) - L, L)
        return lo + np.repeat(base, L) + j * np.repeat(step, L)

    own = part(lens, 0, n_own)
    gh = part(glens, n_own, n_cols - n_own)
    tot = lens + glens
    rp = np.concatenate([[0], np.cumsum(tot)])
    col = np.empty(rp[-1], dtype=np.int64)
    pos_own = np.repeat(rp[:-1], lens) + (np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens))
    pos_gh = np.repeat(rp[:-1] + lens, glens) + (np.arange(glens.sum()) - np.repeat(np.cumsum(glens) - glens, glens))
    col[pos_own] = own
    col[pos_gh] = gh
    return Csr(n, n_cols, rp, col, None, n_own, name)


def geometric_lengths(n, mean, seed, cap=None):
    rng = np.random.default_rng(seed)
    L = rng.geometric(1.0 / mean, n).astype(np.int64)
    return np.minimum(L, cap) if cap else L


def expand_blocks(B, Rr, Cc, name=None):
    """The scalar CSR of a block pattern B (one entry per block): rows Rr r + q hold the columns Cc m + t."""
    bl = B.row_len
    lens = np.repeat(bl * Cc, Rr)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(rp[-1], dtype=np.int64)
    bc = B.col.astype(np.int64)
    for q in range(Rr):
        rows = np.arange(B.n_rows) * Rr + q
        start = np.repeat(rp[rows], bl * Cc)
        within = np.arange((bl * Cc).sum()) - np.repeat(np.cumsum(bl * Cc) - bl * Cc, bl * Cc)
        col[start + within] = np.repeat(bc, Cc) * Cc + np.tile(np.arange(Cc), len(bc))
    return Csr(B.n_rows * Rr, B.n_cols * Cc, rp, col, None, B.n_own * Cc, B.name if name is None else name)


def remove_entry(A, k, name=None):
    rp = A.rowptr.astype(np.int64).copy()
    row = int(np.searchsorted(rp, k, side="right") - 1)
    rp[row + 1:] -= 1
    return Csr(A.n_rows, A.n_cols, rp, np.delete(A.col, k), np.delete(A.val, k), A.n_own, A.name if name is None else name)


def add_entry_to_first_row(A, name=None):
    """One more entry in row 0 (a column it does not hold yet): every later row pointer moves by one."""
    row0 = set(A.col[:A.rowptr[1]].tolist())
    c = next(c for c in range(A.n_own) if c not in row0)
    cols0 = np.sort(np.concatenate([A.col[:A.rowptr[1]], [c]]))
    rp = A.rowptr.astype(np.int64).copy()
    rp[1:] += 1
    return Csr(A.n_rows, A.n_cols, rp, np.concatenate([cols0, A.col[A.rowptr[1]:]]), None, A.n_own,
               A.name if name is None else name)


def symmetric_with_diagonal(A, name=None):
    """The square pattern A + A^T + I (what the triangular-solve analysis of a preconditioner set-up expects)."""
    import scipy.sparse as sp
    assert A.n_rows == A.n_cols == A.n_own
    P = sp.csr_matrix((np.ones(A.nnz), A.col, A.rowptr), shape=(A.n_rows, A.n_cols))
    P = (P + P.T + sp.identity(A.n_rows, format="csr")).tocsr()
    P.sort_indices()
    return Csr(A.n_rows, A.n_cols, P.indptr, P.indices, None, A.n_own, A.name if name is None else name)


def with_empty_rows(lens, where):
    L = np.array(lens, dtype=np.int64)
    for a, b in where:
        L[a:b] = 0
    return L


def scalar_patterns():
    """name -> Csr: the irregular scalar patterns (a few 10^4 entries each, at most ~2 10^5)."""
    P = {}
    mixed = geometric_lengths(700, 9, 1, cap=300)

    def add(name, lens, n_cols=4000, seed=None, **kw):
        P[name] = from_lengths(lens, n_cols, len(P) + 10 if seed is None else seed, name=name, **kw)

    add("empty_start", with_empty_rows(mixed, [(0, 5)]))
    add("empty_middle", with_empty_rows(mixed, [(300, 303)]))
    add("empty_last", with_empty_rows(mixed, [(699, 700)]))
    add("empty_64", with_empty_rows(mixed, [(100, 164)]))
    add("empty_65", with_empty_rows(mixed, [(100, 165)]))
    add("empty_65_last", with_empty_rows(mixed, [(635, 700)]))
    add("nnz0", np.zeros(130, dtype=np.int64))
    short = geometric_lengths(300, 4, 2, cap=40)
    for name, big in (("row_2048", K_STREAM_NNZ), ("row_2049", K_STREAM_NNZ + 1), ("row_6144", 3 * K_STREAM_NNZ)):
        L = short.copy()
        L[150] = big
        add(name, L, n_cols=20000)
    add("len_1_2", 1 + (np.arange(1000) % 2))
    add("len_1", np.ones(333, dtype=np.int64))
    for mean, n in ((3, 2000), (12, 1500), (60, 800), (150, 500), (300, 300)):
        add(f"geom_{mean}", geometric_lengths(n, mean, 20 + mean, cap=1500), n_cols=6000)
    even = 2 * geometric_lengths(600, 5, 3, cap=200)
    add("even", even, seed=77)
    P["odd_after_0"] = add_entry_to_first_row(P["even"], name="odd_after_0")
    # runs that end on either residue mod 2, the last one on the last entry of the arrays: 64-row runs of 3-entry rows (a
    # run of 192 entries: even ends) and of rows 3, 3, .., 2 (191: ends alternate), then a short last run
    add("ends_even", np.concatenate([np.full(64 * 5 + 6, 3), [4]]))
    L = np.full(64 * 6 + 9, 3)
    L[63::64] = 2
    add("ends_alternate", L)
    add("ends_alternate_plus_1", np.concatenate([L, [1]]))   # the arrays' last entry at the other residue
    # ghost columns
    g_edge = np.zeros(700, dtype=np.int64)
    g_edge[:40] = 2
    g_edge[-30:] = 3
    add("ghost_edges", mixed, n_cols=4400, n_own=4000, ghost_lens=g_edge)
    add("ghost_every_row", mixed, n_cols=4400, n_own=4000, ghost_lens=1 + (np.arange(700) % 3))
    add("ghost_only", np.zeros(500, dtype=np.int64), n_cols=900, n_own=0, ghost_lens=geometric_lengths(500, 7, 4, cap=100))
    add("ghost_one_row_interior_first", mixed, n_cols=4400, n_own=4000, ghost_lens=(np.arange(700) == 699) * 2)
    P["amg_like"] = amg_like(1200, 40, 5)
    return P


def amg_like(n, mean_row, seed):
    """A coarse-operator-like square pattern: random far columns, a band of near ones and the diagonal, nonsymmetric."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        k = int(np.clip(rng.geometric(1.0 / mean_row), 1, n // 4))
        c = np.unique(np.concatenate([rng.integers(0, n, k), np.clip(i + rng.integers(-30, 31, 8), 0, n - 1), [i]]))
        rows.append(len(c))
        cols.append(c)
    return Csr(n, n, np.concatenate([[0], np.cumsum(rows)]), np.concatenate(cols), None, n, "amg_like")


def block_patterns():
    """name -> (R, C, Csr): node-structured patterns (expanded from block patterns), and one that is not."""
    P = {}
    bl = geometric_lengths(400, 7, 6, cap=120)

    def add(name, Rr, Cc, blens, nb_cols=2600, **kw):
        B = from_lengths(blens, nb_cols, len(P) + 50, **kw)
        P[name] = (Rr, Cc, expand_blocks(B, Rr, Cc, name=name))

    for Rr, Cc in ((2, 2), (2, 1), (1, 2), (1, 1)):
        t = f"{Rr}x{Cc}"
        add(f"blk{t}_mixed", Rr, Cc, with_empty_rows(bl, [(10, 12), (200, 330)]))
        add(f"blk{t}_empty_tail", Rr, Cc, with_empty_rows(bl, [(330, 400)]))      # trailing runs without a block
        add(f"blk{t}_nnz0", Rr, Cc, np.zeros(70, dtype=np.int64))
        L = bl.copy()
        L[77] = K_BLK_MAX
        add(f"blk{t}_row_{K_BLK_MAX}", Rr, Cc, L)
        L = bl.copy()
        L[77] = K_BLK_MAX + 1
        add(f"blk{t}_row_{K_BLK_MAX + 1}", Rr, Cc, L)
        gl = np.zeros(400, dtype=np.int64)
        gl[:20] = 1
        gl[-25:] = 2
        add(f"blk{t}_ghost_edges", Rr, Cc, bl, nb_cols=2900, n_own=2600, ghost_lens=gl)
        add(f"blk{t}_ghost_every_row", Rr, Cc, bl, nb_cols=2900, n_own=2600, ghost_lens=np.ones(400, dtype=np.int64))
    for Rr, Cc in ((2, 2), (2, 1), (1, 2)):
        A = P[f"blk{Rr}x{Cc}_mixed"][2]
        P[f"blk{Rr}x{Cc}_broken"] = (Rr, Cc, remove_entry(A, A.nnz // 2, name=f"blk{Rr}x{Cc}_broken"))
    return P


def pair_patterns():
    """name -> (A, B): two matrices over the same rows, A with 2 x 2 node structure (every row pointer even), B 2 x 1 — the
    velocity block row [F  B~^T] of the Jacobian — with runs where only one of them holds entries, and block rows where
    one of them takes the whole cap."""
    P = {}
    nb = 420
    la = geometric_lengths(nb, 9, 8, cap=150)
    lb = geometric_lengths(nb, 4, 9, cap=60)

    def add(name, LA, LB, seed, a_kw=None, **kw):
        A = expand_blocks(from_lengths(LA, 2400, seed, **(a_kw or {})), 2, 2, name=name + ":A")
        B = expand_blocks(from_lengths(LB, 1300, seed + 1, **kw), 2, 1, name=name + ":B")
        P[name] = (A, B)

    add("pair_mixed", la, lb, 60)
    add("pair_B_empty_runs", la, with_empty_rows(lb, [(0, 130), (300, 420)]), 62)
    add("pair_A_empty_runs", with_empty_rows(la, [(0, 130), (290, 420)]), lb, 64)
    add("pair_both_empty_tail", with_empty_rows(la, [(340, 420)]), with_empty_rows(lb, [(340, 420)]), 66)
    add("pair_A_nnz0", np.zeros(nb, dtype=np.int64), lb, 68)
    add("pair_B_nnz0", la, np.zeros(nb, dtype=np.int64), 70)
    L, M = la.copy(), lb.copy()
    L[50], M[50] = K_BLK_MAX, 0            # A takes the whole cap of the blocked plan
    L[90], M[90] = 0, K_BLK_MAX            # B does
    L[130], M[130] = K_BLK_MAX - 7, 7      # together exactly the cap
    L[170], M[170] = K_STREAM_NNZ // 4, 0  # 2 x 2: 2048 scalars per row of A: the cap of the scalar plan
    add("pair_caps", L, M, 72)
    L, M = la.copy(), lb.copy()
    L[50], M[50] = K_BLK_MAX - 7, 8        # one block too many
    add("pair_over_cap", L, M, 74)
    gl = np.zeros(nb, dtype=np.int64)
    gl[:15] = 1
    gl[-15:] = 2
    add("pair_ghost", la, lb, 76, n_own=1200, ghost_lens=gl)
    # ghost columns in both (F has them in every multi-rank run), in other rows and other numbers than B's
    ga = np.zeros(nb, dtype=np.int64)
    ga[:25] = 2
    ga[-10:] = 1
    ga[200] = 3
    add("pair_ghost_both", la, lb, 78, a_kw=dict(n_own=2250, ghost_lens=ga), n_own=1200, ghost_lens=gl)
    return P


def big_mixed(n_rows=1 << 20, seed=99):
    """About 2^20 rows of mixed lengths (mean ~ 8, a few of several hundred), with stretches of empty rows."""
    L = geometric_lengths(n_rows, 8, seed, cap=900)
    L[5000:5100] = 0
    L[-3:] = 0
    L[123456] = K_STREAM_NNZ
    return from_lengths(L, 1 << 20, seed + 1, name="big_mixed")


def generator_blocks(nx, ny):
    """The generator's F, B~, B~^T, M_p as (name, R, C, Csr)."""
    from navier_stokes_solver_amd import problem as Pm
    pr = Pm.generate(nx, ny, nu=1.0 / 90.0, mode=1, state=1, inlet_bc=0)
    out = []
    for name, m, Rr, Cc in (("F", pr.F, 2, 2), ("Bt", pr.Bt, 2, 1), ("B", pr.B, 1, 2), ("Mp", pr.Mp, 1, 1)):
        out.append((name, Rr, Cc, Csr(m.rows, m.cols, m.rowptr, m.col, m.val, m.cols, f"{name}_{nx}x{ny}")))
    return out
