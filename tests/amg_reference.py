"""Host reference for the kernels of the AMG set-up (tests/test_gpu_amg_kernels.py, nsk_internal.h: nsk_debug_amg).

Everything here is EXACT: integers are Python / int64 integers, floating point is a sequence of single IEEE double
operations in the order stated below (numpy element-wise operations and Python floats round once per operation and never
fuse), and results are compared through their bit patterns (`bits`: -0.0, NaN payloads and last bits all count).

What the reference fixes:
  scan        out[i] = in[0] + .. + in[i-1] in 64 bits, stored as the low 32 bits; out[n] the total
  block       rows [r0, r1), the entries with r0 <= col < r1 in the row's order, columns shifted by r0
  diag        d = the stored a_ii (0.0 when the row lists none): ad = |d|, dinv = 1 / d, or 1 when d == 0 (+0.0 and -0.0)
  strength    t2 = fl(t t); entry (i, j), j != i, is strong when fl(v v) > fl(fl(t2 ad_i) ad_j)   — strict
              flag word (rp[i] >> 4) + i + c, bit l  <->  entry 16 c + l of row i; words no row owns are not written
              key_i = 1 << 62 | (mix32(i) >> 2) << 31 | i for rows with a strong entry, else 0; agg_i = -1 / -2
  pull 1      out_i = max(key_i, key_j over strong j) for the rows with need_i == stamp (all rows when stamp < 0); a root's
              is its own key; the other rows keep what out held
  pull 2      the same over pull 1's result, for undecided rows only
  decide      undecided i: k2 == key -> root (state 2); k2 a root's -> out (0); else m = k2 & (2^31 - 1) (31 bits): out when
              row m found its own key (k2_m == key_m); everything read from the round's snapshot
  mark        need = stamp for the undecided rows and their (outgoing) strong neighbours
  roots       numbered in row order from `first`
  join        rows with agg == -1: the strong neighbour j with agg_in[j] >= 0 (roots_only: and j a root) of the largest
              float32(|a_ij|), strict `>` in row order (the first of equal floats stays), read from the snapshot agg_in
  weights     count_a = rows of aggregate a, pw_a = 1 / sqrt(count_a) (both operations correctly rounded)
  prolongator row i, column `mine` of the sorted distinct aggregates {agg_i} + {agg_j}: acc = (mine == agg_i ? pw : 0.0),
              then acc = fl(acc - fl(fl(fl(c dinv_i) a_ik) pw_mine)) for the entries k of the row with agg_col == mine, in
              row order
  product     C = A B: every accumulator starts at +0.0 and receives fl(a_ik b_kj) in the order of A's row; columns sorted
  transpose   rows = columns of A, each sorted by column (= A's row index)
  rows_sort   every row by column, the value travels with its column
  start       x_i = ((i * 2654435761 mod 2^32) >> 8 & 0xffff) / 65536 - 0.5

The case matrices are named and seeded (`case(name)`); tests/test_amg_reference.py asserts that each holds the rows it is
named for.  `mutate` arguments break one rule the way a wrong kernel would; the CPU tests show that a case catches each.
"""
from __future__ import annotations

import functools

import numpy as np

u64 = np.uint64
LPR = 16                 # lanes per row of the graph kernels
SCAN_CHUNK = 2048        # elements per workgroup of the scan; the middle kernel takes 1024 chunks per trip
SORT_STAGE = 2048        # columns of a row the sort stages
SCAN_CAP = 2147483000    # Scratch::scan: a total above this is error -80
TIER_LANES = (8, 16, 64)
TIER_SLOTS = (64, 128, 512)
THRESHOLD = 1e-4


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Mat:
    """CSR, rows in ANY order unless stated; int32 indices, float64 values."""

    def __init__(self, n_rows, n_cols, rp, col, val, name=""):
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.rp = np.ascontiguousarray(rp, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.name = name
        assert len(self.rp) == self.n_rows + 1 and self.rp[0] == 0 and len(self.col) == len(self.val) == self.rp[-1]
        assert self.nnz == 0 or (self.col.min() >= 0 and self.col.max() < self.n_cols)

    @property
    def nnz(self):
        return int(self.rp[-1])

    @property
    def lens(self):
        return np.diff(self.rp.astype(np.int64))

    @property
    def row(self):
        return np.repeat(np.arange(self.n_rows, dtype=np.int64), self.lens)

    def scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.val, self.col, self.rp), shape=(self.n_rows, self.n_cols))

    def same(self, other):
        return (self.n_rows == other.n_rows and self.n_cols == other.n_cols and np.array_equal(self.rp, other.rp)
                and np.array_equal(self.col, other.col) and np.array_equal(bits(self.val), bits(other.val)))


def from_rows(n_cols, rows, name=""):
    """rows: per row a list of (column, value)."""
    lens = [len(r) for r in rows]
    col = [c for r in rows for c, _ in r]
    val = [v for r in rows for _, v in r]
    return Mat(len(rows), n_cols, np.concatenate([[0], np.cumsum(lens)]), np.asarray(col, dtype=np.int64),
               np.asarray(val, dtype=np.float64), name)


def from_scipy(A, name=""):
    A = A.tocsr()
    A.sort_indices()
    return Mat(A.shape[0], A.shape[1], A.indptr, A.indices, A.data, name)


# ------------------------------------------------------------------ scan, block, diagonal
def scan(x, mutate=None):
    """(out as the int32 array the kernel stores, the 64-bit total)."""
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros(len(x) + 1, dtype=np.int64)
    np.cumsum(x, out=out[1:])
    total = int(out[-1])
    if mutate == "drop_carry":       # the middle kernel forgets what the earlier trips of 1024 chunks summed to
        trip = SCAN_CHUNK * 1024
        for b in range(trip, len(x), trip):
            out[b:min(b + trip, len(x))] -= out[b]
    return out.astype(np.int32), total


def block(A, r0, r1, mutate=None):
    rows = []
    for i in range(r0, r1):
        ks = range(A.rp[i], A.rp[i + 1])
        rows.append([(int(A.col[k]) - (0 if mutate == "global_columns" else r0), A.val[k]) for k in ks if r0 <= A.col[k] < r1])
    if mutate == "global_columns":
        lens = [len(r) for r in rows]
        return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.asarray([c for r in rows for c, _ in r], dtype=np.int32),
                np.asarray([v for r in rows for _, v in r], dtype=np.float64))
    B = from_rows(max(r1 - r0, 1), rows)
    return B.rp, B.col, B.val


def diag(A):
    d = np.zeros(A.n_rows)
    on = A.col == A.row
    assert np.all(np.bincount(A.row[on], minlength=A.n_rows) <= 1), "a row lists its diagonal once"
    d[A.row[on]] = A.val[on]
    with np.errstate(divide="ignore"):
        dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    return np.abs(d), dinv


# ------------------------------------------------------------------ aggregation
def mix32(h):
    h = h.astype(u64)
    h ^= h >> u64(16); h = (h * u64(0x7feb352d)) & u64(0xffffffff)
    h ^= h >> u64(15); h = (h * u64(0x846ca68b)) & u64(0xffffffff)
    h ^= h >> u64(16)
    return h


def state(key):
    return (np.asarray(key, dtype=u64) >> u64(62)).astype(np.int64)


def flag_words(nnz, n_rows):
    return nnz // LPR + n_rows + 2


def flag_index(A):
    """Per entry: (word, bit) of its strength flag."""
    rp = A.rp.astype(np.int64)
    pos = np.arange(A.nnz, dtype=np.int64) - rp[A.row]
    return (rp[A.row] >> 4) + A.row + pos // LPR, pos % LPR


def strength(A, ad, t, mutate=None):
    """(strong per entry, the flag words — 0xFFFF where no row owns the word —, key, agg, undecided)."""
    t2 = np.float64(t) * np.float64(t)
    v, row, col = A.val, A.row, A.col.astype(np.int64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        rhs = t2 * (ad[row] * ad[col]) if mutate == "product_first" else (t2 * ad[row]) * ad[col]
        lhs = v * v
        strong = (col != row) & ((lhs >= rhs) if mutate == "ge" else (lhs > rhs))
    n = A.n_rows
    fw = np.full(flag_words(A.nnz, n), 0xFFFF, dtype=np.uint16)
    rp = A.rp.astype(np.int64)
    steps = -(-A.lens // LPR)
    base = (rp[:-1] >> 4) + np.arange(n)
    owned = np.repeat(base, steps) + (np.arange(steps.sum()) - np.repeat(np.cumsum(steps) - steps, steps))
    fw[owned] = 0
    w, b = flag_index(A)
    np.bitwise_or.at(fw, w[strong], (1 << b[strong]).astype(np.uint16))
    has = np.zeros(n, bool)
    has[row[strong]] = True
    idx = np.arange(n, dtype=u64)
    key = np.where(has, (u64(1) << u64(62)) | ((mix32(idx) >> u64(2)) << u64(31)) | idx, u64(0)).astype(u64)
    return strong, fw, key, np.where(has, -1, -2).astype(np.int32), int(has.sum())


def strong_from_flags(A, fw):
    w, b = flag_index(A)
    return ((fw[w] >> b.astype(np.uint16)) & 1).astype(bool)


def _row_max(A, strong, v):
    out = v.copy()
    np.maximum.at(out, A.row[strong], v[A.col[strong]])
    return out


def pull(A, strong, key, vin, out, pass_, need=None, stamp=-1):
    """One launch of mis_pull: `out` is what the array held; returns what it holds afterwards."""
    key, vin, out = np.asarray(key, dtype=u64), np.asarray(vin, dtype=u64), np.asarray(out, dtype=u64).copy()
    m = _row_max(A, strong, vin)
    s = state(key)
    if pass_ == 2:
        rows = s == 1
    else:
        rows = np.ones(A.n_rows, bool) if stamp < 0 else np.asarray(need) == stamp
        root = rows & (s == 2)
        out[root] = key[root]
        rows = rows & (s != 2)
    out[rows] = m[rows]
    return out


def decide(key, k2):
    key, k2 = np.asarray(key, dtype=u64), np.asarray(k2, dtype=u64)
    und = state(key) == 1
    becomes_root = und & (k2 == key)
    sees_root = und & ~becomes_root & (state(k2) == 2)
    m = np.where(und, (k2 & u64(0x7fffffff)).astype(np.int64), 0)
    sees_root_to_be = und & ~becomes_root & ~sees_root & (k2[m] == key[m])
    out = key.copy()
    out[becomes_root] = (key[becomes_root] & ~(u64(3) << u64(62))) | (u64(2) << u64(62))
    out[sees_root | sees_root_to_be] = 0
    return out, int((state(out) == 1).sum())


def mark(A, strong, key, stamp, need):
    need = np.asarray(need, dtype=np.int32).copy()
    und = state(key) == 1
    need[und] = stamp
    need[A.col[strong & und[A.row]]] = stamp
    return need


def root_ids(key, agg, first=0, mutate=None):
    agg = np.asarray(agg, dtype=np.int32).copy()
    r = np.flatnonzero(state(key) == 2)
    if mutate == "by_key":
        r = r[np.argsort(np.asarray(key, dtype=u64)[r], kind="stable")]
    agg[r] = first + np.arange(len(r))
    return agg, len(r)


def join(A, strong, key, roots_only, agg_in, agg_out, mutate=None):
    """One launch of join: rows with agg_in != -1 copy it; the others take their strongest candidate's, or stay -1."""
    agg_in = np.asarray(agg_in, dtype=np.int32)
    out = np.asarray(agg_out, dtype=np.int32).copy()
    out[agg_in != -1] = agg_in[agg_in != -1]
    live = out.copy() if mutate == "live" else None      # (the mutation: earlier rows' joins are seen)
    st = state(key)
    for i in np.flatnonzero(agg_in == -1):
        src = live if live is not None else agg_in
        best, bagg = -1.0, -1
        for k in range(A.rp[i], A.rp[i + 1]):
            j = A.col[k]
            if not strong[k] or src[j] < 0 or (roots_only and st[j] != 2):
                continue
            w = abs(A.val[k]) if mutate == "double" else float(np.float32(abs(A.val[k])))
            if w > best or (mutate == "last" and w == best):
                best, bagg = w, int(src[j])
        out[i] = bagg
        if live is not None:
            live[i] = bagg
    return out


def agg_weights(agg, nc):
    agg = np.asarray(agg)
    count = np.bincount(agg[agg >= 0], minlength=nc).astype(np.int32)
    with np.errstate(divide="ignore"):
        return count, 1.0 / np.sqrt(count.astype(np.float64))


class Aggregation:
    pass


def aggregate(A, ad=None, t=THRESHOLD, mutate=None, max_rounds=None):
    """The whole of aggregate() with the set-up's stamping rule; .und[r] = undecided rows before round r, .stamped[r] =
    pass 1 of round r ran on the marked rows only, .keys[r] = the keys after round r."""
    n = A.n_rows
    R = Aggregation()
    ad = diag(A)[0] if ad is None else ad
    strong, fw, key, agg, und = strength(A, ad, t, "ge" if mutate == "ge" else "product_first" if mutate == "product_first" else None)
    R.strong, R.fw, R.key0 = strong, fw, key
    need = np.full(n, -1, dtype=np.int32)
    k1 = np.full(n, u64(0xFFFFFFFFFFFFFFFF), dtype=u64)
    k2 = k1.copy()
    R.und, R.stamped, R.keys = [], [], []
    stamp, stamp_base = -1, 0
    if 0 < und < n // 2:
        stamp_base += 1
        stamp = stamp_base
        need = mark(A, strong, key, stamp, need)
    while und > 0:
        if len(R.und) > n:
            raise RuntimeError("the independent-set rounds do not end")      # (the set-up's error -82)
        if max_rounds is not None and len(R.und) >= max_rounds:
            break                                                            # (a mutated model may never end)
        R.und.append(und)
        R.stamped.append(stamp >= 0)
        if mutate == "stale_pull1":       # pass 1 on the marked rows, pass 2 reading rows pass 1 skipped
            k1 = pull(A, strong, key, key, k1, 1, np.where(state(key) == 1, stamp, -7) if stamp >= 0 else need, stamp)
        else:
            k1 = pull(A, strong, key, key, k1, 1, need, stamp)
        k2 = pull(A, strong, key, k1, k2, 2)
        key, und = decide(key, k2)
        R.keys.append(key)
        stamp = -1
        if 0 < und < n // 2:
            stamp_base += 1
            stamp = stamp_base
            need = mark(A, strong, key, stamp, need)
    R.key = key
    agg, nc = root_ids(key, agg, 0, "by_key" if mutate == "by_key" else None)
    R.agg_roots = agg
    jm = mutate if mutate in ("last", "double") else None
    R.agg_a = join(A, strong, key, 1, agg, np.full(n, -9, np.int32), jm)
    R.agg = join(A, strong, key, 0, R.agg_a, np.full(n, -9, np.int32), "live" if mutate == "live" else jm)
    R.nc = nc
    R.count, R.pw = agg_weights(R.agg, nc) if nc > 0 else (np.zeros(0, np.int32), np.zeros(0))
    return R


def aggregate_numpy(A):
    """DESIGN.md 5a restated with numpy (whole-array rounds, no row order anywhere): the second, independent statement of
    the aggregation rule that oracle/nsk_oracle_amg.c and the device kernels follow."""
    A = A.tocsr()
    A.sort_indices()
    n = A.shape[0]
    rp, col, val = A.indptr, A.indices, A.data
    row = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    d[row[col == row]] = np.abs(val[col == row])
    strong = (col != row) & (val * val > (1e-4 * 1e-4) * d[row] * d[col])
    has = np.zeros(n, bool)
    has[row[strong]] = True
    u = np.uint64

    def mix32(h):
        h = h.astype(u)
        h ^= h >> u(16); h = (h * u(0x7feb352d)) & u(0xffffffff)
        h ^= h >> u(15); h = (h * u(0x846ca68b)) & u(0xffffffff)
        h ^= h >> u(16)
        return h
    idx = np.arange(n, dtype=u)
    key = np.where(has, (u(1) << u(62)) | ((mix32(idx) >> u(2)) << u(31)) | idx, u(0)).astype(u)
    srow, scol = row[strong], col[strong]

    def pull(v):                                        # max over the row itself and its strong (directed) neighbours
        out = v.copy()
        np.maximum.at(out, srow, v[scol])
        return out
    while np.any((key >> u(62)) == 1):
        k2 = pull(pull(key))
        und = (key >> u(62)) == 1
        becomes_root = und & (k2 == key)
        sees_root = und & ((k2 >> u(62)) == 2)
        m = (k2 & u(0x7fffffff)).astype(np.int64)      # the row whose key was found
        sees_root_to_be = und & ~becomes_root & ~sees_root & ((k2 >> u(62)) == 1) & becomes_root[m]
        key = np.where(becomes_root, (key & ~(u(3) << u(62))) | (u(2) << u(62)), key)
        key = np.where(sees_root | sees_root_to_be, u(0), key)
    is_root = (key >> u(62)) == 2
    agg = np.where(has, -1, -2).astype(np.int64)
    agg[is_root] = np.arange(is_root.sum())
    for roots_only in (True, False):
        snap = agg.copy()
        for i in np.flatnonzero(snap == -1):
            ks = np.arange(rp[i], rp[i + 1])
            ks = ks[strong[ks] & (snap[col[ks]] >= 0)]
            if roots_only:
                ks = ks[is_root[col[ks]]]
            if len(ks):
                w = np.abs(val[ks]).astype(np.float32)
                agg[i] = snap[col[ks[np.argmax(w)]]]    # (argmax: the first of equal weights)
    return agg


# ------------------------------------------------------------------ ordered sums
def _ordered(init, gid, terms, sub):
    """acc[g] = init[g], then one term after the other in the order given (gid: group of every term, groups contiguous
    and in order): one rounded operation per term."""
    acc = np.asarray(init, dtype=np.float64).copy()
    if len(gid) == 0:
        return acc
    first = np.concatenate([[True], gid[1:] != gid[:-1]])
    start = np.flatnonzero(first)
    pos = np.arange(len(gid)) - np.repeat(start, np.diff(np.concatenate([start, [len(gid)]])))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(int(pos.max()) + 1):
            sel = pos == s
            g = gid[sel]
            acc[g] = acc[g] - terms[sel] if sub else acc[g] + terms[sel]
    return acc


def prolongator(A, agg, pw, dinv, c):
    """P = (I - c D^-1 A) Phat as the kernel forms it; columns = aggregates, sorted."""
    agg = np.asarray(agg, dtype=np.int64)
    n = A.n_rows
    row, a = A.row, agg[A.col]
    own = agg >= 0
    keys = np.concatenate([row[a >= 0] * (2 ** 31) + a[a >= 0], np.flatnonzero(own) * (2 ** 31) + agg[own]])
    uk = np.unique(keys)
    crow, ccol = uk >> 31, uk & (2 ** 31 - 1)
    rp = np.concatenate([[0], np.cumsum(np.bincount(crow, minlength=n))])
    init = np.where(ccol == agg[crow], pw[ccol], 0.0)
    k = np.flatnonzero(a >= 0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        si = np.float64(c) * dinv
        terms = ((si[row[k]] * A.val[k]) * pw[a[k]])
    g = np.searchsorted(uk, row[k] * (2 ** 31) + a[k])
    order = np.argsort(g, kind="stable")         # (stable: the terms of one accumulator stay in row order)
    val = _ordered(init, g[order], terms[order], True)
    return Mat(n, max(int(len(pw)), 1), rp, ccol, val)


def product(A, B, mutate=None):
    """C = A B; B's rows hold distinct columns."""
    la = B.lens[A.col]
    k = np.repeat(np.arange(A.nnz, dtype=np.int64), la)
    q = np.arange(la.sum(), dtype=np.int64) - np.repeat(np.cumsum(la) - la, la) + np.repeat(B.rp.astype(np.int64)[A.col], la)
    i, j = A.row[k], B.col[q].astype(np.int64)
    key = i * (2 ** 31) + j
    uk = np.unique(key)
    g = np.searchsorted(uk, key)
    if mutate == "reverse":
        k = -k
    order = np.lexsort((k, g))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        terms = A.val[np.abs(k)] * B.val[q]
    val = _ordered(np.zeros(len(uk)), g[order], terms[order], False)
    rp = np.concatenate([[0], np.cumsum(np.bincount(uk >> 31, minlength=A.n_rows))])
    return Mat(A.n_rows, B.n_cols, rp, uk & (2 ** 31 - 1), val)


def transpose(A):
    order = np.argsort(A.col, kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(A.col, minlength=A.n_cols))])
    return Mat(A.n_cols, A.n_rows, rp, A.row[order], A.val[order])


def rows_sort(A, mutate=None):
    """(col, val) with every row sorted by column."""
    col, val = A.col.copy(), A.val.copy()
    for i in range(A.n_rows):
        a0, a1 = int(A.rp[i]), int(A.rp[i + 1])
        if mutate == "no_tail" and a1 - a0 > SORT_STAGE:
            # the rank counts the staged columns only: entries land on each other, the rest of the row is never written
            c, v = A.col[a0:a1], A.val[a0:a1]
            col[a0:a1], val[a0:a1] = -1, np.nan
            for e in range(a1 - a0):
                r = int((c[:SORT_STAGE] < c[e]).sum())
                col[a0 + r], val[a0 + r] = c[e], v[e]
            continue
        o = np.argsort(A.col[a0:a1], kind="stable")
        col[a0:a1], val[a0:a1] = A.col[a0:a1][o], A.val[a0:a1][o]
    return col, val


def start_vector(n):
    h = (np.arange(n, dtype=u64) * u64(2654435761)) & u64(0xffffffff)
    return ((h >> u64(8)) & u64(0xffff)).astype(np.float64) / 65536.0 - 0.5


# ------------------------------------------------------------------ case matrices
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
DIAG_PLACES = ["first", "last", "late", "absent"]        # late: at position >= 16 of the row (rows of 17 entries and more)


def _values(rng, m):
    """Negative off-diagonals over 10^-6 .. 1: a part of them is weak at the default threshold."""
    return -(rng.uniform(0.1, 1.0, m) * 10.0 ** rng.integers(-6, 1, m))


def lengths(n, seed=11, name=None):
    """Row i: LENGTHS[i % 15] entries (unsorted), the diagonal first / last / at position >= 16 / absent by (i // 15) % 4;
    diagonal values positive, negative, +0.0 and -0.0."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        ln = min(LENGTHS[i % 15], n - 1)
        place = DIAG_PLACES[(i // 15) % 4]
        if ln == 0:
            rows.append([])
            continue
        have_diag = place != "absent"
        others = rng.permutation(np.delete(np.arange(n), i))[:ln - have_diag]
        ent = list(zip(others.tolist(), _values(rng, len(others)).tolist()))
        if have_diag:
            d = [3.0, -2.5, 7.0, 0.0, 1.5, -0.0, 4.0][(i // 30) % 7] if i >= 30 else 2.0 + (i % 5)
            pos = 0 if place == "first" else len(ent) if place == "last" else (int(rng.integers(16, ln)) if ln >= 17 else len(ent))
            ent.insert(pos, (i, d))
        rows.append(ent)
    return from_rows(n, rows, name or f"lengths{n}")


def ties():
    """Threshold 0.5 (t2 = 0.25 exactly), powers of two: v^2 equal to, one ulp above and one ulp below t2 ad_i ad_j."""
    p4, s4 = np.nextafter(4.0, 0.0), np.nextafter(4.0, 8.0)
    rows = [
        [(0, 4.0), (1, 2.0)],                       # 4 > 4: weak — a row of weak entries only: agg -2, key 0
        [(1, 4.0), (0, -2.0), (2, 2.0)],            # (1, 0) equal: weak; (1, 2): 4 > pred(4): strong
        [(1, 2.0), (2, p4)],                        # 4 > (0.25 pred(4)) 4 = pred(4): strong
        [(3, s4), (4, 2.0)],                        # 4 > succ(4): weak — all weak
        [(3, 2.0), (4, 4.0), (5, 3.0)],             # (4, 3) one ulp below: weak; (4, 5) strong
        [(4, 1.0), (5, 4.0), (6, 3.0)],             # (5, 4) weak while (4, 5) is strong: one direction only
        [(5, 3.0), (6, 4.0)],
        [(7, 4.0)],                                 # diagonal only
    ]
    return from_rows(8, rows, "ties"), 0.5


def ties_order():
    """Threshold 2^-500: fl(fl(t2 ad_i) ad_j) = 2^200 where ad_i ad_j overflows; v = 2^101 is strong in the stated order."""
    b, v = 2.0 ** 600, 2.0 ** 101
    rows = [[(0, b), (1, v)], [(0, -v), (1, b), (2, 2.0 ** 99)], [(1, v), (2, b)]]
    return from_rows(3, rows, "ties_order"), 2.0 ** -500


TIE_LO, TIE_HI = 1.0, 1.0 + 2.0 ** -40          # equal as floats, different as doubles
TIE_PAIRS = [(3, 20), (3, 9), (3, 70), (17, 30), (40, 41), (0, 79)]   # positions in the row: other step / lane / unroll group


def float_ties():
    """n = 200, sorted rows, full diagonal.  Rows 0 .. 2 |TIE_PAIRS| - 1 are tie rows: 80 off-diagonal entries (the rows 20, 22,
    .. 178) of weight 0.5 except two of weight TIE_LO / TIE_HI at the pair's positions — row 2 p holds the larger double
    first, row 2 p + 1 second.  The other rows are a chain.  Returns (A, positions [(row, k_first, k_second)])."""
    n = 200
    rows, where = [], []
    for r in range(2 * len(TIE_PAIRS)):
        p1, p2 = TIE_PAIRS[r // 2]
        w = np.full(80, 0.5)
        w[p1], w[p2] = (TIE_HI, TIE_LO) if r % 2 == 0 else (TIE_LO, TIE_HI)
        rows.append([(r, 4.0)] + [(20 + 2 * e, -w[e]) for e in range(80)])
        where.append((r, 1 + p1, 1 + p2))
    for i in range(len(rows), n):
        ent = [(i - 1, -1.0)] if i > len(rows) else []
        ent.append((i, 4.0))
        if i + 1 < n:
            ent.append((i + 1, -1.0))
        rows.append(ent)
    return from_rows(n, rows, "float_ties"), where


def float_ties_join_inputs(A):
    """What JOIN gets on float_ties: every entry strong, every row but the tie rows a root with an aggregate of its own."""
    n = A.n_rows
    t = 2 * len(TIE_PAIRS)
    strong = A.col != A.row
    idx = np.arange(n, dtype=u64)
    key = (u64(2) << u64(62)) | idx
    key[:t] = (u64(1) << u64(62)) | idx[:t]
    agg = np.arange(n, dtype=np.int32) + 1000
    agg[:t] = -1
    return strong, key, agg


def laplace2d(k):
    import scipy.sparse as sp
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(k, k))
    return (sp.kron(sp.identity(k), T) + sp.kron(T, sp.identity(k))).tocsr()


def directed_scipy():
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    n = 1500
    R = sp.random(n, n, density=0.004, random_state=7, format="csr")
    R.data = -(rng.uniform(0, 1, R.nnz) * 10.0 ** rng.integers(-6, 1, R.nnz))
    R.setdiag(0)
    R.eliminate_zeros()
    D = sp.diags(np.asarray(abs(R).sum(1)).ravel() + 1.0)
    return (R + D).tocsr()


@functools.lru_cache(maxsize=None)
def case(name):
    """The named square matrices of the graph kernels (default threshold unless the name says otherwise)."""
    import scipy.sparse as sp
    if name.startswith("lengths"):
        return lengths(int(name[7:]))
    if name == "lap40":
        return from_scipy(laplace2d(40), name)
    if name == "path700":
        return from_scipy(sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(700, 700)), name)
    if name == "directed":
        return from_scipy(directed_scipy(), name)
    if name == "float_ties":
        return float_ties()[0]
    if name == "ties":
        return ties()[0]
    if name == "ties_order":
        return ties_order()[0]
    raise KeyError(name)


GRAPH_CASES = ["lengths300", "lengths255", "lengths256", "lengths257", "lap40", "path700", "directed", "float_ties"]
FULL_DIAGONAL = ["lap40", "path700", "directed", "float_ties"]       # what the oracle's aggregates are compared on
THRESHOLDS = {"ties": 0.5, "ties_order": 2.0 ** -500}


# ---- row products
B_LENGTHS = [0, 1, 8, 9, 16, 17, 64, 65, 100]
PRODUCT_COLS = 600
WIDTHS = [63, 64, 65, 127, 128, 129, 511, 512, 513]


@functools.lru_cache(maxsize=None)
def product_b():
    """B: rows 0 .. 8 hold B_LENGTHS[r] entries, the columns 0 .. len - 1 (value 1.0 at column 7 wherever a row holds it);
    row 9 + c holds column c alone."""
    rng = np.random.default_rng(21)
    rows = []
    for ln in B_LENGTHS:
        rows.append([(c, 1.0 if c == 7 else float(rng.uniform(-2, 2))) for c in rng.permutation(ln).tolist()])
    for c in range(PRODUCT_COLS):
        rows.append([(c, float(rng.uniform(-2, 2)))])
    return from_rows(PRODUCT_COLS, rows, "product_b")


ORDER_TERMS = [1.0, 2.0 ** -53, -1.0, 2.0 ** -53]     # in this order 2^-53, reversed 2^-52


def _candidate_rows():
    """Rows of A over product_b, with the number of distinct columns of their product."""
    rng = np.random.default_rng(22)
    B = product_b()
    out = [[], [(5, 1.5)], [(0, 2.0)], [(0, 2.0), (1, -1.0), (0 + 9, 0.5)]]
    out.append([(2, ORDER_TERMS[0]), (3, ORDER_TERMS[1]), (4, ORDER_TERMS[2]), (5, ORDER_TERMS[3])])      # column 7: four terms
    for L in (8, 16, 64):
        for ln in (L, L + 1, 4 * L, 4 * L + 1):
            # unit rows (distinct columns below ln), some of them twice through a long row of B
            cols = (9 + rng.permutation(ln)).tolist()
            for pos, r in ((0, 4), (ln // 2, 6), (ln - 1, 8)):
                if B_LENGTHS[r] <= ln:
                    cols[pos] = r
            out.append([(c, float(rng.uniform(-2, 2))) for c in cols])
    for r in range(len(B_LENGTHS)):
        out.append([(r, -0.75), (9 + 3, 0.25)])
    res = []
    for ent in out:
        cols = set()
        for j, _ in ent:
            cols.update(B.col[B.rp[j]:B.rp[j + 1]].tolist())
        res.append((ent, len(cols)))
    return res


@functools.lru_cache(maxsize=None)
def product_a(width):
    """A over product_b whose widest product row holds exactly `width` distinct columns (row 0: the unit rows of the columns
    0 .. width - 1 in random order, and the long rows of B that fit), with every candidate row that is no wider."""
    rng = np.random.default_rng(100 + width)
    first = [(9 + c, float(rng.uniform(-2, 2))) for c in rng.permutation(width).tolist()]
    for r, ln in enumerate(B_LENGTHS):
        if ln <= width:
            first.insert(int(rng.integers(0, len(first))), (r, float(rng.uniform(-2, 2))))
    rows = [first] + [ent for ent, d in _candidate_rows() if d <= width]
    return from_rows(product_b().n_rows, rows, f"product_a{width}")


def tier_for(width):
    """The first tier whose hash set takes a row of `width` distinct columns (3: none, error -81)."""
    return next((t for t, s in enumerate(TIER_SLOTS) if width <= s), 3)


# ---- prolongator
PROLONG_MODULI = [40, 100, 300]      # aggregates: widest rows take tier 0, 1, 2


@functools.lru_cache(maxsize=None)
def prolong_case(modulus):
    """(A, agg, pw, dinv, c): the lengths pattern with a row of 600 entries, agg = a hash of the row modulo `modulus`, -2 on
    every ninth row (own aggregate -2, neighbours at -2); row 46 (a single entry, no diagonal) has an aggregate of its own
    that its neighbour does not have."""
    n = 700
    A0 = lengths(n, seed=13)
    rng = np.random.default_rng(31 + modulus)
    rows = [list(zip(A0.col[A0.rp[i]:A0.rp[i + 1]].tolist(), A0.val[A0.rp[i]:A0.rp[i + 1]].tolist())) for i in range(n)]
    long_cols = rng.permutation(n)[:600]
    rows[44] = list(zip(long_cols.tolist(), _values(rng, 600).tolist()))
    A = from_rows(n, rows, f"prolong{modulus}")
    agg = (mix32(np.arange(n, dtype=u64)) % u64(modulus)).astype(np.int32)
    agg[::9] = -2
    agg[46] = modulus
    nc = modulus + 1
    count, pw = agg_weights(agg, nc)
    pw = np.where(count > 0, pw, 1.0)
    _, dinv = diag(A)
    return A, agg, pw, dinv, (4.0 / 3.0) / 1.7


# ---- sort, transpose, scan, block
SORT_LENGTHS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 3000]


@functools.lru_cache(maxsize=None)
def sort_case(order):
    """Rows of SORT_LENGTHS entries, `order` = reversed / random; value = column + row / 16 (a value on the wrong column shows)."""
    rng = np.random.default_rng(41)
    rows = []
    for i, ln in enumerate(SORT_LENGTHS):
        c = np.sort(rng.permutation(5000)[:ln])
        c = c[::-1] if order == "reversed" else rng.permutation(c)
        rows.append([(int(x), float(x) + i / 16.0) for x in c])
    return from_rows(5000, rows, f"sort_{order}")


@functools.lru_cache(maxsize=None)
def transpose_case():
    """300 x 37: column 5 in every row that has entries, columns 0, 11 and 36 in none, rows 7 and 150 empty."""
    rng = np.random.default_rng(51)
    rows = []
    free = [c for c in range(37) if c not in (0, 5, 11, 36)]
    for i in range(300):
        if i in (7, 150):
            rows.append([])
            continue
        cs = [5] + rng.permutation(free)[:int(rng.integers(0, 6))].tolist()
        cs = rng.permutation(cs).tolist()
        rows.append([(c, i * 64.0 + c) for c in cs])
    return from_rows(37, rows, "transpose")


SCAN_SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4096 + 5, 2048 * 1024 + 1]


def scan_input(n, seed=61):
    return np.random.default_rng(seed + n % 1000).integers(0, 7, n).astype(np.int32)


def scan_cap_input(total):
    """4096 entries whose sum is `total`."""
    x = np.full(4096, total // 4096, dtype=np.int64)
    x[:total - int(x.sum())] += 1
    assert int(x.sum()) == total and x.max() < 2 ** 31
    return x.astype(np.int32)


BLOCK_RANGES = [(0, 650), (1, 650), (300, 650)]


@functools.lru_cache(maxsize=None)
def block_case():
    """lengths with n = 700; rows 310 .. 315 hold columns >= 660 only (nothing of them is inside a range that ends at 650)."""
    n = 700
    A0 = lengths(n, seed=17)
    rng = np.random.default_rng(71)
    rows = [list(zip(A0.col[A0.rp[i]:A0.rp[i + 1]].tolist(), A0.val[A0.rp[i]:A0.rp[i + 1]].tolist())) for i in range(n)]
    for i in range(310, 316):
        cs = 660 + rng.permutation(40)[:5 + i - 310]
        rows[i] = [(int(c), float(i)) for c in cs]
    return from_rows(n, rows, "block")
