// nsk_amg.cpp — see nsk_amg.hpp
#include "nsk_amg.hpp"

#include <memory>
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <chrono>
#include <cmath>

#include <cstdint>
#include <cstring>

#include "nsk_amg_kernels.h"
#include "nsk_internal.h"

namespace nsk {
namespace {

constexpr int kMaxLevels = 10;      // ML "max levels"
constexpr int kCoarseMax = 128;     // ML "coarse: max size"
constexpr int kDenseLimit = 2048;   // a level that does not coarsen any more is still solved directly up to here
constexpr double kThreshold = 1e-4; // deal.II aggregation_threshold
constexpr double kOmega = 4.0 / 3.0;
constexpr int kEigIts = 10;
constexpr double kEigBoost = 1.1;
constexpr double kChebyAlpha = 20.0;

// dense inverse of the coarsest level (the reference's "Amesos-KLU" direct solve, on the host there too)
std::vector<double> dense_inverse(int n, const std::vector<int> &rp, const std::vector<int> &col, const std::vector<double> &val) {
  std::vector<double> M((size_t)n * n, 0.0), I((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    for (int k = rp[i]; k < rp[i + 1]; ++k) M[(size_t)i * n + col[k]] += val[k];
    I[(size_t)i * n + i] = 1.0;
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(M[(size_t)r * n + c]) > std::fabs(M[(size_t)piv * n + c])) piv = r;
    if (piv != c)
      for (int j = 0; j < n; ++j) {
        std::swap(M[(size_t)c * n + j], M[(size_t)piv * n + j]);
        std::swap(I[(size_t)c * n + j], I[(size_t)piv * n + j]);
      }
    const double d = 1.0 / M[(size_t)c * n + c];
    for (int j = 0; j < n; ++j) { M[(size_t)c * n + j] *= d; I[(size_t)c * n + j] *= d; }
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = M[(size_t)r * n + c];
      if (f == 0.0) continue;
      for (int j = 0; j < n; ++j) { M[(size_t)r * n + j] -= f * M[(size_t)c * n + j]; I[(size_t)r * n + j] -= f * I[(size_t)c * n + j]; }
    }
  }
  return I;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

amgk::Mat mat(const Csr &A) { return amgk::Mat{A.n_rows, A.n_cols, A.rowptr.p, A.col.p, A.val.p}; }

// Device arrays of the test hook (debug_amg): each an allocation of its own at its exact size, kGuard bytes with all bits
// set in front of it and behind it.
struct Guarded {
  static constexpr size_t kGuard = 256;   // (the array keeps the alignment hipMalloc gives)
  struct Item {
    DBuf<char> buf;
    size_t bytes;
  };
  hipStream_t s;
  std::vector<Item> items;
  explicit Guarded(hipStream_t st) : s(st) {}
  // count elements, from h (null: all bits set)
  template <class T>
  T *put(const T *h, size_t count) {
    items.emplace_back();
    Item &it = items.back();
    it.bytes = count * sizeof(T);
    it.buf.alloc(it.bytes + 2 * kGuard);
    NSK_HIP(hipMemsetAsync(it.buf.p, 0xFF, it.buf.n, s));
    T *p = reinterpret_cast<T *>(it.buf.p + kGuard);
    if (h && it.bytes) NSK_HIP(hipMemcpyAsync(p, h, it.bytes, hipMemcpyHostToDevice, s));
    return p;
  }
  // 32-bit guard words that no longer hold all bits (a word is counted once however many of its bytes changed)
  int changed() {
    int bad = 0;
    std::vector<unsigned char> g(2 * kGuard);
    for (Item &it : items) {
      NSK_HIP(hipMemcpyAsync(g.data(), it.buf.p, kGuard, hipMemcpyDeviceToHost, s));
      NSK_HIP(hipMemcpyAsync(g.data() + kGuard, it.buf.p + kGuard + it.bytes, kGuard, hipMemcpyDeviceToHost, s));
      NSK_HIP(hipStreamSynchronize(s));
      for (size_t w = 0; w < 2 * kGuard; w += 4) bad += !(g[w] == 0xFF && g[w + 1] == 0xFF && g[w + 2] == 0xFF && g[w + 3] == 0xFF);
    }
    return bad;
  }
};

// Scratch of the set-up.  Work arrays of a level come from an arena that lives across set-ups (a Newton run rebuilds
// the hierarchy before every solve, NSSolverStationary.cpp:621-626, always with the same sizes): the first set-up
// allocates what it needs piece by piece and records the largest level's total, the following ones take slices.
struct Scratch {
  Ctx *ctx;
  DBuf<char> &arena;
  size_t &want;
  size_t top = 0, level_total = 0;
  std::vector<DBuf<char>> spill;
  DBuf<long long> total;
  DBuf<int> counters;   // [0] undecided rows, [1] error word of the row products, [2] signs met on a level's diagonal
  int rounds = 0;       // independent-set rounds so far (NSK_AMG_TIMING)
  Guarded *exact = nullptr;   // test hook: every take() is an allocation of its own at its exact size between guard words
  Scratch(Ctx *c, DBuf<char> &arena_, size_t &want_) : ctx(c), arena(arena_), want(want_) {
    total.alloc(1);
    counters.alloc(3);
  }
  template <class T>
  T *take(size_t count) {
    if (exact) return exact->put<T>(nullptr, count);
    const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
    level_total += bytes;
    if (top + bytes <= arena.n) {
      T *p = reinterpret_cast<T *>(arena.p + top);
      top += bytes;
      return p;
    }
    spill.emplace_back();
    spill.back().alloc(bytes);
    return reinterpret_cast<T *>(spill.back().p);
  }
  void end_level() {   // (the caller has synchronised: nothing in flight reads the level's scratch any more)
    want = std::max(want, level_total);
    spill.clear();
    top = level_total = 0;
  }
  // out[0..n] = exclusive prefix sums of in[0..n); returns the total (one host sync)
  int64_t scan(int n, const int *in, int *out) {
    long long *tmp = take<long long>(amgk::scan_tmp_words(n));
    amgk::scan_exclusive(ctx->stream, n, in, out, tmp, total.p);
    long long t = 0;
    NSK_HIP(hipMemcpyAsync(&t, total.p, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    if (t > 2147483000LL) throw Error(-80, "AMG: level operator too large for 32-bit indices");
    return (int64_t)t;
  }
  int read_counter(int which) {
    int v = 0;
    NSK_HIP(hipMemcpyAsync(&v, counters.p + which, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return v;
  }
  void zero_counter(int which) { NSK_HIP(hipMemsetAsync(counters.p + which, 0, sizeof(int), ctx->stream)); }
};

// what a device-built matrix still needs before the SpMV kernels can take it: the row pointers on the host for the
// row-run plan (n + 1 ints; the pattern itself stays on the device)
void finish_csr(Ctx *ctx, Csr &D, int n_rows, int n_cols, int64_t nnz) {
  D.n_rows = n_rows;
  D.n_cols = D.n_own_cols = n_cols;
  D.nnz = nnz;
  D.h_rowptr.resize((size_t)n_rows + 1);
  NSK_HIP(hipMemcpyAsync(D.h_rowptr.data(), D.rowptr.p, sizeof(int) * ((size_t)n_rows + 1), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  D.lpr = pick_lpr(D.nnz, D.n_rows);
  D.present = true;
  D.build_stream_plan(ctx->stream);
}

// C = A B (product 0) or C = (I - c D^-1 A) Phat (product 1): count and prefix sum (row pointers into rp, n + 1 ints),
// then fill; the narrowest tier first (8 lanes per row; first_tier = 1 where rows are known to hold more than 64
// distinct columns), the next one when a row holds more distinct columns than the tier's hash set takes
struct ProductPlan {
  int tier;
  int64_t nnz;
};
ProductPlan product_rows(Scratch &S, const amgk::RowProduct &P, int product, int first_tier, int *rp) {
  hipStream_t s = S.ctx->stream;
  const int n = P.A.n_rows;
  int *len = S.take<int>((size_t)n + 1);
  const char *hook = std::getenv("NSK_AMG_ROW_TIER");   // test hook: start with the 16- or 64-lane kernels
  int tier = hook ? std::max(first_tier, std::min(2, std::atoi(hook))) : first_tier;
  for (;; ++tier) {
    S.zero_counter(1);
    amgk::product_count(s, P, product, tier, len, S.counters.p + 1);
    if (S.read_counter(1) == 0) break;
    if (tier == 2) throw Error(-81, "AMG set-up: a row of a level operator has more than 512 distinct columns");
  }
  return ProductPlan{tier, S.scan(n, len, rp)};
}
void row_product(Scratch &S, const amgk::RowProduct &P, int product, int n_cols, int first_tier, Csr &C) {
  const int n = P.A.n_rows;
  C.rowptr.alloc((size_t)n + 1);
  const ProductPlan pl = product_rows(S, P, product, first_tier, C.rowptr.p);
  C.col.alloc((size_t)std::max<int64_t>(pl.nnz, 1));
  C.val.alloc((size_t)std::max<int64_t>(pl.nnz, 1));
  S.zero_counter(1);
  amgk::product_fill(S.ctx->stream, P, product, pl.tier, C.rowptr.p, C.col.p, C.val.p, S.counters.p + 1);
  if (S.read_counter(1) != 0) throw Error(-84, "AMG set-up: the fill of a row product found a row its count had not");
  finish_csr(S.ctx, C, n, n_cols, pl.nnz);
}
// the same into scratch: an intermediate product that is never multiplied with a vector
amgk::Mat row_product_scratch(Scratch &S, const amgk::RowProduct &P, int product, int n_cols, int first_tier) {
  const int n = P.A.n_rows;
  int *rp = S.take<int>((size_t)n + 1);
  const ProductPlan pl = product_rows(S, P, product, first_tier, rp);
  int *col = S.take<int>((size_t)pl.nnz);
  double *val = S.take<double>((size_t)pl.nnz);
  S.zero_counter(1);
  amgk::product_fill(S.ctx->stream, P, product, pl.tier, rp, col, val, S.counters.p + 1);
  if (S.read_counter(1) != 0) throw Error(-84, "AMG set-up: the fill of a row product found a row its count had not");
  return amgk::Mat{n, n_cols, rp, col, val};
}

void transpose(Scratch &S, const Csr &A, Csr &T) {
  Ctx *ctx = S.ctx;
  hipStream_t s = ctx->stream;
  const int m = A.n_cols;
  int *count = S.take<int>((size_t)m + 1);
  NSK_HIP(hipMemsetAsync(count, 0, sizeof(int) * ((size_t)m + 1), s));
  amgk::col_count(s, (long)A.nnz, A.col.p, count);
  T.rowptr.alloc((size_t)m + 1);
  const int64_t nnz = S.scan(m, count, T.rowptr.p);
  int *cursor = S.take<int>((size_t)m + 1);
  NSK_HIP(hipMemcpyAsync(cursor, T.rowptr.p, sizeof(int) * ((size_t)m + 1), hipMemcpyDeviceToDevice, s));
  int *tcol = S.take<int>((size_t)nnz);
  double *tval = S.take<double>((size_t)nnz);
  T.col.alloc((size_t)std::max<int64_t>(nnz, 1));
  T.val.alloc((size_t)std::max<int64_t>(nnz, 1));
  amgk::transpose_scatter(s, mat(A), cursor, tcol, tval);
  amgk::rows_sort(s, m, T.rowptr.p, tcol, tval, T.col.p, T.val.p);
  finish_csr(ctx, T, m, A.n_rows, nnz);
}

// aggregates of the level: returns their number; agg and pw are level scratch
int aggregate(Scratch &S, const Csr &A, const double *ad, int *&agg, double *&pw) {
  Ctx *ctx = S.ctx;
  hipStream_t s = ctx->stream;
  const int n = A.n_rows;
  const amgk::Mat M = mat(A);
  uint16_t *flag = S.take<uint16_t>(amgk::flag_words((long)A.nnz, n));
  int *need = S.take<int>((size_t)n), *other = S.take<int>((size_t)n);
  uint64_t *key = S.take<uint64_t>((size_t)n), *k1 = S.take<uint64_t>((size_t)n), *k2 = S.take<uint64_t>((size_t)n);
  uint64_t *key_next = S.take<uint64_t>((size_t)n);
  agg = S.take<int>((size_t)n);
  pw = nullptr;
  int *is_root = S.take<int>((size_t)n), *scan = S.take<int>((size_t)n + 1);
  NSK_HIP(hipMemsetAsync(need, 0xff, sizeof(int) * (size_t)n, s));
  int stamp_base = 0;
  // synchronous independent-set rounds over the connections in `bits`; every round decides at least the undecided row
  // with the largest key.  Returns the number of roots found and gives them the aggregate ids first, first + 1, ...
  auto roots = [&](const uint16_t *bits, int undecided, int first) {
    int stamp = -1;
    if (undecided > 0 && undecided < n / 2) {   // few candidates from the start
      stamp = ++stamp_base;
      amgk::mis_mark(s, M, bits, key, stamp, need);
    }
    for (int round = 0; undecided > 0; ++round) {
      if (round > n) throw Error(-82, "AMG set-up: the independent-set rounds do not end");
      amgk::mis_pull(s, M, bits, 1, key, need, stamp, key, k1);
      amgk::mis_pull(s, M, bits, 2, key, need, stamp, k1, k2);
      S.zero_counter(0);
      amgk::mis_decide(s, n, key, k2, key_next, S.counters.p);
      std::swap(key, key_next);
      undecided = S.read_counter(0);
      // while most rows are undecided pass 1 covers all rows; afterwards only what the undecided rows will read
      stamp = -1;
      if (undecided > 0 && undecided < n / 2) {
        stamp = ++stamp_base;
        amgk::mis_mark(s, M, bits, key, stamp, need);
      }
      ++S.rounds;
    }
    amgk::root_flags(s, n, key, is_root);
    const int found = (int)S.scan(n, is_root, scan);
    amgk::root_ids(s, n, key, scan, first, agg);
    return found;
  };
  S.zero_counter(0);
  amgk::strength(s, M, ad, kThreshold, flag, key, agg, S.counters.p);
  const int nc = roots(flag, S.read_counter(0), 0);
  amgk::join(s, M, flag, key, 1, agg, other);    // (A) rows next to a root
  amgk::join(s, M, flag, key, 0, other, agg);    // (B) the rest joins its strongest pass-A neighbour
  if (nc > 0) {
    int *count = S.take<int>((size_t)nc);
    NSK_HIP(hipMemsetAsync(count, 0, sizeof(int) * (size_t)nc, s));
    amgk::agg_sizes(s, n, agg, count);
    pw = S.take<double>((size_t)nc);
    amgk::agg_weights(s, nc, count, pw);
  }
  return nc;
}

}  // namespace

int64_t device_product_pattern(Ctx *ctx, const Csr &A, const Csr &B, DBuf<int> &rp, DBuf<int> &col) {
  DBuf<char> no_arena;   // (work arrays come from individual allocations: this runs once per sparsity pattern)
  size_t want = 0;
  Scratch S(ctx, no_arena, want);
  amgk::RowProduct P{};
  P.A = amgk::Mat{A.n_rows, A.n_cols, A.rowptr.p, A.col.p, A.val.p};
  P.B = amgk::Mat{B.n_rows, B.n_cols, B.rowptr.p, B.col.p, B.val.p};
  rp.alloc((size_t)A.n_rows + 1);
  const ProductPlan pl = product_rows(S, P, 0, 0, rp.p);
  col.alloc((size_t)std::max<int64_t>(pl.nnz, 1));
  DBuf<double> val;   // (the kernels form the values too; only the pattern is wanted)
  val.alloc((size_t)std::max<int64_t>(pl.nnz, 1));
  S.zero_counter(1);
  amgk::product_fill(ctx->stream, P, 0, pl.tier, rp.p, col.p, val.p, S.counters.p + 1);
  if (S.read_counter(1) != 0) throw Error(-84, "device_product_pattern: the fill found a row its count had not");
  ctx->sync();
  return pl.nnz;
}

// ---------------------------------------------------------------- test hook (nsk_internal.h: nsk_debug_amg)
namespace {
void dbg_check_mat(const nsk_dbg_amg_mat &M, bool need_val) {
  if (M.n_rows < 1 || M.n_cols < 1 || !M.rowptr || (need_val && !M.val)) throw Error(-61, "nsk_debug_amg: matrix shape");
  if (M.rowptr[0] != 0) throw Error(-58, "nsk_debug_amg: rowptr does not start at 0");
  for (int i = 0; i < M.n_rows; ++i)
    if (M.rowptr[i + 1] < M.rowptr[i]) throw Error(-58, "nsk_debug_amg: rowptr not monotone");
  const int64_t nnz = M.rowptr[M.n_rows];
  if (nnz > 0 && !M.col) throw Error(-61, "nsk_debug_amg: matrix shape");
  for (int64_t k = 0; k < nnz; ++k)
    if (M.col[k] < 0 || M.col[k] >= M.n_cols) throw Error(-59, "nsk_debug_amg: column id out of range");
}
amgk::Mat dbg_put_mat(Guarded &G, const nsk_dbg_amg_mat &M) {
  const size_t nnz = (size_t)M.rowptr[M.n_rows];
  return amgk::Mat{M.n_rows, M.n_cols, G.put(M.rowptr, (size_t)M.n_rows + 1), G.put(M.col, nnz), G.put(M.val, nnz)};
}
// a Csr over arrays it does not own (aggregate() and transpose() take a Csr)
struct BorrowedCsr {
  Csr A;
  BorrowedCsr(const amgk::Mat &M, int64_t nnz) {
    A.n_rows = M.n_rows;
    A.n_cols = A.n_own_cols = M.n_cols;
    A.nnz = nnz;
    A.rowptr.p = const_cast<int *>(M.rp);
    A.col.p = const_cast<int *>(M.col);
    A.val.p = const_cast<double *>(M.val);
    A.present = true;
  }
  ~BorrowedCsr() { A.rowptr.p = nullptr; A.col.p = nullptr; A.val.p = nullptr; }
};
}  // namespace

int debug_amg(Ctx *ctx, const nsk_dbg_amg_args *a, int32_t *info) {
  hipStream_t s = ctx->stream;
  for (int k = 0; k < 16; ++k) info[k] = 0;
  if (!a || !a->out64) throw Error(-61, "nsk_debug_amg: arguments");
  for (int k = 0; k < 8; ++k) a->out64[k] = k >= 4 && k < 7 ? -1 : 0;
  const int op = a->op;
  if (op < NSK_DBG_AMG_SCAN || op > NSK_DBG_AMG_START_VECTOR) throw Error(-65, "nsk_debug_amg: unknown op");
  const bool uses_A = op != NSK_DBG_AMG_SCAN && op != NSK_DBG_AMG_MIS_DECIDE && op != NSK_DBG_AMG_ROOTS &&
                      op != NSK_DBG_AMG_AGG_WEIGHTS && op != NSK_DBG_AMG_START_VECTOR;
  const bool graph = op == NSK_DBG_AMG_MIS_PULL || op == NSK_DBG_AMG_MIS_MARK || op == NSK_DBG_AMG_JOIN;
  if (uses_A) dbg_check_mat(a->A, true);
  const int n = uses_A ? a->A.n_rows : a->n;
  if (n < 0) throw Error(-61, "nsk_debug_amg: n");
  const int64_t nnz = uses_A ? a->A.rowptr[n] : 0;
  const size_t fwords = uses_A ? amgk::flag_words((long)nnz, n) : 0;
  const bool square = op == NSK_DBG_AMG_BLOCK || op == NSK_DBG_AMG_DIAG || op == NSK_DBG_AMG_STRENGTH || graph ||
                      op == NSK_DBG_AMG_AGGREGATE;
  if (square && a->A.n_cols != n) throw Error(-61, "nsk_debug_amg: a square matrix");
  if ((op == NSK_DBG_AMG_STRENGTH || graph) && (a->flag_words != (int64_t)fwords || !(op == NSK_DBG_AMG_STRENGTH ? (const void *)a->flag_out : (const void *)a->flag)))
    throw Error(-61, "nsk_debug_amg: flag words");
  if (graph && !a->key) throw Error(-61, "nsk_debug_amg: key");

  Guarded G(s);
  DBuf<char> no_arena;
  size_t want = 0;
  Scratch S(ctx, no_arena, want);
  S.exact = &G;
  const amgk::Tally t0 = amgk::tally();
  struct Out {
    void *host;
    const void *dev;
    size_t bytes;
  };
  std::vector<Out> outs;
  auto out = [&](auto *host, const auto *dev, size_t count) {
    if (host && count) outs.push_back(Out{(void *)host, (const void *)dev, count * sizeof(*host)});
  };
  auto finish = [&]() {
    for (const Out &o : outs) NSK_HIP(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s));
    ctx->sync();
    NSK_HIP(hipGetLastError());
    info[0] = G.changed();
    const amgk::Tally &t1 = amgk::tally();
    info[5] = (int32_t)(t1.pull1_stamped - t0.pull1_stamped);
    info[6] = (int32_t)(t1.pull1_all - t0.pull1_all);
    info[7] = (int32_t)(t1.pull2 - t0.pull2);
    info[8] = (int32_t)(t1.join[1] - t0.join[1]);
    info[9] = (int32_t)(t1.join[0] - t0.join[0]);
    for (int p = 0; p < 2; ++p)
      for (int t = 0; t < 3; ++t) {
        info[10 + t] += (int32_t)(t1.product[p][t][0] - t0.product[p][t][0]);
        info[13 + t] += (int32_t)(t1.product[p][t][1] - t0.product[p][t][1]);
      }
    info[4] = (info[10] + info[11] + info[12] ? 1 : 0) | (info[13] + info[14] + info[15] ? 2 : 0);
  };

  try {
    switch (op) {
      case NSK_DBG_AMG_SCAN: {
        if (!a->i_in && n > 0) throw Error(-61, "nsk_debug_amg: SCAN input");
        const int *in = G.put(a->i_in, (size_t)n);
        int *o = G.put<int>(nullptr, (size_t)n + 1);
        out(a->i_out, o, (size_t)n + 1);
        out(a->out64, S.total.p, 1);
        (void)S.scan(n, in, o);
        break;
      }
      case NSK_DBG_AMG_BLOCK: {
        const int r0 = a->r0, r1 = a->r1;
        if (r0 < 0 || r1 < r0 || r1 > n) throw Error(-61, "nsk_debug_amg: BLOCK range");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        int *len = S.take<int>((size_t)(r1 - r0) + 1);
        amgk::block_count(s, M, r0, r1, len);
        int *rp = G.put<int>(nullptr, (size_t)(r1 - r0) + 1);
        const int64_t bn = S.scan(r1 - r0, len, rp);
        if (bn > a->out_cap) throw Error(-61, "nsk_debug_amg: out_cap");
        int *col = G.put<int>(nullptr, (size_t)bn);
        double *val = G.put<double>(nullptr, (size_t)bn);
        amgk::block_fill(s, M, r0, r1, rp, col, val);
        a->out64[0] = bn;
        out(a->out_rp, rp, (size_t)(r1 - r0) + 1);
        out(a->out_col, col, (size_t)bn);
        out(a->out_val, val, (size_t)bn);
        break;
      }
      case NSK_DBG_AMG_DIAG: {
        const amgk::Mat M = dbg_put_mat(G, a->A);
        double *ad = G.put<double>(nullptr, (size_t)n), *dinv = G.put<double>(nullptr, (size_t)n);
        amgk::diag(s, M, ad, dinv);
        out(a->d_out, ad, (size_t)n);
        out(a->d_out2, dinv, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_STRENGTH: {
        if (!a->ad) throw Error(-61, "nsk_debug_amg: ad");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        const double *ad = G.put(a->ad, (size_t)n);
        uint16_t *flag = G.put<uint16_t>(nullptr, fwords);
        uint64_t *key = G.put<uint64_t>(nullptr, (size_t)n);
        int *agg = G.put<int>(nullptr, (size_t)n);
        S.zero_counter(0);
        amgk::strength(s, M, ad, a->threshold, flag, key, agg, S.counters.p);
        a->out64[0] = S.read_counter(0);
        out(a->flag_out, flag, fwords);
        out(a->k_out, key, (size_t)n);
        out(a->i_out, agg, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_MIS_PULL: {
        if ((a->pass != 1 && a->pass != 2) || !a->i_in || !a->k_out || (a->pass == 2 && !a->key2))
          throw Error(-61, "nsk_debug_amg: MIS_PULL arguments");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        const uint16_t *flag = G.put(a->flag, fwords);
        const uint64_t *key = G.put(a->key, (size_t)n);
        const int *need = G.put(a->i_in, (size_t)n);
        const uint64_t *in = a->pass == 1 ? key : G.put(a->key2, (size_t)n);   // (pass 1 reads the keys, as the set-up's does)
        uint64_t *o = G.put((const uint64_t *)a->k_out, (size_t)n);
        amgk::mis_pull(s, M, flag, a->pass, key, need, a->stamp, in, o);
        out(a->k_out, o, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_MIS_DECIDE: {
        if (!a->key || !a->key2 || n < 1) throw Error(-61, "nsk_debug_amg: MIS_DECIDE arguments");
        for (int i = 0; i < n; ++i)   // (the row a found key names is read)
          if ((a->key[i] >> 62) == 1 && (int64_t)(a->key2[i] & 0x7fffffffu) >= n) throw Error(-59, "nsk_debug_amg: a key names no row");
        const uint64_t *key = G.put(a->key, (size_t)n), *key2 = G.put(a->key2, (size_t)n);
        uint64_t *o = G.put<uint64_t>(nullptr, (size_t)n);
        S.zero_counter(0);
        amgk::mis_decide(s, n, key, key2, o, S.counters.p);
        a->out64[0] = S.read_counter(0);
        out(a->k_out, o, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_MIS_MARK: {
        if (!a->i_in) throw Error(-61, "nsk_debug_amg: need");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        const uint16_t *flag = G.put(a->flag, fwords);
        const uint64_t *key = G.put(a->key, (size_t)n);
        int *need = G.put(a->i_in, (size_t)n);
        amgk::mis_mark(s, M, flag, key, a->stamp, need);
        out(a->i_out, need, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_ROOTS: {
        if (!a->key || !a->i_in || n < 1) throw Error(-61, "nsk_debug_amg: ROOTS arguments");
        const uint64_t *key = G.put(a->key, (size_t)n);
        int *agg = G.put(a->i_in, (size_t)n);
        int *is_root = S.take<int>((size_t)n), *scan = S.take<int>((size_t)n + 1);
        amgk::root_flags(s, n, key, is_root);
        a->out64[0] = S.scan(n, is_root, scan);
        amgk::root_ids(s, n, key, scan, a->first, agg);
        out(a->i_out, agg, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_JOIN: {
        if (!a->i_in || !a->i_out) throw Error(-61, "nsk_debug_amg: JOIN arguments");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        const uint16_t *flag = G.put(a->flag, fwords);
        const uint64_t *key = G.put(a->key, (size_t)n);
        const int *agg_in = G.put(a->i_in, (size_t)n);
        int *agg_out = G.put((const int *)a->i_out, (size_t)n);
        amgk::join(s, M, flag, key, a->roots_only != 0, agg_in, agg_out);
        out(a->i_out, agg_out, (size_t)n);
        break;
      }
      case NSK_DBG_AMG_AGG_WEIGHTS: {
        const int nc = a->nc;
        if (!a->i_in || n < 1 || nc < 1) throw Error(-61, "nsk_debug_amg: AGG_WEIGHTS arguments");
        for (int i = 0; i < n; ++i)
          if (a->i_in[i] >= nc) throw Error(-59, "nsk_debug_amg: aggregate id out of range");
        const int *agg = G.put(a->i_in, (size_t)n);
        int *count = G.put<int>(nullptr, (size_t)nc);
        NSK_HIP(hipMemsetAsync(count, 0, sizeof(int) * (size_t)nc, s));
        amgk::agg_sizes(s, n, agg, count);
        double *pw = G.put<double>(nullptr, (size_t)nc);
        amgk::agg_weights(s, nc, count, pw);
        out(a->i_out, count, (size_t)nc);
        out(a->d_out, pw, (size_t)nc);
        break;
      }
      case NSK_DBG_AMG_AGGREGATE: {
        if (!a->ad) throw Error(-61, "nsk_debug_amg: ad");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        BorrowedCsr A(M, nnz);
        const double *ad = G.put(a->ad, (size_t)n);
        int *agg = nullptr;
        double *pw = nullptr;
        const int nc = aggregate(S, A.A, ad, agg, pw);
        a->out64[0] = nc;
        a->out64[1] = S.rounds;
        a->out64[2] = amgk::tally().pull1_stamped - t0.pull1_stamped;
        out(a->i_out, agg, (size_t)n);
        if (nc > 0) out(a->d_out, pw, (size_t)nc);
        break;
      }
      case NSK_DBG_AMG_PRODUCT:
      case NSK_DBG_AMG_PRODUCT_COUNT: {
        const int product = a->product, ft = a->first_tier;
        if (product < 0 || product > 1 || ft < 0 || ft > 2) throw Error(-61, "nsk_debug_amg: product or tier");
        amgk::RowProduct P{};
        if (product == 0) {
          dbg_check_mat(a->B, true);
          if (a->B.n_rows != a->A.n_cols) throw Error(-61, "nsk_debug_amg: shapes of A and B");
          P.A = dbg_put_mat(G, a->A);
          P.B = dbg_put_mat(G, a->B);
        } else {
          const int nc = a->nc;
          if (a->A.n_cols != n || nc < 1 || !a->i_in || !a->pw || !a->dinv) throw Error(-61, "nsk_debug_amg: prolongator arguments");
          for (int i = 0; i < n; ++i)
            if (a->i_in[i] >= nc) throw Error(-59, "nsk_debug_amg: aggregate id out of range");
          P.A = dbg_put_mat(G, a->A);
          P.agg = G.put(a->i_in, (size_t)n);
          P.pw = G.put(a->pw, (size_t)nc);
          P.dinv = G.put(a->dinv, (size_t)n);
          P.c = a->c;
        }
        info[1] = product;
        if (op == NSK_DBG_AMG_PRODUCT_COUNT) {
          int *len = G.put<int>(nullptr, (size_t)n + 1);
          S.zero_counter(1);
          amgk::product_count(s, P, product, ft, len, S.counters.p + 1);
          a->out64[0] = S.read_counter(1);
          out(a->i_out, len, (size_t)n);
          info[2] = ft == 0 ? 8 : ft == 1 ? 16 : 64;
          info[3] = ft == 0 ? 64 : ft == 1 ? 128 : 512;
          break;
        }
        for (int t = ft; t <= 2; ++t) {   // the error word of every tier, each from a count of its own
          int *len = G.put<int>(nullptr, (size_t)n + 1);
          S.zero_counter(1);
          amgk::product_count(s, P, product, t, len, S.counters.p + 1);
          a->out64[4 + t] = S.read_counter(1);
        }
        int *rp = G.put<int>(nullptr, (size_t)n + 1);
        const ProductPlan pl = product_rows(S, P, product, ft, rp);
        a->out64[0] = pl.nnz;
        a->out64[1] = pl.tier;
        if (pl.nnz > a->out_cap) throw Error(-61, "nsk_debug_amg: out_cap");
        int *col = G.put<int>(nullptr, (size_t)pl.nnz);
        double *val = G.put<double>(nullptr, (size_t)pl.nnz);
        S.zero_counter(1);
        amgk::product_fill(s, P, product, pl.tier, rp, col, val, S.counters.p + 1);
        a->out64[2] = S.read_counter(1);
        info[2] = pl.tier == 0 ? 8 : pl.tier == 1 ? 16 : 64;
        info[3] = pl.tier == 0 ? 64 : pl.tier == 1 ? 128 : 512;
        out(a->out_rp, rp, (size_t)n + 1);
        out(a->out_col, col, (size_t)pl.nnz);
        out(a->out_val, val, (size_t)pl.nnz);
        if (a->out64[2] != 0) throw Error(-84, "AMG set-up: the fill of a row product found a row its count had not");
        break;
      }
      case NSK_DBG_AMG_TRANSPOSE: {
        const amgk::Mat M = dbg_put_mat(G, a->A);
        BorrowedCsr A(M, nnz);
        if (nnz > a->out_cap) throw Error(-61, "nsk_debug_amg: out_cap");
        Csr T;
        transpose(S, A.A, T);
        a->out64[0] = T.nnz;
        // (the result leaves the device here: T is gone when finish() runs)
        if (a->out_rp) NSK_HIP(hipMemcpyAsync(a->out_rp, T.rowptr.p, sizeof(int) * ((size_t)T.n_rows + 1), hipMemcpyDeviceToHost, s));
        if (a->out_col && T.nnz) NSK_HIP(hipMemcpyAsync(a->out_col, T.col.p, sizeof(int) * (size_t)T.nnz, hipMemcpyDeviceToHost, s));
        if (a->out_val && T.nnz) NSK_HIP(hipMemcpyAsync(a->out_val, T.val.p, sizeof(double) * (size_t)T.nnz, hipMemcpyDeviceToHost, s));
        ctx->sync();
        break;
      }
      case NSK_DBG_AMG_ROWS_SORT: {
        if (nnz > a->out_cap) throw Error(-61, "nsk_debug_amg: out_cap");
        const amgk::Mat M = dbg_put_mat(G, a->A);
        int *col = G.put<int>(nullptr, (size_t)nnz);
        double *val = G.put<double>(nullptr, (size_t)nnz);
        amgk::rows_sort(s, n, M.rp, M.col, M.val, col, val);
        out(a->out_col, col, (size_t)nnz);
        out(a->out_val, val, (size_t)nnz);
        break;
      }
      case NSK_DBG_AMG_START_VECTOR: {
        double *x = G.put<double>(nullptr, (size_t)n);
        amgk::start_vector(s, n, x);
        out(a->d_out, x, (size_t)n);
        break;
      }
    }
  } catch (const Error &e) {
    if (e.code == -61 || e.code == -58 || e.code == -59) throw;   // (refused on the host: nothing ran)
    finish();   // what the operation left behind still comes back: the 64-bit total of a scan, the guard words
    throw;
  }
  finish();
  return 0;
}

// lambda = kEigBoost x ||(D^-1 A)^k x0|| / ||(D^-1 A)^(k-1) x0|| after kEigIts steps, x0(i) = start_entry(i), on the device
double Amg::estimate_lambda_device(AmgLevel &L) {
  const int n = L.n;
  hipStream_t st = ctx->stream;
  const int sl = ctx->alloc_slots(2);
  amgk::start_vector(st, n, L.r.p);
  vec_dot(st, ctx->ws, n, L.r.p, L.r.p, ctx->slot(sl), 1);
  vec_scale(st, n, sref(1.0, nullptr, ctx->slot(sl + 1)), L.r.p);            // (n > 0: entry 0 of the start vector is -0.5)
  for (int it = 0; it < kEigIts; ++it) {
    mv(*L.A, L.r.p, L.w.p);
    vec_mul(st, n, L.dinv.p, L.w.p);                                         // y = D^-1 A x
    vec_dot(st, ctx->ws, n, L.w.p, L.w.p, ctx->slot(sl), 1);                  // rank-local: no all-reduce
    vec_equ(st, n, sref(1.0, nullptr, ctx->slot(sl + 1)), L.w.p, L.r.p);      // x = y / ||y||
  }
  const double lam = ctx->read_slots(sl + 1, 1)[0];
  ctx->slot_top = sl;
  return kEigBoost * lam;
}

// The hierarchy under one level-0 operator that is already on the device with its SpMV plan (the caller's block itself,
// or the diagonal sub-block of a shard).
void Amg::build(AmgHierarchy &H, Csr *A0, std::unique_ptr<Csr> own0) {
  hipStream_t s = ctx->stream;
  const bool timing = std::getenv("NSK_AMG_TIMING") != nullptr;   // phase times of the set-up on stderr
  double tp = now_ms();
  auto lap = [&](int l, const char *what) {
    if (!timing) return;
    ctx->sync();
    const double t = now_ms();
    std::fprintf(stderr, "amg set-up: level %d %-22s %9.2f ms\n", l, what, t - tp);
    tp = t;
  };
  Scratch S(ctx, arena, arena_want);
  std::unique_ptr<Csr> next = std::move(own0);   // the operator the next level owns
  Csr *cur = A0;
  for (int l = 0;; ++l) {
    auto L = std::make_unique<AmgLevel>();
    if (next) { L->own_A = std::move(*next); next.reset(); cur = &L->own_A; }
    L->A = cur;
    const Csr &A = *cur;
    const int n = A.n_rows;
    L->n = n;
    double *ad = S.take<double>((size_t)n);
    L->dinv.alloc((size_t)n);
    if (one_sign_diag) S.zero_counter(2);
    amgk::diag(s, mat(A), ad, L->dinv.p, one_sign_diag ? reinterpret_cast<unsigned *>(S.counters.p + 2) : nullptr);
    if (one_sign_diag) {
      const int signs = S.read_counter(2);   // 1: all positive, 2: all negative
      if (signs != 1 && signs != 2)
        throw Error(-85, "AMG set-up: the diagonal of level " + std::to_string(l) + " holds " +
                             ((signs & 4) ? "a zero (or a row lists none)" : "both signs"));
    }
    L->r.alloc((size_t)n);
    L->w.alloc((size_t)n);
    // (level 0 on 2 x 2 node blocks under fused_cheby: the fused smoother steps need a second iterate)
    if (l == 0 && fused_cheby && use_bsr && A.blk_ok && A.blk_R == 2 && A.blk_C == 2 && (blk_residual || value_bits == 32))
      L->x2.alloc((size_t)n);
    lap(l, "diagonal");
    L->lam = estimate_lambda_device(*L);
    if (!(L->lam > 0.0) || !std::isfinite(L->lam))
      throw Error(-83, "AMG set-up: the power iteration on level " + std::to_string(l) + " did not give a finite eigenvalue estimate");
    lap(l, "lambda (power its)");
    if (l > 0) { L->x.alloc((size_t)n); L->b.alloc((size_t)n); }
    int nc = 0;
    int *agg = nullptr;
    double *pw = nullptr;
    if (n > kCoarseMax && l + 1 < kMaxLevels) nc = aggregate(S, A, ad, agg, pw);
    lap(l, "aggregation");
    if (timing) std::fprintf(stderr, "amg set-up: level %d %d aggregates after %d independent-set rounds (all levels so far)\n", l, nc, S.rounds);
    if (nc <= 0 || nc >= n) {
      if (n <= kDenseLimit) {   // the coarsest operator goes to the host once, its inverse comes back
        std::vector<int> rp((size_t)n + 1), col((size_t)A.nnz);
        std::vector<double> val((size_t)A.nnz);
        NSK_HIP(hipMemcpyAsync(rp.data(), A.rowptr.p, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
        NSK_HIP(hipMemcpyAsync(col.data(), A.col.p, sizeof(int) * (size_t)A.nnz, hipMemcpyDeviceToHost, s));
        NSK_HIP(hipMemcpyAsync(val.data(), A.val.p, sizeof(double) * (size_t)A.nnz, hipMemcpyDeviceToHost, s));
        ctx->sync();
        L->inv.upload(dense_inverse(n, rp, col, val), s);
      }
      ctx->sync();
      S.end_level();
      H.lev.push_back(std::move(L));
      break;
    }
    amgk::RowProduct pp{mat(A), amgk::Mat{}, agg, pw, L->dinv.p, kOmega / L->lam};
    row_product(S, pp, 1, nc, 1, L->P);   // (16 lanes: the row's terms, up to 98 on the Q3 block, are staged in LDS)
    lap(l, "smoothed prolongator");
    transpose(S, L->P, L->R);
    lap(l, "transpose");
    const amgk::Mat AP = row_product_scratch(S, amgk::RowProduct{mat(A), mat(L->P), nullptr, nullptr, nullptr, 0.0}, 0, nc, 0);
    lap(l, "A P");
    next = std::make_unique<Csr>();
    row_product(S, amgk::RowProduct{mat(L->R), AP, nullptr, nullptr, nullptr, 0.0}, 0, nc, 1, *next);   // (a coarse row: some 40 columns and more)
    lap(l, "R (A P)");
    L->has_coarse = true;
    ctx->sync();
    S.end_level();
    if (value_bits == 32) to_f32(*L, l);
    H.lev.push_back(std::move(L));
  }
  // (the last level: its operator is multiplied only where it is too large for a dense inverse)
  if (value_bits == 32 && !H.lev.back()->inv.p) to_f32(*H.lev.back(), (int)H.lev.size() - 1);
}

void Amg::check_overflow(Csr &M, int level, const char *which) {
  unsigned over = 0;
  NSK_HIP(hipMemcpyAsync(&over, M.f32_overflow.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  ctx->sync();
  if (over)
    throw Error(-48, "NSK_OPT_AMG_PRECISION = 32: " + std::to_string(over) + " value(s) of level " + std::to_string(level) +
                         "'s " + which + " are finite in fp64 but outside the range of fp32");
}

// The set-up is done with the level: nothing reads the double values of its operators any more (they are kept: the test
// hook downloads them).  An operator without a stream plan keeps the CSR-vector kernel on its double values.
void Amg::to_f32(AmgLevel &L, int level) {
  struct Item { Csr *M; const char *which; };
  const Item items[3] = {{L.A == &L.own_A ? &L.own_A : nullptr, "A"}, {L.has_coarse ? &L.P : nullptr, "P"}, {L.has_coarse ? &L.R : nullptr, "R"}};
  for (const Item &it : items)
    if (it.M && it.M->stream_ok) { it.M->amg32 = 2; it.M->refresh_f32(ctx->stream, true); }
  for (const Item &it : items)
    if (it.M && it.M->amg32) check_overflow(*it.M, level, it.which);
}

void Amg::setup(Ctx *c, Csr &F, const std::vector<int> &shard_off) {
  ctx = c;
  const double t0 = now_ms();
  clear();
  built_bits = value_bits;
  F.amg32 = 0;   // (the set-up multiplies by the double values; a copy left by the last hierarchy stays allocated meanwhile)
  if (F.n_rows <= 0) return;
  try {
    build_all(F, shard_off);
  } catch (...) {   // (-48 from any level's conversion among them: no copy of F stays behind that nobody names)
    F.amg32 = 0;
    F.drop_unused_f32();
    throw;
  }
  F.drop_unused_f32();
  ctx->sync();
  for (long &c : form_launches) c = 0;   // (the set-up's own products are not the cycle's)
  setup_host_ms = now_ms() - t0;
  if (std::getenv("NSK_AMG_TIMING")) std::fprintf(stderr, "amg set-up: total %.1f ms\n", setup_host_ms);
}

void Amg::build_all(Csr &F, const std::vector<int> &shard_off) {
  std::vector<int> off = shard_off;
  if (off.size() < 2) off = {0, F.n_rows};
  const bool single_full = off.size() == 2 && F.n_cols == F.n_own_cols && F.n_cols == F.n_rows;
  shards.resize(off.size() - 1);
  if (arena.n < arena_want) arena.alloc(arena_want + arena_want / 16);
  for (size_t sidx = 0; sidx + 1 < off.size(); ++sidx) {
    const int r0 = off[sidx], r1 = off[sidx + 1];
    shards[sidx].offset = r0;
    if (single_full) {
      build(shards[sidx], &F, nullptr);
      level0 = &F;
      continue;
    }
    // the shard's diagonal block as a matrix of its own (ghost columns and other shards' columns dropped)
    Scratch S(ctx, arena, arena_want);
    auto B = std::make_unique<Csr>();
    const amgk::Mat M{F.n_rows, F.n_cols, F.rowptr.p, F.col.p, F.val.p};
    int *len = S.take<int>((size_t)(r1 - r0) + 1);
    amgk::block_count(ctx->stream, M, r0, r1, len);
    B->rowptr.alloc((size_t)(r1 - r0) + 1);
    const int64_t nnz = S.scan(r1 - r0, len, B->rowptr.p);
    B->col.alloc((size_t)std::max<int64_t>(nnz, 1));
    B->val.alloc((size_t)std::max<int64_t>(nnz, 1));
    amgk::block_fill(ctx->stream, M, r0, r1, B->rowptr.p, B->col.p, B->val.p);
    finish_csr(ctx, *B, r1 - r0, r1 - r0, nnz);
    S.end_level();
    build(shards[sidx], nullptr, std::move(B));
  }
  if (level0 && value_bits == 32) {
    // Level 0 is the caller's block: the cycle reads its 2 x 2 fp32 copy, the one the inner solves read under
    // NSK_OPT_INNER_MATRIX_PRECISION = 32 (whichever of the two wants it first converts it), or its scalar fp32 values
    // where it has no such copy.  Named only now: the set-up above multiplied by the double values.
    const bool blk22 = use_bsr && F.blk_ok && F.blk_R == 2 && F.blk_C == 2;
    F.amg32 = blk22 ? 1 : F.stream_ok ? 2 : 0;
    if (F.amg32 && !F.f32_current()) {
      F.refresh_f32(ctx->stream, true);
      check_overflow(F, 0, "A");
    }
  }
}

void Amg::mv(Csr &A, const double *x, double *y, int mode, const double *z) {
  // (no ghost tail; 16-bit offsets only where level 0 is the caller's S, which carries them: y = A x and y = z - A x, both
  // with a kernel in either precision; the rule: amg_spmv_form, nsk_core.hpp)
  const SpmvForm f = form_of(A, mode, all_aligned16(x, y, z));
  if (is_f32(f)) {
    // the caller's block: values written since the conversion, or vectors off the pair alignment for the first time
    if (f == SpmvForm::stream_f32 && !(A.amg32 & 2)) { A.amg32 |= 2; A.val32_version = -1; }
    if (A.val32_version != A.values_version) A.refresh_f32(ctx->stream, false);   // (stream-ordered: no host sync)
  }
  A.spmv_launch(ctx->stream, f, x, nullptr, y, mode, z);
  ++form_launches[(int)f];
  ++ctx->st.spmv_calls;
  ctx->st.spmv_bytes += (double)A.spmv_bytes() + (mode ? 8.0 * A.n_rows : 0.0);
}

// degree-2 Chebyshev polynomial in D^-1 A on [lam / alpha, lam]
void Amg::cheby(AmgLevel &L, const double *b, double *x, bool zero_init) {
  hipStream_t s = ctx->stream;
  const double lmax = L.lam, lmin = lmax / kChebyAlpha;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  const double rho = 1.0 / sigma;
  if (zero_init) vec_cheby_step(s, L.n, 0.0, 1.0 / theta, L.dinv.p, b, L.w.p, x, 1);
  else {
    mv(*L.A, x, L.r.p, 2, b);  // r = b - A x
    vec_cheby_step(s, L.n, 0.0, 1.0 / theta, L.dinv.p, L.r.p, L.w.p, x, 0);
  }
  const double rho_new = 1.0 / (2.0 * sigma - rho);
  mv(*L.A, x, L.r.p, 2, b);
  vec_cheby_step(s, L.n, rho_new * rho, 2.0 * rho_new / delta, L.dinv.p, L.r.p, L.w.p, x, 0);
}

// Level 0 on 2 x 2 node blocks under fused_cheby: whether this call's smoothers run their steps in the
// epilogue of the residual products.  Coarse levels, shard copies (no node blocks), forms without node blocks and
// vectors off the pair alignment keep the two-launch steps.
bool Amg::fusable(const AmgLevel &L, const double *b, const double *x) const {
  if (!fused_cheby || !L.x2.p || !L.has_coarse) return false;
  return is_blk(fused_form(L, b, x));
}

// the form of a fused step on these vectors: every vector the kernel moves as pairs enters the rule's alignment argument
SpmvForm Amg::fused_form(const AmgLevel &L, const double *b, const double *x) const {
  return form_of(*L.A, 2, all_aligned16(b, x, L.x2.p, L.w.p, L.dinv.p));
}

void Amg::fused_step(AmgLevel &L, SpmvForm f, const double *x_in, double *x_out, const double *b, double c1, double c2) {
  Csr &A = *L.A;
  if (is_f32(f) && A.val32_version != A.values_version) A.refresh_f32(ctx->stream, false);   // (as Amg::mv)
  if (A.cheby_launch(ctx->stream, f, x_in, nullptr, x_out, b, L.dinv.p, L.w.p, c1, c2) != 0)
    throw Error(-1, "AMG: the fused Chebyshev step was refused (x_out == x_in, or a vector off the 16-byte alignment)");
  ++form_launches[(int)f];
  ++fused_launches;
  ++ctx->st.spmv_calls;
  // the product's bytes (its y is x_out, its gather x_in) + b + dinv + w read and written
  ctx->st.spmv_bytes += (double)A.spmv_bytes() + 32.0 * A.n_rows;
}

// cheby() with every step that follows a residual fused into it: the same arithmetic in the same order (cheby_w is the
// one update of both), so the same bits.  A fused step cannot run in place; the iterate alternates between x and L.x2 and
// ends in x: zero guess -> x2 -> x, and x -> x2 -> x.
void Amg::cheby_fused(AmgLevel &L, const double *b, double *x, bool zero_init) {
  const double lmax = L.lam, lmin = lmax / kChebyAlpha;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
  const double rho = 1.0 / sigma;
  const SpmvForm f = fused_form(L, b, x);
  if (zero_init) vec_cheby_step(ctx->stream, L.n, 0.0, 1.0 / theta, L.dinv.p, b, L.w.p, L.x2.p, 1);
  else fused_step(L, f, x, L.x2.p, b, 0.0, 1.0 / theta);
  const double rho_new = 1.0 / (2.0 * sigma - rho);
  fused_step(L, f, L.x2.p, x, b, rho_new * rho, 2.0 * rho_new / delta);
}

void Amg::vcycle(AmgHierarchy &H, int l, const double *b, double *x) {
  AmgLevel &L = *H.lev[l];
  if (!L.has_coarse) {
    if (L.inv.p) dense_mv(ctx->stream, L.n, L.inv.p, b, x);
    else { cheby(L, b, x, true); cheby(L, b, x, false); }
    return;
  }
  AmgLevel &C = *H.lev[l + 1];
  const bool fused = l == 0 && fusable(L, b, x);
  if (fused) cheby_fused(L, b, x, true);
  else cheby(L, b, x, true);
  mv(*L.A, x, L.r.p, 2, b);
  mv(L.R, L.r.p, C.b.p);
  vcycle(H, l + 1, C.b.p, C.x.p);
  mv(L.P, C.x.p, x, 1);  // x += P x_c
  if (fused) cheby_fused(L, b, x, false);
  else cheby(L, b, x, false);
}

void Amg::apply(const double *b, double *x) {
  for (AmgHierarchy &H : shards) vcycle(H, 0, b + H.offset, x + H.offset);
}

double Amg::smoother_bytes(const AmgLevel &L, double a) const {
  const double n8 = 8.0 * L.n;
  // two launches per step: four residuals (+ z) and four Chebyshev updates of 5 vector streams each
  if (!(fused_cheby && L.x2.p && is_blk(form_of(*L.A, 2, true)))) return 4 * (a + n8) + n8 * 5 * 4;
  // fused steps: the zero-guess update, the restricted residual, and three products that also stream b, dinv
  // and w read and written (r is never stored; the c1 = 0 step does not read w and is counted as if it did)
  return n8 * 5 + (a + n8) + 3 * (a + 4 * n8);
}

size_t Amg::apply_bytes() const {
  size_t by = 0;
  for (const AmgHierarchy &H : shards)
    for (const auto &L : H.lev) {
      // pre-smoother 1 SpMV (zero guess), residual 1, post-smoother 2; restriction, prolongation (+ 8 n for the add);
      // four Chebyshev updates of 5 vector streams each (fewer streams where the steps are fused: smoother_bytes)
      if (L->has_coarse) by += (size_t)smoother_bytes(*L, (double)L->A->spmv_bytes()) + L->P.spmv_bytes() + 8 * (size_t)L->n +
                               L->R.spmv_bytes();
      else if (L->inv.p) by += (size_t)L->n * L->n * 8;
      else by += 3 * (L->A->spmv_bytes() + 8 * (size_t)L->n) + (size_t)L->n * 8 * 5 * 4;
    }
  return by;
}

double Amg::format_bytes(int shard, int level) const {
  double by = 0;
  for (size_t sh = 0; sh < shards.size(); ++sh) {
    if (shard >= 0 && (int)sh != shard) continue;
    const AmgHierarchy &H = shards[sh];
    for (size_t l = 0; l < H.lev.size(); ++l) {
      if (level >= 0 && (int)l != level) continue;
      const AmgLevel &L = *H.lev[l];
      const double n8 = 8.0 * L.n;
      // (the forms of aligned vectors: what the cycle takes on the library's own)
      const double a = L.A->format_bytes(form_of(*L.A, 2, true)) + n8;
      if (L.has_coarse) by += smoother_bytes(L, a - n8) + L.P.format_bytes(form_of(L.P, 1, true)) + n8 + L.R.format_bytes(form_of(L.R, 0, true));
      else if (L.inv.p) by += (double)L.n * L.n * 8;
      else by += 3 * a + n8 * 5 * 4;
    }
  }
  return by;
}

int64_t Amg::debug_level(int shard, int level, int which, int32_t *rowptr, int32_t *col, double *val, double *dio) {
  if (shard < 0 || shard >= (int)shards.size() || level < 0 || level >= n_levels(shard)) throw Error(-61, "nsk_debug_amg_level: shard or level");
  AmgLevel &L = *shards[shard].lev[level];
  if (which == 3) return L.inv.p ? 1 : 0;
  if (which < 0 || which > 3 || (which != 0 && !L.has_coarse)) throw Error(-61, "nsk_debug_amg_level: the level has no such operator");
  const Csr &M = which == 0 ? *L.A : which == 1 ? L.P : L.R;
  hipStream_t s = ctx->stream;
  if (rowptr) NSK_HIP(hipMemcpyAsync(rowptr, M.rowptr.p, sizeof(int) * ((size_t)M.n_rows + 1), hipMemcpyDeviceToHost, s));
  if (col && M.nnz) NSK_HIP(hipMemcpyAsync(col, M.col.p, sizeof(int) * (size_t)M.nnz, hipMemcpyDeviceToHost, s));
  if (val && M.nnz) NSK_HIP(hipMemcpyAsync(val, M.val.p, sizeof(double) * (size_t)M.nnz, hipMemcpyDeviceToHost, s));
  if (dio && which == 0) {
    if (L.inv.p) NSK_HIP(hipMemcpyAsync(dio, L.inv.p, sizeof(double) * (size_t)L.n * L.n, hipMemcpyDeviceToHost, s));
    else NSK_HIP(hipMemcpyAsync(dio, L.dinv.p, sizeof(double) * (size_t)L.n, hipMemcpyDeviceToHost, s));
  }
  ctx->sync();
  return M.nnz;
}

}  // namespace nsk
