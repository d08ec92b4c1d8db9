// nsk_debug.cpp — the test hooks and diagnostics of nsk_internal.h, in that header's order.  Each runs ONE kernel or one
// set-up function through the entry points the library itself calls; none is part of the public ABI.
#include <algorithm>
#include <cstring>

#include "nsk_handle.hpp"
#include "nsk_internal.h"

namespace {
// set-up kernels on positions shifted by `base` (nsk_debug_ilu0_at_offset, nsk_debug_schur_at_offset)
std::vector<int> shifted(const int32_t *p, size_t n, int64_t base) {
  std::vector<int> v(n);
  for (size_t i = 0; i < n; ++i) {
    const int64_t q = (int64_t)p[i] + base;
    if (q < 0 || q > INT32_MAX) throw Error(-62, "position beyond int32");
    v[i] = (int)q;
  }
  return v;
}
DBuf<int> on_device(const int *h, size_t n) {
  DBuf<int> d;
  d.upload(h, n, nullptr);
  return d;
}
DBuf<double> on_device(const double *h, size_t n) {
  DBuf<double> d;
  d.upload(h, n, nullptr);
  return d;
}

// A device vector of T (double, float) in an allocation of its own: `front` guard words before it and `back` behind it,
// every bit of them set.  How many, each hook's description in nsk_internal.h says
constexpr int kDbgFront = 2, kDbgBack = 4;   // nsk_debug_spmv, nsk_debug_tri: 16 bytes in front (the alignment stays)
template <typename T>
struct DbgVec {
  DBuf<T> buf;
  T *p = nullptr;
  size_t len = 0, off = 0;
  void put(const T *h, size_t n, size_t front, size_t back, hipStream_t st) {
    len = n;
    off = front;
    buf.alloc(len + front + back);
    NSK_HIP(hipMemsetAsync(buf.p, 0xFF, sizeof(T) * buf.n, st));
    p = buf.p + off;
    if (len) NSK_HIP(hipMemcpyAsync(p, h, sizeof(T) * len, hipMemcpyHostToDevice, st));
  }
  // guard words that changed; out (may be null) receives the vector
  int fetch(T *out, Ctx &c) {
    if (!buf.p) return 0;
    std::vector<T> all(buf.n);
    NSK_HIP(hipMemcpyAsync(all.data(), buf.p, sizeof(T) * all.size(), hipMemcpyDeviceToHost, c.stream));
    c.sync();
    if (out) std::copy(all.begin() + off, all.begin() + off + len, out);
    T ones;
    memset(&ones, 0xFF, sizeof(T));
    int bad = 0;
    for (size_t i = 0; i < all.size(); ++i) {
      if (i == off) i += len;
      if (i < all.size()) bad += memcmp(&all[i], &ones, sizeof(T)) != 0;
    }
    return bad;
  }
};

// what nsk_set_block_csr does with a block, on a Csr of the hook's own
void dbg_fill_csr(Csr &A, const nsk_dbg_spmv_mat &M, hipStream_t st) {
  if (M.n_rows < 1 || M.n_cols < 0 || M.n_own_cols < 0 || M.n_own_cols > M.n_cols || M.rowptr[0] != 0)
    throw Error(-61, "nsk_debug_spmv: matrix shape");
  for (int i = 0; i < M.n_rows; ++i)
    if (M.rowptr[i + 1] < M.rowptr[i]) throw Error(-58, "nsk_debug_spmv: rowptr not monotone");
  const int64_t nnz = M.rowptr[M.n_rows];
  for (int64_t k = 0; k < nnz; ++k)
    if (M.col[k] < 0 || M.col[k] >= M.n_cols) throw Error(-59, "nsk_debug_spmv: column id out of range");
  A.n_rows = M.n_rows;
  A.n_cols = M.n_cols;
  A.n_own_cols = M.n_own_cols;
  A.nnz = nnz;
  A.h_rowptr.assign(M.rowptr, M.rowptr + M.n_rows + 1);
  A.h_col.assign(M.col, M.col + nnz);
  A.rowptr.upload(M.rowptr, (size_t)M.n_rows + 1, st);
  A.col.upload(M.col, (size_t)nnz, st);
  A.val.upload(M.val, (size_t)nnz, st);
  ++A.values_version;
  A.lpr = pick_lpr(nnz, M.n_rows);
  A.present = true;
  A.build_stream_plan(st);
}
}  // namespace

extern "C" {

// diagnostics (nsk_internal.h): one apply of a scalar triangular preconditioner with in-kernel time stamps
int nsk_debug_tri_trace(nsk_handle h, int which, int64_t *out16, int max_runs, int *grid) {
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  TriSolve *T = which == NSK_TRI_VELOCITY ? &h->tF : h->tP;
  if (!T) return 0;                                   // (the pressure slot under NSK_OPT_SCHUR_AMG: no triangular factor)
  if (!(T->stream_ready && T->sync_free)) return 0;   // only the scalar single-launch kernels carry the stamps
  const int n_wg = T->n_Lsf + T->n_Usf;
  VecPool &p = which == NSK_TRI_VELOCITY ? h->pool_u : h->pool_p;
  const Lease bv(p, true), xv(p, true);
  vec_set(h->s(), p.n, bv, 1.0);
  T->apply(bv, xv);   // warm
  DBuf<long long> dbg;
  dbg.alloc((size_t)n_wg * 16);
  NSK_HIP(hipMemsetAsync(dbg.p, 0, sizeof(long long) * dbg.n, h->s()));
  T->sf_dbg = dbg.p;
  T->apply(bv, xv);
  T->sf_dbg = nullptr;
  const int n = std::min(max_runs, n_wg);
  NSK_HIP(hipMemcpyAsync(out16, dbg.p, sizeof(long long) * (size_t)n * 16, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  if (grid) *grid = -T->n_Lsf;
  h->check_sync_free();
  return n_wg;
  NSK_CATCH(h)
}

int nsk_local_group_id_mode(int nranks, int on_stream, void *out128) {   // nsk_internal.h
  if (nranks < 1 || !out128) return -1;
  make_local_group(nranks, out128, on_stream);
  return 0;
}

int nsk_abort_local_group(const void *uid128) { return abort_local_group(uid128); }   // nsk_internal.h

// Host-only (no handle, no GPU): the ordering TriSolve::analyze would choose for this pattern.  nsk_internal.h
int nsk_debug_tri_ordering(int n, const int32_t *rowptr, const int32_t *col, int n_sub, const int32_t *sub_off,
                           int want_block2, const double *xy, int group, int32_t *perm_out, int32_t *info4,
                           uint8_t *chain_out) {
  try {
    std::vector<int> off;
    if (n_sub > 1 && sub_off) off.assign(sub_off, sub_off + n_sub + 1);
    TriOrdering O;
    O.build(n, rowptr, col, ORDER_MULTICOLOR, off, want_block2 != 0, xy, group);
    for (int i = 0; i < n; ++i) perm_out[i] = O.perm[i];
    info4[0] = O.n_colors;
    info4[1] = O.gmax;
    info4[2] = O.block2 ? 1 : 0;
    info4[3] = (int)O.cpos.size();
    if (chain_out)
      for (size_t i = 0; i < O.cpos.size(); ++i) chain_out[i] = (uint8_t)(O.cpos[i] | (O.clen[i] << 4));
    return 0;
  } catch (const std::exception &) {
    return -1;
  }
}

int nsk_debug_ilu0_at_offset(int what, int n, const int32_t *rowptr, const int32_t *col, double *val_inout, int64_t base) {
  try {
    const int nnz = rowptr[n];
    std::vector<int> diag((size_t)n, -1), rows((size_t)n), lvl((size_t)n + 1);
    int max_row = 1;
    for (int i = 0; i < n; ++i) {
      rows[i] = i;
      lvl[i] = i;
      max_row = std::max(max_row, rowptr[i + 1] - rowptr[i]);
      for (int k = rowptr[i]; k < rowptr[i + 1]; ++k) if (col[k] == i) diag[i] = k;
      if (diag[i] < 0) throw Error(-62, "row without a diagonal");
    }
    lvl[n] = n;
    const std::vector<int> rp = shifted(rowptr, (size_t)n + 1, base), dg = shifted(diag.data(), (size_t)n, base);
    DBuf<int> d_rp = on_device(rp.data(), rp.size()), d_dg = on_device(dg.data(), dg.size()), d_col = on_device(col, (size_t)nnz),
              d_rows = on_device(rows.data(), rows.size()), d_lvl = on_device(lvl.data(), lvl.size());
    DBuf<double> d_val = on_device(val_inout, (size_t)nnz);
    NSK_HIP(hipDeviceSynchronize());
    const int *colb = d_col.p - base;   // entry `base + k` of these is entry k of the arrays that exist
    double *valb = d_val.p - base;
    if (what == 0)
      for (int i = 0; i < n; ++i) ilu0_factor_level(nullptr, 1, d_rows.p + i, d_rp.p, d_dg.p, colb, valb, max_row);
    else
      ilu0_factor_serial(nullptr, d_lvl.p, d_rows.p, 0, n, d_rp.p, d_dg.p, colb, valb, max_row);
    NSK_HIP(hipMemcpy(val_inout, d_val.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
    return 0;
  } catch (const std::exception &) {
    return -1;
  }
}

int nsk_debug_schur_at_offset(int n_p, int n_u, const int32_t *b_rp, const int32_t *b_col, const double *b_val,
                              const double *dinv, const int32_t *bt_rp, const int32_t *bt_col, const double *bt_val,
                              const int32_t *s_rp, const int32_t *s_col, double *s_val_out, int64_t base) {
  try {
    const int nb = b_rp[n_p], nbt = bt_rp[n_u], ns = s_rp[n_p];
    int max_row = 1;
    for (int i = 0; i < n_p; ++i) max_row = std::max(max_row, s_rp[i + 1] - s_rp[i]);
    const std::vector<int> brp = shifted(b_rp, (size_t)n_p + 1, base), btrp = shifted(bt_rp, (size_t)n_u + 1, base),
                           srp = shifted(s_rp, (size_t)n_p + 1, base);
    DBuf<int> d_brp = on_device(brp.data(), brp.size()), d_btrp = on_device(btrp.data(), btrp.size()),
              d_srp = on_device(srp.data(), srp.size()), d_bcol = on_device(b_col, (size_t)nb),
              d_btcol = on_device(bt_col, (size_t)nbt), d_scol = on_device(s_col, (size_t)ns);
    DBuf<double> d_bval = on_device(b_val, (size_t)nb), d_btval = on_device(bt_val, (size_t)nbt), d_dinv = on_device(dinv, (size_t)n_u), d_sval;
    d_sval.alloc((size_t)ns);
    NSK_HIP(hipDeviceSynchronize());
    const CsrView B{n_p, n_u, d_brp.p, d_bcol.p - base, d_bval.p - base}, Bt{n_u, n_p, d_btrp.p, d_btcol.p - base, d_btval.p - base};
    spgemm_bdbt_numeric(nullptr, B, d_dinv.p, nullptr, Bt, Bt, d_srp.p, d_scol.p - base, d_sval.p - base, n_p, max_row);
    NSK_HIP(hipMemcpy(s_val_out, d_sval.p, sizeof(double) * (size_t)ns, hipMemcpyDeviceToHost));
    return 0;
  } catch (const std::exception &) {
    return -1;
  }
}

// test hook (nsk_internal.h): one Krylov vector operation on caller vectors, through the entry points the solvers call
int nsk_debug_krylov(nsk_handle h, int op, int n, int m, int offset, const double *par, int n_vec, double *const *vec,
                     const int64_t *len, double *slots64, int32_t *info8) {
  NSK_TRY_DEV(h)
  Ctx &c = h->ctx;
  static const int kVecs[] = {2, 1, 3, 2, 4, -1, -1, -1, 3, 0, 6, 4, 3, -1, -1, -1, -1, -1, -1, 2, 3};   // vectors per op (-1: m + 1)
  if (op < NSK_DBG_KRY_DOT || op > NSK_DBG_KRY_EQU_F32) throw Error(-65, "nsk_debug_krylov: unknown op");
  // the ops on an fp32 basis: vec[k] of the basis (k >= 1; EQU_F32: vec[1]) lives on the device as floats, in an allocation
  // of its own behind which kGuardF guard floats sit; the caller's doubles must be fp32 values, and come back widened
  const bool f32_basis = op >= NSK_DBG_KRY_MULTI_DOT_ALL_F32 && op <= NSK_DBG_KRY_GS_COLUMN_F32;
  auto is_float = [&](int k) { return (f32_basis && k >= 1) || (op == NSK_DBG_KRY_EQU_F32 && k == 1); };
  const bool multi = kVecs[op] < 0;
  const bool chunk = op == NSK_DBG_KRY_MULTI_DOT || op == NSK_DBG_KRY_MULTI_AXPY;   // (one launch of the chunked kernels)
  if (multi && (m < 1 || m > (chunk ? 8 : kMgsMaxVecs))) throw Error(-61, "nsk_debug_krylov: m");
  if (n < 1 || (offset != 0 && offset != 1) || n_vec != (multi ? m + 1 : kVecs[op]))
    throw Error(-61, "nsk_debug_krylov: n, offset or number of vectors");
  for (int k = 0; k < n_vec; ++k)
    if (len[k] != ((op == NSK_DBG_KRY_DENSE_MV && k == 0) ? (int64_t)n * n : (int64_t)n))
      throw Error(-61, "nsk_debug_krylov: vector length");
  // every vector in an allocation of its own: `offset` guard words in front, kGuard behind; kGuardF floats behind an fp32 one
  constexpr int kGuard = 4, kGuardF = 8;
  hipStream_t st = h->s();
  std::vector<DbgVec<double>> dv((size_t)n_vec);
  std::vector<DbgVec<float>> fv((size_t)n_vec);
  std::vector<double *> d((size_t)n_vec, nullptr);
  std::vector<float *> f((size_t)n_vec, nullptr);
  std::vector<float> hf;
  for (int k = 0; k < n_vec; ++k) {
    if (is_float(k)) {
      hf.resize((size_t)len[k]);
      for (int64_t i = 0; i < len[k]; ++i) {
        hf[(size_t)i] = (float)vec[k][i];
        if ((double)hf[(size_t)i] != vec[k][i]) throw Error(-61, "nsk_debug_krylov: a basis entry is no fp32 value");
      }
      fv[k].put(hf.data(), (size_t)len[k], 0, kGuardF, st);
      NSK_HIP(hipStreamSynchronize(st));   // (hf is filled again for the next vector)
      f[k] = fv[k].p;
      continue;
    }
    dv[k].put(vec[k], (size_t)len[k], (size_t)offset, kGuard, st);
    d[k] = dv[k].p;
  }
  const SlotLease so(c, 64);
  NSK_HIP(hipMemsetAsync(c.slot(so), 0xFF, sizeof(double) * 64, st));
  auto set_slots = [&](int count) {
    NSK_HIP(hipMemcpyAsync(c.slot(so), par, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, st));
  };
  c.red_paths = 0;
  const long gs_launches = c.gs_launches;
  int path = -1;
  switch (op) {
    case NSK_DBG_KRY_DOT: c.dot(n, d[0], d[1], so); break;
    case NSK_DBG_KRY_NORM2: c.norm2(n, d[0], so); break;
    case NSK_DBG_KRY_AXPY_DOT: c.axpy_dot(n, sref(par[0]), d[0], d[1], d[2], so); break;
    case NSK_DBG_KRY_AXPY_NORM2: c.axpy_norm2(n, sref(par[0]), d[0], d[1], so); break;
    case NSK_DBG_KRY_CG_UPDATE: c.cg_update(n, sref(par[0]), d[0], d[1], d[2], d[3], so); break;
    case NSK_DBG_KRY_MULTI_DOT: c.multi_dot(n, d[0], d.data() + 1, m, so); break;
    case NSK_DBG_KRY_MULTI_AXPY:
      set_slots(m);
      c.multi_axpy(n, d[0], d.data() + 1, m, so, par[m] != 0.0 ? so + m : -1);
      break;
    case NSK_DBG_KRY_GS_COLUMN: {
      const int mode = (int)par[0];
      if (mode < 0 || mode > 2) throw Error(-61, "nsk_debug_krylov: Gram-Schmidt mode 0, 1 or 2");
      c.mgs_tier = 0;
      const long fallbacks = c.mgs_fallbacks;
      // (a sweep whose wait ran out is redone on w as it came in)
      arnoldi_column(c, n, d[0], d.data() + 1, m, so, mode, [&] {
        NSK_HIP(hipMemcpyAsync(d[0], vec[0], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
      });
      if (mode == 0) path = c.mgs_fallbacks == fallbacks ? c.mgs_tier : 0;
      break;
    }
    case NSK_DBG_KRY_DOT3: c.dot3(n, d[0], d[1], d[2], so); break;
    case NSK_DBG_KRY_CG_SCALARS:
      set_slots(7);
      cg_fused_scalars(st, c.slot(so), (int)par[7]);
      break;
    case NSK_DBG_KRY_CG_FUSED_UPDATE:
      set_slots(7);
      vec_cg_fused_update(st, n, c.slot(so), d[0], d[1], d[2], d[3], d[4], d[5]);
      break;
    case NSK_DBG_KRY_CHEBY: vec_cheby_step(st, n, par[0], par[1], d[0], d[1], d[2], d[3], (int)par[2]); break;
    case NSK_DBG_KRY_DENSE_MV: dense_mv(st, n, d[0], d[1], d[2]); break;
    case NSK_DBG_KRY_MULTI_DOT_ALL:
      c.multi_dot_all(n, d[0], d.data() + 1, m, so);
      c.allreduce_slots(so, m);
      break;
    case NSK_DBG_KRY_MULTI_AXPY_ALL:
      set_slots(m);
      c.multi_axpy_all(n, d[0], d.data() + 1, m, so, par[m] != 0.0 ? so + m : -1);
      break;
    case NSK_DBG_KRY_MULTI_ADD: c.multi_add(n, d[0], d.data() + 1, par, m); break;
    case NSK_DBG_KRY_MULTI_DOT_ALL_F32: {
      const bool rider = par[0] != 0.0;
      c.multi_dot_all_f32(n, d[0], f.data() + 1, m, rider, so);
      c.allreduce_slots(so, m + (rider ? 1 : 0));
      break;
    }
    case NSK_DBG_KRY_MULTI_AXPY_ALL_F32:
      set_slots(m);
      c.multi_axpy_all_f32(n, d[0], f.data() + 1, m, so, par[m] != 0.0 ? so + m : -1);
      break;
    case NSK_DBG_KRY_GS_COLUMN_F32: {
      const int mode = (int)par[0];
      if (mode < 1 || mode > 2) throw Error(-61, "nsk_debug_krylov: fp32 basis: Gram-Schmidt mode 1 or 2");
      if (!c.f32_basis_applies(mode)) throw Error(-61, "nsk_debug_krylov: fp32 basis: the pair forms only");
      arnoldi_column(c, n, d[0], (double *const *)nullptr, m, so, mode, [] {}, f.data() + 1);
      break;
    }
    case NSK_DBG_KRY_EQU:
      set_slots(1);
      vec_equ(st, n, sref(1.0, nullptr, c.slot(so)), d[0], d[1]);
      break;
    case NSK_DBG_KRY_EQU_F32:
      set_slots(1);
      vec_equ_f32(st, n, sref(1.0, nullptr, c.slot(so)), d[0], f[1], d[2]);
      break;
  }
  int bad_guards = 0;
  for (int k = 0; k < n_vec; ++k) {
    if (is_float(k)) {
      hf.resize((size_t)len[k]);
      bad_guards += fv[k].fetch(hf.data(), c);
      for (int64_t i = 0; i < len[k]; ++i) vec[k][i] = (double)hf[(size_t)i];
    } else {
      bad_guards += dv[k].fetch(vec[k], c);
    }
  }
  memcpy(slots64, c.read_slots(so, 64), sizeof(double) * 64);
  info8[0] = (int32_t)c.red_paths;
  info8[1] = path;
  info8[2] = std::min(c.n_cu, kMgsThreads);
  info8[3] = bad_guards;
  info8[4] = (int32_t)(c.gs_launches - gs_launches);
  for (int k = 5; k < 8; ++k) info8[k] = 0;
  return 0;
  NSK_CATCH(h)
}

// test hook (nsk_internal.h): one SpMV kernel form on the caller's CSR, through the plan builders and launchers the handle uses

int nsk_debug_spmv(nsk_handle h, int form, int lpr, int mode, int misalign, int c0, int c1, const nsk_dbg_spmv_mat *Am,
                   const nsk_dbg_spmv_mat *Bm, double *y, const double *z, const double *d, const double *dinv,
                   int32_t *rowblk_out, int rowblk_cap, int32_t *info) {
  NSK_TRY_DEV(h)
  Ctx &c = h->ctx;
  hipStream_t st = h->s();
  for (int k = 0; k < 16; ++k) info[k] = 0;
  info[0] = -1;
  if (form < NSK_DBG_SPMV_CSRV || form > NSK_DBG_SPMV_BLK22_RES_F32) throw Error(-65, "nsk_debug_spmv: unknown form");
  const bool two = form == NSK_DBG_SPMV_STREAM2 || form == NSK_DBG_SPMV_BLK_FUSED;
  const bool res = form == NSK_DBG_SPMV_BLK22_RES || form == NSK_DBG_SPMV_BLK22_RES_F32;   // y = z - A x and nothing else
  const bool modes = form == NSK_DBG_SPMV_CSRV || form == NSK_DBG_SPMV_STREAM || form == NSK_DBG_SPMV_STREAM_I16 ||
                     form == NSK_DBG_SPMV_STREAM_F32 || form == NSK_DBG_SPMV_STREAM_I16_F32 || res;
  const bool epi = form == NSK_DBG_SPMV_BLK21_EPI;
  if (!Am || !y || two != (Bm != nullptr)) throw Error(-61, "nsk_debug_spmv: matrices");
  if (mode < 0 || mode > 2 || (mode != 0 && !modes) || (mode == 2 && !z) || (res && mode != 2)) throw Error(-61, "nsk_debug_spmv: mode");
  if (epi && !(d && dinv)) throw Error(-61, "nsk_debug_spmv: the epilogue needs d and dinv");
  if ((two || form == NSK_DBG_SPMV_CSRV) && c0 >= 0) throw Error(-61, "nsk_debug_spmv: this form runs whole plans only");
  int R = 1, C = 1;
  if (form == NSK_DBG_SPMV_BLK22 || form == NSK_DBG_SPMV_BLK22_F32 || form == NSK_DBG_SPMV_BLK_FUSED || res) R = C = 2;
  if (form == NSK_DBG_SPMV_BLK21 || epi) R = 2;
  if (form == NSK_DBG_SPMV_BLK12) C = 2;
  const bool blocked = form >= NSK_DBG_SPMV_BLK22 && form != NSK_DBG_SPMV_STREAM2 && form != NSK_DBG_SPMV_STREAM_I16 && form != NSK_DBG_SPMV_STREAM_I16_F32;
  if ((misalign & 4) && R == 2) throw Error(-61, "nsk_debug_spmv: the R = 2 forms store pairs, y is 16-byte aligned");
  if (two && Bm->n_rows != Am->n_rows) throw Error(-61, "nsk_debug_spmv: both matrices over the same rows");

  Csr A, B;
  dbg_fill_csr(A, *Am, st);
  if (two) dbg_fill_csr(B, *Bm, st);
  info[2] = A.lpr;
  info[3] = R;
  info[4] = C;
  info[5] = A.stream_ok;
  info[6] = A.stream_ok && A.even_rows;

  // the plan of the form: rb (host copy of the runs), entries per run from ea (+ eb)
  std::vector<int> rb;
  const std::vector<int> *ea = &A.h_rowptr, *eb = nullptr;
  DBuf<int> fused_rb;
  const int *d_rb = nullptr;
  int ib0 = 0, ib1 = 0, refused = 0;
  auto download = [&](const DBuf<int> &src, int nblk) {
    rb.resize((size_t)nblk + 1);
    NSK_HIP(hipMemcpyAsync(rb.data(), src.p, sizeof(int) * rb.size(), hipMemcpyDeviceToHost, st));
    c.sync();
    d_rb = src.p;
  };
  const bool i16 = form == NSK_DBG_SPMV_STREAM_I16 || form == NSK_DBG_SPMV_STREAM_I16_F32;
  if (form == NSK_DBG_SPMV_STREAM || form == NSK_DBG_SPMV_STREAM_F32 || i16) {
    if (!A.stream_ok) refused = 1;
    else { download(A.rowblk, A.nblk); ib0 = A.int_b0; ib1 = A.int_b1; }
    if (!refused && i16) {
      A.build_index16(st, true);
      if (!A.off16.p) refused = 5;
    }
  } else if (form == NSK_DBG_SPMV_STREAM2) {
    if (!A.even_rows) refused = 3;   // (jacobian_vmult asks for F.even_rows: the kernel reads F in aligned pairs)
    else if (!fused_row_plan(A, B, rb)) refused = 4;
    else { eb = &B.h_rowptr; fused_rb.upload(rb, st); d_rb = fused_rb.p; ib1 = (int)rb.size() - 1; }
  } else if (blocked) {
    A.build_blocked(R, C, st);
    if (two) B.build_blocked(2, 1, st);
    info[7] = A.blk_ok && (!two || B.blk_ok);
    if (!info[7] || (two && A.blk_rows != B.blk_rows)) refused = 2;
    else if (two) {
      if (!fused_blk_plan(A, B, rb)) refused = 4;
      else { ea = &A.h_blk_rowptr; eb = &B.h_blk_rowptr; fused_rb.upload(rb, st); d_rb = fused_rb.p; ib1 = (int)rb.size() - 1; }
    } else { download(A.blk_rowblk, A.blk_nblk); ea = &A.h_blk_rowptr; ib0 = A.blk_int_b0; ib1 = A.blk_int_b1; }
  }
  info[15] = refused;
  if (refused) return 1;
  const int nblk = (int)rb.size() - 1;   // (-1: CSR-vector, no runs)
  if (form != NSK_DBG_SPMV_CSRV) {
    info[8] = nblk;
    info[9] = ib0;
    info[10] = ib1;
    for (int b = 0; b < nblk; ++b) {
      const int e = (*ea)[rb[b + 1]] - (*ea)[rb[b]] + (eb ? (*eb)[rb[b + 1]] - (*eb)[rb[b]] : 0);
      info[11] = std::max(info[11], rb[b + 1] - rb[b]);
      info[12] = std::max(info[12], e);
    }
    if (rowblk_out) std::copy(rb.begin(), rb.begin() + std::min<size_t>(rb.size(), (size_t)std::max(0, rowblk_cap)), rowblk_out);
    if (c0 < 0) { c0 = 0; c1 = nblk; }
    if (c0 > c1 || c1 > nblk) throw Error(-61, "nsk_debug_spmv: run range");
  }

  // operands: every vector between guard words; the ghost tails, B's x_own and y / z 8 bytes off where asked for
  const int og = misalign & 1, ob = (misalign >> 1) & 1, oy = (misalign >> 2) & 1;
  DbgVec<double> xa, xag, xb, xbg, yv, zv, dv, div;
  xa.put(Am->x_own, (size_t)A.n_own_cols, kDbgFront, kDbgBack, st);
  xag.put(Am->x_ghost, (size_t)(A.n_cols - A.n_own_cols), kDbgFront + og, kDbgBack, st);
  if (two) {
    xb.put(Bm->x_own, (size_t)B.n_own_cols, kDbgFront + ob, kDbgBack, st);
    xbg.put(Bm->x_ghost, (size_t)(B.n_cols - B.n_own_cols), kDbgFront + og, kDbgBack, st);
  }
  yv.put(y, (size_t)A.n_rows, kDbgFront + oy, kDbgBack, st);
  if (z) zv.put(z, (size_t)A.n_rows, kDbgFront + oy, kDbgBack, st);
  if (epi) { dv.put(d, (size_t)A.n_rows, kDbgFront, kDbgBack, st); div.put(dinv, (size_t)A.n_rows, kDbgFront, kDbgBack, st); }

  const int n_run = c1 - c0;
  switch (form) {
    case NSK_DBG_SPMV_CSRV:
      if (lpr == 0) lpr = A.lpr;
      if (lpr != 2 && lpr != 4 && lpr != 8 && lpr != 16 && lpr != 32 && lpr != 64) throw Error(-61, "nsk_debug_spmv: lpr");
      info[2] = nsk::spmv(st, A.view(), lpr, xa.p, xag.p, yv.p, mode, zv.p);
      break;
    // the single-matrix run forms through the handle's launcher (16-bit offsets: built above for the I16 forms only)
    case NSK_DBG_SPMV_STREAM: case NSK_DBG_SPMV_STREAM_I16:
      info[1] = A.spmv_launch(st, SpmvForm::stream, xa.p, xag.p, yv.p, mode, zv.p, c0, c1);
      break;
    case NSK_DBG_SPMV_STREAM_F32: case NSK_DBG_SPMV_STREAM_I16_F32:
      A.inner32 = 2;
      A.refresh_f32(st, false);
      info[1] = A.spmv_launch(st, SpmvForm::stream_f32, xa.p, xag.p, yv.p, mode, zv.p, c0, c1);
      break;
    case NSK_DBG_SPMV_BLK22: case NSK_DBG_SPMV_BLK21: case NSK_DBG_SPMV_BLK12: case NSK_DBG_SPMV_BLK11:
      A.spmv_launch(st, SpmvForm::blk, xa.p, xag.p, yv.p, 0, nullptr, c0, c1);
      break;
    case NSK_DBG_SPMV_BLK22_F32:
      A.inner32 = 1;
      A.refresh_f32(st, false);
      A.spmv_launch(st, SpmvForm::blk_f32, xa.p, xag.p, yv.p, 0, nullptr, c0, c1);
      break;
    case NSK_DBG_SPMV_BLK22_RES:
      nsk::spmv_blk22_residual(st, A.blk_view(), d_rb + c0, n_run, xa.p, xag.p, yv.p, zv.p);
      break;
    case NSK_DBG_SPMV_BLK22_RES_F32:
      A.amg32 = 1;
      A.refresh_f32(st, false);
      A.spmv_launch(st, SpmvForm::blk_f32, xa.p, xag.p, yv.p, 2, zv.p, c0, c1);
      break;
    case NSK_DBG_SPMV_BLK21_EPI:
      nsk::spmv_blk_stream(st, A.blk_view(), 2, 1, d_rb + c0, n_run, xa.p, xag.p, yv.p, dv.p, div.p);
      break;
    case NSK_DBG_SPMV_STREAM2:
      info[1] = nsk::spmv2_stream(st, A.view(), xa.p, xag.p, B.view(), xb.p, xbg.p, d_rb, nblk, yv.p);
      break;
    case NSK_DBG_SPMV_BLK_FUSED:
      nsk::spmv_blk_fused22_21(st, A.blk_view(), xa.p, xag.p, B.blk_view(), xb.p, xbg.p, d_rb, nblk, yv.p);
      break;
  }
  NSK_HIP(hipGetLastError());
  info[0] = form;
  info[14] = form == NSK_DBG_SPMV_CSRV ? 0 : n_run;
  int bad = yv.fetch(y, c);
  for (DbgVec<double> *v : {&xa, &xag, &xb, &xbg, &zv, &dv, &div}) bad += v->fetch(nullptr, c);
  info[13] = bad;
  return 0;
  NSK_CATCH(h)
}

// test hook (nsk_internal.h): one TriSolve on the caller's CSR — analyze, numeric, n_apply applies — and what it chose
int nsk_debug_tri(nsk_handle h, const nsk_dbg_tri_args *a, int32_t *info) {
  NSK_TRY_DEV(h)
  Ctx &c = h->ctx;
  hipStream_t st = h->s();
  for (int k = 0; k < 40; ++k) info[k] = 0;
  if (!a || a->n < 1 || !a->rowptr || !a->col || !a->val || a->rowptr[0] != 0 || a->n_apply < 1 || !a->b || !a->x ||
      !a->perm_out || !a->factor_out)
    throw Error(-61, "nsk_debug_tri: arguments");
  if (a->kind < 0 || a->kind > 1 || a->ordering < ORDER_NATURAL || a->ordering > ORDER_MULTICOLOR || a->group < 1)
    throw Error(-61, "nsk_debug_tri: kind, ordering or group");
  const int n = a->n;
  for (int i = 0; i < n; ++i)
    if (a->rowptr[i + 1] < a->rowptr[i]) throw Error(-58, "nsk_debug_tri: rowptr not monotone");
  const int64_t nnz = a->rowptr[n];
  for (int i = 0; i < n; ++i)
    for (int k = a->rowptr[i]; k < a->rowptr[i + 1]; ++k)
      if (a->col[k] < 0 || a->col[k] >= n || (k > a->rowptr[i] && a->col[k - 1] >= a->col[k]))
        throw Error(-59, "nsk_debug_tri: column ids out of range or not sorted");
  std::vector<int> sub;
  if (a->n_sub > 1) {
    if (!a->sub_off || a->sub_off[0] != 0 || a->sub_off[a->n_sub] != n) throw Error(-61, "nsk_debug_tri: sub-domain offsets");
    for (int k = 0; k < a->n_sub; ++k)
      if (a->sub_off[k + 1] < a->sub_off[k]) throw Error(-61, "nsk_debug_tri: sub-domain offsets");
    sub.assign(a->sub_off, a->sub_off + a->n_sub + 1);
  }
  // the colour-ordered working vector belongs to the blocked single-launch solve (H::setup): anything else is not forced
  if (a->x_layout != 0 && !(a->want_block2 && a->sync_free)) {
    info[16] = 1;
    return 1;
  }

  Csr A;   // what nsk_set_block_csr leaves of a block, as far as the analysis and numeric() read it
  A.n_rows = A.n_cols = A.n_own_cols = n;
  A.nnz = nnz;
  A.h_rowptr.assign(a->rowptr, a->rowptr + n + 1);
  A.h_col.assign(a->col, a->col + nnz);
  A.rowptr.upload(a->rowptr, (size_t)n + 1, st);
  A.col.upload(a->col, (size_t)nnz, st);
  A.val.upload(a->val, (size_t)nnz, st);
  A.present = true;

  TriSolve T;
  T.use_stream = a->use_stream != 0;
  T.sync_free = a->sync_free != 0;
  T.tiny_bytes = a->tiny_bytes;
  T.host_analysis = a->host_analysis != 0;
  T.want_index16 = a->want_index16 != 0;
  T.want_f32 = a->want_f32 != 0;
  T.x_layout = a->x_layout != 0 ? 1 : 0;
  T.analyze(&c, A, a->kind, a->ordering, sub, a->want_block2 != 0, a->xy, a->group);
  // guard words behind the intermediate vector (analyze() sized it n + 1; nothing reads its size afterwards)
  T.y.alloc((size_t)n + 1 + kDbgBack);
  NSK_HIP(hipMemsetAsync(T.y.p, 0xFF, sizeof(double) * T.y.n, st));
  if (T.x_layout) {   // the colour-ordered working vector too (apply() keeps a vector that is long enough)
    T.xc.alloc((size_t)n + 1 + kDbgBack);
    NSK_HIP(hipMemsetAsync(T.xc.p, 0xFF, sizeof(double) * T.xc.n, st));
  }
  T.numeric(A.val.p);
  NSK_HIP(hipGetLastError());

  std::vector<DbgVec<double>> bv((size_t)a->n_apply), xv((size_t)a->n_apply);
  for (int k = 0; k < a->n_apply; ++k) {
    bv[k].put(a->b + (size_t)k * n, (size_t)n, kDbgFront, kDbgBack, st);
    xv[k].put(a->x + (size_t)k * n, (size_t)n, kDbgFront, kDbgBack, st);
  }
  for (int k = 0; k < a->n_apply; ++k) T.apply(bv[k].p, xv[k].p);
  NSK_HIP(hipGetLastError());
  int bad = 0;
  for (int k = 0; k < a->n_apply; ++k) {
    bad += xv[k].fetch(a->x + (size_t)k * n, c);
    bad += bv[k].fetch(nullptr, c);
  }
  for (const DBuf<double> *iv : {&T.y, &T.xc}) {
    if (iv->n != (size_t)n + 1 + kDbgBack) continue;   // (xc: only where the hook allocated it)
    std::vector<double> tail(kDbgBack);
    NSK_HIP(hipMemcpyAsync(tail.data(), iv->p + n + 1, sizeof(double) * kDbgBack, hipMemcpyDeviceToHost, st));
    c.sync();
    for (double v : tail) {
      uint64_t bits;
      memcpy(&bits, &v, 8);
      bad += bits != ~0ull;
    }
  }

  // the permutation, and the factor at the caller's positions
  for (int i = 0; i < n; ++i) a->perm_out[i] = T.perm.empty() ? i : T.perm[i];
  {
    std::vector<double> fv((size_t)T.nnz);
    std::vector<int> sp((size_t)T.nnz);
    if (T.nnz) {
      NSK_HIP(hipMemcpyAsync(fv.data(), T.val.p, sizeof(double) * fv.size(), hipMemcpyDeviceToHost, st));
      NSK_HIP(hipMemcpyAsync(sp.data(), T.srcpos.p, sizeof(int) * sp.size(), hipMemcpyDeviceToHost, st));
    }
    c.sync();
    uint64_t nan_bits = 0x7FF8000000000000ull;
    double nanv;
    memcpy(&nanv, &nan_bits, 8);
    for (int64_t k = 0; k < nnz; ++k) a->factor_out[k] = nanv;
    for (size_t k = 0; k < fv.size(); ++k) {
      if (sp[k] < 0 || sp[k] >= nnz) throw Error(-62, "nsk_debug_tri: a source position outside the matrix");
      a->factor_out[sp[k]] = fv[k];
    }
  }

  const int path = T.last_path;
  const bool scalar_halves = path == TRI_PATH_SF_SCALAR || path == TRI_PATH_COLOUR_SCALAR;
  const bool halves = scalar_halves || path == TRI_PATH_SF_BLOCKED || path == TRI_PATH_COLOUR_BLOCKED;
  info[0] = path;
  info[1] = halves && T.f32 ? 32 : 64;
  info[2] = !scalar_halves ? 0 : T.Loff16.p ? 16 : 32;
  info[3] = !scalar_halves ? 0 : T.Uoff16.p ? 16 : 32;
  info[4] = T.gmax;
  info[5] = T.n_colors;
  info[6] = T.n_levels_L;
  info[7] = T.n_levels_U;
  if (T.stream_ready || T.block2_ready) {
    for (int half = 0; half < 2; ++half) {
      const DBuf<int4> &D = half ? T.Udesc : T.Ldesc;
      std::vector<int4> d(D.n);
      if (D.n) NSK_HIP(hipMemcpyAsync(d.data(), D.p, sizeof(int4) * D.n, hipMemcpyDeviceToHost, st));
      c.sync();
      info[8 + 2 * half] = (int)D.n;
      info[9 + 2 * half] = (half ? T.n_Usf : T.n_Lsf) - (int)D.n;
      for (const int4 &r : d) {
        info[12] = std::max(info[12], r.y - r.x);
        info[13] = std::max(info[13], r.w - r.z);
      }
    }
  }
  if (T.sf_err.p) {
    int e = 0;
    NSK_HIP(hipMemcpy(&e, T.sf_err.p, sizeof(int), hipMemcpyDeviceToHost));
    info[14] = e != 0;
  }
  info[15] = bad;
  info[17] = (a->want_block2 && !T.block2_ready ? 1 : 0) | (a->want_index16 && !(scalar_halves && T.Loff16.p) ? 2 : 0) |
             (a->want_f32 && info[1] != 32 ? 4 : 0) |
             (a->ordering == ORDER_NATURAL && n >= 4096 && !T.ring_ready ? 8 : 0);
  info[18] = T.lpr;
  for (const TriSolve::Step &s : T.schedL) ++info[s.serial ? 20 : 19];
  for (const TriSolve::Step &s : T.schedU) ++info[s.serial ? 29 : 28];
  info[21] = T.last_tiny;
  info[22] = T.ring_ready ? T.ringL.n_pass : 0;
  if (a->kind == 0)
    for (const TriSolve::Step &s : T.schedN) ++info[s.serial ? 24 : 23];
  info[25] = T.stream_ready;
  info[26] = T.block2_ready;
  info[27] = T.dev_analysis;
  info[30] = T.max_row_nnz;
  info[31] = (int32_t)T.nnz;
  info[32] = path == TRI_PATH_SF_BLOCKED && T.x_layout != 0;
  return 0;
  NSK_CATCH(h)
}

// test hook (nsk_internal.h): one operation of the AMG set-up on the caller's arrays (nsk_amg.cpp: debug_amg)
int nsk_debug_amg(nsk_handle h, const nsk_dbg_amg_args *a, int32_t *info) {
  NSK_TRY_DEV(h)
  return debug_amg(&h->ctx, a, info);
  NSK_CATCH(h)
}

int nsk_debug_index_width(nsk_handle h, int b, int32_t *out3) {
  NSK_TRY(h)
  if (b != NSK_BLK_S && b != NSK_BLK_MP) throw Error(-62, "nsk_debug_index_width: S or M_p");
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  const Csr &A = h->blk[b];
  const TriSolve &T = b == NSK_BLK_S ? h->tS : h->tMp;
  out3[0] = !A.present || h->form_of(A) != SpmvForm::stream ? 0 : A.off16.p ? 16 : 32;
  // (S under NSK_OPT_SCHUR_AMG: no factor in this set-up, whatever an earlier one left in tS)
  const bool halves = T.stream_ready && T.halves_in_use() && !(b == NSK_BLK_S && h->schur_amg_active);
  out3[1] = !halves ? 0 : T.Loff16.p ? 16 : 32;
  out3[2] = !halves ? 0 : T.Uoff16.p ? 16 : 32;
  return 0;
  NSK_CATCH(h)
}

int nsk_debug_spmv_form(int blk_ok, int stream_ok, int inner32, int use_stream, int use_bsr, int mode, int inner) {   // nsk_internal.h
  return (int)spmv_form(blk_ok != 0, stream_ok != 0, inner32, use_stream != 0, use_bsr != 0, mode, inner != 0);
}

int nsk_debug_amg_spmv_form(int blk_ok, int stream_ok, int amg32, int use_bsr, int mode, int aligned16) {   // nsk_internal.h
  return (int)amg_spmv_form(blk_ok != 0, stream_ok != 0, amg32 != 0, use_bsr != 0, mode, aligned16 != 0);
}

int64_t nsk_debug_amg_level(nsk_handle h, int shard, int level, int which, int32_t *rowptr, int32_t *col, double *val,
                            double *dinv_or_inverse) {   // nsk_internal.h
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if (!h->amg_active) throw Error(-62, "nsk_debug_amg_level: the current set-up has no velocity AMG");
  h->amg_ready();
  return h->amgF.debug_level(shard, level, which, rowptr, col, val, dinv_or_inverse);
  NSK_CATCH(h)
}

int nsk_debug_amg_forms(nsk_handle h, int64_t *out5) {   // nsk_internal.h
  for (int k = 0; k < 5; ++k) out5[k] = h->amg_active ? h->amgF.form_launches[k] : 0;
  return 0;
}

int nsk_debug_schur_amg_forms(nsk_handle h, int64_t *out5) {   // nsk_internal.h
  for (int k = 0; k < 5; ++k) out5[k] = h->schur_amg_active ? h->amgS.form_launches[k] : 0;
  return 0;
}

int nsk_debug_amg_spmv_form2(int blk_ok, int stream_ok, int amg32, int use_bsr, int mode, int aligned16, int blk_residual) {   // nsk_internal.h
  return (int)amg_spmv_form(blk_ok != 0, stream_ok != 0, amg32 != 0, use_bsr != 0, mode, aligned16 != 0, blk_residual != 0);
}

int nsk_debug_env_parse(int kind, const char *text) {   // nsk_internal.h
  return kind == 0 ? parse_env_precision(text) : kind == 1 ? parse_env_switch(text) : -2;
}

int nsk_debug_setup_plan(const int *req9, const int *env8, int type, int variant, int *out12) {   // nsk_internal.h
  const SetupRequest req = {req9[0], req9[1], req9[2], req9[3], req9[4], req9[5], req9[6], req9[7], req9[8]};
  const SetupEnv env = {env8[0], env8[1], env8[2], env8[3], env8[4], env8[5], env8[6], env8[7]};
  const SetupPlan p = resolve_setup(req, env, type, variant);
  const int out[12] = {p.factor32, p.amg_bits_F, p.want_amgF, p.fused_cheby, p.want_amgS, p.amg_bits_S,
                       p.inner32,  p.matfree,    p.basis32,   p.kindF,       p.kindP,     p.velocity_amg_wanted};
  std::copy(out, out + 12, out12);
  return 12;
}

int nsk_debug_amg_fused(nsk_handle h, int64_t *out1) {   // nsk_internal.h
  *out1 = h->amg_active ? h->amgF.fused_launches : 0;
  return 0;
}

// test hook (nsk_internal.h): one fused Chebyshev step, and the two launches it replaces, on the same device data
int nsk_debug_cheby_fused(nsk_handle h, const nsk_dbg_spmv_mat *Am, const double *b, const double *dinv, const double *w,
                          double c1, double c2, int fp32, int in_place, double *w_out, double *x_out, double *r_ref,
                          double *w_ref, double *x_ref, int32_t *info4) {
  NSK_TRY_DEV(h)
  Ctx &c = h->ctx;
  hipStream_t st = h->s();
  for (int k = 0; k < 4; ++k) info4[k] = 0;
  if (!Am || !b || !dinv || !w) throw Error(-61, "nsk_debug_cheby_fused: arguments");
  if (Am->n_rows % 2 || Am->n_own_cols < Am->n_rows) throw Error(-61, "nsk_debug_cheby_fused: an even number of rows, no more than owned columns");
  Csr A;
  dbg_fill_csr(A, *Am, st);
  A.build_blocked(2, 2, st);
  if (!A.blk_ok) { info4[2] = 2; return 1; }
  const SpmvForm f = fp32 ? SpmvForm::blk_f32 : SpmvForm::blk;
  if (fp32) { A.amg32 = 1; A.refresh_f32(st, false); }
  const size_t n = (size_t)A.n_rows;
  DbgVec<double> xi, xg, bv, dv, wf, xo, rr, wr, xr;
  xi.put(Am->x_own, (size_t)A.n_own_cols, kDbgFront, kDbgBack, st);
  xg.put(Am->x_ghost, (size_t)(A.n_cols - A.n_own_cols), kDbgFront, kDbgBack, st);
  bv.put(b, n, kDbgFront, kDbgBack, st);
  dv.put(dinv, n, kDbgFront, kDbgBack, st);
  wf.put(w, n, kDbgFront, kDbgBack, st);
  wr.put(w, n, kDbgFront, kDbgBack, st);
  xo.put(b, n, kDbgFront, kDbgBack, st);          // (overwritten: the fused launch sets every entry of x_out)
  rr.put(b, n, kDbgFront, kDbgBack, st);
  xr.put(Am->x_own, n, kDbgFront, kDbgBack, st);   // the two-launch step updates x in place: a copy of x_in's rows
  if (in_place) {
    // the refusal, and nothing else: the launcher must not touch the device
    const int rc = A.cheby_launch(st, f, xi.p, xg.p, xi.p, bv.p, dv.p, wf.p, c1, c2);
    if (rc == 0) throw Error(-1, "nsk_debug_cheby_fused: an in-place fused step was launched");
    throw Error(-61, "fused Chebyshev step: x_out must not be x_in (other workgroups are still gathering it)");
  }
  if (A.cheby_launch(st, f, xi.p, xg.p, xo.p, bv.p, dv.p, wf.p, c1, c2) != 0) throw Error(-1, "nsk_debug_cheby_fused: the launcher refused");
  A.spmv_launch(st, f, xi.p, xg.p, rr.p, 2, bv.p);
  vec_cheby_step(st, (int)n, c1, c2, dv.p, rr.p, wr.p, xr.p, 0);
  NSK_HIP(hipGetLastError());
  info4[1] = A.blk_nblk;
  int bad = wf.fetch(w_out, c) + xo.fetch(x_out, c) + rr.fetch(r_ref, c) + wr.fetch(w_ref, c) + xr.fetch(x_ref, c);
  for (DbgVec<double> *v : {&xi, &xg, &bv, &dv}) bad += v->fetch(nullptr, c);
  info4[0] = bad;
  return 0;
  NSK_CATCH(h)
}

int nsk_debug_pool_counts(nsk_handle h, int32_t *out6) {   // nsk_internal.h
  int k = 0;
  for (const VecPool *p : {&h->pool_u, &h->pool_p, &h->pool_b}) {
    out6[k++] = (int32_t)p->all.size();
    out6[k++] = (int32_t)p->free_list.size();
  }
  return 0;
}

int64_t nsk_debug_asm(nsk_handle h, int what, void *out, int64_t cap) {   // nsk_internal.h
  NSK_TRY_DEV(h)
  const auto &A = h->asmd;
  if (!A.ready || A.simplex || !A.mf_valid) throw Error(-66, "nsk_debug_asm: no Q3/Q2 assembly on the handle (call nsk_assemble)");
  const void *src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case NSK_DBG_ASM_CQ: src = A.cq.p; bytes = sizeof(double) * (size_t)A.n_cells * kAsmCellDoubles; break;
    case NSK_DBG_ASM_D0: src = A.d0.p; bytes = sizeof(double); break;
    case NSK_DBG_ASM_NODE_CELLS: src = A.node_cells.p; bytes = sizeof(int) * A.node_cells.n; break;
    case NSK_DBG_ASM_NODE_OFF: src = A.node_off.p; bytes = A.node_off.n; break;
    case NSK_DBG_ASM_NODE_SELF: src = A.node_self.p; bytes = sizeof(int) * A.node_self.n; break;
    case NSK_DBG_ASM_PDOF_CELLS: src = A.pdof_cells.p; bytes = sizeof(int) * A.pdof_cells.n; break;
    default: throw Error(-65, "nsk_debug_asm: unknown item");
  }
  if (!out || cap < (int64_t)bytes) throw Error(-61, "nsk_debug_asm: out is too small");
  if (bytes) NSK_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return (int64_t)bytes;
  NSK_CATCH(h)
}

}  // extern "C"
