// nsk_capi.cpp — the public C ABI of include/nsk.h on the handle of nsk_handle.hpp, but for the device-assembly group
// (nsk_capi_assembly.cpp).  The preconditioners and the solve behind it: nsk_precond.cpp; the test hooks: nsk_debug.cpp.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "../../include/nsk_threads.h"
#include <omp.h>
#include "nsk_handle.hpp"
#include "nsk_internal.h"

extern "C" {

int nsk_get_unique_id(void *out128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -20;
  std::memcpy(out128, &id, sizeof(id));
  return 0;
}

int nsk_local_group_id(int nranks, void *out128) {
  if (nranks < 1 || !out128) return -1;
  make_local_group(nranks, out128, 0);
  return 0;
}

static void cap_host_threads() {  // see nsk_threads.h: the symbolic phases and the AMG set-up are OpenMP loops
  static bool done = false;
  if (done) return;
  done = true;
  if (getenv("OMP_NUM_THREADS")) return;
  const int q = nsk_cpu_budget();
  if (q < omp_get_max_threads()) omp_set_num_threads(q);
}

nsk_handle nsk_create(int rank, int nranks, int device_id, const void *uid) {
  cap_host_threads();
  H *h = new H();
  try {
    h->ctx.init(device_id);
    h->ctx.warn_text = &h->err;
    h->ctx.comm.init(rank, nranks, uid, device_id);

  } catch (const std::exception &e) {
    fprintf(stderr, "nsk_create: %s\n", e.what());
    delete h;
    return nullptr;
  }
  return h;
}

void nsk_destroy(nsk_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->ctx.device);
  (void)hipStreamSynchronize(h->ctx.stream);
  h->drop_pending();
  h->basis32_u.destroy();
  h->pool_u.destroy();
  h->pool_p.destroy();
  h->pool_b.destroy();
  h->ctx.destroy();
  delete h;
}

const char *nsk_last_error(nsk_handle h) { return h ? h->err.c_str() : "null handle"; }

int nsk_set_partition(nsk_handle h, int space, int64_t b, int64_t e, int n_ghost, const int32_t *gids) {
  NSK_TRY(h)
  if (space < 0 || space > 1 || e < b || n_ghost < 0) throw Error(-50, "nsk_set_partition: bad arguments");
  if (h->pools_ready) throw Error(-51, "partition is fixed once vectors exist");
  Space &S = h->sp[space];
  S.n = (int)(e - b);
  S.ng = n_ghost;
  S.gbegin = b;
  S.gend = e;
  S.ghost_gid.assign(gids, gids + n_ghost);
  // support points handed over for another row count are void (xy() would hand the ordering an array sized for it)
  h->support[space].clear();
  h->tF_ok = h->tMp_ok = h->tS_ok = false;
  return 0;
  NSK_CATCH(h)
}

int nsk_set_support_points(nsk_handle h, int space, const double *xy) {
  NSK_TRY(h)
  if (space < 0 || space > 1) throw Error(-50, "nsk_set_support_points: bad space");
  const Space &S = h->sp[space];
  if (xy) h->support[space].assign(xy, xy + 2 * (size_t)S.n);
  else h->support[space].clear();
  h->tF_ok = h->tMp_ok = h->tS_ok = false;   // the orderings of the triangular factors depend on them
  return 0;
  NSK_CATCH(h)
}

int nsk_set_halo_plan(nsk_handle h, int space, int nn, const int32_t *peer, const int32_t *send_ptr,
                      const int32_t *send_idx, const int32_t *recv_ptr) {
  NSK_TRY_DEV(h)
  if (space < 0 || space > 1 || nn < 0) throw Error(-52, "nsk_set_halo_plan: bad arguments");
  Space &S = h->sp[space];
  S.peers.assign(peer, peer + nn);
  S.send_ptr.assign(send_ptr, send_ptr + nn + 1);
  S.recv_ptr.assign(recv_ptr, recv_ptr + nn + 1);
  S.n_send = nn ? send_ptr[nn] : 0;
  for (int k = 0; k < S.n_send; ++k)
    if (send_idx[k] < 0 || send_idx[k] >= S.n) throw Error(-53, "halo plan: send index outside the owned range");
  if (nn && recv_ptr[nn] != S.ng) throw Error(-54, "halo plan: receive counts do not cover the ghost list");
  S.d_send_idx.upload(send_idx, (size_t)S.n_send, h->s());
  S.d_send_buf.alloc((size_t)std::max(1, S.n_send));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_set_block_csr(nsk_handle h, int b, int n_rows, int n_cols, const int32_t *rowptr, const int32_t *col,
                      const double *val) {
  NSK_TRY_DEV(h)
  if (b < 0 || b > NSK_BLK_BT_GHOST) throw Error(-55, "nsk_set_block_csr: bad block id");
  const int rs = (b == NSK_BLK_F || b == NSK_BLK_BT) ? 0 : 1;   // row space
  const int cs = (b == NSK_BLK_F || b == NSK_BLK_B) ? 0 : 1;    // column space
  const Space &R = h->sp[rs], &Cc = h->sp[cs];
  const int want_rows = b == NSK_BLK_BT_GHOST ? h->sp[0].ng : R.n;
  if (n_rows != want_rows) throw Error(-56, "nsk_set_block_csr: row count does not match the partition");
  if (n_cols != Cc.n + Cc.ng) throw Error(-57, "nsk_set_block_csr: column count does not match owned+ghost");
  const int64_t nnz = rowptr[n_rows];
  for (int i = 0; i < n_rows; ++i)
    if (rowptr[i + 1] < rowptr[i]) throw Error(-58, "nsk_set_block_csr: rowptr not monotone");
  bool bad_col = false;
#pragma omp parallel for schedule(static) reduction(|| : bad_col)
  for (int64_t k = 0; k < nnz; ++k) bad_col = bad_col || col[k] < 0 || col[k] >= n_cols;
  if (bad_col) throw Error(-59, "nsk_set_block_csr: column id out of range");
  Csr &A = h->blk[b];
  Phase ph("hand-off of one block");
  A.n_rows = n_rows;
  A.n_cols = n_cols;
  A.n_own_cols = Cc.n;
  A.nnz = nnz;
  A.h_rowptr.assign(rowptr, rowptr + n_rows + 1);
  A.h_col.resize((size_t)nnz);
#pragma omp parallel for schedule(static)
  for (int64_t c = 0; c < (nnz + (1 << 20) - 1) >> 20; ++c)   // (1.7 GB at 1200x400: a serial copy was a third of the hand-off)
    std::memcpy(A.h_col.data() + (c << 20), col + (c << 20), sizeof(int) * (size_t)std::min<int64_t>(1 << 20, nnz - (c << 20)));
  A.rowptr.upload(rowptr, (size_t)n_rows + 1, h->s());
  A.col.upload(col, (size_t)nnz, h->s());
  A.val.upload(val, (size_t)nnz, h->s());
  if (b == NSK_BLK_MP) ++h->mp_values_version;
  ++A.values_version;
  A.release_f32();   // (a new pattern: the next set-up converts again)
  if (b == NSK_BLK_F) h->asmd.mf_valid = false;   // (values from outside: not the last assembly's any more)
  A.lpr = pick_lpr(nnz, n_rows);
  A.present = true;
  A.build_stream_plan(h->s());
  if (b == NSK_BLK_MP) h->index16_for(A, "M_p");
  if (b == NSK_BLK_F) A.build_blocked(2, 2, h->s());
  if (b == NSK_BLK_BT) A.build_blocked(2, 1, h->s());
  if (b == NSK_BLK_B) A.build_blocked(1, 2, h->s());
  h->ctx.sync();
  if (b == NSK_BLK_F || b == NSK_BLK_BT) { h->jrow_ok = h->jblk_ok = false; h->jrow_nblk = h->jblk_nblk = 0; }
  // a new pattern invalidates cached symbolic data
  if (b == NSK_BLK_F) {
    h->tF_ok = false;
    h->amgF.clear();
    if (h->amg_active) h->amg_pending = true;
  }
  if (b == NSK_BLK_MP) h->tMp_ok = false;
  if (b == NSK_BLK_B || b == NSK_BLK_BT || b == NSK_BLK_BT_GHOST) { h->s_symbolic = false; h->tS_ok = false; }
  return 0;
  NSK_CATCH(h)
}

int nsk_update_values(nsk_handle h, int b, const double *val) {
  NSK_TRY_DEV(h)
  if (b < 0 || b > NSK_BLK_BT_GHOST || !h->blk[b].present) throw Error(-60, "nsk_update_values: block not set");
  Csr &A = h->blk[b];
  NSK_HIP(hipMemcpyAsync(A.val.p, val, sizeof(double) * (size_t)A.nnz, hipMemcpyHostToDevice, h->s()));
  if (b == NSK_BLK_MP) ++h->mp_values_version;
  if (b == NSK_BLK_F) h->asmd.mf_valid = false;
  ++A.values_version;
  A.refresh_blocked(h->s());
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

// "v must be one of these, else -61 with this text": the plain cases of nsk_set_option
static int one_of(double v, std::initializer_list<double> allowed, const char *text) {
  for (const double a : allowed)
    if (v == a) return (int)v;
  throw Error(-61, text);
}

int nsk_set_option(nsk_handle h, int opt, double v) {
  NSK_TRY(h)
  SetupRequest &req = h->req;
  switch (opt) {
    case NSK_OPT_TRI_ORDERING: h->tri_ordering = v != 0.0 ? ORDER_MULTICOLOR : ORDER_NATURAL; break;
    case NSK_OPT_SUBDOMAINS: h->subdomains = std::max(1, (int)v); break;
    case NSK_OPT_FUSE_BLOCK_ROW: h->fuse_block_row = v != 0.0; break;
    case NSK_OPT_STREAM_KERNELS: h->use_stream = v != 0.0; break;
    case NSK_OPT_TRI_SYNC_FREE: h->sync_free_mode = one_of(v, {0, 1, 2}, "NSK_OPT_TRI_SYNC_FREE: 0, 1 or 2"); break;
    case NSK_IOPT_FAULT_INJECT:
      h->fault_inject = (int)v;
      h->ctx.mgs_fault = (h->fault_inject & 4) != 0;
      break;
    case NSK_OPT_TRI_LINE_GROUPS: h->line_groups = one_of(v, {0, 1, 2}, "NSK_OPT_TRI_LINE_GROUPS: 0, 1 or 2"); break;
    case NSK_OPT_MASS_ORDERING: h->mp_ordering = one_of(v, {-1, 0, 1}, "NSK_OPT_MASS_ORDERING: -1, 0 or 1"); break;
    case NSK_IOPT_GROUP_U:
    case NSK_IOPT_GROUP_P:   // (a range, not a list: 1.5 is taken as 1, as it always was)
      if (v < 1.0 || v > (double)kTriGroupMax) throw Error(-61, "line-group size: 1 .. 3");
      (opt == NSK_IOPT_GROUP_U ? h->group_u : h->group_p) = (int)v;
      break;
    case NSK_IOPT_FUSED_MGS: h->ctx.fused_mgs = v != 0.0; break;
    case NSK_IOPT_GS_ONE_LAUNCH: h->ctx.gs_one_launch = one_of(v, {0, 1, 2}, "one-launch Gram-Schmidt sweeps: 0, 1 or 2"); break;
    case NSK_IOPT_FGMRES_SKIP_UNUSED: h->skip_unused = one_of(v, {0, 1}, "NSK_IOPT_FGMRES_SKIP_UNUSED: 0 or 1") != 0; break;
    case NSK_IOPT_OVERLAP_HALO: h->overlap_halo = v != 0.0; break;
    case NSK_IOPT_TINY_BYTES: h->tF.tiny_bytes = h->tMp.tiny_bytes = h->tS.tiny_bytes = v; break;
    case NSK_OPT_BSR_VELOCITY: h->use_bsr = v != 0.0; break;   // (part of the key of F's analysis: setup_velocity_factor)
    case NSK_OPT_VELOCITY_AMG: req.velocity_amg = v != 0.0; break;
    case NSK_IOPT_TIMEOP_BETWEEN: h->timeop_between = (int)v; break;
    case NSK_IOPT_INDEX16:
      h->index16 = v != 0.0;
      (void)hipSetDevice(h->ctx.device);
      for (int b : {NSK_BLK_MP, NSK_BLK_S})
        if (h->blk[b].present && h->blk[b].stream_ok) h->index16_for(h->blk[b], b == NSK_BLK_S ? "S" : "M_p");
      h->ctx.sync();
      h->tS_ok = h->tMp_ok = false;   // the factors' halves are rebuilt by the next set-up
      break;
    case NSK_IOPT_HOST_ANALYSIS:
      h->tF.host_analysis = h->tS.host_analysis = h->tMp.host_analysis = v != 0.0;
      h->tF_ok = h->tS_ok = h->tMp_ok = false;
      break;
    case NSK_OPT_BLAS1_PAIRS:
      h->blas1_pairs = one_of(v, {-1, 0, 1}, "NSK_OPT_BLAS1_PAIRS: -1, 0 or 1");
      h->ctx.ws.pairs = v < 0.0 ? (h->variant == 0) : (int)v;
      break;
    case NSK_OPT_SCHUR_SIGN: h->schur_sign = one_of(v, {1, -1}, "NSK_OPT_SCHUR_SIGN: +1 or -1"); break;
    case NSK_OPT_FACTOR_PRECISION: req.factor_precision = one_of(v, {64, 32}, "NSK_OPT_FACTOR_PRECISION: 64 or 32"); break;
    case NSK_OPT_INNER_MATRIX_PRECISION: req.inner_matrix_precision = one_of(v, {64, 32}, "NSK_OPT_INNER_MATRIX_PRECISION: 64 or 32"); break;
    case NSK_OPT_INNER_BASIS_PRECISION: req.inner_basis_precision = one_of(v, {64, 32}, "NSK_OPT_INNER_BASIS_PRECISION: 64 or 32"); break;
    case NSK_OPT_AMG_PRECISION: req.amg_precision = one_of(v, {64, 32}, "NSK_OPT_AMG_PRECISION: 64 or 32"); break;
    case NSK_OPT_INNER_MATRIX_FREE_F: req.matrix_free_f = one_of(v, {0, 1}, "NSK_OPT_INNER_MATRIX_FREE_F: 0 or 1"); break;
    case NSK_OPT_SCHUR_AMG: req.schur_amg = one_of(v, {0, 1}, "NSK_OPT_SCHUR_AMG: 0 or 1"); break;
    case NSK_OPT_ASIMPLE_VELOCITY_AMG: req.asimple_velocity_amg = one_of(v, {0, 1}, "NSK_OPT_ASIMPLE_VELOCITY_AMG: 0 or 1"); break;
    case NSK_IOPT_AMG_FUSED_CHEBY: req.amg_fused_cheby = one_of(v, {-1, 0, 1}, "NSK_IOPT_AMG_FUSED_CHEBY: -1, 0 or 1"); break;
    case NSK_IOPT_TRI_X_LAYOUT:
      h->x_layout_mode = v == 0.0 ? 0 : 2;
      h->tF_ok = false;
      break;
    case NSK_OPT_INNER_FUSED_GS: h->inner_fused_gs = one_of(v, {0, 1, 2}, "NSK_OPT_INNER_FUSED_GS: 0, 1 or 2"); break;
    case NSK_OPT_OUTER_FUSED_GS: h->outer_fused_gs = v != 0.0; break;
    case NSK_OPT_CG_SINGLE_REDUCTION: h->cg_fused = v != 0.0; break;
    default: throw Error(-61, "nsk_set_option: unknown option");
  }
  h->push_tri_options();
  return 0;
  NSK_CATCH(h)
}

int nsk_setup_preconditioner(nsk_handle h, int type, int variant, double alpha) {
  NSK_TRY_DEV(h)
  h->setup(type, variant, alpha);
  return 0;
  NSK_CATCH_ABORT(h)
}

int nsk_upload_system(nsk_handle h, const double *ru, const double *rp, const double *xu, const double *xp) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  const size_t bu = sizeof(double) * (size_t)h->n_u(), bp = sizeof(double) * (size_t)h->n_p();
  NSK_HIP(hipMemcpyAsync(h->rhs_b, ru, bu, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(h->rhs_b + h->n_u(), rp, bp, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(h->x_b, xu, bu, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(h->x_b + h->n_u(), xp, bp, hipMemcpyHostToDevice, h->s()));
  h->ctx.sync();
  h->asmd.x_is_result = h->asmd.sx_delta_valid = false;   // (the caller's vector, no solve's result)
  return 0;
  NSK_CATCH(h)
}

int nsk_solve_resident(nsk_handle h, int solver, double tol, int max_iter, int *iters, double *final_res) {
  NSK_TRY_DEV(h)
  const int rc = h->solve_resident(solver, tol, max_iter, iters, final_res);
  h->asmd.x_is_result = true;   // x_b is delta_owned until an assembly writes the next initial guess (nsk_assemble, P2/P1)
  h->asmd.sx_delta_valid = false;
  return rc;
  NSK_CATCH_ABORT(h)
}

int nsk_download_solution(nsk_handle h, double *xu, double *xp) {
  NSK_TRY_DEV(h)
  NSK_HIP(hipMemcpyAsync(xu, h->x_b, sizeof(double) * (size_t)h->n_u(), hipMemcpyDeviceToHost, h->s()));
  NSK_HIP(hipMemcpyAsync(xp, h->x_b + h->n_u(), sizeof(double) * (size_t)h->n_p(), hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_solve(nsk_handle h, int solver, double tol, int max_iter, const double *ru, const double *rp, double *xu,
              double *xp, int *iters, double *final_res) {
  int rc = nsk_upload_system(h, ru, rp, xu, xp);
  if (rc < 0) return rc;
  const int rs = nsk_solve_resident(h, solver, tol, max_iter, iters, final_res);
  if (rs < 0) return rs;
  rc = nsk_download_solution(h, xu, xp);
  return rc < 0 ? rc : rs;
}

int nsk_spmv(nsk_handle h, int b, const double *x, double *y, int add) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  if (b < 0 || b > NSK_BLK_S || !h->blk[b].present) throw Error(-62, "nsk_spmv: block not set");
  Csr &A = h->blk[b];
  const int rs = (b == NSK_BLK_F || b == NSK_BLK_BT) ? 0 : 1, cs = (b == NSK_BLK_F || b == NSK_BLK_B) ? 0 : 1;
  if (b == NSK_BLK_BT_GHOST) throw Error(-63, "nsk_spmv: ghost rows are not an operator");
  VecPool &pc = cs == 0 ? h->pool_u : h->pool_p, &pr = rs == 0 ? h->pool_u : h->pool_p;
  const Lease xv(pc, true), yv(pr, true);
  NSK_HIP(hipMemcpyAsync(xv, x, sizeof(double) * (size_t)pc.n, hipMemcpyHostToDevice, h->s()));
  if (add) NSK_HIP(hipMemcpyAsync(yv, y, sizeof(double) * (size_t)pr.n, hipMemcpyHostToDevice, h->s()));
  h->halo(cs, pc.view(xv));
  h->spmv_nohalo(A, pc.view(xv), yv, add ? 1 : 0);
  NSK_HIP(hipMemcpyAsync(y, yv, sizeof(double) * (size_t)pr.n, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_jacobian_vmult(nsk_handle h, const double *xu, const double *xp, double *yu, double *yp) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  const Lease xb(h->pool_b, true), yb(h->pool_b, true);
  NSK_HIP(hipMemcpyAsync(xb, xu, sizeof(double) * (size_t)h->n_u(), hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(xb + h->n_u(), xp, sizeof(double) * (size_t)h->n_p(), hipMemcpyHostToDevice, h->s()));
  h->jacobian_vmult(h->bb(xb), yb);
  NSK_HIP(hipMemcpyAsync(yu, yb, sizeof(double) * (size_t)h->n_u(), hipMemcpyDeviceToHost, h->s()));
  NSK_HIP(hipMemcpyAsync(yp, yb + h->n_u(), sizeof(double) * (size_t)h->n_p(), hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_dot(nsk_handle h, int n, const double *x, const double *y, double *dot_out, double *norm_out) {
  NSK_TRY_DEV(h)
  DBuf<double> dx, dy;
  dx.upload(x, (size_t)n, h->s());
  dy.upload(y, (size_t)n, h->s());
  const SlotLease sl(h->ctx, 4);
  h->ctx.dot(n, dx.p, dy.p, sl);
  h->ctx.norm2(n, dx.p, sl + 1);
  const double *r = h->ctx.read_slots(sl, 3);
  if (dot_out) *dot_out = r[0];
  if (norm_out) *norm_out = r[2];
  return 0;
  NSK_CATCH(h)
}

// One BLAS-1 operation of the path on caller vectors (a4: the TrilinosWrappers::MPI::Vector family as the solvers use
// it).  op: 0 copy y=x | 1 equ y=a x | 2 axpy y+=a x | 3 sadd y=c y+a x | 4 axpy2 y+=a x+c z | 5 scale y*=a | 6 mul y.*=d
// | 7 submul y-=d.*x | 8 sub_then_mul y=(y-x).*d | 9 recip y=1/d | 10 add_and_dot y+=a x, s=y.z | 11 y+=a x, s=y.y
int nsk_vec_op(nsk_handle h, int op, int n, double a, double c, const double *x, double *y, const double *z, const double *d,
               double *scalar_out) {
  NSK_TRY_DEV(h)
  if (n <= 0 || op < 0 || op > 11) throw Error(-50, "nsk_vec_op: bad arguments");
  DBuf<double> dx, dy, dz, dd;
  hipStream_t s = h->s();
  dx.upload(x, (size_t)n, s);
  dy.upload(y, (size_t)n, s);
  dz.upload(z, (size_t)n, s);
  dd.upload(d, (size_t)n, s);
  const SlotLease sl(h->ctx, 2);
  double sc = 0.0;
  switch (op) {
    case 0: vec_copy(s, n, dx.p, dy.p); break;
    case 1: vec_equ(s, n, sref(a), dx.p, dy.p); break;
    case 2: vec_axpy(s, n, sref(a), dx.p, dy.p); break;
    case 3: vec_sadd(s, n, sref(c), sref(a), dx.p, dy.p); break;
    case 4: vec_axpy2(s, n, sref(a), dx.p, sref(c), dz.p, dy.p); break;
    case 5: vec_scale(s, n, sref(a), dy.p); break;
    case 6: vec_mul(s, n, dd.p, dy.p); break;
    case 7: vec_submul(s, n, dd.p, dx.p, dy.p); break;
    case 8: vec_sub_then_mul(s, n, dx.p, dd.p, dy.p); break;
    case 9: vec_recip(s, n, dd.p, dy.p); break;
    case 10: h->ctx.axpy_dot(n, sref(a), dx.p, dy.p, dz.p, sl); sc = h->ctx.read_slots(sl, 1)[0]; break;
    default: h->ctx.axpy_norm2(n, sref(a), dx.p, dy.p, sl); sc = h->ctx.read_slots(sl, 1)[0]; break;
  }
  NSK_HIP(hipMemcpyAsync(y, dy.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
  h->ctx.sync();
  if (scalar_out) *scalar_out = sc;
  return 0;
  NSK_CATCH(h)
}

int nsk_tri_apply(nsk_handle h, int which, const double *b, double *x) {
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  TriSolve *T = which == NSK_TRI_VELOCITY ? &h->tF : h->tP;
  VecPool &p = which == NSK_TRI_VELOCITY ? h->pool_u : h->pool_p;
  const Lease bv(p, true), xv(p, true);
  NSK_HIP(hipMemcpyAsync(bv, b, sizeof(double) * (size_t)p.n, hipMemcpyHostToDevice, h->s()));
  if (which == NSK_TRI_VELOCITY && h->amg_active) { h->amg_ready(); h->amgF.apply(bv, xv); }  // the velocity preconditioner is the AMG
  else if (which != NSK_TRI_VELOCITY && h->schur_amg_active) h->amgS.apply(bv, xv);           // NSK_OPT_SCHUR_AMG: so is S's
  else T->apply(bv, xv);
  NSK_HIP(hipMemcpyAsync(x, xv, sizeof(double) * (size_t)p.n, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  h->check_sync_free();
  return 0;
  NSK_CATCH(h)
}

int nsk_amg_info(nsk_handle h, int shard, int level, int64_t *rows, int64_t *nnz, double *lambda_max) {
  NSK_TRY(h)
  if (h->amg_active) h->amg_ready();
  if (!h->amg_active || shard < 0 || shard >= (int)h->amgF.shards.size()) return 0;
  const int nl = h->amgF.n_levels(shard);
  if (level >= 0 && level < nl) {
    if (rows) *rows = h->amgF.level_rows(shard, level);
    if (nnz) *nnz = h->amgF.level_nnz(shard, level);
    if (lambda_max) *lambda_max = h->amgF.level_lambda(shard, level);
  }
  return nl;
  NSK_CATCH(h)
}

int nsk_amg_value_bytes(nsk_handle h, int32_t *bytes) {
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if (h->amg_active) h->amg_ready();
  *bytes = h->amg_active ? h->amgF.value_bytes() : 0;
  return 0;
  NSK_CATCH(h)
}

int nsk_schur_amg_info(nsk_handle h, int shard, int level, int64_t *rows, int64_t *nnz, double *lambda_max) {
  NSK_TRY(h)
  if (!h->schur_amg_active || shard < 0 || shard >= (int)h->amgS.shards.size()) return 0;
  const int nl = h->amgS.n_levels(shard);
  if (level >= 0 && level < nl) {
    if (rows) *rows = h->amgS.level_rows(shard, level);
    if (nnz) *nnz = h->amgS.level_nnz(shard, level);
    if (lambda_max) *lambda_max = h->amgS.level_lambda(shard, level);
  }
  return nl;
  NSK_CATCH(h)
}

int nsk_schur_amg_apply(nsk_handle h, const double *b, double *x) {
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if (!h->schur_amg_active) throw Error(-62, "nsk_schur_amg_apply: the current set-up has no AMG on S");
  const Lease bv(h->pool_p, true), xv(h->pool_p, true);
  NSK_HIP(hipMemcpyAsync(bv, b, sizeof(double) * (size_t)h->n_p(), hipMemcpyHostToDevice, h->s()));
  h->amgS.apply(bv, xv);
  NSK_HIP(hipMemcpyAsync(x, xv, sizeof(double) * (size_t)h->n_p(), hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_tri_get_value_bytes(nsk_handle h, int which, int32_t *bytes) {
  NSK_TRY(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if ((which == NSK_TRI_VELOCITY && h->amg_active) || (which != NSK_TRI_VELOCITY && h->schur_amg_active)) *bytes = 0;   // no triangular factor in this setup
  else *bytes = (which == NSK_TRI_VELOCITY ? &h->tF : h->tP)->value_bytes();
  return 0;
  NSK_CATCH(h)
}

int nsk_inner_value_bytes(nsk_handle h, int b, int32_t *bytes) {
  NSK_TRY(h)
  if (b != NSK_BLK_F && b != NSK_BLK_S && b != NSK_BLK_MP) throw Error(-62, "nsk_inner_value_bytes: F, S or M_p");
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  *bytes = !h->inner_solve_on(b) || (b == NSK_BLK_F && h->matfree_in_effect()) ? 0 : h->inner_width(h->blk[b]);
  return 0;
  NSK_CATCH(h)
}

int nsk_inner_basis_bytes(nsk_handle h, int32_t *bytes) {
  NSK_TRY(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  *bytes = h->inner_basis_width();
  return 0;
  NSK_CATCH(h)
}

int nsk_inner_spmv(nsk_handle h, int b, const double *x, double *y) {
  NSK_TRY_DEV(h)
  if (b != NSK_BLK_F && b != NSK_BLK_S && b != NSK_BLK_MP) throw Error(-62, "nsk_inner_spmv: F, S or M_p");
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if (!h->blk[b].present) throw Error(-62, "nsk_inner_spmv: block not set");
  const int space = b == NSK_BLK_F ? 0 : 1;
  VecPool &pool = space == 0 ? h->pool_u : h->pool_p;
  const Lease xv(pool, true), yv(pool, true);
  NSK_HIP(hipMemcpyAsync(xv, x, sizeof(double) * (size_t)pool.n, hipMemcpyHostToDevice, h->s()));
  h->spmv_halo(h->blk[b], space, pool.view(xv), yv);
  NSK_HIP(hipMemcpyAsync(y, yv, sizeof(double) * (size_t)pool.n, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH_ABORT(h)
}

int nsk_inner_matrix_free(nsk_handle h, int32_t *on) {
  NSK_TRY(h)
  *on = h->matfree_in_effect() ? 1 : 0;
  return 0;
  NSK_CATCH(h)
}

int nsk_matfree_f(nsk_handle h, const double *x, double *y) {
  NSK_TRY_DEV(h)
  h->matfree_check("nsk_matfree_f");
  const Lease xv(h->pool_u, true), yv(h->pool_u, true);
  NSK_HIP(hipMemcpyAsync(xv, x, sizeof(double) * (size_t)h->pool_u.n, hipMemcpyHostToDevice, h->s()));
  h->matfree_apply(h->pool_u.view(xv), yv);
  NSK_HIP(hipMemcpyAsync(y, yv, sizeof(double) * (size_t)h->pool_u.n, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_tri_get_perm(nsk_handle h, int which, int32_t *perm) {
  NSK_TRY(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  TriSolve *T = which == NSK_TRI_VELOCITY ? &h->tF : h->tP;
  if (which == NSK_TRI_VELOCITY && h->amg_active) {  // no triangular factor in this setup
    for (int i = 0; i < h->n_u(); ++i) perm[i] = i;
    return 0;
  }
  if (which != NSK_TRI_VELOCITY && h->schur_amg_active) {  // nor here: the V-cycle on S (NSK_OPT_SCHUR_AMG)
    for (int i = 0; i < h->n_p(); ++i) perm[i] = i;
    return 0;
  }
  for (int i = 0; i < T->n; ++i) perm[i] = T->perm.empty() ? i : T->perm[i];
  return 0;
  NSK_CATCH(h)
}

int nsk_precond_vmult(nsk_handle h, const double *su, const double *sp_, double *du, double *dp, int calls) {
  NSK_TRY_DEV(h)
  if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  const Lease sb(h->pool_b, true), db(h->pool_b, true);
  const size_t bu = sizeof(double) * (size_t)h->n_u(), bp = sizeof(double) * (size_t)h->n_p();
  NSK_HIP(hipMemcpyAsync(sb, su, bu, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(sb + h->n_u(), sp_, bp, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(db, du, bu, hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(db + h->n_u(), dp, bp, hipMemcpyHostToDevice, h->s()));
  int rc = 0;
  DVec d = h->bb(db);
  const DVec sv = h->bb(sb);
  try {
    for (int k = 0; k < calls; ++k) h->prec_vmult(d, sv);
  } catch (NoConvergence &e) {
    rc = e.code;
  }
  NSK_HIP(hipMemcpyAsync(du, db, bu, hipMemcpyDeviceToHost, h->s()));
  NSK_HIP(hipMemcpyAsync(dp, db + h->n_u(), bp, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  h->check_sync_free();
  return rc;
  NSK_CATCH_ABORT(h)
}

int64_t nsk_block_nnz(nsk_handle h, int b) {
  if (!h || b < 0 || b > NSK_BLK_S || !h->blk[b].present) return -1;
  return h->blk[b].nnz;
}

int nsk_get_block(nsk_handle h, int b, int32_t *rowptr, int32_t *col, double *val) {
  NSK_TRY_DEV(h)
  if (b < 0 || b > NSK_BLK_S || !h->blk[b].present) throw Error(-64, "nsk_get_block: block not set");
  Csr &A = h->blk[b];
  std::copy(A.h_rowptr.begin(), A.h_rowptr.end(), rowptr);
  std::copy(A.h_col.begin(), A.h_col.end(), col);
  NSK_HIP(hipMemcpyAsync(val, A.val.p, sizeof(double) * (size_t)A.nnz, hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_get_stats(nsk_handle h, nsk_stats *o) {
  NSK_TRY(h)
  const Stats &st = h->ctx.st;
  o->setup_ms = h->setup_ms;
  o->solve_ms = h->solve_ms;
  o->outer_iters = h->outer_iters;
  o->inner_u_its = h->inner_u;
  o->inner_p_its = h->inner_p;
  o->prec_applies = h->prec_applies;
  o->spmv_calls = st.spmv_calls;
  o->tri_applies = st.tri_applies;
  o->reductions = st.reductions;
  o->host_syncs = st.host_syncs;
  o->spmv_bytes = st.spmv_bytes;
  o->tri_bytes = st.tri_bytes;
  o->blas1_bytes = st.blas1_bytes;
  // (a factor of F an earlier set-up left behind is not this set-up's while a hierarchy holds the velocity slot: DESIGN 5x)
  const bool factor_u = h->tF_ok && !h->amg_active;
  o->n_colors_u = factor_u ? h->tF.n_colors : 0;
  o->n_levels_u = factor_u ? h->tF.n_levels_L : 0;
  o->n_colors_p = h->tP ? h->tP->n_colors : 0;
  o->n_levels_p = h->tP ? h->tP->n_levels_L : 0;
  o->nnz_s = h->blk[NSK_BLK_S].present ? h->blk[NSK_BLK_S].nnz : 0;
  o->sync_free_fallbacks = h->sync_free_fallbacks;
  o->cur_outer_iters = h->progress_step;
  o->cur_residual = h->progress_value;
  o->overlapped_spmvs = h->overlapped_spmvs;
  o->ring_applies = h->ctx.st.ring_applies;
  o->columns_skipped = st.columns_skipped;
  return 0;
  NSK_CATCH(h)
}

int nsk_abort_group(nsk_handle h) {   // callable from any thread
  if (!h) return -1;
  h->ctx.comm.abort_group();
  return 0;
}

int nsk_cancel(nsk_handle h) {   // callable from another thread while a solve runs on this handle
  if (!h) return -1;
  h->cancel = 1;
  return 0;
}

int nsk_get_history(nsk_handle h, double *out, int cap) {
  NSK_TRY(h)
  const int n = (int)h->history.size();
  for (int i = 0; i < std::min(n, cap); ++i) out[i] = h->history[(size_t)i];
  return n;
  NSK_CATCH(h)
}

int nsk_reset_stats(nsk_handle h) {
  NSK_TRY(h)
  h->ctx.st = Stats{};
  h->inner_u = h->inner_p = h->prec_applies = h->outer_iters = 0;
  h->overlapped_spmvs = 0;
  return 0;
  NSK_CATCH(h)
}

int nsk_profile_begin(nsk_handle h, int op, int max_samples) {
  NSK_TRY_DEV(h)
  if (max_samples < 1 || max_samples > 4096) throw Error(-66, "nsk_profile_begin: 1..4096 samples");
  h->sampler.add(op, max_samples);
  return 0;
  NSK_CATCH(h)
}

int nsk_profile_read(nsk_handle h, int op, double *avg_ms, int *n_samples, double *bytes, int64_t *n_calls,
                     double *bytes_format) {
  NSK_TRY_DEV(h)
  h->ctx.sync();
  EventSampler::Slot *S = h->sampler.find(op);
  if (!S) throw Error(-68, "nsk_profile_read: op was not being sampled");
  double tot = 0.0;
  for (int i = 0; i < S->used; ++i) {
    float ms = 0.f;
    NSK_HIP(hipEventElapsedTime(&ms, S->e0[i], S->e1[i]));
    tot += ms;
  }
  if (avg_ms) *avg_ms = S->used ? tot / S->used : 0.0;
  if (n_samples) *n_samples = S->used;
  if (n_calls) *n_calls = S->seen;
  if (bytes) {
    if (op >= 0 && op <= NSK_BLK_S) *bytes = (double)h->blk[op].spmv_bytes();
    else if (op == 20 && h->asimple_amg_active) *bytes = (double)h->amgF.apply_bytes();   // class 20 is the V-cycle on F then
    else if (op == 20) *bytes = (double)h->tF.apply_bytes();
    else if (op == 21 && h->schur_amg_active) *bytes = (double)h->amgS.apply_bytes();   // class 21 is the V-cycle on S then
    else if (op == 21 && h->tP) *bytes = (double)h->tP->apply_bytes();
    else *bytes = 0.0;
  }
  if (bytes_format) {   // what the storage format in use really holds (<= the CSR figure for the node-block copies)
    // (F, S, M_p with fp32 copies for the inner solves: the fp32 format — see nsk.h, NSK_OPT_INNER_MATRIX_PRECISION)
    if (op == NSK_BLK_F && h->matfree_in_effect()) *bytes_format = h->matfree_bytes();
    else if (op >= 0 && op <= NSK_BLK_S) *bytes_format = h->blk[op].format_bytes(h->form_of(h->blk[op], 0, true));
    else if (op == 20 && h->asimple_amg_active) *bytes_format = h->amgF.format_bytes();
    else if (op == 20) *bytes_format = h->tF.format_bytes();
    else if (op == 21 && h->schur_amg_active) *bytes_format = h->amgS.format_bytes();
    else if (op == 21 && h->tP) *bytes_format = h->tP->format_bytes();
    else *bytes_format = 0.0;
  }
  return 0;
  NSK_CATCH(h)
}

int nsk_profile_end(nsk_handle h) {
  NSK_TRY_DEV(h)
  h->ctx.sync();
  h->sampler.release();
  return 0;
  NSK_CATCH(h)
}

int nsk_time_op(nsk_handle h, int op, int reps, double *avg_ms, double *bytes) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  if (reps < 1) reps = 1;
  // everything this call borrows goes back on every way out: events, vectors (`held`: the operands an op takes on top
  // of the three block vectors), reduction slots.  The operands stay borrowed while the op is timed, so the operation
  // of NSK_IOPT_TIMEOP_BETWEEN gets vectors of its own (it used to be handed the timed op's x back): one or two more
  // pool vectors in that mode
  const Event e0, e1;
  const Lease xl(h->pool_b, true), yl(h->pool_b, true), zl(h->pool_b, true);
  double *const xb = xl, *const yb = yl, *const zb = zl;   // (the operations below capture plain pointers)
  std::vector<Lease> held;
  vec_set(h->s(), h->N(), xb, 1.0);
  vec_set(h->s(), h->N(), zb, 0.5);
  const SlotLease slots(h->ctx, 4);
  const int sl = slots;
  double by = 0.0;
  std::function<void()> f;
  if (op >= 0 && op <= NSK_BLK_S && op != NSK_BLK_BT_GHOST) {
    if (!h->blk[op].present) throw Error(-62, "nsk_time_op: block not set");
    Csr &A = h->blk[op];
    const int cs = (op == NSK_BLK_F || op == NSK_BLK_B) ? 0 : 1;
    // operand from the pool of its own space, as the inner solvers hand it over (owned | ghost contiguous, aligned)
    VecPool &pc = cs == 0 ? h->pool_u : h->pool_p;
    double *xs = held.emplace_back(pc, true);
    vec_set(h->s(), pc.n, xs, 1.0);
    const DVec xv = pc.view(xs);
    by = (double)A.spmv_bytes();
    f = [=, &A]() { h->halo(cs, xv); h->spmv_nohalo(A, xv, yb, 0); };
  } else if (op == 50 + NSK_BLK_F || op == 50 + NSK_BLK_MP || op == 50 + NSK_BLK_S) {
    // the inner solves' SpMV of that block, with the values and kernel they read (fp32 copy or double)
    const int b = op - 50;
    if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
    if (!h->blk[b].present) throw Error(-62, "nsk_time_op: block not set");
    Csr &A = h->blk[b];
    const int cs = b == NSK_BLK_F ? 0 : 1;
    VecPool &pc = cs == 0 ? h->pool_u : h->pool_p;
    double *xs = held.emplace_back(pc, true);
    vec_set(h->s(), pc.n, xs, 1.0);
    const DVec xv = pc.view(xs);
    by = b == NSK_BLK_F && h->matfree_in_effect() ? h->matfree_bytes() : A.format_bytes(h->form_of(A, 0, true));
    f = [=, &A]() { h->spmv_halo(A, cs, xv, yb); };
  } else if (op == 56) {
    // the matrix-free product with F on the state of the last assembly, whatever the option says (nsk_matfree_f)
    h->matfree_check("nsk_time_op");
    double *xs = held.emplace_back(h->pool_u, true);
    vec_set(h->s(), h->pool_u.n, xs, 1.0);
    const DVec xv = h->pool_u.view(xs);
    by = h->matfree_bytes();
    f = [=]() { h->matfree_apply(xv, yb); };
  } else if (op == 57) {
    // one V-cycle of the current set-up; bytes: what the stored formats hold for it (op 20: the algorithmic count)
    if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
    if (!h->amg_active) throw Error(-62, "nsk_time_op: the current set-up has no velocity AMG");
    h->amg_ready();
    by = h->amgF.format_bytes();
    f = [=]() { h->amgF.apply(xb, yb); };
  } else if (op == 10) {
    Csr &F = h->blk[NSK_BLK_F], &Bt = h->blk[NSK_BLK_BT], &B = h->blk[NSK_BLK_B];
    by = (double)F.spmv_bytes() + (double)Bt.spmv_bytes() + (double)B.spmv_bytes();
    f = [=]() { h->jacobian_vmult(h->bb(xb), yb); };
  } else if (op == 20 || op == 21) {
    if (h->prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
    TriSolve *T = op == 20 ? &h->tF : h->tP;
    if (op == 20 && h->amg_active) {  // the velocity preconditioner of this setup is the AMG V-cycle
      h->amg_ready();
      by = (double)h->amgF.apply_bytes();
      f = [=]() { h->amgF.apply(xb, yb); };
    } else if (op == 21 && h->schur_amg_active) {  // and the pressure one the V-cycle on S (NSK_OPT_SCHUR_AMG)
      by = (double)h->amgS.apply_bytes();
      f = [=]() { h->amgS.apply(xb, yb); };
    } else {
      by = (double)T->apply_bytes();
      f = [=]() { T->apply(xb, yb); };
    }
  } else if (op == 30) {
    by = 16.0 * h->N();
    f = [=]() { h->ctx.dot(h->N(), xb, zb, sl); };
  } else if (op == 31) {
    by = 24.0 * h->N();
    f = [=]() { vec_axpy(h->s(), h->N(), sref(1e-9), xb, zb); };
  } else if (op == 32) {
    by = 32.0 * h->N();
    f = [=]() { h->ctx.axpy_dot(h->N(), sref(1e-9), xb, zb, yb, sl); };
  } else if (op == 33 || op == 34) {
    // the fused Gram-Schmidt passes of the inner FGMRES on F: 8 basis vectors + w, velocity-sized, from the pool
    const int n = h->n_u();
    auto vs = std::make_shared<std::vector<double *>>();
    for (int k = 0; k < 9; ++k) {
      vs->push_back(held.emplace_back(h->pool_u, true));
      vec_set(h->s(), n, vs->back(), 1.0 / (k + 1));
    }
    const int cs = h->ctx.alloc_slots(10);
    by = op == 33 ? 8.0 * n * 9 : 8.0 * n * 10;
    f = [=]() {
      if (op == 33) h->ctx.multi_dot(n, (*vs)[8], vs->data(), 8, cs, true);
      else h->ctx.multi_axpy(n, (*vs)[8], vs->data(), 8, cs, -1);
    };
  } else if (op >= 35 && op <= 37) {
    // the same sweeps over a whole basis of 30 (Ctx::multi_dot_all / multi_axpy_all with the norm) and the cycle-end update
    // of 29 terms (Ctx::multi_add), as NSK_IOPT_GS_ONE_LAUNCH launches them; bytes: what the chosen form moves
    const int n = h->n_u(), m = op == 37 ? 29 : 30;
    auto vs = std::make_shared<std::vector<double *>>();
    for (int k = 0; k <= m; ++k) {
      vs->push_back(held.emplace_back(h->pool_u, true));
      vec_set(h->s(), n, vs->back(), 1.0 / (k + 1));
    }
    const int cs = h->ctx.alloc_slots(m + 2);
    NSK_HIP(hipMemsetAsync(h->ctx.slot(cs), 0, sizeof(double) * (m + 2), h->s()));   // (update: coefficients 0, w stays put)
    auto yz = std::make_shared<std::vector<double>>((size_t)m, 1e-9);
    f = [=]() {
      if (op == 35) h->ctx.multi_dot_all(n, (*vs)[m], vs->data(), m, cs);
      else if (op == 36) h->ctx.multi_axpy_all(n, (*vs)[m], vs->data(), m, cs, cs + m);
      else h->ctx.multi_add(n, (*vs)[m], vs->data(), yz->data(), m);
    };
    const double b0 = h->ctx.st.blas1_bytes;
    f();
    by = h->ctx.st.blas1_bytes - b0;
  } else if (op == 40 || op == 41) {
    // host round trip of one device scalar (what every Krylov iteration pays for its SolverControl check): wall time
    const double t0 = wall_ms();
    for (int r = 0; r < reps; ++r) {
      if (op == 41) h->ctx.dot(h->N(), xb, zb, sl);
      (void)h->ctx.read_slots(sl, 1);
    }
    if (avg_ms) *avg_ms = (wall_ms() - t0) / reps;
    if (bytes) *bytes = op == 41 ? 16.0 * h->N() : 0.0;
    return 0;
  } else {
    throw Error(-65, "nsk_time_op: unknown op");
  }
  f();  // warm-up
  float ms = 0.f;
  const int bw = h->timeop_between;
  if (bw >= 0 && bw <= NSK_BLK_S && bw != NSK_BLK_BT_GHOST && h->blk[bw].present) {
    // another kernel's SpMV between two repetitions, outside the brackets: one pair of events per repetition
    Csr &A = h->blk[bw];
    VecPool &pc = (bw == NSK_BLK_F || bw == NSK_BLK_B) ? h->pool_u : h->pool_p;
    VecPool &pr = (bw == NSK_BLK_F || bw == NSK_BLK_BT) ? h->pool_u : h->pool_p;
    const Lease xs(pc, true), ys(pr, true);
    vec_set(h->s(), pc.n, xs, 1.0);
    const DVec xv = pc.view(xs);
    for (int r = 0; r < reps; ++r) {
      h->spmv_nohalo(A, xv, ys, 0);
      NSK_HIP(hipEventRecord(e0, h->s()));
      f();
      NSK_HIP(hipEventRecord(e1, h->s()));
      NSK_HIP(hipEventSynchronize(e1));
      float one = 0.f;
      NSK_HIP(hipEventElapsedTime(&one, e0, e1));
      ms += one;
    }
  } else {
    NSK_HIP(hipEventRecord(e0, h->s()));
    for (int r = 0; r < reps; ++r) f();
    NSK_HIP(hipEventRecord(e1, h->s()));
    NSK_HIP(hipEventSynchronize(e1));
    NSK_HIP(hipEventElapsedTime(&ms, e0, e1));
  }
  if (avg_ms) *avg_ms = (double)ms / reps;
  if (bytes) *bytes = by;
  h->check_sync_free();
  return 0;
  NSK_CATCH(h)
}

}  // extern "C"
