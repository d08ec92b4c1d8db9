// nsk_precond.cpp — the block preconditioners of the path and the outer solve, on the handle of nsk_handle.hpp.
//
// Host-side mirror of
//   PreconditionBlockDiagonal   NSSolverStationary.hpp:115-167 | NSSolver.hpp:138-190
//   PreconditionBlockTriangular NSSolverStationary.hpp:170-238 | NSSolver.hpp:193-257
//   PreconditionaSIMPLE         NSSolverStationary.hpp:240-335 | NSSolver.hpp:259-384
//   solve_system()              NSSolverStationary.cpp:579-647 | NSSolver.cpp:601-672
// with every vector and matrix resident in HBM and all arithmetic in nsk_kernels.hip.
#include <algorithm>
#include <exception>
#include <thread>

#include <omp.h>
#include "nsk_handle.hpp"

// S pattern = structural product of B and [Bt ; Bt_ghost]  (EpetraExt MatrixMatrix::Multiply)
void H::schur_symbolic() {
  Csr &B = blk[NSK_BLK_B], &Bt = blk[NSK_BLK_BT], &Btg = blk[NSK_BLK_BT_GHOST], &S = blk[NSK_BLK_S];
  if (!Bt.present) throw Error(-41, "aSIMPLE needs block (0,1)");
  if (sp[0].ng > 0 && !Btg.present) throw Error(-42, "aSIMPLE on several ranks needs NSK_BLK_BT_GHOST");
  const int np = B.n_rows, ncols = sp[1].n + sp[1].ng;
  // One rank (no ghost columns): the structural product on the device, with the row-product kernels of the AMG set-up
  // (hash sets in LDS, rows sorted) — 0.73 s of host work at 1200x400 otherwise, the longest item of the first set-up
  // once the factors' analysis had moved to the device.  NSK_IOPT_HOST_ANALYSIS: the host loop.
  bool on_device = !tS.host_analysis && sp[0].ng == 0 && sp[1].ng == 0 && B.n_cols == Bt.n_rows && np > 0;
  DBuf<int> rp_d, col_d;
  int64_t nnz_s = 0;
  if (on_device) {
    try {
      nnz_s = device_product_pattern(&ctx, B, Bt, rp_d, col_d);
    } catch (const Error &e) {   // (a row with more than 512 distinct columns, say: the host loop below has no such limit)
      if (verbose()) fprintf(stderr, "[nsk] Schur pattern on the device: %s — host loop instead\n", e.what());
      on_device = false;
    }
  }
  if (on_device) {
    S.n_rows = np;
    S.n_cols = ncols;
    S.n_own_cols = sp[1].n;
    S.nnz = nnz_s;
    S.h_rowptr.resize((size_t)np + 1);
    S.h_col.resize((size_t)nnz_s);
    NSK_HIP(hipMemcpyAsync(S.h_rowptr.data(), rp_d.p, sizeof(int) * ((size_t)np + 1), hipMemcpyDeviceToHost, s()));
    NSK_HIP(hipMemcpyAsync(S.h_col.data(), col_d.p, sizeof(int) * (size_t)nnz_s, hipMemcpyDeviceToHost, s()));
    ctx.sync();
    s_max_row = 0;
    for (int i = 0; i < np; ++i) s_max_row = std::max(s_max_row, S.h_rowptr[i + 1] - S.h_rowptr[i]);
    if (s_max_row > 448) throw Error(-43, "Schur row too long for the LDS-staged SpGEMM kernel");
    S.rowptr = std::move(rp_d);
    S.col = std::move(col_d);
    S.col.n = (size_t)nnz_s;
    S.val.alloc((size_t)S.nnz);
    S.lpr = pick_lpr(S.nnz, S.n_rows);
    S.present = true;
    S.build_stream_plan(s());
    index16_for(S, "S");
    ctx.sync();
    s_symbolic = true;
    return;
  }
  std::vector<int> rp(np + 1, 0);
  std::vector<std::vector<int>> rows(np);
#pragma omp parallel
  {
    std::vector<int> mark(ncols, -1), cols;
#pragma omp for schedule(dynamic, 256)
    for (int i = 0; i < np; ++i) {
      cols.clear();
      for (int k = B.h_rowptr[i]; k < B.h_rowptr[i + 1]; ++k) {
        const int m = B.h_col[k];
        const Csr &R = m < B.n_own_cols ? Bt : Btg;
        const int mr = m < B.n_own_cols ? m : m - B.n_own_cols;
        for (int q = R.h_rowptr[mr]; q < R.h_rowptr[mr + 1]; ++q) {
          const int j = R.h_col[q];
          if (mark[j] != i) { mark[j] = i; cols.push_back(j); }
        }
      }
      std::sort(cols.begin(), cols.end());
      rows[i] = cols;
    }
  }
  s_max_row = 0;
  for (int i = 0; i < np; ++i) {
    rp[i + 1] = rp[i] + (int)rows[i].size();
    s_max_row = std::max(s_max_row, (int)rows[i].size());
  }
  if (s_max_row > 448) throw Error(-43, "Schur row too long for the LDS-staged SpGEMM kernel");
  S.n_rows = np;
  S.n_cols = ncols;
  S.n_own_cols = sp[1].n;
  S.nnz = rp[np];
  S.h_rowptr = rp;
  S.h_col.resize((size_t)S.nnz);
#pragma omp parallel for schedule(static)
  for (int i = 0; i < np; ++i) std::copy(rows[i].begin(), rows[i].end(), S.h_col.begin() + rp[i]);
  S.rowptr.upload(S.h_rowptr, s());
  S.col.upload(S.h_col, s());
  S.val.alloc((size_t)S.nnz);
  S.lpr = pick_lpr(S.nnz, S.n_rows);
  S.present = true;
  S.build_stream_plan(s());
  index16_for(S, "S");
  ctx.sync();
  s_symbolic = true;
}

void H::setup(int type, int variant_, double alpha_) {
  if (type < 0 || type > 2) throw Error(-44, "Invalid preconditioner type. Use 0: blockDiagonal, 1: blockTriangular, 2: aSIMPLE.");
  ensure_pools();
  drop_pending();   // a fresh preconditioner object: the application the last solve left over fed the old one's state
  ctx.ws.pairs = blas1_pairs < 0 ? (variant_ == 0) : blas1_pairs;   // NSK_OPT_BLAS1_PAIRS
  push_tri_options();
  // what this set-up takes of the options and their environment overrides (nsk_handle.hpp: resolve_setup)
  const SetupPlan plan = resolve_setup(req, setup_env(), type, variant_);
  // (numeric() reallocates the halves when the storage precision of the factors' off-diagonal values changes)
  tF.want_f32 = tS.want_f32 = tMp.want_f32 = plan.factor32;
  // working-vector layout of the blocked velocity factor: colour-ordered whenever it runs single-launch (its
  // per-level kernels only know the caller's order).  The scalar factors always solve on colour-ordered vectors.
  const int f_layout = (x_layout_mode != 0 && sync_free_mode == 2) ? 1 : 0;
  if (tF.x_layout != f_layout) { tF.x_layout = f_layout; tF_ok = false; }
  const double t0 = wall_ms();
  prec_type = type;
  variant = variant_;
  alpha = alpha_;
  const int key = ((((tri_ordering * 1000 + subdomains) * 2 + (xy(0) ? 1 : 0)) * 2 + (xy(1) ? 1 : 0)) * 100 + group_u * 10 + group_p) * 2 +
                  mass_ordering(type, variant_);
  setup_hierarchies(plan);
  setup_velocity_factor(plan, key);
  if (type == 2) setup_schur(plan, key);
  else setup_mass(plan, key);
  setup_f32_copies(plan);
  check_f32_overflow();
  // fp32 basis of the inner FGMRES on F: a set-up that does not want the vectors frees them
  basis32_wanted = plan.basis32;
  if (inner_basis_width() != 4) basis32_u.destroy();
  setup_ms = wall_ms() - t0;
}

// A set-up the device kernels of a hierarchy cannot finish (-80..-85: a row of a product over their 512 columns and its
// kin) leaves the ILU factor in charge; -48 and HIP errors are errors
static bool amg_kernels_gave_up(const Error &e) { return e.code <= -80 && e.code >= -85; }

// What the two hierarchies take of the plan; the one of F in stationary aSIMPLE is built here, with its fallback
void H::setup_hierarchies(const SetupPlan &plan) {
  Csr &F = blk[NSK_BLK_F];
  amg_active = plan.velocity_amg_wanted;
  amg_pending = false;
  asimple_amg_active = false;
  // (fp32 storage of the V-cycle's operators: the hierarchy converts when it is built, Amg::setup)
  amgF.value_bits = plan.amg_bits_F;
  amgF.use_bsr = use_bsr != 0;
  // level 0 on F's node blocks, and the smoother steps in those products' epilogues: this hierarchy alone
  amgF.blk_residual = plan.want_amgF;
  amgF.fused_cheby = plan.fused_cheby;
  if (plan.want_amgF) {
    // Built here and not on first use: it can fail, and ILU(F) must then still be possible — said once per handle
    Phase ph("AMG hierarchy of F (device)");
    try {
      amgF.setup(&ctx, F, sub_offsets(0));
      amg_active = asimple_amg_active = true;
    } catch (const Error &e) {
      amgF.release();
      F.amg32 = 0;
      amgF.blk_residual = amgF.fused_cheby = false;
      amgF.value_bits = 64;
      if (!amg_kernels_gave_up(e)) { prec_type = -1; throw; }
      if (!asimple_amg_warned) {
        asimple_amg_warned = true;
        fprintf(stderr, "[nsk] warning: NSK_OPT_ASIMPLE_VELOCITY_AMG = 1, but the hierarchy of F cannot be built (%s): ILU(F) preconditions the inner FGMRES on F\n",
                e.what());
      }
    }
    if (asimple_amg_active) drop_velocity_factor();
  }
  // S's hierarchy is built where S is formed (setup_schur); a set-up that does not want it frees it here, before the
  // velocity factor takes its storage
  schur_amg_active = false;
  amgS.value_bits = plan.amg_bits_S;
  amgS.use_bsr = false;
  amgS.one_sign_diag = true;
  if (!plan.want_amgS) amgS.release();
}

// "Analyse a factor unless it is analysed under this key": true when `analyse` ran
template <class Analyse>
static bool analyse_unless_held(bool &ok, int &held, int key, Analyse analyse) {
  if (ok && held == key) return false;
  analyse();
  ok = true;
  held = key;
  return true;
}

void H::analyse_S() { tS.analyze(&ctx, blk[NSK_BLK_S], 0, tri_ordering, sub_offsets(1), false, xy(1), group_p); }

// The velocity slot: the hierarchy that stands, the one built on first use, or ILU(F) / SGS(F) analysed and factorised
void H::setup_velocity_factor(const SetupPlan &plan, int key) {
  // (asimple_amg_active: the hierarchy stands; no factor of F.  S's pattern and factor, where ILU(S) is wanted, are formed
  // in setup_schur on this thread: the side thread exists to overlap F's analysis, of which there is none)
  if (asimple_amg_active) return;
  // F's analysis is on 2 x 2 node blocks or scalar by NSK_OPT_BSR_VELOCITY: its key holds that bit as well
  const int key_F = key * 2 + (use_bsr ? 1 : 0);
  if (amg_active) {
    amgF.clear();
    amg_pending = true;
    return;
  }
  amgF.release();
  Csr &F = blk[NSK_BLK_F];
  // First aSIMPLE set-up of a pattern: the Schur pattern and the analysis of its factor need nothing of F's analysis —
  // a second host thread does them meanwhile (both are host-side integer work with serial stretches: 1.7 s next to
  // 3.3 s at 1200x400 instead of behind them)
  std::thread side;
  std::exception_ptr side_err;
  bool side_done_s = false;
  // (not under NSK_OPT_SCHUR_AMG: S's factor is not analysed then, and the pattern is formed in setup_schur)
  if (prec_type == 2 && !plan.want_amgS && (!tF_ok || tF_key != key_F) && (!tS_ok || tS_key != key)) {
    side = std::thread([&] {
      try {
        (void)hipSetDevice(ctx.device);
        if (!s_symbolic) {
          Phase ph("Schur pattern (host, side thread)");
          schur_symbolic();
        }
        Phase ph("analyse S factor (host, side thread)");
        analyse_S();
        side_done_s = true;
      } catch (...) {
        side_err = std::current_exception();
      }
    });
  }
  struct Joiner {   // (F's analysis may throw: never leave the scope with the thread running)
    std::thread &t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{side};
  analyse_unless_held(tF_ok, tF_key, key_F, [&] {
    Phase ph("analyse F factor (host)");
    tF.analyze(&ctx, F, plan.kindF, tri_ordering, sub_offsets(0), use_bsr && F.blk_ok && F.blk_R == 2 && F.blk_C == 2, xy(0),
               group_u);
  });
  tF.kind = plan.kindF;
  if (side.joinable()) side.join();
  if (side_err) std::rethrow_exception(side_err);
  if (side_done_s) { tS_ok = true; tS_key = key; }   // (written here, on the calling thread, after the join)
  Phase ph("factorise F (device)");
  tF.numeric(F.val.p);
  if (verbose()) ctx.sync();
}

// aSIMPLE: S = B D^-1 Bt formed, and its preconditioner — the V-cycle of amgS, or ILU(S)
void H::setup_schur(const SetupPlan &plan, int key) {
  Csr &F = blk[NSK_BLK_F], &S = blk[NSK_BLK_S], &B = blk[NSK_BLK_B], &Bt = blk[NSK_BLK_BT], &Btg = blk[NSK_BLK_BT_GHOST];
  if (!s_symbolic) {
    Phase ph("Schur pattern (host)");
    schur_symbolic();
  }
  if (!D) { D = pool_u.get(true); Dinv = pool_u.get(true); tmp_u = pool_u.get(true); }
  if (!tmp_p) tmp_p = pool_p.get(true);
  if (!delta_p) delta_p = pool_p.get(true);
  if (!tmp_b) tmp_b = pool_b.get(true);
  // D = diag(F), D^-1 (NSSolverStationary.hpp:259-264); ghosts of D^-1 feed the SpGEMM
  extract_diag(s(), F.view(), D, Dinv);
  halo(0, pool_u.view(Dinv));
  spgemm_bdbt_numeric(s(), B.view(), Dinv, Dinv + n_u(), Bt.view(), Btg.present ? Btg.view() : Bt.view(), S.rowptr.p,
                      S.col.p, S.val.p, S.n_rows, std::max(1, s_max_row));
  if (schur_sign < 0) vec_scale(s(), (int)S.nnz, sref(-1.0), S.val.p);   // opt-in deviation (nsk.h: NSK_OPT_SCHUR_SIGN)
  ++S.values_version;
  tP = nullptr;
  if (plan.want_amgS) setup_schur_hierarchy();
  if (!schur_amg_active) {
    analyse_unless_held(tS_ok, tS_key, key, [&] {
      Phase ph("analyse S factor (host)");
      analyse_S();
    });
    tS.kind = 0;
    tS.numeric(S.val.p);
    tP = &tS;
  }
  // delta_p.reinit(...) in initialize(): zero
  vec_set(s(), n_p(), delta_p, 0.0);
}

// S changes with every set-up: the hierarchy is rebuilt every time, in the set-up and not on first use (the CG on S runs
// in every application).  A set-up the device kernels cannot finish — a row of a product over their 512 columns, a
// diagonal of S that is not of one sign — leaves ILU(S) in charge, said once per handle
void H::setup_schur_hierarchy() {
  Csr &S = blk[NSK_BLK_S];
  Phase ph("AMG hierarchy of S (device)");
  try {
    amgS.setup(&ctx, S, sub_offsets(1));
    schur_amg_active = true;
  } catch (const Error &e) {
    amgS.release();
    S.amg32 = 0;
    if (!amg_kernels_gave_up(e)) throw;
    if (!schur_amg_warned) {
      schur_amg_warned = true;
      fprintf(stderr, "[nsk] warning: NSK_OPT_SCHUR_AMG = 1, but the hierarchy of S cannot be built (%s): ILU(S) preconditions the inner CG on S\n",
              e.what());
    }
  }
}

// The block preconditioners: the factor of M_p, kept while neither its values nor its analysis change
void H::setup_mass(const SetupPlan &plan, int key) {
  Csr &Mp = blk[NSK_BLK_MP];
  if (!Mp.present) throw Error(-45, "this preconditioner needs pressure_mass.block(1,1)");
  const bool analysed = analyse_unless_held(tMp_ok, tMp_key, key, [&] {
    tMp.analyze(&ctx, Mp, plan.kindP, mass_ordering(prec_type, variant), sub_offsets(1), false, xy(1), group_p);
  });
  if (analysed) mp_factored_version = -1;
  tMp.kind = plan.kindP;
  if (mp_factored_version != mp_values_version || mp_factored_kind != plan.kindP || tMp.storage_stale()) {
    Phase ph("factorise Mp (device)");
    tMp.numeric(Mp.val.p);
    mp_factored_version = mp_values_version;
    mp_factored_kind = plan.kindP;
  }
  tP = &tMp;
  if (!tmp_p) tmp_p = pool_p.get(true);
}

// fp32 values of the inner solves' matrices.  A block without an inner solve in this set-up, or whose SpMV would not take
// a stream kernel, keeps no copy (and 64 frees them all).
void H::setup_f32_copies(const SetupPlan &plan) {
  matfree_wanted = plan.matfree;
  for (int b : {(int)NSK_BLK_F, (int)NSK_BLK_MP, (int)NSK_BLK_S}) {
    Csr &A = blk[b];
    // (F while its products are matrix-free: no stored value is read, so no copy is made)
    const bool wanted = plan.inner32 && A.present && inner_solve_on(b) && !(b == NSK_BLK_F && matfree_in_effect());
    // the copy this block would hold: F's 2 x 2 blocks (the only shape build_blocked gives F, and the only one of the
    // blocked fp32 kernel), else the scalar values — kept where the rule gives the inner product an _f32 form for it
    A.inner32 = !wanted ? 0 : b == NSK_BLK_F ? 1 : 2;
    if (!is_f32(form_of(A, 0, true))) A.inner32 = 0;
    // (F's copies may also serve the V-cycle, level 0 being F itself: Amg::setup names them in amg32 when the hierarchy is
    // built and this loop leaves them alone meanwhile; without an fp32 AMG in this set-up nothing of it remains)
    // (S the same way under NSK_OPT_SCHUR_AMG, where amgS.setup has named its copy already)
    if (!(b == NSK_BLK_F && amgF.value_bits == 32) && !(b == NSK_BLK_S && schur_amg_active && amgS.value_bits == 32)) A.amg32 = 0;
    if (!A.inner32 && !A.amg32) { A.release_f32(); continue; }
    if (A.inner32) A.refresh_f32(s(), true);
  }
  ctx.sync();
}

// A value outside the range of fp32 in a copy just made: error -48, and no preconditioner
void H::check_f32_overflow() {
  for (int b : {(int)NSK_BLK_F, (int)NSK_BLK_MP, (int)NSK_BLK_S}) {
    Csr &A = blk[b];
    if (!A.inner32) continue;
    unsigned over = 0;
    NSK_HIP(hipMemcpy(&over, A.f32_overflow.p, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (over) {
      for (Csr *c : {&blk[NSK_BLK_F], &blk[NSK_BLK_MP], &blk[NSK_BLK_S]}) c->release_f32();
      amgF.clear();
      amgS.clear();
      schur_amg_active = false;
      if (asimple_amg_active) amg_active = asimple_amg_active = false;   // (the hierarchy of DESIGN 5v: cleared with the rest)
      amg_pending = false;
      prec_type = -1;  // no preconditioner: call nsk_setup_preconditioner again (e.g. with the option at 64)
      static const char *names[6] = {"F (block 0,0)", "Bt", "B", "M_p (pressure mass)", "Bt ghost rows", "S (Schur approximation)"};
      throw Error(-48, std::string("NSK_OPT_INNER_MATRIX_PRECISION = 32: ") + std::to_string(over) + " value(s) of " +
                           names[b] + " are finite in fp64 but outside the range of fp32");
    }
  }
}

void H::prec_vmult(DVec &dst, const DVec &src) {
  if (pending.v) {
    // the application the last solve did not need: this one starts from the state it leaves (counted as work done)
    const SolverFGMRES::Pending p = pending;
    pending = SolverFGMRES::Pending{};
    const Lease z = Lease::adopt(pool_b, p.z), v = Lease::adopt(pool_b, p.v);
    DVec pz = bb(p.z);
    prec_vmult(pz, bb(p.v));
  }
  ++prec_applies;
  Csr &F = blk[NSK_BLK_F], &B = blk[NSK_BLK_B], &Bt = blk[NSK_BLK_BT];
  DVec du = ub(dst.own), dp = pb(dst.own);
  const DVec su = ub(src.own), spv = pb(src.own);
  const int nu = n_u(), np = n_p();
  MatVec A_F = [&](const DVec &x, double *y) { spmv_halo(F, 0, x, y); };
  PrecVmult P_F = [&](DVec &d, const DVec &r) {
    if (asimple_amg_active) { amg_ready(); velocity_apply_sampled(r.own, d.own); }   // (class 20 is the cycle on F then)
    else if (amg_active) { amg_ready(); amgF.apply(r.own, d.own); }
    else tri_apply_sampled(tF, 20, r.own, d.own);
  };
  PrecVmult P_P = [&](DVec &d, const DVec &r) { pressure_apply_sampled(r.own, d.own); };
  const SlotLease sl(ctx, 4);
  auto norm_of = [&](const double *v, int n) { ctx.norm2(n, v, sl); return ctx.read_slots(sl + 1, 1)[0]; };

  if (prec_type == 0 || prec_type == 1) {
    Csr &Mp = blk[NSK_BLK_MP];
    MatVec A_M = [&](const DVec &x, double *y) { spmv_halo(Mp, 1, x, y); };
    int max_u, max_p;
    double tol_u, tol_p;
    if (prec_type == 0) {
      if (variant == 0) { max_u = 100001; max_p = 100000; tol_u = 1e-1 * norm_of(su.own, nu); tol_p = 1e-1 * norm_of(spv.own, np); }
      else { max_u = max_p = 1000; tol_u = tol_p = 1e-1; }
    } else {
      if (variant == 0) { max_u = 10000001; max_p = 100000; tol_u = 1e-2 * norm_of(su.own, nu); tol_p = 1e-2 * norm_of(spv.own, np); }
      else { max_u = 2000001; max_p = 2000000; tol_u = 1e-4 * norm_of(su.own, nu); tol_p = 1e-5 * norm_of(spv.own, np); }
    }
    SolverControl cu(max_u, tol_u), cp(max_p, tol_p);
    try {
      SolverFGMRES sv(ctx, pool_u, cu);
      inner_fgmres_options(sv);
      sv.solve(A_F, du, su, P_F);
      inner_u += cu.last_step();
      if (prec_type == 0) {
        SolverCG sc(ctx, pool_p, cp);
        sc.fused = cg_fused;
        sc.solve(A_M, dp, spv, P_P);
      } else {
        // tmp.reinit; B->vmult(tmp, dst_u); tmp.sadd(-1, src_p)  =>  tmp = src_p - B u
        halo(0, du);
        spmv_nohalo(B, du, tmp_p, 2, spv.own);
        DVec tp = pool_p.view(tmp_p);
        SolverCG sc(ctx, pool_p, cp);
        sc.fused = cg_fused;
        sc.solve(A_M, dp, tp, P_P);
      }
      inner_p += cp.last_step();
    } catch (NoConvergence &e) {
      throw NoConvergence(3, e.last_step, e.last_residual);
    }
    return;
  }
  if (variant == 0) {
    // stationary aSIMPLE (NSSolverStationary.hpp:282-311)
    Csr &S = blk[NSK_BLK_S];
    MatVec A_S = [&](const DVec &x, double *y) { spmv_halo(S, 1, x, y); };
    try {
      SolverControl cF(100000, 1e-1 * norm_of(su.own, nu));
      SolverFGMRES sF(ctx, pool_u, cF);
      inner_fgmres_options(sF);
      sF.solve(A_F, du, su, P_F);                       // F u~ = src_u
      inner_u += cF.last_step();
      halo(0, du);
      spmv_nohalo(B, du, tmp_p, 2, spv.own);             // tmp_p = src_p - B u~
      SolverControl cS(100000, 1e-1 * norm_of(tmp_p, np));
      SolverCG sS(ctx, pool_p, cS);
      sS.fused = cg_fused;
      DVec dlt = pool_p.view(delta_p), tp = pool_p.view(tmp_p);
      sS.solve(A_S, dlt, tp, P_P);                      // S delta_p = tmp_p, stale delta_p as start
      inner_p += cS.last_step();
    } catch (NoConvergence &e) {
      throw NoConvergence(3, e.last_step, e.last_residual);
    }
    vec_scale(s(), np, sref(alpha), delta_p);           // delta_p *= alpha
    DVec dlt = pool_p.view(delta_p);
    halo(1, dlt);
    spmv_nohalo(Bt, dlt, tmp_u, 0);                      // tmp_u = B^T delta_p
    vec_submul(s(), nu, Dinv, tmp_u, du.own);            // u = u~ - D^-1 tmp_u
    vec_copy(s(), np, delta_p, dp.own);
    return;
  }
  // unsteady aSIMPLE (NSSolver.hpp:294-350): ILU applies only
  tri_apply_sampled(tF, 20, su.own, du.own);
  halo(0, du);
  spmv_nohalo(B, du, tmp_p, 1, spv.own);                 // tmp_p = src_p + B~ u   (vmult_add)
  tri_apply_sampled(*tP, 21, tmp_p, dp.own);
  vec_scale(s(), np, sref(1.0 / alpha), dp.own);         // p /= alpha
  halo(1, dp);
  Csr &BT = Bt;
  if (BT.blk_ok && use_stream && use_bsr && BT.blk_R == 2 && BT.blk_C == 1) {
    // u .*= D ; u = (u - B~^T p) .* D^-1 in the epilogue of the B~^T product (same roundings, two passes fewer)
    nsk::spmv_blk_stream(s(), BT.blk_view(), 2, 1, BT.blk_rowblk.p, BT.blk_nblk, dp.own, dp.ghost, du.own, D, Dinv);
    ++ctx.st.spmv_calls;
    ctx.st.spmv_bytes += (double)BT.spmv_bytes() + 24.0 * nu;
  } else {
    vec_mul(s(), nu, D, du.own);                         // u .*= D
    spmv_nohalo(Bt, dp, tmp_u, 0);
    vec_sub_then_mul(s(), nu, tmp_u, Dinv, du.own);      // u = (u - B~^T p) .* D^-1
  }
}

int H::solve_once(int solver, double tol, int max_iter, int *iters, double *final_res) {
  SolverControl control(max_iter, tol);
  control.progress_step = &progress_step;
  control.progress_value = &progress_value;
  history.clear();
  control.history = &history;
  control.cancel = &cancel;
  MatVec A = [&](const DVec &x, double *y) { jacobian_vmult(x, y); };
  PrecVmult P = [&](DVec &d, const DVec &r) { prec_vmult(d, r); };
  DVec x = bb(x_b);
  const DVec b = bb(rhs_b);
  int rc = 0;
  const int slot_mark = ctx.slot_top;
  SolverFGMRES::Pending left_over;   // (handed over only where the solve ends at a check: never together with an older one)
  struct Keep {
    H &h; SolverFGMRES::Pending &p;
    ~Keep() { if (p.v) { h.drop_pending(); h.pending = p; } }
  } keep{*this, left_over};
  try {
    if (solver == 0) { SolverGMRES sv(ctx, pool_b, control); sv.solve(A, x, b, P); }
    else if (solver == 1) {
      SolverFGMRES sv(ctx, pool_b, control);
      sv.fused_gs = outer_fused_gs ? 1 : 0;
      if (skip_unused) {
        // unsteady aSIMPLE is two triangular applies that overwrite dst.  The block preconditioners start their inner
        // solves from dst and keep nothing else: the application at a cycle's end feeds the next cycle's z_j, the one at
        // the solve's end nothing (z_j goes back to the pool).  Stationary aSIMPLE also keeps delta_p: see `pending`
        const bool asimple = prec_type == 2;
        sv.skip_unused = asimple && variant != 0 ? SolverFGMRES::stateless : SolverFGMRES::defer;
        if (asimple && variant == 0) sv.pending = &left_over;
      }
      sv.solve(A, x, b, P);
    }
    else { SolverBicgstab sv(ctx, pool_b, control); sv.solve(A, x, b, P); }
  } catch (NoConvergence &e) {
    rc = e.code;
  }
  ctx.slot_top = slot_mark;
  ctx.sync();
  check_sync_free();
  outer_iters += control.last_step();
  if (iters) *iters = control.last_step();
  if (final_res) *final_res = control.last_value();
  return rc;
}

// The single-launch triangular solves wait in-kernel with bounded spins.  If a wait ever gives up (error -70: e.g.
// another process holds part of the GPU, so not all workgroups of the persistent launch are resident), the solve is
// redone from the caller's initial guess with one launch per colour and a fresh preconditioner object (stale inner
// state must not leak).  The error is agreed on by all ranks (check_sync_free), so every rank retries.
int H::solve_resident(int solver, double tol, int max_iter, int *iters, double *final_res) {
  if (prec_type < 0) throw Error(-46, "call nsk_setup_preconditioner first");
  if (solver < 0 || solver > 2) throw Error(-47, "Invalid solver type. Use 0: GMRES, 1: FGMRES, 2: Bicgstab.");
  const double t0 = wall_ms();
  lazy_setup_ms = 0;
  cancel = 0;
  const bool guarded = sync_free_mode > 0;
  if (guarded) {   // keep the initial guess: a failed attempt leaves garbage in x_b
    if (!x_keep) x_keep = pool_b.get(false);
    vec_copy(s(), N(), x_b, x_keep);
  }
  int rc;
  try {
    rc = solve_once(solver, tol, max_iter, iters, final_res);
  } catch (const Error &e) {
    if (e.code != -70 || !guarded) throw;
    const long undo = outer_iters;
    sync_free_mode = 0;   // (setup() below pushes it into the factors)
    ++sync_free_fallbacks;
    ctx.warn("single-launch triangular solve: a producer/consumer wait ran out of spins (workgroups not resident in "
             "dispatch order: another process on the GPU?); the solve is redone from the caller's initial guess with one "
             "launch per colour — factors re-ordered WITHOUT line groups, which only the single-launch kernels know — and "
             "this handle keeps that slower path (NSK_OPT_TRI_SYNC_FREE = 0)");
    setup(prec_type, variant, alpha);
    vec_copy(s(), N(), x_keep, x_b);
    outer_iters = undo;
    rc = solve_once(solver, tol, max_iter, iters, final_res);
  }
  solve_ms = wall_ms() - t0 - lazy_setup_ms;
  return rc;
}
