// nsk_handle.hpp — the handle behind include/nsk.h (struct nsk_handle_s), the timing helpers it uses and the macros every
// entry point opens and closes with; in front of the handle, what a set-up takes of its options: the one reader of their
// environment overrides (setup_env) and the resolver (resolve_setup).  Included by the four files that implement the handle
// and the C ABI:
//   nsk_precond.cpp        the block preconditioners and the outer solve (H::setup, H::prec_vmult, H::solve_*)
//   nsk_capi.cpp           the public ABI of include/nsk.h
//   nsk_capi_assembly.cpp  its device-assembly group (nsk_assembly_*, nsk_state_*, nsk_assemble, nsk_forces*, nsk_record_*)
//   nsk_debug.cpp          the test hooks of nsk_internal.h
#pragma once
#include <chrono>
#include <exception>
#include <string>
#include <vector>

#include "../../include/nsk.h"
#include "nsk_solver.hpp"
#include "nsk_amg.hpp"
#include "nsk_assembly.hpp"
#include "nsk_tri.hpp"

using namespace nsk;   // (the handle is a global C type; its members are written in the library's names)

inline double wall_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// NSK_VERBOSE=1: one stderr line per host-side phase of a hand-off / set-up (where the seconds of a large mesh go)
inline bool verbose() {
  static const bool v = getenv("NSK_VERBOSE") && atoi(getenv("NSK_VERBOSE")) > 0;
  return v;
}
struct Phase {
  const char *name;
  double t0;
  explicit Phase(const char *n) : name(n), t0(wall_ms()) {}
  ~Phase() {
    if (verbose()) fprintf(stderr, "[nsk] %-34s %9.1f ms\n", name, wall_ms() - t0);
  }
};

// HIP-event sampler: brackets launches of up to four operation classes inside a running solve
struct EventSampler {
  struct Slot {
    int op = -1, cap = 0, used = 0;
    long seen = 0;  // every call of the op while sampling is on, also beyond the cap
    std::vector<hipEvent_t> e0, e1;
  };
  Slot slots[4];
  int n = 0;
  void add(int op, int cap) {
    if (n >= 4) throw Error(-67, "profile: at most four ops");
    Slot &S = slots[n++];
    S.op = op;
    S.cap = cap;
    S.used = 0;
    S.e0.resize(cap);
    S.e1.resize(cap);
    for (int i = 0; i < cap; ++i) { (void)hipEventCreate(&S.e0[i]); (void)hipEventCreate(&S.e1[i]); }
  }
  Slot *want(int o) {
    for (int k = 0; k < n; ++k)
      if (slots[k].op == o) {
        ++slots[k].seen;
        return slots[k].used < slots[k].cap ? &slots[k] : nullptr;
      }
    return nullptr;
  }
  Slot *find(int o) {
    for (int k = 0; k < n; ++k)
      if (slots[k].op == o) return &slots[k];
    return nullptr;
  }
  void release() {
    for (int k = 0; k < n; ++k) {
      for (size_t i = 0; i < slots[k].e0.size(); ++i) { (void)hipEventDestroy(slots[k].e0[i]); (void)hipEventDestroy(slots[k].e1[i]); }
      slots[k] = Slot{};
    }
    n = 0;
  }
};

// One sampled operation: e0 when the scope opens, e1 (and the sample counted) when it closes; nothing while `op` is not
// being sampled or its samples are used up
struct Sampled {
  EventSampler::Slot *smp;
  hipStream_t s;
  Sampled(EventSampler &es, int op, hipStream_t st) : smp(es.want(op)), s(st) {
    if (smp) (void)hipEventRecord(smp->e0[smp->used], s);
  }
  Sampled(const Sampled &) = delete;
  ~Sampled() {
    if (smp) (void)hipEventRecord(smp->e1[smp->used++], s);
  }
};
struct Event {   // a timing event of one scope
  hipEvent_t e = nullptr;
  Event() { NSK_HIP(hipEventCreate(&e)); }
  Event(const Event &) = delete;
  ~Event() { (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

// Row runs of the fused velocity block row y_u = F x_u + Bt x_p: the cap bounds both matrices' entries together
// (jacobian_vmult; the test hook nsk_debug_spmv builds its two-matrix plans with the same calls)
inline bool fused_blk_plan(const Csr &F, const Csr &Bt, std::vector<int> &rb) {
  return build_rowblocks(F.h_blk_rowptr.data(), Bt.h_blk_rowptr.data(), F.blk_rows, kBlkMax, nullptr, rb);
}
inline bool fused_row_plan(const Csr &F, const Csr &Bt, std::vector<int> &rb) {
  return build_rowblocks(F.h_rowptr.data(), Bt.h_rowptr.data(), F.n_rows, kStreamNnz, nullptr, rb);
}

// ================================================================== what a set-up takes of the options and the environment
// The environment overrides of the set-up's options (A/B runs with unchanged callers): two parsers of the text alone.
// Precision: atoi, 32 or 64 give that value, anything else — no text included — 0, "unset"
inline int parse_env_precision(const char *e) {
  const int v = e ? std::atoi(e) : 0;
  return v == 32 || v == 64 ? v : 0;
}
// Switch: exactly "0" or "1"; anything else — no text included — -1, "unset"
inline int parse_env_switch(const char *e) {
  if (e && e[0] == '0' && !e[1]) return 0;
  if (e && e[0] == '1' && !e[1]) return 1;
  return -1;
}
struct SetupEnv {
  int factor_precision, inner_matrix_precision, inner_basis_precision, amg_precision;   // 0 unset, 32, 64
  int matrix_free_f, schur_amg, asimple_velocity_amg, amg_fused_cheby;                  // -1 unset, 0, 1
};
// The only reader of these eight variables: once per process (a function-local static: rank threads set up concurrently)
inline const SetupEnv &setup_env() {
  static const SetupEnv env = {parse_env_precision(std::getenv("NSK_FACTOR_PRECISION")),
                               parse_env_precision(std::getenv("NSK_INNER_MATRIX_PRECISION")),
                               parse_env_precision(std::getenv("NSK_INNER_BASIS_PRECISION")),
                               parse_env_precision(std::getenv("NSK_AMG_PRECISION")),
                               parse_env_switch(std::getenv("NSK_INNER_MATRIX_FREE_F")),
                               parse_env_switch(std::getenv("NSK_SCHUR_AMG")),
                               parse_env_switch(std::getenv("NSK_ASIMPLE_VELOCITY_AMG")),
                               parse_env_switch(std::getenv("NSK_AMG_FUSED_CHEBY"))};
  return env;
}
// What the caller asked for (nsk_set_option writes here); the first eight in SetupEnv's order
struct SetupRequest {
  int factor_precision = 64;         // NSK_OPT_FACTOR_PRECISION: 64, or 32 (single-precision off-diagonal values of the split halves)
  int inner_matrix_precision = 64;   // NSK_OPT_INNER_MATRIX_PRECISION: 64, or 32 (fp32 values of F, S, M_p in the inner solves)
  int inner_basis_precision = 64;    // NSK_OPT_INNER_BASIS_PRECISION: 64, or 32 (fp32 Krylov basis of the inner FGMRES on F)
  int amg_precision = 64;            // NSK_OPT_AMG_PRECISION: 64, or 32 (fp32 values of the V-cycle's A, P, R on every level)
  int matrix_free_f = 0;             // NSK_OPT_INNER_MATRIX_FREE_F
  int schur_amg = 0;                 // NSK_OPT_SCHUR_AMG
  int asimple_velocity_amg = 0;      // NSK_OPT_ASIMPLE_VELOCITY_AMG
  int amg_fused_cheby = -1;          // NSK_IOPT_AMG_FUSED_CHEBY: -1 fused smoother steps where that hierarchy allows them, 0, 1
  int velocity_amg = 1;              // NSK_OPT_VELOCITY_AMG
};
// What one set-up of (type, variant) takes of the two: an override that is set wins, one that is unset leaves the option
struct SetupPlan {
  bool factor32;              // fp32 off-diagonal values of the three factors
  int amg_bits_F;             // 32 only where this set-up wants a hierarchy of F and the precision resolves to 32
  bool want_amgF;             // the V-cycle on F in place of ILU(F): stationary aSIMPLE only
  bool fused_cheby;           // its smoother steps in the residual products' epilogues (the option's -1 counts as on)
  bool want_amgS;             // the V-cycle on S in place of ILU(S): stationary aSIMPLE only
  int amg_bits_S;             // (one knob for "operators a V-cycle multiplies by": NSK_OPT_AMG_PRECISION governs S's too)
  bool inner32;               // fp32 values of the inner solves' matrices
  bool matfree;               // matrix-free F in the inner FGMRES
  bool basis32;               // fp32 basis of the inner FGMRES on F
  // kinds: blockDiagonal stationary = SSOR/SSOR, unsteady = ILU/ILU; blockTriangular = (AMG->ILU)/ILU; aSIMPLE = ILU/ILU
  int kindF, kindP;
  // PreconditionBlockTriangular, stationary: preconditioner_velocity is an AMG (NSSolverStationary.hpp:225,231)
  bool velocity_amg_wanted;
};
inline SetupPlan resolve_setup(const SetupRequest &req, const SetupEnv &env, int type, int variant) {
  const bool stationary_asimple = type == 2 && variant == 0;
  const int amg_precision = env.amg_precision ? env.amg_precision : req.amg_precision;
  SetupPlan p;
  p.factor32 = (env.factor_precision ? env.factor_precision : req.factor_precision) == 32;
  p.velocity_amg_wanted = type == 1 && variant == 0 && req.velocity_amg != 0;
  p.want_amgF = stationary_asimple && (env.asimple_velocity_amg >= 0 ? env.asimple_velocity_amg : req.asimple_velocity_amg) == 1;
  p.amg_bits_F = (p.velocity_amg_wanted || p.want_amgF) && amg_precision == 32 ? 32 : 64;
  p.fused_cheby = p.want_amgF && (env.amg_fused_cheby >= 0 ? env.amg_fused_cheby : req.amg_fused_cheby) != 0;
  p.want_amgS = stationary_asimple && (env.schur_amg >= 0 ? env.schur_amg : req.schur_amg) == 1;
  p.amg_bits_S = p.want_amgS && amg_precision == 32 ? 32 : 64;
  p.inner32 = (env.inner_matrix_precision ? env.inner_matrix_precision : req.inner_matrix_precision) == 32;
  p.matfree = (env.matrix_free_f >= 0 ? env.matrix_free_f : req.matrix_free_f) == 1;
  p.basis32 = (env.inner_basis_precision ? env.inner_basis_precision : req.inner_basis_precision) == 32;
  p.kindF = p.kindP = (type == 0 && variant == 0) ? 1 : 0;
  return p;
}

struct nsk_handle_s {
  Ctx ctx;
  EventSampler sampler;
  std::string err;
  Space sp[2];
  Csr blk[6];
  VecPool pool_u, pool_p, pool_b;
  bool pools_ready = false;
  int tri_ordering = ORDER_MULTICOLOR, subdomains = 1, fuse_block_row = 1, use_stream = 1;
  int inner_fused_gs = 1;
  bool outer_fused_gs = false, cg_fused = false;
  int use_bsr = 1;
  int sync_free_fallbacks = 0;
  // support points of the owned DoFs (nsk_set_support_points) and the line-group sizes of the triangular factors
  std::vector<double> support[2];
  int line_groups = 2, group_u = 2, group_p = 3;   // NSK_OPT_TRI_LINE_GROUPS (2 = by size), NSK_IOPT_GROUP_U / _P
  int mp_ordering = -1;                            // NSK_OPT_MASS_ORDERING: -1 by preconditioner (see mass_ordering), 0 natural, 1 multicolour
  // Ordering of the pressure-mass factor.  In the UNSTEADY block-diagonal preconditioner the pressure block is about one
  // ILU(M_p)-preconditioned CG step (absolute tolerance 1e-1 against unit-norm Krylov vectors, NSSolver.hpp:155-176), and
  // whether restarted FGMRES(30) converges hangs on that one application: with a multicolour M_p factor it stalls from
  // 100x70 upwards (the CPU restatement stalls the same way given the same permutation), with the caller's order it takes
  // the reference's 241 / 403 / 432 iterations.  So that factor keeps the caller's order there.
  int mass_ordering(int type, int variant_) const {
    if (mp_ordering >= 0) return mp_ordering;
    return (type == 0 && variant_ == 1) ? (int)ORDER_NATURAL : tri_ordering;
  }
  // Measured on MI355X: the groups pay where a colour does not fill the GPU and the solve is a chain of
  // hand-offs (600x200: ILU(S) apply -30 %, ILU(F) -7 %), and cost where it is bandwidth-bound (1200x400: ILU(F) +8 %)
  static constexpr int kGroupRowsU = 4000000, kGroupRowsP = 1000000;
  const double *xy(int space) const {
    if (!line_groups || support[space].size() != 2 * (size_t)sp[space].n) return nullptr;
    // line groups exist in the single-launch kernels only (the per-colour kernels do not know the chains): a handle that
    // runs — or has fallen back to — one launch per colour orders its factors without them
    if (sync_free_mode < (space == 0 ? 2 : 1)) return nullptr;
    if (line_groups == 2 && sp[space].n > (space == 0 ? kGroupRowsU : kGroupRowsP)) return nullptr;
    return support[space].data();
  }
  int x_layout_mode = 2;   // NSK_IOPT_TRI_X_LAYOUT
  int sync_free_mode = 2;  // 0 off, 1 scalar factors (S, Mp), 2 also the 2x2-blocked velocity factor
  int fault_inject = 0;    // NSK_IOPT_FAULT_INJECT
  DBuf<int> jrow_blk, jblk_blk;  // row runs of the fused (F | Bt) block row: CSR and blocked variants
  int jrow_nblk = 0, jblk_nblk = 0;
  bool jrow_ok = false, jblk_ok = false;

  int prec_type = -1, variant = 0;
  double alpha = 0.5;
  TriSolve tF, tMp, tS;
  SetupRequest req;         // the options a set-up resolves against the environment (resolve_setup)
  Amg amgF;                 // velocity AMG of the stationary block-triangular preconditioner
  // NSK_OPT_SCHUR_AMG: in the stationary aSIMPLE set-up one V-cycle of amgS, built from S at every set-up,
  // preconditions the inner CG on S instead of ILU(S).  schur_amg_active: the current set-up runs it — tS is then neither
  // analysed nor factorised and tP is null; every reader of tP asks schur_amg_active first
  Amg amgS;
  bool schur_amg_active = false, schur_amg_warned = false;
  void pressure_apply_sampled(const double *b, double *x) {   // profile class 21: ILU(S) / ILU(M_p) / SGS, or the cycle on S
    if (!schur_amg_active) return tri_apply_sampled(*tP, 21, b, x);
    Sampled smp(sampler, 21, s());
    amgS.apply(b, x);
  }
  // NSK_OPT_ASIMPLE_VELOCITY_AMG: in the stationary aSIMPLE set-up one V-cycle of amgF, built inside the set-up,
  // preconditions the inner FGMRES on F instead of ILU(F).  asimple_amg_active: the current set-up runs it — amg_active is
  // then true as well (every reader of the velocity slot behaves as under the velocity AMG of blockTriangular) and tF is
  // neither analysed nor factorised nor held
  bool asimple_amg_active = false, asimple_amg_warned = false;
  void velocity_apply_sampled(const double *b, double *x) {   // profile class 20 while asimple_amg_active: the cycle on F
    Sampled smp(sampler, 20, s());
    amgF.apply(b, x);
  }
  // No ILU(F) in this set-up: its storage goes, what the handle's options gave it stays
  void drop_velocity_factor() {
    TriSolve fresh;
    fresh.tiny_bytes = tF.tiny_bytes;
    fresh.host_analysis = tF.host_analysis;
    fresh.x_layout = tF.x_layout;
    fresh.want_f32 = tF.want_f32;
    tF = std::move(fresh);
    tF_ok = false;
    tF_key = -1;
    push_tri_options();
  }
  int schur_sign = 1;       // NSK_OPT_SCHUR_SIGN: +1 the reference's S = B D^-1 Bt, -1 the negated (SIMPLE's) one
  int blas1_pairs = -1;     // NSK_OPT_BLAS1_PAIRS: -1 by variant (stationary on, unsteady off), 0, 1
  // what the last set-up took of NSK_OPT_INNER_BASIS_PRECISION (the option or NSK_INNER_BASIS_PRECISION), and the fp32
  // vectors, kept from solve to solve.  Whether a solve reads them is SolverFGMRES::reads_f32_basis: the fused sweeps in
  // their pair forms
  bool basis32_wanted = false;
  BasisPool32 basis32_u;
  int inner_basis_width() const {
    if (!inner_solve_on(NSK_BLK_F)) return 0;
    return basis32_wanted && ctx.f32_basis_applies(inner_fused_gs) ? 4 : 8;
  }
  void inner_fgmres_options(SolverFGMRES &sv) {
    sv.fused_gs = inner_fused_gs;
    sv.skip_unused = inner_skip();
    sv.basis32 = basis32_wanted ? &basis32_u : nullptr;
  }
  // pressure_mass does not depend on the state: its values only change when the caller hands over new ones, and a
  // factor of the same values under the same analysis is the same factor — it is kept (the natural-order ILU(0) of M_p
  // at 600x200 takes 0.47 s per set-up, one workgroup walking 4 001 levels: 8.5 s of config 5's first time level)
  long mp_values_version = 0, mp_factored_version = -1;
  int mp_factored_kind = -1;
  bool amg_active = false;  // the current setup preconditions F with amgF instead of tF
  int timeop_between = -1;  // NSK_IOPT_TIMEOP_BETWEEN
  // The hierarchy is built on first use: PreconditionAMG::initialize is called before every solve (NSSolverStationary.hpp:231),
  // also before the many solves of a Newton run that stop at step 0 without ever applying the preconditioner; building it
  // when the first vmult arrives (or before the block's values change) gives the same results without those set-ups.
  // Under NSK_OPT_ASIMPLE_VELOCITY_AMG the set-up builds the hierarchy itself and nothing is pending after it; only
  // nsk_set_block_csr(F) without a new set-up comes through here, and then WITHOUT the set-up's fallback to ILU(F) (whose
  // storage is gone): errors -80..-85 fail that solve
  bool amg_pending = false;
  void amg_ready() {
    if (!amg_pending) return;
    amg_pending = false;
    const double t0 = wall_ms();
    try {
      amgF.setup(&ctx, blk[NSK_BLK_F], sub_offsets(0));
    } catch (...) {   // no half-built hierarchy: the next application tries (and reports) again
      amgF.clear();
      amg_pending = true;
      throw;
    }
    setup_ms += wall_ms() - t0;
    lazy_setup_ms += wall_ms() - t0;   // set-up work that ran inside a solve: counted as set-up, not as solve time
  }
  double lazy_setup_ms = 0;
  bool tF_ok = false, tMp_ok = false, tS_ok = false, s_symbolic = false;
  int tF_key = -1, tMp_key = -1, tS_key = -1;
  TriSolve *tP = nullptr;
  int s_max_row = 0;
  double *D = nullptr, *Dinv = nullptr, *tmp_p = nullptr, *delta_p = nullptr, *tmp_u = nullptr, *tmp_b = nullptr;
  double *rhs_b = nullptr, *x_b = nullptr, *x_keep = nullptr;
  volatile long progress_step = 0;      // outer iterations / residual of the running solve (nsk_get_stats from another thread)
  volatile double progress_value = 0.0;
  volatile int cancel = 0;              // nsk_cancel: ends the running outer solve at its next SolverControl check
  std::vector<double> history;          // residuals the outer SolverControl saw in the last solve (nsk_get_history)
  long inner_u = 0, inner_p = 0, prec_applies = 0, outer_iters = 0;
  double setup_ms = 0, solve_ms = 0;
  // NSK_IOPT_FGMRES_SKIP_UNUSED.  The outer FGMRES does not run the preconditioner application in front of the
  // check that ends a solve: no iterate reads its result.  Stationary aSIMPLE carries state from one application to the
  // next (delta_p, the CG's starting guess), so that application is kept — source and destination, two pool_b vectors
  // — and runs in front of the next one, whoever asks for it (a second solve on this set-up, nsk_precond_vmult).  It is
  // dropped wherever delta_p starts from zero again: every set-up (the sync-free fallback's included), nsk_destroy.
  bool skip_unused = true;
  SolverFGMRES::Pending pending;
  void drop_pending() {
    if (pending.v) pool_b.put(pending.v);
    if (pending.z) pool_b.put(pending.z);
    pending = SolverFGMRES::Pending{};
  }
  // policy of the inner FGMRES on F: its preconditioner — the ILU(0) / SGS apply, or the V-cycle (Amg::apply: the first
  // smoother step of every level and the coarse solve SET x, so x is never read before it is written) — overwrites dst
  // from src and keeps nothing from call to call
  int inner_skip() const { return skip_unused ? SolverFGMRES::stateless : SolverFGMRES::reference; }

  // ---- device assembly and Newton state (nsk_assembly_*, nsk_state_*, nsk_assemble) ----
  struct AsmData {
    bool ready = false, dirichlet_set = false, have_bc = false, state_set = false;
    long n_cells = 0;
    int cell_of_dof0 = -1;
    DBuf<int> cell_u, cell_p, node_cells, node_self, pdof_cells;
    DBuf<unsigned char> cell_flags, node_off, dirichlet;
    DBuf<double> tables, cq, bc;
    double *sol_u = nullptr, *sol_p = nullptr, *eval_u = nullptr, *eval_p = nullptr;  // pool vectors [owned | ghost]
    // P2/P1 triangles (nsk_assembly_set_simplex)
    bool simplex = false;
    long sx_blocks = 0, sx_pos00 = 0;
    DBuf<int> sx_blk_ptr, sx_blk_ent, sx_node_ptr, sx_node_ent, sx_vert_ptr, sx_vert_ent;
    DBuf<long> sx_pos0, sx_pos1;
    DBuf<double> sx_grad, sx_area, sx_outlet;
    // P2/P1: nsk_assemble writes the next solve's initial guess over the resident result of the last one (x_b), and the
    // line search assembles between its steps: the result is copied here first, and nsk_state_update reads the copy
    // (delta_owned of the reference outlives assemble_system()).  x_is_result: x_b holds a solve's result no assembly
    // has overwritten yet (set by nsk_solve_resident, cleared by nsk_upload_system)
    double *sx_delta = nullptr;   // pool_b vector [u_owned | p_owned | ...]
    bool sx_delta_valid = false, x_is_result = false;
    double *old_u = nullptr;  // solution_old of the time loop (velocity part; the pressure is not used)
    bool have_old = false;
    double assemble_ms = 0;
    // matrix-free F (NSK_OPT_INNER_MATRIX_FREE_F): F.val and cq come from ONE Q3 assembly with these
    // parameters.  Set by nsk_assemble / nsk_time_assemble, cleared by every other writer of F or of the cell data
    bool mf_valid = false;
    double mf_nu = 0, mf_inv_dt = 0;
    int mf_stokes = 0;
    DBuf<double> d0, mf_wk;   // the Dirichlet diagonal of that assembly; the cells' shares of their node rows
    // forces over boundary id 10 (nsk_forces_set_faces / nsk_forces_set_edges): void with the cell data
    bool forces_set = false;
    long n_faces = 0;         // faces (Q3/Q2, 4 points each) or edges (P2/P1, 2 points each)
    DBuf<int> face_cell;
    DBuf<unsigned char> face_side;
    DBuf<double> face_tab, force_slots, force_out;   // 672 doubles | (nx, ny, length) per edge; 2 per point; local + total
    // the VTU record in file layout (nsk_record_set_cells / nsk_state_get_record): void with the cell data
    bool record_set = false;
    long rec_cells = 0;
    int rec_sub = 1;
    DBuf<int> rec_cell;
    DBuf<double> rec_wu, rec_wp, rec_out;   // (s+1)^2 x 16, (s+1)^2 x 9; 3 + 1 doubles per point (P2/P1: per vertex)
    // the gradient tables of nsk_record_set_gradient: void with the record's list
    bool rec_grad_set = false;
    DBuf<double> rec_dx, rec_dy, rec_fout;  // (s+1)^2 x 16 each; vorticity | divergence, one double per point each
    // P2/P1: the record's points as local ids (nsk_record_set_points): void with the cell data
    bool rec_points_set = false;
    long rec_points = 0;
    DBuf<int> rec_unode, rec_pdof;          // per point: velocity node and pressure DoF, owned or ghost
  } asmd;
  bool matfree_wanted = false;  // what the last set-up took of NSK_OPT_INNER_MATRIX_FREE_F (the option or the environment)
  bool matfree_warned = false;
  // why a handle that wants the matrix-free product multiplies by the assembled block (nullptr: it does not)
  const char *matfree_obstacle() const {
    if (asmd.simplex) return "the handle assembles P2/P1 triangles";
    if (ctx.comm.nranks > 1) return "the handle is one of several ranks";
    if (subdomains > 1) return "NSK_OPT_SUBDOMAINS > 1";
    if (!asmd.ready || !asmd.mf_valid) return "block (0,0) does not hold the values of the last nsk_assemble";
    return nullptr;
  }
  // would the next inner product with F be matrix-free?
  bool matfree_in_effect() const { return matfree_wanted && inner_solve_on(NSK_BLK_F) && !matfree_obstacle(); }
  // the kernels alone (nsk_matfree_f, nsk_time_op 56): one rank, Q3 cells, a valid assembly
  void matfree_check(const char *who) const {
    if (asmd.simplex || ctx.comm.nranks > 1) throw Error(-65, std::string(who) + ": matrix-free F covers congruent Q3/Q2 cells on one rank only");
    if (!asmd.ready || !asmd.mf_valid)
      throw Error(-66, std::string(who) + ": block (0,0) does not hold the values of a device assembly (call nsk_assemble)");
  }
  double matfree_bytes() const { return asm_matfree_F_bytes(asm_view(), asmd.mf_stokes); }
  void matfree_apply(const DVec &x, double *y) {
    {
      Sampled smp(sampler, NSK_BLK_F, s());
      asm_matfree_F(s(), asm_view(), asmd.cq.p, asmd.mf_nu, asmd.mf_inv_dt, asmd.mf_stokes, asmd.d0.p, x.own, x.ghost,
                    asmd.mf_wk.p, y);
    }
    ++ctx.st.spmv_calls;
    ctx.st.spmv_bytes += matfree_bytes();
  }
  AsmMesh asm_view() const {
    return AsmMesh{asmd.n_cells, sp[0].n / 2, sp[1].n, asmd.cell_of_dof0, asmd.cell_u.p, asmd.cell_p.p, asmd.cell_flags.p,
                   asmd.node_cells.p, asmd.node_off.p, asmd.node_self.p, asmd.pdof_cells.p, asmd.dirichlet.p,
                   asmd.tables.p};
  }

  int n_u() const { return sp[0].n; }
  int n_p() const { return sp[1].n; }
  int N() const { return sp[0].n + sp[1].n; }
  DVec ub(double *base) const { return DVec{base, base + N(), n_u()}; }
  DVec pb(double *base) const { return DVec{base + n_u(), base + N() + sp[0].ng, n_p()}; }
  DVec bb(double *base) const { return DVec{base, base + N(), N()}; }
  hipStream_t s() { return ctx.stream; }

  void ensure_pools() {
    if (pools_ready) return;
    if (!blk[NSK_BLK_F].present || !blk[NSK_BLK_B].present) throw Error(-40, "set blocks F and B before this call");
    pool_u.init(&ctx, sp[0].n, sp[0].ng);
    pool_p.init(&ctx, sp[1].n, sp[1].ng);
    pool_b.init(&ctx, N(), sp[0].ng + sp[1].ng);
    rhs_b = pool_b.get(true);
    x_b = pool_b.get(true);
    pools_ready = true;
  }
  void halo(int space, const DVec &x) { ctx.comm.halo_exchange(sp[space], x, s()); }
  // Does the current set-up run an inner solve on block b (FGMRES on F, CG on S or M_p)?
  bool inner_solve_on(int b) const {
    if (prec_type < 0) return false;
    if (b == NSK_BLK_F) return prec_type != 2 || variant == 0;
    if (b == NSK_BLK_MP) return prec_type != 2;
    if (b == NSK_BLK_S) return prec_type == 2 && variant == 0;
    return false;
  }
  // The kernel form of a product with A under the handle's options (the rule: nsk::spmv_form); inner: that of
  // the inner solves (spmv_halo), which read the fp32 copy where A holds one for that form (y = A x only)
  SpmvForm form_of(const Csr &A, int mode = 0, bool inner = false) const { return A.spmv_form(use_stream != 0, use_bsr != 0, mode, inner); }
  // Bytes per value the inner solves' SpMV of A reads: 4 on an fp32 copy, else 8
  int inner_width(const Csr &A) const { return is_f32(form_of(A, 0, true)) ? 4 : 8; }
  // (the 8 n_rows of z are counted for mode 1 only, Ctx::spmv counts them for mode 2 as well: see there)
  void spmv_nohalo(Csr &A, const DVec &x, double *y, int mode = 0, const double *z = nullptr, bool inner = false) {
    {
      Sampled smp(sampler, (int)(&A - blk), s());
      A.spmv_launch(s(), form_of(A, mode, inner), x.own, x.ghost, y, mode, z);
    }
    ++ctx.st.spmv_calls;
    ctx.st.spmv_bytes += (double)A.spmv_bytes() + (mode == 1 ? 8.0 * A.n_rows : 0.0);
  }
  // y = A x including the ghost import of x.  Several ranks: the rows without ghost columns (all but the first and last
  // lattice columns of the strip) are computed on a second stream while the halo exchange occupies the main one; the
  // boundary rows follow it.  Row-run plans are cut at the interior range (Csr::find_interior), so the three launches
  // are sub-ranges of the same plan.
  // This is the SpMV of the preconditioner's inner solves (and of nsk_inner_spmv): where A holds an fp32 copy
  // (NSK_OPT_INNER_MATRIX_PRECISION = 32) it reads that, converted again first when val has changed since.
  // NSK_IOPT_INDEX16: 16-bit column offsets in the scalar stream kernels of S and M_p (SpMV and the split ILU / SGS halves)
  // wherever every run qualifies; 0: int32 columns everywhere
  bool index16 = true;
  void index16_for(Csr &A, const char *name) {
    A.build_index16(s(), index16);
    if (verbose() && index16 && A.stream_ok && !A.off16.p)
      fprintf(stderr, "[nsk] %s: a run of the stream plan spans 65 536 columns or more — int32 column ids stay in use\n", name);
  }
  bool overlap_halo = true;   // NSK_IOPT_OVERLAP_HALO
  long overlapped_spmvs = 0;
  void spmv_halo(Csr &A, int space, const DVec &x, double *y) {
    if (matfree_wanted && &A == &blk[NSK_BLK_F]) {
      // NSK_OPT_INNER_MATRIX_FREE_F: the same operator from the cell data of the last assembly — or, announced once, the
      // assembled block where that is not F any more (or the handle is of a kind the kernels do not cover)
      const char *why = matfree_obstacle();
      if (!why) {
        halo(space, x);
        matfree_apply(x, y);
        return;
      }
      if (!matfree_warned) {
        matfree_warned = true;
        fprintf(stderr, "[nsk] warning: NSK_OPT_INNER_MATRIX_FREE_F = 1, but %s: the inner FGMRES multiplies by the assembled F\n", why);
      }
    }
    const SpmvForm form = form_of(A, 0, true);
    if (is_f32(form) && A.val32_version != A.values_version) A.refresh_f32(s(), false);   // (stream-ordered: no host sync)
    const bool blocked = is_blk(form);
    const int b0 = blocked ? A.blk_int_b0 : A.int_b0, b1 = blocked ? A.blk_int_b1 : A.int_b1;
    const int nb = blocked ? A.blk_nblk : A.nblk;
    EventSampler::Slot *smp = sampler.find((int)(&A - blk));
    const bool sampling = smp && smp->used < smp->cap;   // (a launch that is being timed stays one launch)
    if (!overlap_halo || ctx.comm.nranks <= 1 || form == SpmvForm::csr_vector || b1 <= b0 || sampling) {
      halo(space, x);
      spmv_nohalo(A, x, y, 0, nullptr, true);
      return;
    }
    if (smp) ++smp->seen;
    ++overlapped_spmvs;
    ctx.ensure_stream2();
    auto part = [&](hipStream_t st, int c0, int c1) { A.spmv_launch(st, form, x.own, x.ghost, y, 0, nullptr, c0, c1); };
    NSK_HIP(hipEventRecord(ctx.ev_fork, s()));                 // x is complete here
    NSK_HIP(hipStreamWaitEvent(ctx.stream2, ctx.ev_fork, 0));
    part(ctx.stream2, b0, b1);                                 // interior rows: owned entries of x only
    NSK_HIP(hipEventRecord(ctx.ev_join, ctx.stream2));
    halo(space, x);                                            // pack + grouped send/recv into x's ghost tail
    part(s(), 0, b0);
    part(s(), b1, nb);
    NSK_HIP(hipStreamWaitEvent(s(), ctx.ev_join, 0));
    ++ctx.st.spmv_calls;
    ctx.st.spmv_bytes += (double)A.spmv_bytes();
  }
  // BlockSparseMatrix::vmult on jacobian_matrix: y_u = F x_u + Bt x_p ; y_p = B x_u (+ 0 x_p)
  void jacobian_vmult(const DVec &xb, double *yb) {
    const DVec xu = ub(xb.own), xp = pb(xb.own);
    ctx.comm.halo_exchange2(sp[0], xu, sp[1], xp, s());   // both ghost imports in one RCCL group
    Csr &F = blk[NSK_BLK_F], &Bt = blk[NSK_BLK_BT], &B = blk[NSK_BLK_B];
    const bool blocked = use_stream && use_bsr && F.blk_ok && Bt.blk_ok && F.blk_R == 2 && Bt.blk_R == 2 &&
                         F.blk_rows == Bt.blk_rows;
    if (fuse_block_row && blocked && !jblk_ok && jblk_nblk == 0) {
      std::vector<int> rb;
      if (fused_blk_plan(F, Bt, rb)) {
        jblk_nblk = (int)rb.size() - 1;
        jblk_blk.upload(rb, s());
        ctx.sync();
        jblk_ok = true;
      } else jblk_nblk = -1;
    }
    if (fuse_block_row && use_stream && !jrow_ok && jrow_nblk == 0 && F.even_rows) {
      std::vector<int> rb;
      if (fused_row_plan(F, Bt, rb)) {
        jrow_nblk = (int)rb.size() - 1;
        jrow_blk.upload(rb, s());
        ctx.sync();
        jrow_ok = true;
      } else jrow_nblk = -1;
    }
    const double fused_bytes = (double)F.spmv_bytes() + (double)Bt.spmv_bytes() - 8.0 * F.n_rows - 4.0 * (F.n_rows + 1);
    if (fuse_block_row && blocked && jblk_ok) {
      nsk::spmv_blk_fused22_21(s(), F.blk_view(), xu.own, xu.ghost, Bt.blk_view(), xp.own, xp.ghost, jblk_blk.p,
                               jblk_nblk, yb);
      ctx.st.spmv_calls += 2;
      ctx.st.spmv_bytes += fused_bytes;
    } else if (fuse_block_row && use_stream && jrow_ok) {
      nsk::spmv2_stream(s(), F.view(), xu.own, xu.ghost, Bt.view(), xp.own, xp.ghost, jrow_blk.p, jrow_nblk, yb);
      ctx.st.spmv_calls += 2;
      ctx.st.spmv_bytes += fused_bytes;
    } else {
      spmv_nohalo(F, xu, yb, 0);
      spmv_nohalo(Bt, xp, yb, 1);
    }
    spmv_nohalo(B, xu, yb + n_u(), 0);
  }
  void tri_apply_sampled(TriSolve &T, int op, const double *b, double *x) {
    Sampled smp(sampler, op, s());
    T.apply(b, x);
  }
  std::vector<int> sub_offsets(int space) const {
    std::vector<int> off;
    if (subdomains <= 1) return off;
    const int n = sp[space].n;
    off.resize(subdomains + 1);
    for (int k = 0; k <= subdomains; ++k) {
      long v = (long)n * k / subdomains;
      if (space == 0) v &= ~1L;  // keep both velocity components of a node together
      off[k] = (int)v;
    }
    off[subdomains] = n;
    return off;
  }
  // Call after a stream sync.  Collective: with several ranks the flag is all-reduced so that every rank
  // takes the same decision (a rank-local fallback would desynchronise the ranks' collectives).
  void check_sync_free() {
    int e = 0;
    for (TriSolve *T : {&tF, &tMp, &tS})
      if (T->sf_err.p) {
        int ei = 0;
        NSK_HIP(hipMemcpy(&ei, T->sf_err.p, sizeof(int), hipMemcpyDeviceToHost));
        if (ei) {
          NSK_HIP(hipMemsetAsync(T->sf_err.p, 0, sizeof(int), s()));
          T->sf_armed = false;
        }
        e |= ei;
      }
    if (ctx.comm.active() && sync_free_mode > 0) {
      const SlotLease sl(ctx, 1);
      vec_set(s(), 1, ctx.slot(sl), e ? 1.0 : 0.0);
      ctx.comm.allreduce_sum(ctx.slot(sl), 1, s());
      e = ctx.read_slots(sl, 1)[0] > 0.0;
    }
    if (e)
      throw Error(-70, "sync-free triangular solve: a producer/consumer wait ran out of spins (results invalid); "
                       "set NSK_OPT_TRI_SYNC_FREE to 0");
  }
  // what the triangular factors take of the handle's options (every nsk_set_option, every set-up)
  void push_tri_options() {
    tMp.sync_free = tS.sync_free = sync_free_mode >= 1;
    tF.sync_free = sync_free_mode == 2;
    tMp.sf_fault = tS.sf_fault = (fault_inject & 1) != 0;
    tF.sf_fault = (fault_inject & 2) != 0;
    tMp.want_index16 = tS.want_index16 = index16;
    tF.use_stream = tMp.use_stream = tS.use_stream = use_stream != 0;
  }
  void schur_symbolic();
  // the set-up and its steps, in the order they run (nsk_precond.cpp)
  void setup(int type, int variant_, double alpha_);
  void setup_hierarchies(const SetupPlan &plan);
  void setup_velocity_factor(const SetupPlan &plan, int key);
  void analyse_S();
  void setup_schur(const SetupPlan &plan, int key);
  void setup_schur_hierarchy();
  void setup_mass(const SetupPlan &plan, int key);
  void setup_f32_copies(const SetupPlan &plan);
  void check_f32_overflow();
  void prec_vmult(DVec &dst, const DVec &src);
  int solve_once(int solver, double tol, int max_iter, int *iters, double *final_res);
  int solve_resident(int solver, double tol, int max_iter, int *iters, double *final_res);
};
using H = nsk_handle_s;

// ================================================================== C ABI: what every entry point opens and closes with
#define NSK_TRY(h) try {
// The same on the handle's device.  The entries that other threads may call while a solve runs (nsk_cancel, nsk_abort_group,
// nsk_get_stats) and the getters of host state keep NSK_TRY: they must not touch the device
#define NSK_TRY_DEV(h) NSK_TRY(h) (void)hipSetDevice((h)->ctx.device);
#define NSK_CATCH(h)                                  \
  }                                                   \
  catch (const Error &e) {                            \
    (h)->err = e.what();                              \
    return e.code;                                    \
  }                                                   \
  catch (const std::exception &e) {                   \
    (h)->err = e.what();                              \
    return -1;                                        \
  }

// entries that run collectives: a rank that fails inside one takes the in-process group down with it, so that the
// peers blocked in the collective get Error -25 instead of waiting for ever (RCCL has its own abort path)
#define NSK_CATCH_ABORT(h)                            \
  }                                                   \
  catch (const Error &e) {                            \
    (h)->err = e.what();                              \
    if (e.code != -25) (h)->ctx.comm.abort_group();   \
    return e.code;                                    \
  }                                                   \
  catch (const std::exception &e) {                   \
    (h)->err = e.what();                              \
    (h)->ctx.comm.abort_group();                      \
    return -1;                                        \
  }
