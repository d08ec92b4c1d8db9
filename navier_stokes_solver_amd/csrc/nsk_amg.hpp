// nsk_amg.hpp — smoothed-aggregation AMG V-cycle for the velocity block.
//
// Replaces TrilinosWrappers::PreconditionAMG (Trilinos ML) as configured by the reference's stationary
// block-triangular preconditioner: `preconditioner_velocity.initialize(*velocity_stiffness)` with the
// deal.II default AdditionalData (lab_new/src/NSSolverStationary.hpp:225,231).  ML's aggregates cannot be
// reproduced bit for bit (its source is the only specification), so this is the same METHOD under the
// same parameters — see DESIGN.md "AMG" for the deterministic details of this specification:
//   uncoupled root-and-neighbours aggregation (strength threshold 1e-4; the roots are a distance-2 maximal independent
//   set found in synchronous rounds, so that it runs row-parallel), one constant near-null-space vector,
//   prolongator smoothing (I - 4/3 / lambda D^-1 A), R = P^T, Galerkin R A P, <= 10 levels,
//   coarsest level (<= 128 unknowns) solved directly, V(1,1) cycle with a degree-2 Chebyshev polynomial in
//   D^-1 A (eigenvalue ratio 20), lambda = 1.1 x (10 power iterations).
// Rank-local like every preconditioner of the reference's stack under additive Schwarz with overlap 0:
// ghost columns are dropped (block Jacobi across ranks / sub-domains).
//
// The same hierarchy and cycle, built from aSIMPLE's S, precondition the inner CG on S under NSK_OPT_SCHUR_AMG (a second
// Amg of the handle): the code below is generic over Csr, "F" names the caller's block.
//
// Set-up and cycle both run on the device: the set-up with the row-parallel kernels of nsk_amg_kernels.hip from the
// block's device copy (only row pointers for the SpMV plans and the coarsest operator, for its dense inverse, visit
// the host), the cycle with the library's CSR-stream SpMV kernels.
//
// NSK_OPT_AMG_PRECISION = 32: the set-up is the same, in double; when a level is finished the values of the
// operators the cycle multiplies by — A, P, R — are rounded to float (Csr::val32; level 0 that is the caller's F: its 2x2
// node-block copy blk_val32) and the cycle's products read those, widened as they land.  Vectors, dinv, the coarsest
// level's dense inverse, the Chebyshev coefficients and all arithmetic stay double.
#pragma once
#include <memory>
#include <vector>

#include "nsk_core.hpp"

struct nsk_dbg_amg_args;

namespace nsk {

struct AmgLevel {
  int n = 0;
  Csr own_A;          // this level's operator when it is not the caller's block itself
  Csr *A = nullptr;   // -> own_A, or the caller's F (level 0 of a single shard without ghost columns)
  Csr P, R;
  bool has_coarse = false;
  double lam = 1.0;
  DBuf<double> dinv, inv, x, b, r, w;
  DBuf<double> x2;    // level 0 under Amg::fused_cheby alone: the second iterate of the fused smoother steps (x_out != x_in)
};

struct AmgHierarchy {
  int offset = 0;  // first row of this shard in the caller's vector
  std::vector<std::unique_ptr<AmgLevel>> lev;
};

struct Amg {
  Ctx *ctx = nullptr;
  std::vector<AmgHierarchy> shards;
  double setup_host_ms = 0;
  // Set by the handle before setup(): bits the operators' values are stored in (64, or 32: NSK_OPT_AMG_PRECISION), and
  // whether level 0 may use F's 2x2 node blocks (NSK_OPT_BSR_VELOCITY)
  int value_bits = 64;
  bool use_bsr = true;
  // The hierarchy preconditions a CG (the Schur AMG, NSK_OPT_SCHUR_AMG): the cycle must be definite, so every level's
  // diagonal has to carry one sign and no zero — Error -85 from the set-up otherwise (checked where dinv is formed)
  bool one_sign_diag = false;
  // The velocity hierarchy stationary aSIMPLE builds under NSK_OPT_ASIMPLE_VELOCITY_AMG; both false for every
  // other hierarchy (the velocity AMG of blockTriangular, the one of S), which keep their kernel forms and bits.
  // blk_residual: in double, r = b - A x on a level with 2 x 2 node blocks (level 0 when it is F itself) takes
  // spmv_blk22_residual instead of the scalar stream kernel (the rule: amg_spmv_form's last argument).
  // fused_cheby: on such a level — double or fp32 blocks — the smoother steps that follow a residual run in that
  // product's epilogue (nsk::spmv_blk22_cheby), alternating between x and the level's x2; NSK_IOPT_AMG_FUSED_CHEBY
  bool blk_residual = false, fused_cheby = false;
  long fused_launches = 0;                   // fused smoother steps of the cycles since the set-up (test hook)
  long form_launches[5] = {0, 0, 0, 0, 0};   // products of the cycles since the set-up, by SpmvForm (test hook)
  int value_bytes() const { return shards.empty() ? 0 : built_bits / 8; }   // of the hierarchy that stands
  // F: device block with host pattern; shard_off: empty = one shard
  void setup(Ctx *ctx, Csr &F, const std::vector<int> &shard_off);
  void apply(const double *b, double *x);
  void clear() {
    shards.clear();
    level0 = nullptr;
    for (long &c : form_launches) c = 0;
    fused_launches = 0;
  }   // (the set-up's scratch arena stays for the next set-up)
  void release() {                   // the preconditioner is no longer in use
    clear();
    arena.release();
  }
  int n_levels(int shard = 0) const { return shards.empty() ? 0 : (int)shards[shard].lev.size(); }
  int level_rows(int shard, int l) const { return shards[shard].lev[l]->n; }
  int64_t level_nnz(int shard, int l) const { return shards[shard].lev[l]->A->nnz; }
  double level_lambda(int shard, int l) const { return shards[shard].lev[l]->lam; }
  size_t apply_bytes() const;  // algorithmic bytes of one V-cycle (SURVEY 8d formulas)
  // the same count on what the stored formats hold (fp32 values, node blocks), vectors as in apply_bytes; level >= 0: that
  // level of that shard alone
  double format_bytes(int shard = -1, int level = -1) const;
  // Test hook behind nsk_debug_amg_level (nsk_internal.h)
  int64_t debug_level(int shard, int level, int which, int32_t *rowptr, int32_t *col, double *val, double *dinv_or_inverse);

 private:
  void build_all(Csr &F, const std::vector<int> &shard_off);   // every shard's hierarchy, then level 0's fp32 copy
  void build(AmgHierarchy &H, Csr *A0, std::unique_ptr<Csr> own0);
  DBuf<char> arena;        // work arrays of the set-up, kept across set-ups (nsk_amg.cpp: Scratch)
  size_t arena_want = 0;   // bytes the largest level took so far
  double estimate_lambda_device(AmgLevel &L);
  void cheby(AmgLevel &L, const double *b, double *x, bool zero_init);
  // The same smoothers with every step after a residual fused into it (level 0 under fused_cheby): pre leaves the iterate
  // in x having passed through L.x2, post takes x -> x2 -> x.  fusable: the conditions, on this call's vectors
  bool fusable(const AmgLevel &L, const double *b, const double *x) const;
  SpmvForm fused_form(const AmgLevel &L, const double *b, const double *x) const;
  void cheby_fused(AmgLevel &L, const double *b, double *x, bool zero_init);
  void fused_step(AmgLevel &L, SpmvForm f, const double *x_in, double *x_out, const double *b, double c1, double c2);
  // what the cycle streams on a level with a coarser one besides P and R — four products with A (a bytes each, x and y
  // included) and four smoother steps — by the launches it takes on aligned vectors
  double smoother_bytes(const AmgLevel &L, double a) const;
  void vcycle(AmgHierarchy &H, int l, const double *b, double *x);
  void mv(Csr &A, const double *x, double *y, int mode = 0, const double *z = nullptr);
  SpmvForm form_of(const Csr &A, int mode, bool aligned16) const {
    return amg_spmv_form(A.blk_ok && A.blk_R == 2 && A.blk_C == 2, A.stream_ok, A.amg32 != 0, use_bsr, mode, aligned16,
                         blk_residual);
  }
  void to_f32(AmgLevel &L, int level);   // round the finished level's A (its own), P and R; Error -48 on overflow
  void check_overflow(Csr &M, int level, const char *which);
  int built_bits = 64;
  Csr *level0 = nullptr;   // the caller's block when it is level 0 itself
};

// Structural pattern of C = A B on the device, rows sorted by column (the row-product kernels of the AMG set-up: hash sets
// in LDS, at most 512 distinct columns per row, Error -81 beyond).  A and B without ghost columns.  rp: n_rows + 1 row
// pointers, col: the columns; returns the number of entries.  Used for aSIMPLE's Schur pattern B~ [D^-1] B~^T (round 4).
int64_t device_product_pattern(Ctx *ctx, const Csr &A, const Csr &B, DBuf<int> &rp, DBuf<int> &col);


// Test hook behind nsk_debug_amg (nsk_internal.h): one operation of the set-up on the caller's arrays, on ctx's device and
// stream.  Lives in nsk_amg.cpp so that it calls Scratch::scan, product_rows, transpose() and aggregate() as the set-up does.
int debug_amg(Ctx *ctx, const nsk_dbg_amg_args *a, int32_t *info16);

}  // namespace nsk
