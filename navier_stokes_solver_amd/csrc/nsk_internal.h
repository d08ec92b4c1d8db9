// nsk_internal.h — options of nsk_set_option that are NOT part of the public ABI (include/nsk.h):
// study switches kept for A/B measurements and the fault-injection hook of the tests.
#pragma once
#include <stdint.h>

enum {
  NSK_IOPT_TRI_X_LAYOUT = 6,    // blocked velocity factor: 2 (default) colour-ordered working vector when it runs
                                // single-launch, 0 the caller's order
  NSK_IOPT_FAULT_INJECT = 100,  // bit 0: the scalar triangular solves walk their upper half backwards,
                                // bit 1: the blocked velocity solve walks its upper half backwards — consumers before
                                // producers, so the bounded spins give up and the fallback has to take over;
                                // bit 2: workgroup 0 of the one-launch Gram-Schmidt sweep withholds its first partial sum
  NSK_IOPT_GROUP_U = 103,      // members per line group of the velocity factor (nodes; default 2) and of the scalar
  NSK_IOPT_GROUP_P = 104,      // factors S, Mp (DoFs; default 3); 1 = plain colouring.  See NSK_OPT_TRI_LINE_GROUPS
  NSK_IOPT_TINY_BYTES = 102,    // triangular factors below this many bytes (default 4e6) are solved by ONE workgroup walking
                                // all levels; the tests set 0 to run the streamed kernels on small meshes
  NSK_IOPT_OVERLAP_HALO = 107,  // 1 (default): several ranks — interior rows of the inner solvers' SpMVs (F, S, Mp) run on a
                                // second stream while the halo exchange is in flight; 0: exchange first, then one launch
  NSK_IOPT_HOST_ANALYSIS = 108, // 1: the symbolic set-up of the multicolour triangular factors (permuted pattern, split halves)
                                // on the host as in rounds 1-3; 0 (default): on the device (nsk_setup_kernels.hip) wherever
                                // it applies — no line groups, no sub-domains, no ghost columns.  Same arrays either way
  NSK_IOPT_TIMEOP_BETWEEN = 109, // nsk_time_op: a block id (e.g. NSK_BLK_F) whose SpMV runs BETWEEN two repetitions, outside
                                // the timed brackets (one pair of events per repetition) — the operation as a solver sees
                                // it, with the caches and clocks another kernel leaves behind; -1 (default): back to back
  NSK_IOPT_INDEX16 = 110,       // 1 (default): the scalar stream kernels of S and M_p — SpMV, split ILU / SGS halves — read 16-bit
                                // column offsets on top of one base per run wherever every run of the plan spans fewer than
                                // 65 536 columns (same bits, 2 bytes per entry less); 0: int32 column ids everywhere
  NSK_IOPT_GS_ONE_LAUNCH = 111, // 1 (default): the two fused Gram-Schmidt sweeps of an Arnoldi step (NSK_OPT_INNER_FUSED_GS 1 / 2) and
                                // FGMRES' cycle-end update x += sum y_j z_j run ONE launch each over the whole basis where the pair
                                // kernels apply; 0: one launch per eight basis vectors and one per term, as before;
                                // 2: at most 16 vectors per launch (the measured alternative).  Same bits in all three
  NSK_IOPT_FGMRES_SKIP_UNUSED = 112, // 1 (default): FGMRES checks before it builds a basis column and does not build the one no
                                // iterate reads — in front of the check that ends a solve, the last one of a full restart
                                // cycle (SolverFGMRES::skip_unused): the inner solves on F skip it outright, the
                                // outer solve keeps the preconditioner application a later one depends on.  Same bits;
                                // 0: deal.II's order everywhere (A/B runs, tests).  ONE sequence is not the bits of 0:
                                // stationary aSIMPLE, solve, nsk_update_values (or nsk_assemble) WITHOUT a new
                                // nsk_setup_preconditioner, solve — the application the first solve left over then runs
                                // on the new values, where the reference order ran it on the old ones (either way a
                                // stale preconditioner; nsk_setup_preconditioner between the solves drops it)
  NSK_IOPT_AMG_FUSED_CHEBY = 113, // -1 (default) / 1: the velocity hierarchy of NSK_OPT_ASIMPLE_VELOCITY_AMG runs the smoother
                                // steps of level 0 in the epilogue of the residual products on F's 2 x 2 node blocks
                                // (Amg::fused_cheby) wherever that level allows it; 0: two launches per step
                                // (A/B runs, tests).  Same bits.  No other hierarchy reads it.  NSK_AMG_FUSED_CHEBY=0 / 1
                                // in the environment overrides it for every handle.  Takes effect at the next set-up
  NSK_IOPT_FUSED_MGS = 106      // 1 (default): the modified Gram-Schmidt chain of an Arnoldi step in ONE launch when the
                                // vector fits the registers of the co-resident grid (single rank); 0: one launch per link
};

#ifdef __cplusplus
extern "C" {
#endif
/* Diagnostics: one apply of the scalar single-launch triangular preconditioner `which` with in-kernel time stamps
 * (s_memrealtime, 10 ns ticks).  out16 receives 16 int64 per workgroup of the lower launch, then of the upper launch:
 *   [0] start, [1] matrix stream and first look at the gathered entries have landed (products in LDS), [2] wave 0 has
 *   all its entries (polls done), [3] all waves have, [4] results stored, [5] gathered entries that still held the
 *   sentinel at first look, [6] XCC id, [7] rows, [8] non-zeros, [9] descriptor arrived.
 * Returns the number of workgroups (0: this factor does not run the scalar single-launch kernels); *grid = -(workgroups
 * of the lower launch). */
int nsk_debug_tri_trace(struct nsk_handle_s *h, int which, int64_t *out16, int max_runs, int *grid);
/* In-process test transport (nsk_local_group_id) with the mode chosen: on_stream = 1 keeps every collective on the
 * ranks' streams (device-to-device copies into the peers' ghost tails and a summing kernel, ordered by events; the host
 * threads only rendezvous), so the second-stream overlap of the SpMVs and the grouped exchange race as they would under
 * RCCL; on_stream = 0 is nsk_local_group_id (streams synchronised with the host around every collective). */
int nsk_local_group_id_mode(int nranks, int on_stream, void *out128);
/* Take an in-process group down by its id: every rendezvous of the group, pending or later — also of members that are
 * still inside nsk_create — ends with error -25.  For the thread that drives the ranks when one of them failed before
 * it had a handle (nsk_abort_group needs one).  Callable from any thread. */
int nsk_abort_local_group(const void *uid128);
/* Host-only (no handle, no GPU): the multicolour ordering the triangular-solve analysis chooses for a local pattern —
 * perm_out[new] = old; info4 = {colours, largest line group, node structure found, items}; chain_out (may be null): per
 * permuted item position | length << 4 in its line group.  xy: 2 doubles per row or null; group: members per group. */
int nsk_debug_tri_ordering(int n, const int32_t *rowptr, const int32_t *col, int n_sub, const int32_t *sub_off,
                           int want_block2, const double *xy, int group, int32_t *perm_out, int32_t *info4,
                           uint8_t *chain_out);
/* Test hooks for the 32-bit POSITION arithmetic of the set-up kernels (a rank's share of 4800x1600 on four GPUs holds
 * 1.67 G non-zeros in F: positions pass 2^30, where `(lo + hi) >> 1` overflowed in round 3).  The kernels run on a small
 * matrix whose positions — row pointers, diagonal positions — are shifted by `base`, through array base pointers moved
 * back by `base` entries: the index arithmetic of a factor with > 2^30 non-zeros without the 13 GB.  Device 0, stream 0.
 * what = 0: ilu0_factor_level, one launch per row; 1: ilu0_factor_serial (one workgroup walks the rows).  val_inout: the
 * matrix values in, the ILU(0) factor out (rows are factorised in index order). */
int nsk_debug_ilu0_at_offset(int what, int n, const int32_t *rowptr, const int32_t *col, double *val_inout, int64_t base);
/* S = B diag(dinv) Bt on the given structural pattern (spgemm_bdbt_numeric), all three matrices' positions shifted. */
int nsk_debug_schur_at_offset(int n_p, int n_u, const int32_t *b_rp, const int32_t *b_col, const double *b_val,
                              const double *dinv, const int32_t *bt_rp, const int32_t *bt_col, const double *bt_val,
                              const int32_t *s_rp, const int32_t *s_col, double *s_val_out, int64_t base);
/* Test hook for the Krylov vector kernels (tests/test_gpu_krylov_kernels.py): ONE operation `op` (NSK_DBG_KRY_*) through
 * the entry points the solvers call (Ctx:: reductions on the handle's workspace and slots, arnoldi_column, nsk:: launchers).
 * vec[k] (host, len[k] doubles, in/out) is copied into a fresh device buffer of its own that starts `offset` (0 or 1)
 * doubles into the allocation (offset 1: not 16-byte aligned, the pair kernels do not apply) and is followed by guard
 * words; what the op wrote comes back.  The pair choice is the handle's (NSK_OPT_BLAS1_PAIRS).  slots64 receives 64
 * device scalar slots (NaN where the op wrote none); par: the op's scalars.
 *   DOT        x, y                     [0] = x.y
 *   NORM2      x                        [0] = x.x, [1] = |x|
 *   AXPY_DOT   x, y, w    par a         y += a x ; [0] = y.w
 *   AXPY_NORM2 x, y       par a         y += a x ; [0] = y.y, [1] = |y|
 *   CG_UPDATE  d, h, x, g par a         x += a d ; g += a h ; [0] = g.g, [1] = |g|
 *   MULTI_DOT  w, v_0 .. v_{m-1}        [k] = w.v_k                               (m = 1 .. 8)
 *   MULTI_AXPY w, v_0 .. v_{m-1}        par h_0 .. h_{m-1}, norm: w -= sum h_k v_k ; [k] = h_k, norm != 0: [m] = w.w,
 *                                       [m+1] = |w|                               (m = 1 .. 8)
 *   GS_COLUMN  w, v_0 .. v_{m-1}        par mode (NSK_OPT_INNER_FUSED_GS 0 / 1 / 2): arnoldi_column; [k] = h_k, [m] = w.w,
 *                                       [m+1] = |w|                               (m = 1 .. 32)
 *   DOT3       r, u, w                  [0] = r.u, [1] = w.u, [2] = r.r
 *   CG_SCALARS (none)                   par sc_0 .. sc_6, first: cg_fused_scalars on slots [0..7) = sc
 *   CG_FUSED_UPDATE u, w, p, s, x, r    par sc_0 .. sc_6: vec_cg_fused_update with slots [0..7) = sc
 *   CHEBY      dinv, r, w, x            par c1, c2, set_x: vec_cheby_step
 *   DENSE_MV   M (n x n), b, x          x = M b
 *   MULTI_DOT_ALL  w, v_0 .. v_{m-1}    Ctx::multi_dot_all: [k] = w.v_k           (m = 1 .. 32; NSK_IOPT_GS_ONE_LAUNCH chooses
 *   MULTI_AXPY_ALL w, v_0 .. v_{m-1}    Ctx::multi_axpy_all, par and slots as MULTI_AXPY       one launch or chunks of eight)
 *   MULTI_ADD  x, z_0 .. z_{m-1}        par y_0 .. y_{m-1}: Ctx::multi_add, x += sum_j y_j z_j (m = 1 .. 32)
 * The kernels of the fp32 inner basis.  The basis vectors v_k are given as doubles that hold fp32 values (-61
 * otherwise), live on the device as floats — each in an allocation of its own with guard floats behind it — and come
 * back widened; w stays double.  offset = 1 (w not 16-byte aligned) and NSK_OPT_BLAS1_PAIRS = 0 have no fp32 form: -61.
 *   MULTI_DOT_ALL_F32  w, v_0 .. v_{m-1}  par rider: Ctx::multi_dot_all_f32: [k] = w.v_k, rider != 0: [m] = w.w
 *                                         (m = 1 .. 32)
 *   MULTI_AXPY_ALL_F32 w, v_0 .. v_{m-1}  Ctx::multi_axpy_all_f32, par and slots as MULTI_AXPY (m = 1 .. 32)
 *   GS_COLUMN_F32      w, v_0 .. v_{m-1}  par mode (1 / 2): arnoldi_column on the fp32 basis, slots as GS_COLUMN
 *   EQU        x, y                       par a: slot [0] = a ; y = x / a, vec_equ as SolverFGMRES normalises a basis vector
 *   EQU_F32    x, v, vw                   par a: slot [0] = a ; vec_equ_f32: v = fl32(x / a) (comes back widened), vw = v
 * info8: [0] reduction kernels that ran (bit 0: 8-byte-per-lane form, bit 1: pair form), [1] modified Gram-Schmidt path
 * of GS_COLUMN (4 / 8 / 12: the one-launch sweep with that many entries per thread, 0 the chain of launches, -1 not that
 * path), [2] the sweep's grid (co-resident workgroups), [3] guard words that changed (writes outside the vectors), [4] kernel
 * launches of MULTI_DOT_ALL / MULTI_AXPY_ALL / MULTI_ADD / the fused sweeps of GS_COLUMN / the fp32 sweeps.
 * Device and stream of the handle; 0 or a negative error code. */
enum {
  NSK_DBG_KRY_DOT = 0, NSK_DBG_KRY_NORM2 = 1, NSK_DBG_KRY_AXPY_DOT = 2, NSK_DBG_KRY_AXPY_NORM2 = 3, NSK_DBG_KRY_CG_UPDATE = 4,
  NSK_DBG_KRY_MULTI_DOT = 5, NSK_DBG_KRY_MULTI_AXPY = 6, NSK_DBG_KRY_GS_COLUMN = 7, NSK_DBG_KRY_DOT3 = 8,
  NSK_DBG_KRY_CG_SCALARS = 9, NSK_DBG_KRY_CG_FUSED_UPDATE = 10, NSK_DBG_KRY_CHEBY = 11, NSK_DBG_KRY_DENSE_MV = 12,
  NSK_DBG_KRY_MULTI_DOT_ALL = 13, NSK_DBG_KRY_MULTI_AXPY_ALL = 14, NSK_DBG_KRY_MULTI_ADD = 15,
  NSK_DBG_KRY_MULTI_DOT_ALL_F32 = 16, NSK_DBG_KRY_MULTI_AXPY_ALL_F32 = 17, NSK_DBG_KRY_GS_COLUMN_F32 = 18,
  NSK_DBG_KRY_EQU = 19, NSK_DBG_KRY_EQU_F32 = 20
};
int nsk_debug_krylov(struct nsk_handle_s *h, int op, int n, int m, int offset, const double *par, int n_vec,
                     double *const *vec, const int64_t *len, double *slots64, int32_t *info8);
/* Test hook for the sparse matrix-vector kernels (tests/test_gpu_spmv_kernels.py): ONE kernel form on the caller's CSR.
 * The matrix goes into a Csr the way nsk_set_block_csr fills one (pick_lpr, Csr::build_stream_plan, and for the form
 * asked for Csr::build_blocked / refresh_blocked / refresh_f32, the combined row runs of jacobian_vmult for the two-
 * matrix forms) and the product is launched through the nsk:: launchers, so the plan builder and the kernel are tested
 * together.  A form the plan refuses is reported (return value 1, info[15] says why), never forced.
 * A: the matrix with its operand (x_own: n_own_cols doubles, x_ghost: n_cols - n_own_cols); B: the second matrix over
 * the same rows (two-matrix forms; else null).  y (n_rows, in/out), z (n_rows or null: mode 1 adds to y, mode 2 needs
 * it), d / dinv (n_rows, the epilogue form).  Every device vector is an allocation of its own between guard words (all
 * bits set).  misalign: bit 0 the ghost tails, bit 1 B's x_own, bit 2 y (and z) start 8 bytes off a 16-byte boundary —
 * what the call sites promise for them and no more (the ghost tail p + n, pb(x), yb + n_u); bit 2 is refused for the
 * forms that store pairs (R = 2).  lpr: lanes per row of the CSR-vector form, 0 = pick_lpr.  mode: 0 y = A x, 1 y = (z
 * or y) + A x, 2 y = z - A x (CSR-vector and stream fp64 only).  [c0, c1): the runs launched, as spmv_halo launches
 * sub-ranges of one plan; c0 < 0: all of them (the only choice for CSR-vector and the two-matrix forms).
 * rowblk_out (may be null): the first min(runs + 1, rowblk_cap) entries of the row-run plan that was used.
 * info16: [0] form launched (-1 none), [1] VEC of the stream kernel as its launcher returns it (2 / 3; 0: other forms,
 * or an empty run range: nothing launched), [2] lanes per row of the CSR-vector kernel as its launcher returns them
 * (else pick_lpr's choice), [3] R, [4] C, [5] stream_ok, [6] even_rows, [7] blk_ok, [8] runs of the
 * plan used, [9] [10] its interior run range, [11] longest run in rows, [12] in entries (blocks for the blocked forms,
 * both matrices together for the two-matrix forms), [13] guard words that changed, [14] runs launched, [15] why the
 * plan refused: 0 it did not, 1 a row above kStreamNnz, 2 no R x C node structure or a block row above kBlkMax, 3 the
 * first matrix has an odd row pointer (the two-matrix stream form needs even_rows), 4 a row of both matrices together
 * above the cap, 5 (NSK_DBG_SPMV_STREAM_I16) a run spans 65 536 columns or more.  Device and stream of the handle; 0, 1 or
 * a negative error code.
 * NSK_DBG_SPMV_STREAM_I16: the stream kernel on 16-bit column offsets (Csr::build_index16), modes as
 * NSK_DBG_SPMV_STREAM; NSK_DBG_SPMV_STREAM_I16_F32: the same on the fp32 copy of the values (y = A x, and
 * y = z - A x for the Schur AMG's level 0 under NSK_OPT_AMG_PRECISION = 32; mode 1 has no kernel there: -1).
 * NSK_DBG_SPMV_STREAM_F32 takes modes 1 and 2 as well (the velocity AMG's operators under NSK_OPT_AMG_PRECISION = 32).
 * NSK_DBG_SPMV_BLK22_RES / _RES_F32: y = z - A x on 2 x 2 node blocks, double / fp32 values (mode 2 only) — the
 * double form exists for this hook alone, no product of the library launches it. */
enum {
  NSK_DBG_SPMV_CSRV = 0, NSK_DBG_SPMV_STREAM = 1, NSK_DBG_SPMV_STREAM_F32 = 2, NSK_DBG_SPMV_BLK22 = 3,
  NSK_DBG_SPMV_BLK21 = 4, NSK_DBG_SPMV_BLK12 = 5, NSK_DBG_SPMV_BLK11 = 6, NSK_DBG_SPMV_BLK22_F32 = 7,
  NSK_DBG_SPMV_BLK21_EPI = 8, NSK_DBG_SPMV_STREAM2 = 9, NSK_DBG_SPMV_BLK_FUSED = 10, NSK_DBG_SPMV_STREAM_I16 = 11,
  NSK_DBG_SPMV_STREAM_I16_F32 = 12, NSK_DBG_SPMV_BLK22_RES = 13, NSK_DBG_SPMV_BLK22_RES_F32 = 14
};
struct nsk_dbg_spmv_mat {
  int32_t n_rows, n_cols, n_own_cols, pad_;
  const int32_t *rowptr, *col;
  const double *val, *x_own, *x_ghost;
};
int nsk_debug_spmv(struct nsk_handle_s *h, int form, int lpr, int mode, int misalign, int c0, int c1,
                   const struct nsk_dbg_spmv_mat *A, const struct nsk_dbg_spmv_mat *B, double *y, const double *z,
                   const double *d, const double *dinv, int32_t *rowblk_out, int rowblk_cap, int32_t *info16);
/* Test hook for the triangular-solve kernels (tests/test_gpu_tri_kernels.py): ONE TriSolve on the caller's square CSR,
 * built the way the handle builds its factors — analyze, numeric, apply — so that the plan builders and the kernels are
 * tested together; n_apply applies in a row on the one factor (the sentinel the single-launch kernels leave behind for the
 * next apply is state).  Device and stream of the handle.
 * In: the matrix (sorted rows, every column < n, a diagonal entry in every row), kind 0 ILU(0) / 1 SGS, ordering 0 the
 * caller's / 1 multicolour, sub_off (n_sub + 1 offsets of emulated sub-domains, or null), xy (2 doubles per row, or null)
 * and group (members per line group), and what the handle sets on a factor from its options: want_block2, use_stream,
 * sync_free, tiny_bytes, host_analysis, want_index16, want_f32, x_layout (NSK_IOPT_TRI_X_LAYOUT: 0 or 2; the colour-ordered
 * vector exists for the blocked single-launch solve alone — asked for without want_block2 and sync_free the hook returns 1,
 * info[16] = 1, and launches nothing).  b: n_apply right-hand sides of n doubles; x: as many vectors, in (what the
 * kernels find there) and out.
 * Out: x per apply; perm_out[new] = old (the identity in the caller's order); factor_out: the combined factor `val` at the
 * positions of the CALLER's entries (through srcpos) — ILU(0): L below the diagonal (unit diagonal not stored), U on and
 * above it; SGS: the matrix' own values — with NaN at the entries the analysis dropped (cross-shard columns).
 * b, x (one allocation per apply each) sit between guard words, all bits set; the factor's intermediate vector y and
 * the colour-ordered working vector xc, which the kernels address from the start of their allocations, have guard words
 * BEHIND them only (a write in front of either is not seen).
 * info40: [0] the branch apply() took (TRI_PATH_* of nsk_tri.hpp: 1 scalar single-launch, 2 scalar per-colour, 3 blocked
 * single-launch, 4 blocked per-colour, 5 ring, 6 level walker), [1] bits of the off-diagonal values that branch reads
 * (64 / 32), [2] [3] index width of the lower / upper half (16 / 32; 0: the branch reads no scalar halves), [4] gmax,
 * [5] colours, [6] [7] levels of L / U, [8] runs and [9] padding runs of the lower half's single-launch grid, [10] [11] of
 * the upper half's, [12] rows and [13] entries (blocks for the blocked factor) of the longest run of either half,
 * [14] sf_err was raised, [15] guard words that changed, [16] why the hook refused (0: it did not), [17] what was asked
 * for and not granted: bit 0 want_block2 (no node structure, odd n, the caller's order), bit 1 want_index16 (a run spans
 * 65 536 columns or more, or no scalar halves), bit 2 want_f32 (the branch reads the double factor), bit 3 the ring (the
 * caller's order and 4096 rows or more — the hook's reading of when analyze() tries — and ring_ready false), [18] lanes per row of the walker's level steps, [19] level steps and
 * [20] serial steps of the walker's schedule of the lower half, [28] [29] of the upper half (what the walker launches when
 * it is the branch taken), [21] the factor is below tiny_bytes (TriSolve::last_tiny, recorded by apply()), [22] passes of the lower ring (0: no ring was built),
 * [23] level and [24] serial launches of the ILU(0) factorisation (0 for SGS), [25] stream_ready, [26] block2_ready,
 * [27] the symbolic set-up ran on the device (TriSolve::dev_analysis, recorded by analyze()), [30] longest row of the restricted pattern, [31] entries kept, [32] the
 * blocked single-launch solve ran on the colour-ordered working vector (PERMX of tri_blk_sf_kernel); the rest 0.
 * 0, 1 (refused) or a negative error code (-31 no diagonal, -32 a row above 448 entries, ...). */
struct nsk_dbg_tri_args {
  int32_t n, kind, ordering, n_sub;
  const int32_t *rowptr, *col;
  const double *val;
  const int32_t *sub_off;
  const double *xy;
  int32_t group, want_block2, use_stream, sync_free;
  double tiny_bytes;
  int32_t host_analysis, want_index16, want_f32, x_layout;
  int32_t n_apply, pad_;
  const double *b;
  double *x;
  int32_t *perm_out;
  double *factor_out;
};
int nsk_debug_tri(struct nsk_handle_s *h, const struct nsk_dbg_tri_args *a, int32_t *info40);
/* Test hook for the kernels of the AMG set-up (tests/test_gpu_amg_kernels.py): ONE operation `op` on the caller's
 * arrays, through the amgk:: launcher or the function of nsk_amg.cpp the set-up calls (Scratch::scan, product_rows and the
 * fill as row_product runs it, transpose(), aggregate()).  Device and stream of the handle.
 * Every device array the operation reads or writes is an allocation of its own at its exact size — the scratch the
 * functions of nsk_amg.cpp take included: the hook's Scratch hands out exact allocations instead of 256-byte slices —
 * between 64 guard words (32 bits each, all bits set) on either side; the level operators transpose() allocates for its
 * result are the one exception (plain allocations of the library's own).  Arrays the operation does not write everywhere
 * (`flag_out`, MIS_PULL's out) start as the caller's array, or with all bits set where the caller gives none.
 * Inputs are checked on the host: a row pointer that does not start at 0 or decreases -58, a column, aggregate id or
 * key index out of range -59, everything else -61; nothing out of range reaches a kernel.
 *   SCAN          n, i_in                          Scratch::scan: i_out[0..n], out64[0] = the 64-bit total (also when the
 *                                                  scan ends with -80)
 *   BLOCK         A, r0, r1                        block_count, scan, block_fill: out_rp, out_col, out_val, out64[0] = nnz
 *   DIAG          A                                d_out = ad, d_out2 = dinv
 *   STRENGTH      A, ad, threshold, flag_words     flag_out (flag_words 16-bit words, must be amgk::flag_words), k_out = key,
 *                                                  i_out = agg, out64[0] = undecided
 *   MIS_PULL      A, flag, key, i_in = need, pass, stamp, key2 (pass 2: pass 1's result; pass 1 reads key, as the set-up
 *                                                  does), k_out in/out
 *   MIS_DECIDE    n, key, key2                     k_out, out64[0] = undecided
 *   MIS_MARK      A, flag, key, stamp, i_in = need i_out = need
 *   ROOTS         n, key, i_in = agg, first        root_flags, scan, root_ids: i_out = agg, out64[0] = roots
 *   JOIN          A, flag, key, roots_only, i_in = agg_in, i_out = agg_out in/out
 *   AGG_WEIGHTS   n, i_in = agg, nc                agg_sizes, agg_weights: i_out = count (nc), d_out = pw (nc)
 *   AGGREGATE     A, ad                            aggregate(): i_out = agg, d_out = pw (the first out64[0] entries),
 *                                                  out64[0] = nc, [1] = independent-set rounds, [2] = rounds whose pass 1 ran stamped
 *   PRODUCT       A, product, first_tier; product 0: B; product 1: i_in = agg, pw, dinv, c, nc
 *                                                  product_rows, then the fill of the tier it chose: out_rp, out_col, out_val,
 *                                                  out64[0] = nnz, [1] = the tier used, [2] = error word after the fill,
 *                                                  [4 + t] = error word of a count at tier t >= first_tier (-1: not run)
 *   PRODUCT_COUNT the same inputs                  product_count at tier first_tier alone: i_out = len (n), out64[0] = error word
 *   TRANSPOSE     A                                transpose(): out_rp, out_col, out_val (rows sorted), out64[0] = nnz
 *   ROWS_SORT     A (rows in any order)            out_col, out_val
 *   START_VECTOR  n                                d_out = x
 * out_col / out_val hold out_cap entries (-61 when the result has more).  The fill of a row product is only ever launched
 * on the row pointers of a count of the same tier whose error word was 0, as in the set-up: no call asks for another.
 * info16: [0] guard words that changed, [1] product, [2] lanes per row and [3] hash slots of the last row-product launch,
 * [4] bit 0 a count ran, bit 1 a fill ran, [5] launches of mis_pull<1> stamped, [6] of mis_pull<1> over all rows, [7] of
 * mis_pull<2>, [8] of join with roots_only 1, [9] with roots_only 0, [10 + t] counts and [13 + t] fills launched at tier t.
 * 0 or the library's negative error code (-80, -81, -84 as the set-up throws them). */
enum {
  NSK_DBG_AMG_SCAN = 0, NSK_DBG_AMG_BLOCK = 1, NSK_DBG_AMG_DIAG = 2, NSK_DBG_AMG_STRENGTH = 3, NSK_DBG_AMG_MIS_PULL = 4,
  NSK_DBG_AMG_MIS_DECIDE = 5, NSK_DBG_AMG_MIS_MARK = 6, NSK_DBG_AMG_ROOTS = 7, NSK_DBG_AMG_JOIN = 8,
  NSK_DBG_AMG_AGG_WEIGHTS = 9, NSK_DBG_AMG_AGGREGATE = 10, NSK_DBG_AMG_PRODUCT = 11, NSK_DBG_AMG_PRODUCT_COUNT = 12,
  NSK_DBG_AMG_TRANSPOSE = 13, NSK_DBG_AMG_ROWS_SORT = 14, NSK_DBG_AMG_START_VECTOR = 15
};
struct nsk_dbg_amg_mat {
  int32_t n_rows, n_cols;
  const int32_t *rowptr, *col;
  const double *val;
};
struct nsk_dbg_amg_args {
  int32_t op, n, r0, r1, pass, stamp, roots_only, first, product, first_tier, nc, out_cap;
  int64_t flag_words;
  double threshold, c;
  struct nsk_dbg_amg_mat A, B;
  const int32_t *i_in;
  const uint64_t *key, *key2;
  const uint16_t *flag;
  const double *ad, *dinv, *pw;
  int32_t *i_out;
  uint64_t *k_out;
  uint16_t *flag_out;
  double *d_out, *d_out2;
  int32_t *out_rp, *out_col;
  double *out_val;
  int64_t *out64;   /* 8 */
};
int nsk_debug_amg(struct nsk_handle_s *h, const struct nsk_dbg_amg_args *a, int32_t *info16);
/* Which index width the scalar stream kernels of block b (NSK_BLK_S or NSK_BLK_MP) run on after the set-up: out3 = {the
 * block's SpMV, the lower half of its triangular factor, the upper half}; 16: 16-bit offsets, 32: int32 column ids, 0: that
 * operation does not go through the scalar stream kernels on this handle. */
int nsk_debug_index_width(struct nsk_handle_s *h, int b, int32_t *out3);
/* The rule that chooses a block's SpMV kernel (nsk::spmv_form) on bare flags: no handle, no device.  Returns
 * 0 CSR-vector, 1 stream, 2 stream on the fp32 values, 3 blocked, 4 blocked on the fp32 values.  (Declared in
 * include/nsk.h as well: solver.EXPORTS lists it, and that list is the public header's.) */
int nsk_debug_spmv_form(int blk_ok, int stream_ok, int inner32, int use_stream, int use_bsr, int mode, int inner);
/* The rule that chooses the kernel of a product inside the velocity AMG's V-cycle (nsk::amg_spmv_form) on bare
 * flags: no handle, no device.  Same return values.  amg32 = 0 gives nsk_debug_spmv_form(blk_ok, stream_ok, 0, 1, 0, mode, 0)
 * whatever use_bsr and aligned16 are. */
int nsk_debug_amg_spmv_form(int blk_ok, int stream_ok, int amg32, int use_bsr, int mode, int aligned16);
/* One operator of the velocity AMG of the current set-up (built first when it is pending, as nsk_amg_info does), in double as
 * the set-up left it — also under NSK_OPT_AMG_PRECISION = 32, whose fp32 copies are these values rounded.  which: 0 the
 * level's A (n x n; n, nnz from nsk_amg_info), 1 P (n x n of the next level), 2 R (its transpose); 3 is a query: returns 1
 * when the level holds a dense inverse (the coarsest level up to 2 048 rows), else 0, and copies nothing.  rowptr (rows + 1),
 * col, val (nnz each) may each be null; all null is the size query.  dinv_or_inverse (which 0, may be null): the level's
 * dinv, n doubles, or where the level holds a dense inverse that, n x n row-major.  Returns the operator's number of
 * entries, or a negative error code (-61: no such shard, level or operator — the last level has no P and R; -62: the
 * set-up has no AMG). */
int64_t nsk_debug_amg_level(struct nsk_handle_s *h, int shard, int level, int which, int32_t *rowptr, int32_t *col, double *val,
                            double *dinv_or_inverse);
/* Products the V-cycles of the current hierarchy have launched since it was built, by kernel form: out5[f], f as
 * nsk_debug_spmv_form returns it (0 CSR-vector .. 4 blocked on fp32 values); all 0 without an AMG. */
int nsk_debug_amg_forms(struct nsk_handle_s *h, int64_t *out5);
/* The same for the hierarchy of S (NSK_OPT_SCHUR_AMG); all 0 while the set-up preconditions S with ILU(S). */
int nsk_debug_schur_amg_forms(struct nsk_handle_s *h, int64_t *out5);
/* nsk_debug_amg_spmv_form with the rule's last argument: blk_residual = 0 gives nsk_debug_amg_spmv_form's value
 * for every combination of the others; 1 gives 3 (blocked) exactly where amg32 = 0, mode = 2, blk_ok, use_bsr and aligned16
 * all hold, and that value everywhere else. */
int nsk_debug_amg_spmv_form2(int blk_ok, int stream_ok, int amg32, int use_bsr, int mode, int aligned16, int blk_residual);
/* The two parsers of the set-up's environment overrides (nsk_handle.hpp) on the caller's text, which may be null: no handle,
 * no device, no environment read.  kind 0, a precision (NSK_FACTOR_PRECISION and its kin): 32 or 64, else 0 = unset;
 * kind 1, a switch (NSK_SCHUR_AMG and its kin): 0 or 1, else -1 = unset.  Any other kind: -2. */
int nsk_debug_env_parse(int kind, const char *text);
/* What a set-up of (type, variant) takes of the options and the environment (resolve_setup, nsk_handle.hpp) on bare
 * integers: no handle, no device, no environment read.  req9: factor_precision, inner_matrix_precision,
 * inner_basis_precision, amg_precision, matrix_free_f, schur_amg, asimple_velocity_amg, amg_fused_cheby, velocity_amg as
 * nsk_set_option stores them; env8: the first eight as the parsers return them.  out12: factor32, amg_bits_F, want_amgF,
 * fused_cheby, want_amgS, amg_bits_S, inner32, matfree, basis32, kindF, kindP, velocity_amg_wanted.  Returns 12. */
int nsk_debug_setup_plan(const int *req9, const int *env8, int type, int variant, int *out12);
/* Fused smoother steps the V-cycles of the velocity hierarchy have launched since it was built; 0 without one. */
int nsk_debug_amg_fused(struct nsk_handle_s *h, int64_t *out1);
/* ONE fused Chebyshev step alone (nsk::spmv_blk22_cheby) on the caller's CSR matrix A (as nsk_debug_spmv takes
 * it: x_own is x_in, x_ghost the ghost tail; n_own_cols >= n_rows; built into 2 x 2 node blocks as nsk_set_block_csr
 * builds F) and b, dinv, w of n_rows doubles, and the two launches it replaces on the same device data: r_ref = b - A x_in
 * (spmv_blk22_residual, or the fp32 blocked form), then vec_cheby_step(c1, c2, dinv, r_ref, w, x) on copies of w and of
 * x_in's first n_rows entries.  fp32 != 0: both on the fp32 copy of the blocks.  Out (n_rows doubles each, may be null):
 * w_out, x_out of the fused launch; r_ref, w_ref, x_ref of the two.  Every device vector sits between guard words;
 * info4 = {guard words that changed, runs launched, refusal, 0}.  in_place != 0 asks for x_out == x_in: the launcher's
 * refusal comes back as -61 and nothing is launched.  Returns 0; 1 when nothing was launched because the pattern has no
 * 2 x 2 node structure or a block row is above the run cap (info4[2] = 2, as nsk_debug_spmv); a negative error code. */
int nsk_debug_cheby_fused(struct nsk_handle_s *h, const struct nsk_dbg_spmv_mat *A, const double *b, const double *dinv,
                          const double *w, double c1, double c2, int fp32, int in_place, double *w_out, double *x_out,
                          double *r_ref, double *w_ref, double *x_ref, int32_t *info4);
/* Work vectors of the handle's three pools: out6 = {allocated, free} of the velocity, the pressure and the block pool. */
int nsk_debug_pool_counts(struct nsk_handle_s *h, int32_t *out6);
/* Read-only view of what the last nsk_assemble left on a Q3/Q2 handle (tests/test_gpu_asm_kernels.py): copies
 * `what` into out (cap: its size in bytes) and launches nothing.  NSK_DBG_ASM_CQ: the state at the quadrature points,
 * n_cells * 144 doubles ([cell][u0 u1 g00 g01 g10 g11 p uold0 uold1][q]); _D0: the Dirichlet diagonal, 1 double; and what
 * nsk_assembly_set_cells derived from the connectivity: _NODE_CELLS n_nodes * 4 int32 (cell * 16 + local node, -1 unused),
 * _NODE_OFF n_nodes * 64 uint8 (block offset of (cell slot k, column node m) in the node's rows), _NODE_SELF n_nodes
 * int32 (offset of the diagonal block), _PDOF_CELLS n_p * 4 int32 (cell * 9 + local DoF).  Returns the number of bytes
 * copied; -66 before the first assembly (or when block (0,0) or the cell data were written since) and on simplex handles,
 * -61 when cap is too small, -65 for an unknown `what`. */
enum { NSK_DBG_ASM_CQ = 0, NSK_DBG_ASM_D0 = 1, NSK_DBG_ASM_NODE_CELLS = 2, NSK_DBG_ASM_NODE_OFF = 3,
       NSK_DBG_ASM_NODE_SELF = 4, NSK_DBG_ASM_PDOF_CELLS = 5 };
int64_t nsk_debug_asm(struct nsk_handle_s *h, int what, void *out, int64_t cap);
#ifdef __cplusplus
}
#endif
