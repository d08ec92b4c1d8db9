/*
 * nsk.h — C ABI of the MI355X-native velocity-pressure linear-solve path.
 *
 * Drop-in boundary for what the reference does inside
 *   int NSSolverStationary::solve_system()   lab_new/src/NSSolverStationary.cpp:579-647
 *   int NSSolver::solve_system()             lab_new/src/NSSolver.cpp:601-672
 * i.e. "build PreconditionBlockDiagonal / BlockTriangular / aSIMPLE from blocks of
 * jacobian_matrix and pressure_mass, run SolverGMRES / SolverFGMRES / SolverBicgstab
 * on (jacobian_matrix, delta_owned, residual_vector), return last_step()".
 *
 * The reference has no FFI layer (duck-typed C++ templates over deal.II/Trilinos
 * objects); these entry points are what a binding on the reference side would call
 * with the raw arrays of its Epetra objects (INTEGRATION.md shows that stub):
 *   jacobian_matrix.block(i,j).trilinos_matrix().ExtractCrsDataPointers(rowptr,col,val)
 *   ColMap().MyGlobalElements()  -> ghost ids,  Importer() -> halo plan
 *   residual_vector.block(b).trilinos_vector()[0] -> contiguous owned f64
 *
 * Conventions: plain pointers and sizes only; host pointers are caller-owned and only
 * read/written during the call; the library owns all device memory; one opaque handle
 * per rank/GPU; calls on one handle are not thread-safe; collective calls
 * (nsk_setup_preconditioner, nsk_solve*, nsk_spmv with nranks > 1) must be entered by
 * all ranks.  No exception crosses this ABI.
 *
 * Return codes: 0 success; 1 outer solver not converged (iters/final_res still valid —
 * the reference would throw SolverControl::NoConvergence); 2 BiCGStab breakdown
 * restarts exhausted; 3 an inner (preconditioner) solver did not converge;
 * < 0 usage / HIP / RCCL error, text via nsk_last_error():
 *   -10..-11 HIP runtime / out of device scalar slots      -20..-25 RCCL / in-process group transport (-25: a peer of the in-process group failed or left)
 *   -30..-32 triangular-solve analysis (missing diagonal, row too long)
 *   -40..-47 missing blocks, bad preconditioner / solver type, call order
 *   -48 NSK_OPT_INNER_MATRIX_PRECISION = 32: a value of F, S or M_p is finite in fp64 but outside the range of fp32
 *       (NSK_OPT_AMG_PRECISION = 32: the same for a value of A, P or R on a level of the velocity AMG, when it is built)
 *   -50..-59 bad arguments of the hand-off calls           -60..-66 device assembly / Newton state
 *   -69, -71..-73 forces / output patches from the resident state (-69: no cells, or no faces / edges handed over; -71:
 *        faces or a record list on a P2/P1 handle, edges or patches on the other kind; -72: a cell index out of range;
 *        -73: no state); the record calls also -69 without a record list and -60 for subdivisions outside 1..4; the
 *        record's derived fields also -69 without gradient tables, -60 for another mask, -71 under a point list
 *   -70 single-launch triangular solve gave up waiting AND the per-colour retry failed too (see NSK_OPT_TRI_SYNC_FREE)
 *   -80..-85 AMG set-up (operator too large for 32-bit indices, rows too wide, rounds / estimates that do not end; -85:
 *        NSK_OPT_SCHUR_AMG, a level's diagonal with both signs or a zero — the set-up falls back to ILU(S), see there;
 *        under NSK_OPT_ASIMPLE_VELOCITY_AMG these codes do not reach the caller either: the set-up falls back to ILU(F))
 *   -1 any other exception
 */
#ifndef NSK_H
#define NSK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nsk_handle_s *nsk_handle;

/* matrix blocks of the hand-off */
enum {
  NSK_BLK_F = 0,        /* jacobian_matrix.block(0,0)            NSSolverStationary.cpp:584,602,622 */
  NSK_BLK_BT = 1,       /* jacobian_matrix.block(0,1)            NSSolverStationary.cpp:624         */
  NSK_BLK_B = 2,        /* jacobian_matrix.block(1,0)            NSSolverStationary.cpp:604,623     */
  NSK_BLK_MP = 3,       /* pressure_mass.block(1,1)              NSSolverStationary.cpp:585,603     */
  NSK_BLK_BT_GHOST = 4, /* rows of block(0,1) for this rank's ghost velocity DoFs: what EpetraExt's
                           MatrixMatrix::Multiply imports for mmult (NSSolverStationary.hpp:275);
                           only needed when nranks > 1 and the preconditioner is aSIMPLE */
  NSK_BLK_S = 5         /* Schur approximation B diag(F)^-1 B^T (read-only, built by the library) */
};
enum { NSK_SPACE_U = 0, NSK_SPACE_P = 1 };
enum { NSK_SOLVER_GMRES = 0, NSK_SOLVER_FGMRES = 1, NSK_SOLVER_BICGSTAB = 2 };          /* -s */
enum { NSK_PREC_BLOCK_DIAGONAL = 0, NSK_PREC_BLOCK_TRIANGULAR = 1, NSK_PREC_ASIMPLE = 2 }; /* -p */
enum { NSK_VARIANT_STATIONARY = 0, NSK_VARIANT_UNSTEADY = 1 };
/* which triangular preconditioner object */
enum { NSK_TRI_VELOCITY = 0, NSK_TRI_PRESSURE = 1 };

/* options (nsk_set_option) */
enum {
  NSK_OPT_TRI_ORDERING = 0, /* 1 (default): rank-local multicolour permutation for ILU(0)/SGS (few, wide levels);
                               0: the caller's DoF order — exactly what one MPI rank of the reference factorises,
                               but O(nx+ny) narrow levels */
  NSK_OPT_SUBDOMAINS = 1,   /* emulated MPI ranks per GPU for the block-Jacobi ILU/SGS (default 1) */
  NSK_OPT_FUSE_BLOCK_ROW = 2, /* 1 (default): F x_u + Bt x_p in one kernel */
  NSK_OPT_STREAM_KERNELS = 3, /* 1 (default): LDS-staged CSR-stream kernels; 0: CSR-vector kernels */
  NSK_OPT_INNER_FUSED_GS = 4, /* 1 (default): inner FGMRES (on F) orthogonalises with fused classical Gram-Schmidt
                                 (two sweeps, 8 vectors per pass); 0: deal.II's modified Gram-Schmidt (add_and_dot);
                                 2: as 1 with the norm of the new vector from |w|^2 - sum h_i^2 — one cross-rank
                                 reduction per inner iteration instead of two (made for several GPUs; the inner solve
                                 only has to reach 1e-1 relative) */
  NSK_OPT_OUTER_FUSED_GS = 5, /* same for the outer FGMRES; default 0 (modified Gram-Schmidt, as deal.II) */
  NSK_OPT_CG_SINGLE_REDUCTION = 11, /* 0 (default): inner CG (on S / Mp) with deal.II's recurrence — three reductions per
                                 iteration; 1: Chronopoulos-Gear form, ONE fused reduction (one all-reduce) per iteration:
                                 same iterates in exact arithmetic, one more preconditioner + matrix application per solve.
                                 For several GPUs, where every reduction is a latency-bound collective */
  NSK_OPT_BSR_VELOCITY = 7,   /* 1 (default): SpMVs with the jacobian blocks use 2x2 / 2x1 / 1x2 node-block copies when the pattern allows */
  NSK_OPT_TRI_SYNC_FREE = 9,  /* multicolour triangular solves in ONE launch instead of one per colour: rows wait in-kernel for
                                 the entries they depend on (bounded spins on sentinel-filled working vectors, see
                                 csrc/nsk_kernels.h).  0: one launch per colour; 1: scalar factors (S, Mp: one persistent launch
                                 for both halves, all workgroups resident); 2 (default): also the 2x2-blocked velocity factor
                                 (one launch per half).  If a wait ever runs out, the solve is redone with 0 (status 0,
                                 nsk_stats.sync_free_fallbacks counts it) */
  NSK_OPT_VELOCITY_AMG = 10,  /* stationary blockTriangular: 1 (default) precondition F with the smoothed-aggregation AMG
                                 V-cycle (the reference configures TrilinosWrappers::PreconditionAMG there,
                                 NSSolverStationary.hpp:225,231); 0: ILU(0), as the unsteady variant does */
  NSK_OPT_TRI_LINE_GROUPS = 12, /* 2 (default): as 1 for factors small enough to be bound by the chain of colour hand-offs
                                 (velocity block <= 4 M rows, pressure blocks <= 1 M rows per rank: where it was measured to
                                 pay), as 0 for larger ones.  1: when support points were handed over (nsk_set_support_points) the multicolour
                                 ordering colours short LINE GROUPS — neighbours on a line of constant y: pairs of velocity
                                 nodes, triples of pressure DoFs — instead of single DoFs, and the members of a group are
                                 solved one after the other inside a workgroup: fewer colours (12 instead of 17-18 for F,
                                 17 instead of 29-31 for the Schur complement on the reference's lattices) at the same or
                                 lower inner iteration counts; still ILU(0)/SGS of a symmetrically permuted matrix
                                 (nsk_tri_get_perm).  0: colour the DoFs one by one */
  NSK_OPT_MASS_ORDERING = 13,  /* ordering of the pressure-mass factor alone: 0 the caller's order, 1 multicolour, -1 (default)
                                 the caller's order in the UNSTEADY block-diagonal preconditioner and NSK_OPT_TRI_ORDERING
                                 everywhere else.  There the pressure block is about ONE ILU(M_p)-preconditioned CG step
                                 (absolute tolerance 1e-1, NSSolver.hpp:155-176) and whether restarted FGMRES converges hangs
                                 on the quality of that one application: the caller's order reproduces
                                 the factor one MPI rank of the reference builds (same iteration counts as the CPU
                                 restatement: 241 / 403 at 100x70), at O(nx + ny) dependent levels per application */
  NSK_OPT_SCHUR_SIGN = 14,     /* +1 (default): aSIMPLE's S = B~ D^-1 B~^T exactly as the reference forms it
                                 (NSSolverStationary.hpp:275, NSSolver.hpp:288).  -1: S = -B~ D^-1 B~^T, the Schur-complement
                                 approximation SIMPLE is derived with for J = [[F, B~^T], [B~, 0]] — a LABELLED DEVIATION from
                                 the reference, off by default: with the reference's sign the pressure correction comes out
                                 negated, the preconditioned operator has eigenvalues near +1 (velocity) and near -alpha
                                 (pressure), and restarted FGMRES(30) crawls on the indefinite spectrum (3 062
                                 against 580 outer iterations to 1e-10 at 60x20 in the CPU restatement).  Every parity test,
                                 the drivers and the bench headline keep +1 */
  NSK_OPT_BLAS1_PAIRS = 15,    /* dot products / norms / fused Gram-Schmidt sums read PAIRS of entries through 16-byte loads
                                 (6.3+ TB/s instead of 4.0-5.4 with 8 bytes per lane): 1 on, 0 off, -1 (default) on in the
                                 STATIONARY preconditioner variant, off in the unsteady one.  Another lane decomposition is
                                 another summation order, i.e. other last bits in every Krylov coefficient — harmless where
                                 solves converge with room (stationary: iteration counts within a per cent), decisive where
                                 restarted FGMRES sits on an edge: BASELINE config 5's first time step at 600x200 (-p 0) takes
                                 1 061 / 865 / 1 363 outer iterations with the 8-byte sums and 1 162 / no convergence in 100 000
                                 with the 16-byte ones (profiles/r04_cli_first_level_*) */
  NSK_OPT_FACTOR_PRECISION = 16, /* storage precision of the ILU(0) / SGS factors' OFF-DIAGONAL values in the split halves the
                                 multicolour kernels stream: 64 (default) double, as today; 32: rounded to float once per
                                 set-up (the gather behind the numeric factorisation), and the double copies of those halves
                                 are not kept.  What stays double: the numeric ILU(0) itself (it runs on the double
                                 combined factor), the diagonal data (1/d, the 2x2 node diagonals), every vector and all
                                 arithmetic (values are widened as they are loaded).  Applies to the velocity factor (2x2
                                 node blocks) and the S / Mp factors; factors that take the natural-order ring, the level
                                 walker, the single-workgroup path for tiny factors or the velocity AMG keep double —
                                 nsk_tri_get_value_bytes reports what each holds (the AMG's own switch:
                                 NSK_OPT_AMG_PRECISION).  A LABELLED DEVIATION from the reference,
                                 whose Ifpack factors are double: the outer FGMRES stays double and checks the true residual,
                                 the preconditioner alone is perturbed.  Other values: -61.  NSK_FACTOR_PRECISION=32 / 64 in
                                 the environment overrides the option for every handle (A/B runs; other values ignored) */
  NSK_OPT_INNER_MATRIX_PRECISION = 17, /* storage precision of the matrix values the preconditioner's INNER solves multiply by:
                                 the inner FGMRES on F and the inner CG on S (stationary aSIMPLE) or M_p (blockDiagonal,
                                 blockTriangular).  64 (default): double, as today.  32: they read copies of F, S and M_p
                                 rounded to float (F's 2x2 node-block copy, gathered from the double values; S and M_p
                                 scalar), made at every set-up and made again before use whenever the values change
                                 (nsk_update_values, nsk_scale_values, nsk_assemble) without one.  nsk_set_block_csr of
                                 F or M_p hands over a pattern and drops that block's copy: until the
                                 next set-up the inner product of that block reads the double values
                                 (nsk_inner_value_bytes: 8), and the next set-up converts again; a set-up that finds a
                                 value finite in fp64 but outside fp32's range returns -48.  What stays double: vectors,
                                 products, sums and the kernels' LDS partials (values are widened as they are loaded); the
                                 outer J x (fused F | Bt block row, or its per-block SpMVs); B and Bt inside the aSIMPLE
                                 apply; nsk_spmv, nsk_time_op ops 0-5 and nsk_get_block; the numeric ILU(0) and the Schur
                                 SpGEMM, which read the double values.  Blocks whose SpMV takes no stream kernel
                                 (NSK_OPT_STREAM_KERNELS = 0; F without its 2x2 copy, e.g. NSK_OPT_BSR_VELOCITY = 0) stay
                                 double — nsk_inner_value_bytes reports what each inner solve reads.  A LABELLED DEVIATION
                                 from the reference, whose inner solves multiply by the double matrices: every inner solve
                                 stops at a loose tolerance and the outer FGMRES stays double and checks the true residual,
                                 so only the preconditioner is perturbed.  Other values: -61.  NSK_INNER_MATRIX_PRECISION=32
                                 / 64 in the environment overrides the option for every handle (A/B runs; other values
                                 ignored).  Independent of NSK_OPT_FACTOR_PRECISION; the velocity AMG keeps double unless
                                 NSK_OPT_AMG_PRECISION says otherwise */
  NSK_OPT_INNER_BASIS_PRECISION = 18, /* storage precision of the Krylov basis V of the INNER FGMRES on F, which the two fused
                                 Gram-Schmidt sweeps read once each per inner iteration.  64 (default): double, as today and
                                 the same bits.  32: basis vector j IS the rounded vector, v_j = fl32(w / |w|) (owned entries
                                 only), stored by the kernel that also writes it, widened, into ONE double working vector —
                                 the preconditioner reads that, so z_j = M^-1 v_j comes from exactly the stored values and
                                 A Z_m = V_{m+1} H holds to double rounding; V is normalised and orthogonal to ~6e-8 only.
                                 What stays double: w, every coefficient and partial sum, the slots and the all-reduce,
                                 the Householder least squares and the residual estimate, the Z basis and the cycle-end
                                 update.  Takes effect at the next nsk_setup_preconditioner.  The inner solve keeps the
                                 double basis with NSK_OPT_INNER_FUSED_GS = 0 (modified Gram-Schmidt) and with the 8-byte
                                 reduction forms (effective NSK_OPT_BLAS1_PAIRS = 0: the unsteady variant's default) —
                                 nsk_inner_basis_bytes reports what the inner solve reads.  The outer FGMRES basis, GMRES,
                                 BiCGStab and CG are not touched.  A LABELLED DEVIATION from the reference, whose basis is
                                 double: the inner solve stops at a loose tolerance and the outer FGMRES stays double and
                                 checks the true residual, so only the preconditioner is perturbed.  Other values: -61.
                                 NSK_INNER_BASIS_PRECISION=32 / 64 in the environment overrides the option for every handle
                                 (A/B runs; other values ignored).  Independent of the two options above */
  NSK_OPT_INNER_MATRIX_FREE_F = 19, /* how the INNER FGMRES on F multiplies by F on handles that assemble it themselves
                                 (nsk_assembly_set_cells + nsk_assemble: congruent Q3/Q2 cells).  0 (default): the stored
                                 block, as today and the same bits.  1: matrix-free — the same operator in double, applied
                                 from what the last nsk_assemble left on the device (u and grad u at the quadrature points,
                                 the tabulation of the cell, node -> cells, Dirichlet flags and diagonal) without reading a
                                 stored value of F; the sums of asm_F_rows taken in another order, so results differ at
                                 rounding level only.  All three preconditioner types, both variants wherever that solve
                                 exists, the AMG-preconditioned solve included.  Takes effect at the next
                                 nsk_setup_preconditioner.  What keeps the assembled double F: the outer J x and the
                                 true-residual check, nsk_spmv, ILU(0) / SGS, the Schur SpGEMM, the AMG set-up and V-cycle.
                                 VALID only while F holds the values of the last nsk_assemble (or nsk_time_assemble):
                                 nsk_update_values / nsk_scale_values / nsk_set_block_csr of F, nsk_assembly_set_cells,
                                 nsk_assembly_set_dirichlet and nsk_assembly_set_simplex end that, and the next nsk_assemble
                                 restores it.  While it is not valid — and on P2/P1 simplex handles, handles with
                                 nranks > 1 and NSK_OPT_SUBDOMAINS > 1, which are not covered — the stored block is
                                 multiplied and ONE line `[nsk] warning: ...` per handle says so on stderr;
                                 nsk_inner_matrix_free reports which of the two the next product takes.  With
                                 NSK_OPT_INNER_MATRIX_PRECISION = 32 no fp32 copy of F is made while the product is
                                 matrix-free.  Other values: -61.  NSK_INNER_MATRIX_FREE_F=0 / 1 in the environment
                                 overrides the option for every handle (A/B runs; other values count as unset) */
  NSK_OPT_AMG_PRECISION = 20, /* storage precision of the operators the velocity AMG's V-cycle multiplies by (stationary
                                 blockTriangular, NSK_OPT_VELOCITY_AMG = 1).  64 (default): double, as today and the same
                                 bits.  32: the values of every level's A, P and R, on every shard, are stored rounded to
                                 float (nearest even) once the level is finished, and the cycle's products read those:
                                 level 0 that is F itself through F's 2x2 node-block copy (the one the inner solves read
                                 under NSK_OPT_INNER_MATRIX_PRECISION = 32; it exists while either option wants it) with a
                                 y = z - A x node-block kernel, every other operator — coarse levels, P, R, the shards'
                                 diagonal blocks under NSK_OPT_SUBDOMAINS > 1 or several ranks, F without node structure or
                                 under NSK_OPT_BSR_VELOCITY = 0 — through the scalar stream kernels on fp32 values.  What
                                 stays double: the whole set-up (strength, aggregation, the lambda power iterations,
                                 prolongator smoothing, the Galerkin products), every vector, dinv, the coarsest level's
                                 dense inverse and its product, the Chebyshev coefficients, every product, sum and LDS
                                 partial (values are widened as they land), and F itself, which the outer J x, ILU(0), the
                                 Schur SpGEMM and nsk_spmv read.  Takes effect at the next nsk_setup_preconditioner (the
                                 hierarchy is still built on first apply); a value finite in fp64 but outside fp32's range
                                 returns -48 from the call that builds it, naming the level and the operator.
                                 nsk_amg_value_bytes reports what the hierarchy holds.  A LABELLED DEVIATION from the
                                 reference, whose ML hierarchy is double: the V-cycle sits inside the inner FGMRES on F,
                                 which is flexible and stops at a loose tolerance, and the outer FGMRES stays double and
                                 checks the true residual, so only the preconditioner is perturbed.  Other values: -61.
                                 NSK_AMG_PRECISION=32 / 64 in the environment overrides the option for every handle (A/B
                                 runs; other values ignored).  Independent of the three precision options above.  Under
                                 NSK_OPT_SCHUR_AMG it governs the hierarchy of S too: one knob for the operators a V-cycle
                                 multiplies by (S itself, level 0 of one shard, through scalar fp32 values on its 16-bit
                                 column offsets) */
  NSK_OPT_SCHUR_AMG = 21,     /* preconditioner of the inner CG on S in the STATIONARY aSIMPLE set-up (type 2, variant 0).
                                 0 (default): ILU(0) of S, as the reference (Ifpack ILU, NSSolverStationary.hpp:325-326),
                                 as today and the same bits.  1: one V-cycle of a smoothed-aggregation hierarchy of S — the
                                 method, parameters and device set-up of the velocity AMG (nsk_amg_info), built from S at
                                 every nsk_setup_preconditioner right after its values are formed (S changes with every
                                 set-up); sub-domains as NSK_OPT_SUBDOMAINS cuts the pressure space, ghost columns dropped.
                                 ILU(S) is then neither analysed nor factorised: the pressure slot of nsk_tri_apply applies
                                 the cycle, nsk_tri_get_perm gives the identity and nsk_tri_get_value_bytes 0, as the
                                 velocity slot does under the velocity AMG; profile class 21 samples the cycle.  The CG, its
                                 tolerance, its start from the last delta_p and alpha are untouched.  S is symmetric and its
                                 diagonal of one sign, and so is the cycle: CG takes it as it takes ILU(S).  Where the
                                 hierarchy cannot be built — a row of a set-up product over 512 distinct columns (-81), a
                                 diagonal on some level with both signs or a zero (-85), -80..-85 in general — the set-up
                                 factorises ILU(S) as under 0 and ONE line `[nsk] warning: ...` per handle says so on
                                 stderr; nsk_schur_amg_info reports which of the two stands.  Types 0 and 1 and the
                                 unsteady variant ignore the option.  A LABELLED DEVIATION from the reference: the inner
                                 solve stops at 1e-1 and the outer FGMRES checks the true residual, so only the
                                 preconditioner is changed.  Takes effect at the next nsk_setup_preconditioner.  Other
                                 values: -61.  NSK_SCHUR_AMG=0 / 1 in the environment overrides the option for every handle
                                 (A/B runs; other values count as unset) */
  NSK_OPT_ASIMPLE_VELOCITY_AMG = 22
                              /* preconditioner of the inner FGMRES on F in the STATIONARY aSIMPLE set-up (type 2, variant
                                 0).  0 (default): ILU(0) of F, as the reference (Ifpack ILU, NSSolverStationary.hpp:325-326),
                                 as today and the same bits.  1: one V-cycle of the velocity hierarchy — the smoothed-
                                 aggregation AMG of F that blockTriangular uses (nsk_amg_info reports it) — built inside
                                 every nsk_setup_preconditioner; sub-domains as NSK_OPT_SUBDOMAINS cuts the velocity space,
                                 ghost columns dropped.  ILU(F) is then neither analysed nor factorised and its storage is
                                 released: the velocity slot of nsk_tri_apply applies the cycle, nsk_tri_get_perm gives the
                                 identity, nsk_tri_get_value_bytes 0 and nsk_amg_value_bytes the hierarchy's, exactly as
                                 under blockTriangular; profile class 20 samples the cycle.  diag(F), S, the FGMRES, its
                                 tolerance and alpha are untouched.  With one sub-domain level 0 is F itself, read through
                                 its 2 x 2 node blocks (NSK_OPT_BSR_VELOCITY = 1): the residual products take the blocked
                                 kernel and the Chebyshev steps that follow them run in its epilogue — the same bits as the
                                 scalar two-launch steps give, fewer bytes.  NSK_OPT_AMG_PRECISION, NSK_OPT_SCHUR_AMG,
                                 NSK_OPT_INNER_MATRIX_PRECISION and NSK_OPT_INNER_MATRIX_FREE_F combine with it as with
                                 blockTriangular.  Where the hierarchy cannot be built (-80..-85: a row of a set-up product
                                 over 512 distinct columns and its kin) the set-up analyses and factorises ILU(F) as under
                                 0 and ONE line `[nsk] warning: ...` per handle says so on stderr; -48 and HIP errors stay
                                 errors.  (Only the set-up falls back: nsk_set_block_csr of F followed by a solve without a
                                 new nsk_setup_preconditioner rebuilds the hierarchy at its first application, and these
                                 codes then fail that solve.)  Types 0 and 1 and the unsteady variant ignore the option; NSK_OPT_VELOCITY_AMG
                                 keeps meaning blockTriangular only.  A LABELLED DEVIATION from the reference: the inner
                                 solve stops at 1e-1 and the outer FGMRES checks the true residual, so only the
                                 preconditioner is changed.  Takes effect at the next nsk_setup_preconditioner.  Other
                                 values: -61.  NSK_ASIMPLE_VELOCITY_AMG=0 / 1 in the environment overrides the option for
                                 every handle (A/B runs; other values count as unset) */
};

typedef struct {
  double setup_ms, solve_ms;
  int64_t outer_iters, inner_u_its, inner_p_its, prec_applies, spmv_calls, tri_applies, reductions, host_syncs;
  double spmv_bytes, tri_bytes, blas1_bytes; /* algorithmic bytes moved (SURVEY 8d formulas) */
  int32_t n_colors_u, n_levels_u, n_colors_p, n_levels_p;
  int64_t nnz_s;
  int64_t sync_free_fallbacks; /* times a solve fell back to per-colour launches (NSK_OPT_TRI_SYNC_FREE) */
  int64_t cur_outer_iters;     /* progress of the running / last outer solve: iterations done ... */
  double cur_residual;         /* ... and the residual SolverControl saw last (readable from another thread) */
  int64_t overlapped_spmvs;    /* SpMVs whose interior rows ran while the halo exchange was in flight (nranks > 1) */
  int64_t ring_applies;        /* triangular applies in the caller's order that went through the LDS-ring kernel */
  int64_t columns_skipped;     /* FGMRES basis columns that no iterate reads — the one in front of the check that ends a solve,
                                  the last one of a full restart cycle — and that were therefore not built, outer and inner
                                  solves together.  prec_applies, inner_*_its, tri_applies and spmv_calls count work done, so
                                  they do not contain these columns.  Results are the bits of the reference order, with one
                                  exception: stationary aSIMPLE, two solves with new matrix values but NO new
                                  nsk_setup_preconditioner in between — the preconditioner application the first solve did
                                  not need runs in front of the second solve's first one, on the new values */
} nsk_stats;

/* 128-byte RCCL unique id, produced on rank 0 and distributed by the caller (e.g. MPI_Bcast). */
int nsk_get_unique_id(void *out128);

/* Test/development transport: a 128-byte pseudo id that makes the nranks handles created with it in
 * ONE process (one thread per rank) talk through host barriers and device-to-device copies instead
 * of RCCL (which refuses two ranks on one device).  Same data path otherwise. */
int nsk_local_group_id(int nranks, void *out128);

/* One handle per rank.  unique_id may be NULL when nranks == 1. */
nsk_handle nsk_create(int rank, int nranks, int device_id, const void *rccl_unique_id);
void nsk_destroy(nsk_handle h);
const char *nsk_last_error(nsk_handle h);

/* Row partition of one block space: owned global range and ghost global ids (ColMap order). */
int nsk_set_partition(nsk_handle h, int space, int64_t owned_begin, int64_t owned_end, int n_ghost,
                      const int32_t *ghost_gids);
/* Optional: support points of the owned DoFs of one space, xy[2 d] = x, xy[2 d + 1] = y of owned DoF d — what
 * DoFTools::map_dofs_to_support_points(mapping, dof_handler) gives the reference's caller (both velocity components of a
 * node share their point).  Used for the ordering of the triangular factors only (NSK_OPT_TRI_LINE_GROUPS); NULL drops
 * them.  Call after nsk_set_partition and before nsk_setup_preconditioner. */
int nsk_set_support_points(nsk_handle h, int space, const double *xy);
/* Halo plan of one space (what Epetra_Import holds): for neighbour k, send owned local ids
 * send_idx[send_ptr[k]..send_ptr[k+1]) and receive ghost slots [recv_ptr[k], recv_ptr[k+1]). */
int nsk_set_halo_plan(nsk_handle h, int space, int n_neighbors, const int32_t *peer_rank, const int32_t *send_ptr,
                      const int32_t *send_idx, const int32_t *recv_ptr);

/* Local CSR block: int32 local column ids (owned first, ghosts appended), f64 values.
 * The pattern is fixed for the run (jacobian_matrix.reinit(sparsity), NSSolverStationary.cpp:304). */
int nsk_set_block_csr(nsk_handle h, int blk, int n_rows, int n_cols, const int32_t *rowptr, const int32_t *col,
                      const double *val);
/* New values on the same pattern (every Newton iteration). */
int nsk_update_values(nsk_handle h, int blk, const double *val);

int nsk_set_option(nsk_handle h, int opt, double value);

/* Preconditioner::initialize(...)  (NSSolverStationary.hpp:120,176,242; NSSolver.hpp:143,198,263).
 * Symbolic analysis is cached per pattern; numeric work (diag, SpGEMM, ILU) runs on the GPU.
 * The AMG hierarchy of the stationary block-triangular type is built when the preconditioner is first applied (a
 * solve that stops at step 0 never pays for it), from the values block (0,0) holds at that moment: change the block
 * (nsk_update_values, nsk_scale_values, nsk_assemble) and call nsk_setup_preconditioner again before the next solve,
 * as solve_system() does (NSSolverStationary.cpp:621-626). */
int nsk_setup_preconditioner(nsk_handle h, int type, int variant, double alpha);

/* solver.solve(jacobian_matrix, delta_owned, residual_vector, preconditioner):
 * x_u/x_p are the initial guess on entry (delta_owned is not zeroed by the reference) and the
 * solution on exit; *iters = solver_control.last_step(). */
int nsk_solve(nsk_handle h, int solver, double tol_abs, int max_iter, const double *rhs_u, const double *rhs_p,
              double *x_u, double *x_p, int *iters, double *final_res);

/* The same in three steps, for callers that keep vectors resident in HBM between solves. */
int nsk_upload_system(nsk_handle h, const double *rhs_u, const double *rhs_p, const double *x_u, const double *x_p);
int nsk_solve_resident(nsk_handle h, int solver, double tol_abs, int max_iter, int *iters, double *final_res);
int nsk_download_solution(nsk_handle h, double *x_u, double *x_p);

/* ---- single operations of the path (parity tests, micro-benchmarks) ---- */
/* y = A x (add = 0) or y += A x; x has the block's owned column entries (ghosts are imported). */
int nsk_spmv(nsk_handle h, int blk, const double *x_owned, double *y, int add);
/* y = jacobian_matrix * x */
int nsk_jacobian_vmult(nsk_handle h, const double *x_u, const double *x_p, double *y_u, double *y_p);
/* dot(x,y) and ||x||_2 over the owned entries of all ranks */
int nsk_dot(nsk_handle h, int n, const double *x, const double *y, double *dot_out, double *norm_x_out);
/* One vector operation of the path on caller vectors of length n (parity tests of SURVEY 8a row a4).  op: 0 y=x,
 * 1 y=a x (equ), 2 y+=a x (add), 3 y=c y+a x (sadd), 4 y+=a x+c z, 5 y*=a, 6 y.*=d (scale(vec)), 7 y-=d.*x,
 * 8 y=(y-x).*d, 9 y=1/d, 10 add_and_dot: y+=a x, *scalar_out=y.z, 11 y+=a x, *scalar_out=y.y.  y is in/out. */
int nsk_vec_op(nsk_handle h, int op, int n, double a, double c, const double *x, double *y, const double *z,
               const double *d, double *scalar_out);
/* x = M^-1 b with the velocity / pressure preconditioner of the current setup (triangular solves, or one AMG
 * V-cycle for the velocity block of the stationary blockTriangular setup, and for the pressure block of the stationary
 * aSIMPLE set-up under NSK_OPT_SCHUR_AMG) */
int nsk_tri_apply(nsk_handle h, int which, const double *b, double *x);
/* Hierarchy of the velocity AMG of the current setup (replaces TrilinosWrappers::PreconditionAMG,
 * NSSolverStationary.hpp:225): returns the number of levels of sub-domain `shard` (0 when the setup has no AMG)
 * and, for a valid `level`, its size, non-zeros and the lambda_max(D^-1 A) estimate the smoother uses. */
int nsk_amg_info(nsk_handle h, int shard, int level, int64_t *rows, int64_t *nnz, double *lambda_max);
/* bytes per stored value of the operators the V-cycle of the current set-up multiplies by: 4 (NSK_OPT_AMG_PRECISION = 32),
 * 8 (double), 0 when the set-up has no AMG.  Builds a pending hierarchy first, as nsk_amg_info does. */
int nsk_amg_value_bytes(nsk_handle h, int32_t *bytes);
/* Hierarchy of S under NSK_OPT_SCHUR_AMG, with the conventions of nsk_amg_info: the number of levels of sub-domain
 * `shard` — 0 when the current set-up preconditions S otherwise (option off, another type or variant, or the fallback
 * to ILU(S)) — and, for a valid `level`, its size, non-zeros and lambda_max estimate. */
int nsk_schur_amg_info(nsk_handle h, int shard, int level, int64_t *rows, int64_t *nnz, double *lambda_max);
/* x = one V-cycle of that hierarchy on b (owned pressure entries; x is set, not read).  -62 when none stands, -46 before
 * the first set-up. */
int nsk_schur_amg_apply(nsk_handle h, const double *b, double *x);
/* ordering used by that triangular preconditioner: perm[new] = old (identity when natural) */
int nsk_tri_get_perm(nsk_handle h, int which, int32_t *perm);
/* bytes per stored off-diagonal value of that triangular preconditioner as its applies read them in the current set-up:
 * 4 (NSK_OPT_FACTOR_PRECISION = 32 and the factor runs through the split-half kernels), 8 (double), 0 when the slot is no
 * triangular factor (the velocity AMG of the stationary blockTriangular preconditioner; the pressure slot under
 * NSK_OPT_SCHUR_AMG) */
int nsk_tri_get_value_bytes(nsk_handle h, int which, int32_t *bytes);
/* bytes per matrix value the inner solves of the current set-up read for blk (NSK_BLK_F, NSK_BLK_S or NSK_BLK_MP): 4
 * (NSK_OPT_INNER_MATRIX_PRECISION = 32 and the block's SpMV takes a stream kernel), 8 (double), 0 when this set-up runs
 * no inner solve on that block (S under types 0 / 1, M_p under aSIMPLE, every block under the unsteady aSIMPLE) and for
 * F while its inner products are matrix-free (NSK_OPT_INNER_MATRIX_FREE_F = 1 in effect: no stored value is read); -62
 * for other blocks */
int nsk_inner_value_bytes(nsk_handle h, int blk, int32_t *bytes);
/* bytes per entry of the Krylov basis the inner FGMRES on F of the current set-up reads: 4 (NSK_OPT_INNER_BASIS_PRECISION
 * = 32 with the fused Gram-Schmidt sweeps in their pair forms), 8 (double), 0 when this set-up runs no inner FGMRES on F
 * (the unsteady aSIMPLE) */
int nsk_inner_basis_bytes(nsk_handle h, int32_t *bytes);
/* y = A x for blk = NSK_BLK_F, NSK_BLK_S or NSK_BLK_MP with exactly the values, kernel and row runs of the inner solves
 * of the current set-up (same bits as nsk_spmv(.., add = 0) when they read double; the matrix-free product for F while
 * NSK_OPT_INNER_MATRIX_FREE_F = 1 is in effect).  Conventions of nsk_spmv: owned x,
 * ghosts imported, collective when nranks > 1 (the interior rows overlap the halo exchange as in the inner solves). */
int nsk_inner_spmv(nsk_handle h, int blk, const double *x_owned, double *y);
/* *on = 1 when the next product of the inner FGMRES with F would be matrix-free (NSK_OPT_INNER_MATRIX_FREE_F = 1 taken by
 * the last set-up, a set-up with that inner solve, a handle of the covered kind and a valid assembly), else 0 */
int nsk_inner_matrix_free(nsk_handle h, int32_t *on);
/* y = F x by the matrix-free kernels alone, on the state, nu, inv_dt and phase of the last nsk_assemble, whatever the
 * option says (one rank, congruent Q3/Q2 cells; owned x).  -66 when block (0,0) does not hold the values of a device
 * assembly (none yet, or F / the cell data were written since), -65 on simplex handles and with nranks > 1 */
int nsk_matfree_f(nsk_handle h, const double *x_owned, double *y);
/* preconditioner.vmult(dst, src), applied `calls` times on the same object; dst is in/out */
int nsk_precond_vmult(nsk_handle h, const double *src_u, const double *src_p, double *dst_u, double *dst_p,
                      int calls);
/* size and content of a block held by the library (used for NSK_BLK_S) */
int64_t nsk_block_nnz(nsk_handle h, int blk);
int nsk_get_block(nsk_handle h, int blk, int32_t *rowptr, int32_t *col, double *val);
/* Which SpMV kernel a block with these flags runs under these options: the library's one rule on bare values (no handle,
 * no device; described with the other test hooks in csrc/nsk_internal.h).  0 CSR-vector, 1 stream, 2 stream on fp32
 * values, 3 blocked, 4 blocked on fp32 values */
int nsk_debug_spmv_form(int blk_ok, int stream_ok, int inner32, int use_stream, int use_bsr, int mode, int inner);

/* ---------------------------------------------------------------------------------------------------
 * Device assembly of the Newton system and the Newton-loop state.
 * Replaces NSSolverStationary::assemble_system(false, false) (NSSolverStationary.cpp:317-577) for meshes of
 * congruent Q3/Q2 cells (the reference's generated `-m nx,ny` meshes), and the vector updates of solve_newton()
 * (:710-735).  jacobian(0,0) and residual_vector are recomputed on the device from the resident `solution`;
 * blocks (0,1), (1,0) and pressure_mass do not depend on the state and stay as handed over.
 *
 * nsk_assembly_set_cells: the cell loop's connectivity — per cell 16 local velocity NODE ids (local DoF id / 2,
 *   n = b*4 + a) and 9 local pressure DoF ids (what cell->get_dof_indices returns, :532), flags (bit 0: face on
 *   boundary id 8), and the tabulation FEValues / FEFaceValues hold for the congruent cell (:323-331): 944 doubles
 *   phi[16][16], dphi/dx[16][16], dphi/dy[16][16], psi[9][16], JxW[16], outlet-face integrals[16].
 *   cell_of_dof0: local index of the cell whose node 0 is global DoF 0 (-1 on the other ranks); its (0,0) entry
 *   is the value MatrixTools::apply_boundary_values puts on Dirichlet diagonals (:574-575).
 * nsk_assembly_set_dirichlet: flags per owned velocity DoF (boundary ids 6, 7, 10; :540-571) and, optionally,
 *   inhomogeneous values (the inlet profile of the very first iteration).
 * nsk_state_*: `solution` on the device.  set/get move owned entries; save = `evaluation_point = solution`;
 *   update(alpha) = `solution = evaluation_point + alpha * delta_owned` with delta the resident result of the
 *   last solve (:718-721).  Ghost entries are refreshed by a halo exchange.  The result stays available to every
 *   update of one line search, whatever nsk_assemble writes between them (P2/P1 handles copy it before the
 *   assembly writes the next initial guess over it).
 * nsk_assemble: fills block (0,0) (+ Dirichlet clearing), the resident right-hand side and the Dirichlet entries
 *   of the resident initial guess, and returns residual_vector.l2_norm() (:701).  Collective.
 *   stokes != 0 is the reference's Stokes phase (`computing_stokes`, :383-406, :455-458): no convective part,
 *   no residual (right-hand side = outlet term + Dirichlet values).
 *   The Dirichlet diagonal |entry (0,0)| is written by the rank owning global DoF 0 and summed over the ranks (one
 *   word) before the Dirichlet rows and the right-hand side read it — Q3/Q2 and P2/P1 cells alike.
 *   Call nsk_setup_preconditioner afterwards, as solve_system() builds its preconditioner from the new matrix. */
int nsk_assembly_set_cells(nsk_handle h, int64_t n_cells, const int32_t *cell_u_nodes, const int32_t *cell_p_dofs,
                           const uint8_t *cell_flags, const double *tables944, int32_t cell_of_dof0);
int nsk_assembly_set_dirichlet(nsk_handle h, const uint8_t *dirichlet_u, const double *bc_u /* or NULL */);
/* The same for general (non-congruent) P2/P1 triangles — the reference's `-M` path (FE_SimplexP, QGaussSimplex(3),
 * NSSolverStationary.cpp:144-206).  Instead of nsk_assembly_set_cells.  Per cell: 6 velocity NODE ids
 * (vertices, then the midpoints of edges (0,1), (1,2), (2,0)), 3 pressure DoF ids, the gradients of the three
 * barycentric coordinates and the area (what MappingFE / FEValues::reinit give per cell).  The transposed connectivity
 * the gather kernels need is computed by the caller's side once per mesh (navier_stokes_solver_amd/simplex.py:
 * device_handoff): per 2x2 node block of block (0,0) the cells holding both nodes (cell * 36 + local row node * 6 +
 * local column node) and the positions of the block's first entry in the node's two scalar CSR rows; per velocity node
 * and per pressure DoF the cells touching it (cell * 6 + local node, cell * 3 + local vertex); outlet_w[2 node + c] =
 * integral of phi_node n_c over the boundary-id-8 edges.  pos00: position of entry (0,0) of block (0,0).
 * Several ranks (simplex.py: device_rank_handoff): the cells are those touching an owned node or DoF plus the
 * rank's own, in ascending global order; ids are local — owned first, then the ghosts in the order of the partition's
 * ghost lists (velocity ghosts as whole nodes: an odd ghost count is -65), valid below n_u/2 + ng_u/2 and n_p + ng_p;
 * the block, node and vertex lists cover the owned rows, nodes and DoFs; pos00 is the position of the diagonal entry of
 * global DoF 0 on the rank that owns it and -1 on the others (-64 on one rank).  Every id a kernel dereferences is
 * checked here on the host (-64) before anything is launched. */
int nsk_assembly_set_simplex(nsk_handle h, int64_t n_cells, const int32_t *cell_u_nodes, const int32_t *cell_p_dofs,
                             const double *grad_lambda, const double *area, int64_t n_blocks, const int32_t *blk_ptr,
                             const int32_t *blk_ent, const int64_t *blk_pos0, const int64_t *blk_pos1,
                             const int32_t *node_ptr, const int32_t *node_ent, const int32_t *vert_ptr,
                             const int32_t *vert_ent, const double *outlet_w, int64_t pos00);
int nsk_state_set(nsk_handle h, const double *u_owned, const double *p_owned);
int nsk_state_get(nsk_handle h, double *u_owned, double *p_owned);
int nsk_state_save(nsk_handle h);
int nsk_state_update(nsk_handle h, double alpha);
/* solution_old = solution (NSSolver::solve(), NSSolver.cpp:813).  With a saved old state and inv_dt != 0,
 * nsk_assemble adds the time term -(u - u_old)/dt . v to the residual (NSSolver.cpp:460-463); the mass term
 * M/dt of the matrix (:443-446) only needs inv_dt. */
int nsk_state_save_old(nsk_handle h);
int nsk_assemble(nsk_handle h, int stokes, double nu, double inv_dt, double p_out, int inhomogeneous_bc,
                 double *residual_norm);
/* ---------------------------------------------------------------------------------------------------
 * Consumers of the resident `solution`: the forces on the obstacle and the output patches.
 * Replaces the face loop of compute_lift_drag() (NSSolverStationary.cpp:836-897, NSSolver.cpp:876-935) and the reads
 * DataOut::build_patches makes of the solution (:769-796); nothing on the linear-solve path changes.
 *
 * nsk_forces_set_faces: the faces with boundary id 10 of this rank's cells, after nsk_assembly_set_cells — per face the
 *   local cell (index into that call's cell list) and the side (0: the neighbour at i-1 is missing, 1: i+1, 2: j-1,
 *   3: j+1; the fluid cell's outward normal is (-1,0), (1,0), (0,-1), (0,1)) — and what FEFaceValues tabulates for the
 *   congruent cell: 672 doubles, for side s and Gauss point q (4 per face) at (s * 4 + q) * 41 the physical
 *   dphi/dx[16], dphi/dy[16] and psi[9], then JxW[4][4] at 656.  n_faces may be 0 (a rank whose cells do not touch the
 *   obstacle).  nsk_forces_set_edges: the same for P2/P1 handles, after nsk_assembly_set_simplex — per id-10 edge its
 *   cell, the cell's local edge (0: vertices 0-1, 1: 1-2, 2: 2-0) and (n_x, n_y, length) with the fluid cell's outward
 *   normal; two Gauss points per edge.  Cell indices are checked on the host at hand-off (-72).  On several ranks:
 *   the id-10 edges of the rank's OWN cells, indices into that rank's cell list; n_edges may be 0.
 *   nsk_assembly_set_cells / nsk_assembly_set_simplex void the list.
 * nsk_forces: drag_lift[0..1] = -sum over those faces of (nu (grad u + grad u^T) - p I) n JxW from the resident state
 *   (owned entries and the ghost tail, as nsk_assemble reads them), summed over the ranks (Utilities::MPI::sum,
 *   :895-896); local_drag_lift (or NULL): this rank's share.  Collective when nranks > 1.  One work item per (face,
 *   Gauss point) writes its own slot, one workgroup adds the slots in a fixed order: two calls give the same bits.
 * nsk_state_get_patches: for each listed local cell (u_x, u_y) [8 doubles] and p [4 doubles] at its vertices (0,0),
 *   (1,0), (0,1), (1,1) — velocity nodes 0, 3, 12, 15 and pressure DoFs 0, 2, 6, 8 of the cell; the bits of the state,
 *   owned or ghost.  Q3/Q2 handles. */
int nsk_forces_set_faces(nsk_handle h, int64_t n_faces, const int32_t *face_cell, const uint8_t *face_side,
                         const double *tables672);
int nsk_forces_set_edges(nsk_handle h, int64_t n_edges, const int32_t *edge_cell, const uint8_t *edge_local,
                         const double *edge_nl);
int nsk_forces(nsk_handle h, double nu, double *drag_lift, double *local_drag_lift /* or NULL */);
int nsk_state_get_patches(nsk_handle h, int64_t n, const int32_t *cells, double *vel /* 8 per cell */,
                          double *prs /* 4 per cell */);
/* The VTU record in file layout: the bytes of the file's `velocity` and `pressure` arrays, packed on the
 * device, optionally on subdivided patches (DataOut::build_patches(n_subdivisions)).
 * nsk_record_set_cells (Q3/Q2 handles, after nsk_assembly_set_cells): the local cells of the record in file order and
 *   s = subdivisions in 1..4; for s > 1 the tables W_u[pt][n] = L_a(t_k) L_b(t_l) on the GLL nodes (n = b*4 + a) and
 *   W_p[pt][m] on {0, 1/2, 1} (m = b*3 + a), pt = l (s+1) + k, t_k = k / s (nsp_record_tables); for s = 1 they may be
 *   NULL.  Cell indices are checked on the host (-72).  The list, the tables and a result buffer of 4 n_points doubles
 *   stay on the device until nsk_assembly_set_cells / nsk_assembly_set_simplex void them.  n_cells may be 0.
 * nsk_state_get_record: points numbered cell by cell, pt as above (s = 1: the vertices (0,0), (1,0), (0,1), (1,1));
 *   vel3 = (u_x, u_y, +0.0) per point, prs one value per point.  n_points must be n_cells (s+1)^2 (-60).  s = 1 copies
 *   the bits of the state, owned or ghost, as nsk_state_get_patches does; s > 1: value = sum_n W[pt][n] state[n], n
 *   increasing, one accumulator, no atomics: two calls give the same bits.  P2/P1 handles (one rank) need no list: the
 *   record is the mesh's vertices, the first n_p velocity nodes and the pressure DoFs; n_points = n_p.
 * nsk_record_set_points (P2/P1 handles, after nsk_assembly_set_simplex; -71 on Q3/Q2 handles): the record's points as
 *   local ids — per point the velocity node and the pressure DoF of a vertex, owned or ghost (one rank's piece: the
 *   vertices of its own cells).  Ids are checked on the host (-72); n_points may be 0.  nsk_assembly_set_cells /
 *   nsk_assembly_set_simplex void the list.  With a list nsk_state_get_record returns (u_x, u_y, +0.0) and p of the
 *   listed points, the bits of the state, n_points = the list's length; without one it behaves as above (-60 on
 *   several ranks). */
int nsk_record_set_cells(nsk_handle h, int64_t n_cells, const int32_t *cells, int subdivisions,
                         const double *w_u /* (s+1)^2 x 16 */, const double *w_p /* (s+1)^2 x 9 */);
int nsk_record_set_points(nsk_handle h, int64_t n_points, const int32_t *u_node, const int32_t *p_dof);
int nsk_state_get_record(nsk_handle h, int64_t n_points, double *vel3 /* 3 per point */, double *prs /* 1 per point */);
/* Vorticity and divergence at the record's points, from the gradient of the element's own functions — the file
 * shows the solution on bilinear quads (or linear triangles), from which no viewer can recover it.  A second launch beside
 * nsk_state_get_record, whose results keep their bits.
 * nsk_record_set_gradient (Q3/Q2 handles, after nsk_record_set_cells with the same s; needed for s = 1 too, a vertex
 *   derivative reads all 16 nodes): D_x[pt][n] = L'_a(t_k) L_b(t_l) / hx and D_y[pt][n] = L_a(t_k) L'_b(t_l) / hy, laid
 *   out like W_u (n = b*4 + a, pt = l (s+1) + k), each entry the double product of two 1-D values, then one division
 *   (nsp_record_gradient_tables).  The tables stay on the device until nsk_assembly_set_cells, nsk_assembly_set_simplex or
 *   a new nsk_record_set_cells void them.  -60: s differs from the record's; -69: no record list; -71: a P2/P1 handle.
 * nsk_state_get_record_fields: fields is a mask of NSK_FIELD_VORTICITY (d_x u_y - d_y u_x) and NSK_FIELD_DIVERGENCE
 *   (d_x u_x + d_y u_y); out receives n_points doubles per selected field, vorticity first, in the point order of
 *   nsk_state_get_record — each block is the bytes of that array in the file.  Q3/Q2: g_cd = sum_n D_d[pt][n] u_c[n], n
 *   increasing, one accumulator per sum, then g_10 - g_01 and g_00 + g_11; ghost nodes are read from the ghost tail.
 *   P2/P1 (one rank, no tables, n_points = n_p): per vertex (sum_t area_t f_t(v)) / (sum_t area_t) over the vertex's cells
 *   in the order of vert_ptr / vert_ent, f_t(v) the field of cell t's six P2 functions at that vertex; +0.0 at a vertex of
 *   no cell.  No atomics: two calls give the same bits, and a mask of one field gives the bits it has in a mask of both.
 *   -60: mask 0 or an unknown bit, n_points is not the record's; -69: no cells, no record list, or (Q3/Q2) no gradient
 *   tables; -73: no state; -71: a P2/P1 handle with a point list of nsk_record_set_points in force (a rank's piece sees
 *   only its own cells of a vertex on the cut). */
#define NSK_FIELD_VORTICITY 1
#define NSK_FIELD_DIVERGENCE 2
int nsk_record_set_gradient(nsk_handle h, int subdivisions, const double *d_x /* (s+1)^2 x 16 */,
                            const double *d_y /* (s+1)^2 x 16 */);
int nsk_state_get_record_fields(nsk_handle h, int64_t n_points, int fields, double *out /* n_points per field */);
/* values of a resident block times a factor: pressure_mass is assembled with 1/nu (:404, :450), block (1,0)
 * changes sign between the Stokes and the Newton phase (:397 against :444) */
int nsk_scale_values(nsk_handle h, int blk, double factor);
/* resident right-hand side (residual_vector) to the host */
int nsk_download_rhs(nsk_handle h, double *rhs_u, double *rhs_p);
/* device time of one assembly (all kernels), averaged over reps */
int nsk_time_assemble(nsk_handle h, double nu, double inv_dt, int reps, double *avg_ms);

int nsk_get_stats(nsk_handle h, nsk_stats *out);
/* Residuals SolverControl::check saw during the last outer solve, in order (start value, then one per counted
 * iteration; FGMRES / BiCGStab add the true residual at every restart).  Returns how many there were; at most `cap`
 * are copied (the library keeps the first 65536). */
int nsk_get_history(nsk_handle h, double *out, int cap);
/* End the outer solve running on this handle at its next SolverControl check (status 1, iters/final_res valid).
 * The only entry point that may be called from another thread while a solve is in progress. */
int nsk_cancel(nsk_handle h);
/* In-process test transport (nsk_local_group_id) only: take this handle's group down.  Every rank blocked in a
 * collective of the group, and every later collective, returns -25.  The library does this by itself when a rank fails
 * inside nsk_setup_preconditioner / nsk_solve / nsk_solve_resident / nsk_assemble / nsk_precond_vmult or is destroyed;
 * the caller does it when a rank fails on ITS side between two calls (so that the peers' threads can be joined).  No-op
 * on RCCL handles.  Callable from any thread. */
int nsk_abort_group(nsk_handle h);
int nsk_reset_stats(nsk_handle h);

/* Device-side timing of one operation repeated `reps` times between HIP events on the
 * library's stream: op 0..5 = SpMV of block op; 10 = jacobian vmult; 20/21 = velocity /
 * pressure triangular apply; 30 = dot; 31 = axpy; 32 = fused add_and_dot; 50 + blk (50, 53, 55) = the inner
 * solves' SpMV of F, M_p, S (nsk_inner_spmv; needs a set-up); 56 = the matrix-free product with F (nsk_matfree_f:
 * needs a valid assembly, not the option); 57 = one V-cycle of the current set-up's velocity AMG (as op 20 under
 * that set-up).
 * Returns average milliseconds per repetition and the algorithmic bytes of one repetition — for ops 50 + blk the bytes
 * the stored format really moves (fp32 values: 4 bytes each), for op 56 (and op 50 while matrix-free is in effect) the
 * bytes the two kernels move: cell data, the cells' shares written and read, node lists, x and y; for op 57 the bytes the
 * stored formats hold for one cycle (fp32 values, node blocks: NSK_OPT_AMG_PRECISION), where op 20 reports the algorithmic
 * CSR count. */
int nsk_time_op(nsk_handle h, int op, int reps, double *avg_ms, double *bytes);

/* HIP-event sampling of operation classes INSIDE the following solves: every launch of a sampled op
 * (same ids as nsk_time_op: 0..5 SpMV of that block, 20/21 triangular applies; up to four ops at once)
 * is bracketed by events on the library's stream until max_samples are taken. */
int nsk_profile_begin(nsk_handle h, int op, int max_samples);
/* bytes_per_launch: algorithmic bytes (CSR); bytes_format: what the storage format the kernel streams
 * really holds (node-block copies are smaller than CSR) — roofline fractions from the latter cannot exceed 1.
 * With NSK_OPT_INNER_MATRIX_PRECISION = 32, bytes_format of F, S and M_p is the fp32 copy's: with the default fused
 * J x every sampled F and S launch is an inner one; with NSK_OPT_FUSE_BLOCK_ROW = 0 the F samples mix the outer J x's
 * double launches with the inner fp32 ones, and the figure then understates the outer ones. */
int nsk_profile_read(nsk_handle h, int op, double *avg_ms, int *n_samples, double *bytes_per_launch,
                     int64_t *n_calls, double *bytes_format);
int nsk_profile_end(nsk_handle h);

#ifdef __cplusplus
}
#endif
#endif
