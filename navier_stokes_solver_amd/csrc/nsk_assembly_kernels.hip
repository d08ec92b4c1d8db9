// nsk_assembly_kernels.hip — device assembly of the Newton system on congruent Q3/Q2 cells.
//
// Replaces the cell loop of NSSolverStationary::assemble_system(false, false)
// (lab_new/src/NSSolverStationary.cpp:352-537: linearised convection + viscosity into jacobian(0,0), the
// residual -R(u) into residual_vector) and the Dirichlet clearing of MatrixTools::apply_boundary_values
// (:540-575).  The reference scatters 41x41 cell matrices with `jacobian_matrix.add`; here every matrix ROW is
// gathered instead: a wavefront owns one velocity node (two rows), its 64 lanes are the (touching cell, column
// node) pairs, contributions are summed in a fixed order (deterministic, no atomics) and the finished rows are
// written once.  The (0,1), (1,0) blocks and the pressure mass matrix do not depend on the state and stay as
// handed over.
#include <hip/hip_runtime.h>

#include "nsk_assembly.hpp"

namespace nsk {
namespace {

constexpr int BLK = 256;

// tables (doubles): phi 0, dpx 256, dpy 512, psi 768, jxw 912, face 928, K 944, M3 1200
constexpr int T_PHI = 0, T_DPX = 256, T_DPY = 512, T_PSI = 768, T_JXW = 912, T_FACE = 928, T_K = 944, T_M3 = 1200;

// state at the quadrature points of every cell: cq[cell][f][q], f = u0 u1 g00 g01 g10 g11 p uold0 uold1
// (fe_values[velocity].get_function_values / get_function_gradients, fe_values[pressure].get_function_values)
constexpr int CQ = 144;  // doubles per cell
__global__ __launch_bounds__(BLK) void asm_cell_state_kernel(AsmMesh M, const double *__restrict__ su,
                                                             const double *__restrict__ sp,
                                                             const double *__restrict__ so, double *__restrict__ cq) {
  const long t = (long)blockIdx.x * BLK + threadIdx.x;
  const long cell = t >> 4;
  const int q = (int)(t & 15);
  if (cell >= M.n_cells) return;
  const double *T = M.tables;
  double u0 = 0, u1 = 0, g00 = 0, g01 = 0, g10 = 0, g11 = 0, p = 0, o0 = 0, o1 = 0;
#pragma unroll 4
  for (int n = 0; n < 16; ++n) {
    const int node = M.cell_u[cell * 16 + n];
    const double2 uv = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
    const double ph = T[T_PHI + n * 16 + q], dx = T[T_DPX + n * 16 + q], dy = T[T_DPY + n * 16 + q];
    if (so) {  // solution_old (time loop)
      const double2 ov = *reinterpret_cast<const double2 *>(so + 2 * (size_t)node);
      o0 += ov.x * ph; o1 += ov.y * ph;
    }
    u0 += uv.x * ph; u1 += uv.y * ph;
    g00 += uv.x * dx; g01 += uv.x * dy;
    g10 += uv.y * dx; g11 += uv.y * dy;
  }
  for (int m = 0; m < 9; ++m) p += sp[M.cell_p[cell * 9 + m]] * T[T_PSI + m * 16 + q];
  double *o = cq + (size_t)cell * CQ + q;
  o[0] = u0; o[16] = u1; o[32] = g00; o[48] = g01; o[64] = g10; o[80] = g11; o[96] = p; o[112] = o0; o[128] = o1;
}

// |jacobian(0,0) before clearing|: the value MatrixTools::apply_boundary_values puts on Dirichlet rows.
// Written by the rank that owns global DoF 0 (others write 0; the caller all-reduces).
__global__ void asm_d0_kernel(AsmMesh M, const double *__restrict__ cq, double nu, double inv_dt, int stokes, double *out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v = 0.0;
  if (M.cell_of_dof0 >= 0) {
    const double *T = M.tables, *c = cq + (size_t)M.cell_of_dof0 * CQ;
    v = nu * T[T_K] + inv_dt * T[T_M3];
    for (int q = 0; q < 16 && !stokes; ++q) {
      const double ph = T[T_PHI + q];
      const double adv = c[q] * T[T_DPX + q] + c[16 + q] * T[T_DPY + q];
      v += T[T_JXW + q] * ph * (adv + c[32 + q] * ph);
    }
  }
  *out = v;
}

// jacobian(0,0): one wavefront per owned velocity node, lane = touching cell k (4) x column node m (16)
__global__ __launch_bounds__(BLK) void asm_F_rows_kernel(AsmMesh M, const double *__restrict__ cq, double nu, double inv_dt,
                                                         int stokes, const double *__restrict__ d0p,
                                                         const int *__restrict__ rowptr, double *__restrict__ val) {
  __shared__ double rb[4][49 * 4];
  __shared__ double tphi[256], tjxw[16];  // phi[n][q] (n is uniform over 16 lanes: broadcast reads)
  __shared__ double tT[3][256];           // phi, dphi/dx, dphi/dy transposed to [q][m]: lanes m read consecutive words
  __shared__ double cs[4][4][96];         // per wave: the quadrature-point state (u, grad u) of its <= 4 cells
  {
    const int i = threadIdx.x;             // BLK == 256 == one table
    tphi[i] = M.tables[T_PHI + i];
    const int mm = i >> 4, qq = i & 15;
    tT[0][qq * 16 + mm] = M.tables[T_PHI + i];
    tT[1][qq * 16 + mm] = M.tables[T_DPX + i];
    tT[2][qq * 16 + mm] = M.tables[T_DPY + i];
    if (i < 16) tjxw[i] = M.tables[T_JXW + i];
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = (int)blockIdx.x * 4 + wave;  // owned velocity node
  const bool have = r < M.n_unodes;
  for (int i = lane; i < 49 * 4; i += 64) rb[wave][i] = 0.0;
  const int k = lane >> 4, m = lane & 15;
  const int cn = have ? M.node_cells[(size_t)r * 4 + k] : -1;
  if (cn >= 0) {  // the 16 lanes of cell k fetch its 96 values once (6 each)
    const double *c = cq + (size_t)(cn >> 4) * CQ;
#pragma unroll
    for (int f = 0; f < 6; ++f) cs[wave][k][f * 16 + m] = c[f * 16 + m];
  }
  __syncthreads();
  double b00 = 0, b01 = 0, b10 = 0, b11 = 0;
  if (cn >= 0) {
    const int n = cn & 15;
    const double *c = cs[wave][k];
    // Stokes phase (assemble_system(.., true), .cpp:383-406): no convective part
#pragma unroll 4
    for (int q = 0; q < (stokes ? 0 : 16); ++q) {
      const double w = tjxw[q] * tphi[n * 16 + q];
      const double pm = tT[0][q * 16 + m];
      const double adv = c[q] * tT[1][q * 16 + m] + c[16 + q] * tT[2][q * 16 + m];  // (u_old . grad) phi_m
      b00 += w * (adv + c[32 + q] * pm);
      b01 += w * (c[48 + q] * pm);
      b10 += w * (c[64 + q] * pm);
      b11 += w * (adv + c[80 + q] * pm);
    }
    const double kk = nu * M.tables[T_K + n * 16 + m] + inv_dt * M.tables[T_M3 + n * 16 + m];
    b00 += kk;
    b11 += kk;
  }
  const int off = cn >= 0 ? (int)M.node_off[(size_t)r * 64 + lane] : 0;
  for (int ph = 0; ph < 4; ++ph) {  // cells in fixed order: the sum does not depend on the schedule
    if (k == ph && cn >= 0) {
      double *o = &rb[wave][off * 4];
      o[0] += b00; o[1] += b01; o[2] += b10; o[3] += b11;
    }
    __syncthreads();
  }
  if (!have) return;
  const int rp0 = rowptr[2 * r], rp1 = rowptr[2 * r + 1];
  const int nb = (rp1 - rp0) >> 1;
  const bool dir = M.dirichlet[2 * r] != 0;
  const int self = M.node_self[r];
  const double d0 = fabs(*d0p);
  for (int j = lane; j < nb; j += 64) {
    double v00 = rb[wave][j * 4], v01 = rb[wave][j * 4 + 1], v10 = rb[wave][j * 4 + 2], v11 = rb[wave][j * 4 + 3];
    if (dir) {  // cleared row with the reference diagonal
      v01 = v10 = 0.0;
      v00 = v11 = j == self ? d0 : 0.0;
    }
    *reinterpret_cast<double2 *>(val + rp0 + 2 * j) = make_double2(v00, v01);
    *reinterpret_cast<double2 *>(val + rp1 + 2 * j) = make_double2(v10, v11);
  }
}

// residual_vector, velocity rows: -a(u,v) - c(u;u,v) + b(v,p) - outlet Neumann term; Dirichlet rows d0 * value
__global__ __launch_bounds__(BLK) void asm_rhs_u_kernel(AsmMesh M, const double *__restrict__ cq, double nu, double inv_dt,
                                                        double p_out, int stokes, const double *__restrict__ d0p,
                                                        const double *__restrict__ bc, double *__restrict__ rhs,
                                                        double *__restrict__ x0) {
  const int r = (int)(blockIdx.x * BLK + threadIdx.x);
  if (r >= M.n_unodes) return;
  const double *T = M.tables;
  if (M.dirichlet[2 * r]) {
    const double d0 = fabs(*d0p);
    const double v0 = bc ? bc[2 * r] : 0.0, v1 = bc ? bc[2 * r + 1] : 0.0;
    rhs[2 * r] = d0 * v0; rhs[2 * r + 1] = d0 * v1;
    x0[2 * r] = v0; x0[2 * r + 1] = v1;  // apply_boundary_values also fixes the solution vector (delta_owned)
    return;
  }
  double r0 = 0.0, r1 = 0.0;
  for (int k = 0; k < 4; ++k) {
    const int cn = M.node_cells[(size_t)r * 4 + k];
    if (cn < 0) continue;
    const int cell = cn >> 4, n = cn & 15;
    const double *c = cq + (size_t)cell * CQ;
    for (int q = 0; q < (stokes ? 0 : 16); ++q) {   // the Stokes phase skips the residual (`continue`, .cpp:455-458)
      const double w = T[T_JXW + q], ph = T[T_PHI + n * 16 + q], dx = T[T_DPX + n * 16 + q], dy = T[T_DPY + n * 16 + q];
      const double u0 = c[q], u1 = c[16 + q], g00 = c[32 + q], g01 = c[48 + q], g10 = c[64 + q], g11 = c[80 + q],
                   p = c[96 + q];
      // -a(u,v) - c(u;u,v) + b(v,p) - (u - u_old)/dt . v   (the last one: NSSolver.cpp:460-463, inv_dt = 0 otherwise)
      r0 += w * (-nu * (g00 * dx + g01 * dy) - (u0 * g00 + u1 * g01) * ph + p * dx - inv_dt * (u0 - c[112 + q]) * ph);
      r1 += w * (-nu * (g10 * dx + g11 * dy) - (u0 * g10 + u1 * g11) * ph + p * dy - inv_dt * (u1 - c[128 + q]) * ph);
    }
    if (M.cell_flags[cell] & 1) r0 -= p_out * T[T_FACE + n];
  }
  rhs[2 * r] = r0;
  rhs[2 * r + 1] = r1;
}

// residual_vector, pressure rows: + b(u,q)
__global__ __launch_bounds__(BLK) void asm_rhs_p_kernel(AsmMesh M, const double *__restrict__ cq, int stokes,
                                                        double *__restrict__ rhs) {
  const int r = (int)(blockIdx.x * BLK + threadIdx.x);
  if (r >= M.n_pdofs) return;
  if (stokes) { rhs[r] = 0.0; return; }
  const double *T = M.tables;
  double v = 0.0;
  for (int k = 0; k < 4; ++k) {
    const int cm = M.pdof_cells[(size_t)r * 4 + k];
    if (cm < 0) continue;
    const int cell = cm / 9, m = cm % 9;
    const double *c = cq + (size_t)cell * CQ;
    for (int q = 0; q < 16; ++q) v += T[T_JXW + q] * (c[32 + q] + c[80 + q]) * T[T_PSI + m * 16 + q];
  }
  rhs[r] = v;
}

// ---- matrix-free y = jacobian(0,0) x from the state of the last assembly (NSK_OPT_INNER_MATRIX_FREE_F) ----
// The rows of asm_F_rows_kernel, summed in another order: with x_c, dx x_c, dy x_c the input interpolated at the
// quadrature point q of a cell, U and G = grad U from cq, w = JxW[q],
//   a_c  = w (U0 dx x_c + U1 dy x_c + G[c][0] x_0 + G[c][1] x_1 + inv_dt x_c)      (Stokes phase: the inv_dt term only)
//   bx_c = w nu dx x_c,   by_c = w nu dy x_c
//   y[2n+c] = sum_{cells k of n, node_cells order} sum_q phi_n(q) a_c(q) + dphi_n/dx(q) bx_c(q) + dphi_n/dy(q) by_c(q)
// Two launches, no atomics, every sum in a fixed order.  The cell kernel forms the six fluxes of its 16 points in LDS and
// contracts them there with the cell's 16 test functions: what leaves the workgroup is the cell's share of its 16
// node rows (32 doubles) instead of the 96 fluxes, which every one of the 16 nodes would have to read again.
constexpr int MF_CELLS = BLK / 16;   // cells per workgroup
constexpr int MF_FL = 98;            // flux stride per cell in LDS (96 + 2: the 4 cells of a wave start in different banks)
__device__ __forceinline__ double2 mf_load2(const double *__restrict__ own, const double *__restrict__ ghost, int n_own,
                                            int node) {
  if (node < n_own) return *reinterpret_cast<const double2 *>(own + 2 * (size_t)node);
  const double *p = ghost + 2 * (size_t)(node - n_own);   // (the ghost tail of a block vector starts at any word)
  return make_double2(p[0], p[1]);
}
__global__ __launch_bounds__(BLK) void mf_cell_flux_kernel(AsmMesh M, const double *__restrict__ cq, double nu, double inv_dt,
                                                           int stokes, const double *__restrict__ x_own,
                                                           const double *__restrict__ x_ghost, double *__restrict__ wk) {
  __shared__ double tN[3][256];            // phi, dphi/dx, dphi/dy as tabulated: [n][q], lanes q read consecutive words
  __shared__ double tT[3][256];            // the same transposed to [q][n]: lanes n read consecutive words
  __shared__ double tjxw[16];
  __shared__ double xs[MF_CELLS][32];      // the cell's 16 node pairs of x
  __shared__ double fl[MF_CELLS][MF_FL];   // a_0 a_1 bx_0 bx_1 by_0 by_1, 16 points each
  {
    const int i = threadIdx.x, nn = i >> 4, qq = i & 15;   // BLK == 256 == one table
    const double v0 = M.tables[T_PHI + i], v1 = M.tables[T_DPX + i], v2 = M.tables[T_DPY + i];
    tN[0][i] = v0; tN[1][i] = v1; tN[2][i] = v2;
    tT[0][qq * 16 + nn] = v0; tT[1][qq * 16 + nn] = v1; tT[2][qq * 16 + nn] = v2;
    if (i < 16) tjxw[i] = M.tables[T_JXW + i];
  }
  const int lc = threadIdx.x >> 4, l = threadIdx.x & 15;   // l: node m (gather), point q (fluxes), node n (contraction)
  const long cell = (long)blockIdx.x * MF_CELLS + lc;
  const bool have = cell < M.n_cells;
  if (have) {
    const double2 v = mf_load2(x_own, x_ghost, M.n_unodes, M.cell_u[cell * 16 + l]);
    xs[lc][2 * l] = v.x; xs[lc][2 * l + 1] = v.y;
  }
  __syncthreads();
  if (have) {
    const int q = l;
    double x0 = 0, x1 = 0, dx0 = 0, dx1 = 0, dy0 = 0, dy1 = 0;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const double ph = tN[0][m * 16 + q], dx = tN[1][m * 16 + q], dy = tN[2][m * 16 + q];
      const double a = xs[lc][2 * m], b = xs[lc][2 * m + 1];
      x0 += a * ph; x1 += b * ph;
      dx0 += a * dx; dx1 += b * dx;
      dy0 += a * dy; dy1 += b * dy;
    }
    const double w = tjxw[q];
    double a0 = inv_dt * x0, a1 = inv_dt * x1;
    if (!stokes) {
      const double *c = cq + (size_t)cell * CQ + q;
      const double u0 = c[0], u1 = c[16], g00 = c[32], g01 = c[48], g10 = c[64], g11 = c[80];
      a0 += u0 * dx0 + u1 * dy0 + g00 * x0 + g01 * x1;
      a1 += u0 * dx1 + u1 * dy1 + g10 * x0 + g11 * x1;
    }
    const double wn = w * nu;
    double *f = fl[lc];
    f[q] = w * a0; f[16 + q] = w * a1;
    f[32 + q] = wn * dx0; f[48 + q] = wn * dx1;
    f[64 + q] = wn * dy0; f[80 + q] = wn * dy1;
  }
  __syncthreads();
  if (!have) return;
  const int n = l;
  const double *f = fl[lc];
  double r0 = 0, r1 = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const double ph = tT[0][q * 16 + n], dx = tT[1][q * 16 + n], dy = tT[2][q * 16 + n];
    r0 += ph * f[q] + dx * f[32 + q] + dy * f[64 + q];
    r1 += ph * f[16 + q] + dx * f[48 + q] + dy * f[80 + q];
  }
  *reinterpret_cast<double2 *>(wk + (size_t)cell * 32 + 2 * n) = make_double2(r0, r1);
}

// one thread per owned velocity node: its <= 4 cell shares in node_cells order; Dirichlet rows d0 * x (columns are not
// eliminated, as in the assembled block: the other rows read x at Dirichlet nodes like anywhere else)
__global__ __launch_bounds__(BLK) void mf_rows_kernel(AsmMesh M, const double *__restrict__ wk, const double *__restrict__ d0p,
                                                      const double *__restrict__ x_own, double *__restrict__ y) {
  const int r = (int)(blockIdx.x * BLK + threadIdx.x);
  if (r >= M.n_unodes) return;
  double2 o;
  if (M.dirichlet[2 * r]) {
    const double d0 = fabs(*d0p);
    const double2 v = *reinterpret_cast<const double2 *>(x_own + 2 * (size_t)r);
    o = make_double2(d0 * v.x, d0 * v.y);
  } else {
    const int4 nc = *reinterpret_cast<const int4 *>(M.node_cells + (size_t)r * 4);
    const int cn[4] = {nc.x, nc.y, nc.z, nc.w};
    o = make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (cn[k] < 0) continue;
      const double2 v = *reinterpret_cast<const double2 *>(wk + 2 * (size_t)cn[k]);   // (cell * 16 + n) * 2
      o.x += v.x; o.y += v.y;
    }
  }
  *reinterpret_cast<double2 *>(y + 2 * (size_t)r) = o;
}

// ---- consumers of the solution: forces over boundary id 10 and output patches ----
// compute_lift_drag (NSSolverStationary.cpp:836-897): -sum over the obstacle faces of (nu (grad u + grad u^T) - p I) n JxW
// with the fluid cell's outward normal.  One thread per (face, Gauss point) writes its two components to its own slot;
// forces_sum_kernel adds the slots in a fixed order.  No atomics: two calls give the same bits.
// ftab: per (side, point) dphi/dx[16], dphi/dy[16], psi[9]; JxW[4][4] at 656 (nsp_face_tables)
constexpr int FT_STRIDE = 41, FT_JXW = 656;
__global__ __launch_bounds__(BLK) void forces_faces_kernel(long n_faces, const int *__restrict__ cell_u,
                                                           const int *__restrict__ cell_p, const int *__restrict__ face_cell,
                                                           const unsigned char *__restrict__ face_side,
                                                           const double *__restrict__ ftab, const double *__restrict__ su,
                                                           const double *__restrict__ sp, double nu, double *__restrict__ slots) {
  const long t = (long)blockIdx.x * BLK + threadIdx.x;
  if (t >= n_faces * 4) return;
  const long f = t >> 2;
  const int q = (int)(t & 3), side = face_side[f];
  const long cell = face_cell[f];
  const double *T = ftab + (side * 4 + q) * FT_STRIDE;
  double g00 = 0, g01 = 0, g10 = 0, g11 = 0, p = 0;
  for (int n = 0; n < 16; ++n) {
    const int node = cell_u[cell * 16 + n];
    const double2 uv = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
    const double dx = T[n], dy = T[16 + n];
    g00 += uv.x * dx; g01 += uv.x * dy;
    g10 += uv.y * dx; g11 += uv.y * dy;
  }
  for (int m = 0; m < 9; ++m) p += sp[cell_p[cell * 9 + m]] * T[32 + m];
  const double nx = side == 0 ? -1.0 : side == 1 ? 1.0 : 0.0, ny = side == 2 ? -1.0 : side == 3 ? 1.0 : 0.0;
  const double jxw = ftab[FT_JXW + side * 4 + q];
  const double s00 = nu * (g00 + g00) - p, s01 = nu * (g01 + g10), s11 = nu * (g11 + g11) - p;
  slots[2 * t] = -(s00 * nx + s01 * ny) * jxw;
  slots[2 * t + 1] = -(s01 * nx + s11 * ny) * jxw;
}

// one workgroup: thread i adds slots i, i + BLK, ... in that order, then a binary tree over the BLK partial sums
__global__ __launch_bounds__(BLK) void forces_sum_kernel(long n_slots, const double *__restrict__ slots, double *__restrict__ out) {
  __shared__ double a0[BLK], a1[BLK];
  double d = 0.0, l = 0.0;
  for (long i = threadIdx.x; i < n_slots; i += BLK) { d += slots[2 * i]; l += slots[2 * i + 1]; }
  a0[threadIdx.x] = d; a1[threadIdx.x] = l;
  __syncthreads();
  for (int w = BLK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { a0[threadIdx.x] += a0[threadIdx.x + w]; a1[threadIdx.x] += a1[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = a0[0]; out[1] = a1[0]; }
}

// DataOut patches (NSSolverStationary.cpp:769-796): (u_x, u_y) and p at the four vertices (0,0), (1,0), (0,1), (1,1) of
// the listed cells — velocity nodes 0, 3, 12, 15 and pressure DoFs 0, 2, 6, 8.  One thread per (cell, vertex).
__global__ __launch_bounds__(BLK) void state_patches_kernel(long n, const int *__restrict__ cells, const int *__restrict__ cell_u,
                                                            const int *__restrict__ cell_p, const double *__restrict__ su,
                                                            const double *__restrict__ sp, double *__restrict__ vel,
                                                            double *__restrict__ prs) {
  const long t = (long)blockIdx.x * BLK + threadIdx.x;
  if (t >= n * 4) return;
  const long cell = cells[t >> 2];
  const int v = (int)(t & 3);
  const int un = v == 0 ? 0 : v == 1 ? 3 : v == 2 ? 12 : 15, pn = v == 0 ? 0 : v == 1 ? 2 : v == 2 ? 6 : 8;
  const int node = cell_u[cell * 16 + un];
  *reinterpret_cast<double2 *>(vel + 2 * t) = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
  prs[t] = sp[cell_p[cell * 9 + pn]];
}

// The VTU record in file layout: per point (u_x, u_y, +0.0) into vel3 and p into prs, the points numbered
// cell by cell, pt = l (s + 1) + k inside a cell.  One thread per point.
// s = 1: the vertices of state_patches_kernel, copied.
__global__ __launch_bounds__(BLK) void state_record_copy_kernel(long n_points, const int *__restrict__ cells,
                                                                const int *__restrict__ cell_u, const int *__restrict__ cell_p,
                                                                const double *__restrict__ su, const double *__restrict__ sp,
                                                                double *__restrict__ vel3, double *__restrict__ prs) {
  const long t = (long)blockIdx.x * BLK + threadIdx.x;
  if (t >= n_points) return;
  const long cell = cells[t >> 2];
  const int v = (int)(t & 3);
  const int un = v == 0 ? 0 : v == 1 ? 3 : v == 2 ? 12 : 15, pn = v == 0 ? 0 : v == 1 ? 2 : v == 2 ? 6 : 8;
  const int node = cell_u[cell * 16 + un];
  const double2 uv = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
  vel3[3 * t] = uv.x;
  vel3[3 * t + 1] = uv.y;
  vel3[3 * t + 2] = 0.0;
  prs[t] = sp[cell_p[cell * 9 + pn]];
}

// s > 1: build_patches(n_subdivisions) — the cell's 16 velocity nodes and 9 pressure DoFs interpolated at the ppc =
// (s + 1)^2 lattice points of the cell with the tables wu[pt][16], wp[pt][9] (postprocess.record_tables).  One chain per
// value, n increasing, one accumulator: two calls give the same bits, and a table row that is a unit vector (a vertex
// point) returns the entry of the state.
__global__ __launch_bounds__(BLK) void state_record_kernel(long n_points, int ppc, const int *__restrict__ cells,
                                                           const int *__restrict__ cell_u, const int *__restrict__ cell_p,
                                                           const double *__restrict__ wu, const double *__restrict__ wp,
                                                           const double *__restrict__ su, const double *__restrict__ sp,
                                                           double *__restrict__ vel3, double *__restrict__ prs) {
  const long t = (long)blockIdx.x * BLK + threadIdx.x;
  if (t >= n_points) return;
  const long cell = cells[t / ppc];
  const int pt = (int)(t % ppc);
  const double *W = wu + pt * 16;
  double ux = 0.0, uy = 0.0, p = 0.0;
  for (int n = 0; n < 16; ++n) {
    const int node = cell_u[cell * 16 + n];
    const double2 uv = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
    ux += W[n] * uv.x;
    uy += W[n] * uv.y;
  }
  const double *Wp = wp + pt * 9;
  for (int m = 0; m < 9; ++m) p += Wp[m] * sp[cell_p[cell * 9 + m]];
  vel3[3 * t] = ux;
  vel3[3 * t + 1] = uy;
  vel3[3 * t + 2] = 0.0;
  prs[t] = p;
}

// Vorticity and divergence at the record's points: g_cd = sum_n D_d[pt][n] u_c[n] over the cell's 16 nodes with
// the tables dx[pt][16], dy[pt][16] (postprocess.record_gradient_tables), n increasing, one accumulator per sum; then
// vort = g_10 - g_01 and div = g_00 + g_11.  A workgroup takes cpg = BLK / ppc consecutive cells of the record: it stages the
// two tables and its cells' 16 (u_x, u_y) pairs — gathered through cell_u with one 16-byte load per node, owned or ghost —
// in LDS, so the state is read from memory once per cell; thread lc * ppc + pt then forms its point's four sums from LDS.
// vort / div: either may be null (the field was not asked for).  No atomics: two calls give the same bits.
constexpr int RF_MAX_PPC = 25, RF_MAX_CELLS = BLK / 4;
__global__ __launch_bounds__(BLK) void record_fields_kernel(long n_cells, int ppc, int cpg, const int *__restrict__ cells,
                                                            const int *__restrict__ cell_u, const double *__restrict__ dx,
                                                            const double *__restrict__ dy, const double *__restrict__ su,
                                                            double *__restrict__ vort, double *__restrict__ div) {
  __shared__ double sdx[RF_MAX_PPC * 16], sdy[RF_MAX_PPC * 16];
  __shared__ double2 suv[RF_MAX_CELLS * 16];
  const long cell0 = (long)blockIdx.x * cpg;
  const long left = n_cells - cell0;
  const int nc = left < cpg ? (int)left : cpg;
  for (int i = threadIdx.x; i < ppc * 16; i += BLK) { sdx[i] = dx[i]; sdy[i] = dy[i]; }
  for (int i = threadIdx.x; i < nc * 16; i += BLK) {
    const long cell = cells[cell0 + (i >> 4)];
    const int node = cell_u[cell * 16 + (i & 15)];
    suv[i] = *reinterpret_cast<const double2 *>(su + 2 * (size_t)node);
  }
  __syncthreads();
  const int lc = (int)threadIdx.x / ppc, pt = (int)threadIdx.x - lc * ppc;
  if (lc >= nc) return;
  const double *X = sdx + pt * 16, *Y = sdy + pt * 16;
  const double2 *U = suv + lc * 16;
  double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
  for (int n = 0; n < 16; ++n) {
    const double2 uv = U[n];
    g00 += X[n] * uv.x; g01 += Y[n] * uv.x;
    g10 += X[n] * uv.y; g11 += Y[n] * uv.y;
  }
  const long t = (cell0 + lc) * ppc + pt;
  if (vort) vort[t] = g10 - g01;
  if (div) div[t] = g00 + g11;
}

}  // namespace

static void forces_sum(hipStream_t s, long n_slots, const double *slots, double *out2) {
  hipLaunchKernelGGL(forces_sum_kernel, dim3(1), dim3(BLK), 0, s, n_slots, slots, out2);
}
void forces_faces(hipStream_t s, const AsmMesh &M, long n_faces, const int *face_cell, const unsigned char *face_side,
                  const double *ftab, const double *su, const double *sp, double nu, double *slots, double *out2) {
  if (n_faces > 0)
    hipLaunchKernelGGL(forces_faces_kernel, dim3((unsigned)((n_faces * 4 + BLK - 1) / BLK)), dim3(BLK), 0, s, n_faces, M.cell_u,
                       M.cell_p, face_cell, face_side, ftab, su, sp, nu, slots);
  forces_sum(s, n_faces * 4, slots, out2);
}
void state_patches(hipStream_t s, const AsmMesh &M, long n, const int *cells, const double *su, const double *sp, double *vel,
                   double *prs) {
  if (n > 0)
    hipLaunchKernelGGL(state_patches_kernel, dim3((unsigned)((n * 4 + BLK - 1) / BLK)), dim3(BLK), 0, s, n, cells, M.cell_u,
                       M.cell_p, su, sp, vel, prs);
}

void asm_matfree_F(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, const double *d0,
                   const double *x_own, const double *x_ghost, double *wk, double *y) {
  if (M.n_unodes <= 0) return;
  if (M.n_cells > 0)
    hipLaunchKernelGGL(mf_cell_flux_kernel, dim3((unsigned)((M.n_cells + MF_CELLS - 1) / MF_CELLS)), dim3(BLK), 0, s, M, cq, nu,
                       inv_dt, stokes, x_own, x_ghost, wk);
  hipLaunchKernelGGL(mf_rows_kernel, dim3((unsigned)((M.n_unodes + BLK - 1) / BLK)), dim3(BLK), 0, s, M, wk, d0, x_own, y);
}
double asm_matfree_F_bytes(const AsmMesh &M, int stokes) {
  // cell kernel: cell_u (64) + cq fields 0-5 (768, not in the Stokes phase) + its share written (256); rows kernel: the
  // shares read (256 per cell), node_cells (16), one flag, y (16); x once (16 per node) and the tables
  return (double)M.n_cells * (64.0 + (stokes ? 0.0 : 768.0) + 256.0 + 256.0) + (double)M.n_unodes * (16.0 + 1.0 + 16.0 + 16.0) +
         8.0 * (3 * 256 + 16);
}

void asm_cell_state(hipStream_t s, const AsmMesh &M, const double *su, const double *sp, const double *so, double *cq) {
  const long n = (long)M.n_cells * 16;
  if (n > 0) hipLaunchKernelGGL(asm_cell_state_kernel, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, s, M, su, sp, so, cq);
}
void asm_d0(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, double *out) {
  hipLaunchKernelGGL(asm_d0_kernel, dim3(1), dim3(64), 0, s, M, cq, nu, inv_dt, stokes, out);
}
void asm_F_rows(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, const double *d0,
                const int *rowptr, double *val) {
  if (M.n_unodes > 0)
    hipLaunchKernelGGL(asm_F_rows_kernel, dim3((unsigned)((M.n_unodes + 3) / 4)), dim3(BLK), 0, s, M, cq, nu, inv_dt,
                       stokes, d0, rowptr, val);
}
void asm_rhs_u(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, double p_out, int stokes,
               const double *d0, const double *bc, double *rhs, double *x0) {
  if (M.n_unodes > 0)
    hipLaunchKernelGGL(asm_rhs_u_kernel, dim3((unsigned)((M.n_unodes + BLK - 1) / BLK)), dim3(BLK), 0, s, M, cq, nu, inv_dt,
                       p_out, stokes, d0, bc, rhs, x0);
}
void asm_rhs_p(hipStream_t s, const AsmMesh &M, const double *cq, int stokes, double *rhs) {
  if (M.n_pdofs > 0)
    hipLaunchKernelGGL(asm_rhs_p_kernel, dim3((unsigned)((M.n_pdofs + BLK - 1) / BLK)), dim3(BLK), 0, s, M, cq, stokes, rhs);
}

void state_record(hipStream_t s, const AsmMesh &M, long n_cells, int subdivisions, const int *cells, const double *wu,
                  const double *wp, const double *su, const double *sp, double *vel3, double *prs) {
  const int ppc = (subdivisions + 1) * (subdivisions + 1);
  const long n_points = n_cells * ppc;
  if (n_points <= 0) return;
  const dim3 grid((unsigned)((n_points + BLK - 1) / BLK));
  if (subdivisions == 1)
    hipLaunchKernelGGL(state_record_copy_kernel, grid, dim3(BLK), 0, s, n_points, cells, M.cell_u, M.cell_p, su, sp, vel3, prs);
  else
    hipLaunchKernelGGL(state_record_kernel, grid, dim3(BLK), 0, s, n_points, ppc, cells, M.cell_u, M.cell_p, wu, wp, su, sp,
                       vel3, prs);
}

void record_fields(hipStream_t s, const AsmMesh &M, long n_cells, int subdivisions, const int *cells, const double *dx,
                   const double *dy, const double *su, double *vort, double *div) {
  const int ppc = (subdivisions + 1) * (subdivisions + 1), cpg = BLK / ppc;
  if (n_cells <= 0 || ppc > RF_MAX_PPC || cpg > RF_MAX_CELLS) return;
  hipLaunchKernelGGL(record_fields_kernel, dim3((unsigned)((n_cells + cpg - 1) / cpg)), dim3(BLK), 0, s, n_cells, ppc, cpg, cells,
                     M.cell_u, dx, dy, su, vort, div);
}

}  // namespace nsk

// ------------------------------------------------------------------------------------------------------------------
// P2/P1 Taylor-Hood on triangles (the reference's -M path, NSSolverStationary.cpp:144-206: FE_SimplexP(2)^2 x
// FE_SimplexP(1), QGaussSimplex(3)): general, non-congruent cells.  Gather instead of the reference's cell scatter
// (jacobian_matrix.add, .cpp:534), like the Q3/Q2 kernels above, but one thread per 2x2 NODE BLOCK of (0,0): the
// host hands over, per block (row node n, column node m), the list of cells holding both with their local indices
// (1-2 cells for an edge pair, the whole patch for the diagonal); the thread integrates each cell's contribution
// with the 7-point degree-5 rule and adds them in list order — deterministic, no atomics, two assemblies give the
// same bits.  The element state (u, grad u at the quadrature points) is recomputed per (block, cell): a few hundred
// flops against one 32-byte store.
namespace nsk {
namespace {

__constant__ double kTriL[7][3] = {
    {1.0 / 3, 1.0 / 3, 1.0 / 3},
    {0.79742698535308731, 0.10128650732345633, 0.10128650732345633},
    {0.10128650732345633, 0.79742698535308731, 0.10128650732345633},
    {0.10128650732345633, 0.10128650732345633, 0.79742698535308731},
    {0.05971587178976989, 0.47014206410511505, 0.47014206410511505},
    {0.47014206410511505, 0.05971587178976989, 0.47014206410511505},
    {0.47014206410511505, 0.47014206410511505, 0.05971587178976989}};
__constant__ double kTriW[7] = {0.225,
                                0.12593918054482717, 0.12593918054482717, 0.12593918054482717,
                                0.13239415278850616, 0.13239415278850616, 0.13239415278850616};

// value and barycentric derivatives of P2 function k (0-2 vertices, 3-5 edges (0,1), (1,2), (2,0)) at lam
__device__ __forceinline__ void p2(int k, const double *lam, double &v, double dl[3]) {
  dl[0] = dl[1] = dl[2] = 0.0;
  if (k < 3) {
    v = lam[k] * (2.0 * lam[k] - 1.0);
    dl[k] = 4.0 * lam[k] - 1.0;
  } else {
    const int i = k - 3, j = (k - 2) % 3;
    v = 4.0 * lam[i] * lam[j];
    dl[i] = 4.0 * lam[j];
    dl[j] = 4.0 * lam[i];
  }
}
__device__ __forceinline__ void p2_grad(int k, const double *lam, const double *gl /* [3][2] */, double &v, double &gx,
                                        double &gy) {
  double dl[3];
  p2(k, lam, v, dl);
  gx = dl[0] * gl[0] + dl[1] * gl[2] + dl[2] * gl[4];
  gy = dl[0] * gl[1] + dl[1] * gl[3] + dl[2] * gl[5];
}

struct ElemState {   // velocity and its gradient at one quadrature point
  double u[2], g[2][2];
};
__device__ __forceinline__ ElemState elem_state(const int *cu, const double *gl, const double *lam, const double *su) {
  ElemState S{};
  for (int k = 0; k < 6; ++k) {
    double v, gx, gy;
    p2_grad(k, lam, gl, v, gx, gy);
    const double ux = su[2 * (size_t)cu[k]], uy = su[2 * (size_t)cu[k] + 1];
    S.u[0] += ux * v; S.u[1] += uy * v;
    S.g[0][0] += ux * gx; S.g[0][1] += ux * gy;
    S.g[1][0] += uy * gx; S.g[1][1] += uy * gy;
  }
  return S;
}

__global__ __launch_bounds__(256) void simplex_F_blocks_kernel(SimplexMesh M, const double *__restrict__ su, double nu,
                                                              double inv_dt, int stokes, double *__restrict__ val) {
  const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= M.n_blocks) return;
  double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
  for (int e = M.blk_ptr[b]; e < M.blk_ptr[b + 1]; ++e) {
    const int code = M.blk_ent[e], t = code / 36, ln = (code % 36) / 6, lm = code % 6;
    const int *cu = M.cell_u + 6 * (size_t)t;
    const double *gl = M.grad_lam + 6 * (size_t)t;
    const double area = M.area[t];
    double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
    for (int q = 0; q < 7; ++q) {
      const double *lam = kTriL[q];
      const double w = area * kTriW[q];
      double vn, gnx, gny, vm, gmx, gmy;
      p2_grad(ln, lam, gl, vn, gnx, gny);
      p2_grad(lm, lam, gl, vm, gmx, gmy);
      double diag = nu * (gnx * gmx + gny * gmy) + inv_dt * vn * vm;
      if (!stokes) {
        const ElemState S = elem_state(cu, gl, lam, su);
        diag += vn * (S.u[0] * gmx + S.u[1] * gmy);               // phi_n (u . grad) phi_m
        c00 += w * vn * S.g[0][0] * vm; c01 += w * vn * S.g[0][1] * vm;   // phi_n d_d u_c phi_m
        c10 += w * vn * S.g[1][0] * vm; c11 += w * vn * S.g[1][1] * vm;
      }
      c00 += w * diag;
      c11 += w * diag;
    }
    a00 += c00; a01 += c01; a10 += c10; a11 += c11;
  }
  const long p0 = M.blk_pos0[b], p1 = M.blk_pos1[b];
  val[p0] = a00; val[p0 + 1] = a01;
  val[p1] = a10; val[p1 + 1] = a11;
}

// Dirichlet rows: cleared, diagonal d0 = |(0,0) entry before clearing| (MatrixTools::apply_boundary_values, .cpp:574)
__global__ __launch_bounds__(256) void simplex_dirichlet_rows_kernel(int n_u, const int *__restrict__ rowptr,
                                                                    const int *__restrict__ col,
                                                                    const unsigned char *__restrict__ dir,
                                                                    const double *__restrict__ d0, double *__restrict__ val) {
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= n_u || !dir[r]) return;
  const double d = d0[0];
  for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) val[k] = col[k] == r ? d : 0.0;
}
// (pos < 0: another rank owns global DoF 0 and this one adds 0 to the sum over the ranks)
__global__ void simplex_d0_kernel(const double *val, long pos, double *out) { out[0] = pos >= 0 ? fabs(val[pos]) : 0.0; }

__global__ __launch_bounds__(256) void simplex_rhs_u_kernel(SimplexMesh M, const double *__restrict__ su,
                                                           const double *__restrict__ spv, const double *__restrict__ so,
                                                           double nu, double inv_dt, double p_out, int stokes,
                                                           const double *__restrict__ d0, const double *__restrict__ bc,
                                                           double *__restrict__ rhs, double *__restrict__ x0) {
  const int n = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (n >= M.n_unodes) return;
  double r0 = 0.0, r1 = 0.0;
  if (!stokes) {
    for (int e = M.node_ptr[n]; e < M.node_ptr[n + 1]; ++e) {
      const int code = M.node_ent[e], t = code / 6, ln = code % 6;
      const int *cu = M.cell_u + 6 * (size_t)t;
      const int *cp = M.cell_p + 3 * (size_t)t;
      const double *gl = M.grad_lam + 6 * (size_t)t;
      const double area = M.area[t];
      double e0 = 0.0, e1 = 0.0;
      for (int q = 0; q < 7; ++q) {
        const double *lam = kTriL[q];
        const double w = area * kTriW[q];
        double vn, gnx, gny;
        p2_grad(ln, lam, gl, vn, gnx, gny);
        const ElemState S = elem_state(cu, gl, lam, su);
        const double pq = spv[cp[0]] * lam[0] + spv[cp[1]] * lam[1] + spv[cp[2]] * lam[2];
        double t0 = -nu * (S.g[0][0] * gnx + S.g[0][1] * gny) - (S.u[0] * S.g[0][0] + S.u[1] * S.g[0][1]) * vn + pq * gnx;
        double t1 = -nu * (S.g[1][0] * gnx + S.g[1][1] * gny) - (S.u[0] * S.g[1][0] + S.u[1] * S.g[1][1]) * vn + pq * gny;
        if (so && inv_dt != 0.0) {   // -(u - u_old) / dt . v
          double ox = 0.0, oy = 0.0;
          for (int k = 0; k < 6; ++k) {
            double v, dl[3];
            p2(k, lam, v, dl);
            ox += so[2 * (size_t)cu[k]] * v; oy += so[2 * (size_t)cu[k] + 1] * v;
          }
          t0 -= inv_dt * (S.u[0] - ox) * vn;
          t1 -= inv_dt * (S.u[1] - oy) * vn;
        }
        e0 += w * t0;
        e1 += w * t1;
      }
      r0 += e0;
      r1 += e1;
    }
  }
  r0 -= p_out * M.outlet_w[2 * (size_t)n];       // - p_out int phi . n over the id-8 edges (state-independent weights)
  r1 -= p_out * M.outlet_w[2 * (size_t)n + 1];
  for (int c = 0; c < 2; ++c) {
    const size_t r = 2 * (size_t)n + c;
    if (M.dirichlet[r]) {
      const double v = bc ? bc[r] : 0.0;
      rhs[r] = d0[0] * v;
      x0[r] = v;
    } else {
      rhs[r] = c ? r1 : r0;
      x0[r] = 0.0;
    }
  }
}

__global__ __launch_bounds__(256) void simplex_rhs_p_kernel(SimplexMesh M, const double *__restrict__ su, int stokes,
                                                           double *__restrict__ rhs, double *__restrict__ x0) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= M.n_pdofs) return;
  double r = 0.0;
  if (!stokes)
    for (int e = M.vert_ptr[j]; e < M.vert_ptr[j + 1]; ++e) {
      const int code = M.vert_ent[e], t = code / 3, lj = code % 3;
      const int *cu = M.cell_u + 6 * (size_t)t;
      const double *gl = M.grad_lam + 6 * (size_t)t;
      double acc = 0.0;
      for (int q = 0; q < 7; ++q) {
        const ElemState S = elem_state(cu, gl, kTriL[q], su);
        acc += M.area[t] * kTriW[q] * (S.g[0][0] + S.g[1][1]) * kTriL[q][lj];
      }
      r += acc;
    }
  rhs[j] = r;
  x0[j] = 0.0;
}

// Forces on the id-10 edges of a P2/P1 mesh: one thread per (edge, Gauss point), the two points of simplex.lift_drag
// (the integrand is at most quadratic along an edge).  The gradients of the six P2 functions come from the cell's
// grad_lambda.  edge_nl: per edge the fluid cell's outward normal and the length.
__global__ __launch_bounds__(256) void forces_edges_kernel(long n_edges, const int *__restrict__ cell_u,
                                                           const int *__restrict__ cell_p, const double *__restrict__ grad_lam,
                                                           const int *__restrict__ edge_cell,
                                                           const unsigned char *__restrict__ edge_local,
                                                           const double *__restrict__ edge_nl, const double *__restrict__ su,
                                                           const double *__restrict__ spv, double nu, double *__restrict__ slots) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_edges * 2) return;
  const long e = t >> 1;
  const long c = edge_cell[e];
  const int k = edge_local[e], i = k, j = (k + 1) % 3;   // local edge k joins vertices k and (k + 1) % 3
  const double gp = (t & 1) ? 0.78867513459481288 : 0.21132486540518712;   // 1/2 -+ 1/(2 sqrt 3)
  double lam[3] = {0.0, 0.0, 0.0};
  lam[i] = 1.0 - gp;
  lam[j] = gp;
  const int *cu = cell_u + 6 * (size_t)c;
  const int *cp = cell_p + 3 * (size_t)c;
  const double *gl = grad_lam + 6 * (size_t)c;
  double g00 = 0, g01 = 0, g10 = 0, g11 = 0;
  for (int n = 0; n < 6; ++n) {
    double v, gx, gy;
    p2_grad(n, lam, gl, v, gx, gy);
    const double ux = su[2 * (size_t)cu[n]], uy = su[2 * (size_t)cu[n] + 1];
    g00 += ux * gx; g01 += ux * gy;
    g10 += uy * gx; g11 += uy * gy;
  }
  const double p = spv[cp[0]] * lam[0] + spv[cp[1]] * lam[1] + spv[cp[2]] * lam[2];
  const double nx = edge_nl[3 * e], ny = edge_nl[3 * e + 1], w = 0.5 * edge_nl[3 * e + 2];
  const double s00 = nu * (g00 + g00) - p, s01 = nu * (g01 + g10), s11 = nu * (g11 + g11) - p;
  slots[2 * t] = -(s00 * nx + s01 * ny) * w;
  slots[2 * t + 1] = -(s01 * nx + s11 * ny) * w;
}

// The VTU record of a P2/P1 mesh in file layout: the mesh's vertices are the first n_points velocity nodes
// and the pressure DoFs (simplex.py's numbering) — a strided copy, (u_x, u_y, +0.0) per vertex.
__global__ __launch_bounds__(256) void simplex_record_kernel(long n_points, const double *__restrict__ su,
                                                             const double *__restrict__ spv, double *__restrict__ vel3,
                                                             double *__restrict__ prs) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_points) return;
  vel3[3 * t] = su[2 * t];
  vel3[3 * t + 1] = su[2 * t + 1];
  vel3[3 * t + 2] = 0.0;
  prs[t] = spv[t];
}

// The same record for a list of points (one rank's piece): point t is velocity node u_node[t] and pressure DoF
// p_dof[t] of the state [owned | ghost] — a gather, the bits of the state.  The ids were checked on the host.
__global__ __launch_bounds__(256) void simplex_record_points_kernel(long n_points, const int *__restrict__ u_node,
                                                                    const int *__restrict__ p_dof,
                                                                    const double *__restrict__ su,
                                                                    const double *__restrict__ spv, double *__restrict__ vel3,
                                                                    double *__restrict__ prs) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_points) return;
  const size_t n = (size_t)u_node[t];
  vel3[3 * t] = su[2 * n];
  vel3[3 * t + 1] = su[2 * n + 1];
  vel3[3 * t + 2] = 0.0;
  prs[t] = spv[p_dof[t]];
}

// Vorticity and divergence at the vertices of a P2/P1 mesh: the gradient of a P2 field jumps from cell to
// cell, so vertex v gets (sum_t area_t f_t(v)) / (sum_t area_t) over the cells of vert_ptr / vert_ent in list order, f_t(v)
// the field from the gradients of the cell's six P2 functions at lambda = e_lv (p2_grad, as forces_edges_kernel forms them),
// n increasing, one accumulator per sum.  One thread per vertex, no atomics: two calls give the same bits.  A vertex of no
// cell gets +0.0.  vort / div: either may be null.
__global__ __launch_bounds__(256) void simplex_record_fields_kernel(long n_points, const int *__restrict__ cell_u,
                                                                    const double *__restrict__ grad_lam,
                                                                    const double *__restrict__ area,
                                                                    const int *__restrict__ vert_ptr,
                                                                    const int *__restrict__ vert_ent,
                                                                    const double *__restrict__ su, double *__restrict__ vort,
                                                                    double *__restrict__ div) {
  const long v = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_points) return;
  double sw = 0.0, sd = 0.0, sa = 0.0;
  for (int e = vert_ptr[v]; e < vert_ptr[v + 1]; ++e) {
    const int code = vert_ent[e], t = code / 3, lv = code % 3;
    const double lam[3] = {lv == 0 ? 1.0 : 0.0, lv == 1 ? 1.0 : 0.0, lv == 2 ? 1.0 : 0.0};
    const int *cu = cell_u + 6 * (size_t)t;
    const double *gl = grad_lam + 6 * (size_t)t;
    double g00 = 0, g01 = 0, g10 = 0, g11 = 0;
    for (int n = 0; n < 6; ++n) {
      double val, gx, gy;
      p2_grad(n, lam, gl, val, gx, gy);
      const double ux = su[2 * (size_t)cu[n]], uy = su[2 * (size_t)cu[n] + 1];
      g00 += ux * gx; g01 += ux * gy;
      g10 += uy * gx; g11 += uy * gy;
    }
    const double a = area[t];
    sw += a * (g10 - g01);
    sd += a * (g00 + g11);
    sa += a;
  }
  if (vort) vort[v] = sa > 0.0 ? sw / sa : 0.0;
  if (div) div[v] = sa > 0.0 ? sd / sa : 0.0;
}

}  // namespace

void simplex_record_fields(hipStream_t s, const SimplexMesh &M, long n_points, const double *su, double *vort, double *div) {
  if (n_points > 0)
    hipLaunchKernelGGL(simplex_record_fields_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, n_points, M.cell_u,
                       M.grad_lam, M.area, M.vert_ptr, M.vert_ent, su, vort, div);
}

void simplex_record(hipStream_t s, long n_points, const double *su, const double *sp, double *vel3, double *prs) {
  if (n_points > 0)
    hipLaunchKernelGGL(simplex_record_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, n_points, su, sp, vel3,
                       prs);
}

void simplex_record_points(hipStream_t s, long n_points, const int *u_node, const int *p_dof, const double *su, const double *sp,
                           double *vel3, double *prs) {
  if (n_points > 0)
    hipLaunchKernelGGL(simplex_record_points_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, s, n_points, u_node,
                       p_dof, su, sp, vel3, prs);
}

void forces_edges(hipStream_t s, const SimplexMesh &M, long n_edges, const int *edge_cell, const unsigned char *edge_local,
                  const double *edge_nl, const double *su, const double *sp, double nu, double *slots, double *out2) {
  if (n_edges > 0)
    hipLaunchKernelGGL(forces_edges_kernel, dim3((unsigned)((n_edges * 2 + 255) / 256)), dim3(256), 0, s, n_edges, M.cell_u,
                       M.cell_p, M.grad_lam, edge_cell, edge_local, edge_nl, su, sp, nu, slots);
  forces_sum(s, n_edges * 2, slots, out2);
}

void simplex_assemble_blocks(hipStream_t s, const SimplexMesh &M, const double *su, double nu, double inv_dt, int stokes,
                             double *val, double *d0) {
  const int T = 256;
  hipLaunchKernelGGL(simplex_F_blocks_kernel, dim3((unsigned)((M.n_blocks + T - 1) / T)), dim3(T), 0, s, M, su, nu, inv_dt,
                     stokes, val);
  hipLaunchKernelGGL(simplex_d0_kernel, dim3(1), dim3(1), 0, s, val, (long)M.pos00, d0);
}

void simplex_assemble_rows(hipStream_t s, const SimplexMesh &M, const double *su, const double *sp, const double *so, double nu,
                           double inv_dt, double p_out, int stokes, const int *rowptr, const int *col, double *val,
                           const double *d0, const double *bc, double *rhs_u, double *rhs_p, double *x0_u, double *x0_p) {
  const int T = 256;
  hipLaunchKernelGGL(simplex_dirichlet_rows_kernel, dim3((2 * M.n_unodes + T - 1) / T), dim3(T), 0, s, 2 * M.n_unodes, rowptr,
                     col, M.dirichlet, d0, val);
  hipLaunchKernelGGL(simplex_rhs_u_kernel, dim3((M.n_unodes + T - 1) / T), dim3(T), 0, s, M, su, sp, so, nu, inv_dt, p_out,
                     stokes, d0, bc, rhs_u, x0_u);
  hipLaunchKernelGGL(simplex_rhs_p_kernel, dim3((M.n_pdofs + T - 1) / T), dim3(T), 0, s, M, su, stokes, rhs_p, x0_p);
}

}  // namespace nsk
