// nsk_assembly.hpp — device assembly of the Newton system (jacobian(0,0) values and residual_vector) and the
// Newton-loop state kept on the device.  Reference: NSSolverStationary::assemble_system(false, false)
// (lab_new/src/NSSolverStationary.cpp:317-577) and the solution / evaluation_point / delta_owned updates of
// solve_newton() (:710-735).  See nsk_assembly_kernels.hip for the kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace nsk {

struct AsmMesh {  // device pointers
  long n_cells;
  int n_unodes, n_pdofs;   // owned velocity nodes / pressure DoFs
  int cell_of_dof0;        // local cell whose node 0 is global DoF 0, or -1
  const int *cell_u;       // [n_cells][16] local velocity node ids (owned first, ghosts after)
  const int *cell_p;       // [n_cells][9] local pressure DoF ids
  const unsigned char *cell_flags;  // bit 0: outlet face
  const int *node_cells;   // [n_unodes][4]: cell * 16 + local node, or -1
  const unsigned char *node_off;    // [n_unodes][64]: block position of (cell k, column node m) in the node's row
  const int *node_self;    // [n_unodes]: block position of the diagonal block
  const int *pdof_cells;   // [n_pdofs][4]: cell * 9 + local node, or -1
  const unsigned char *dirichlet;   // per owned velocity DoF
  const double *tables;    // phi, dphi/dx, dphi/dy, psi, JxW, outlet face integrals, K, M3 (1456 doubles)
};

constexpr int kAsmCellDoubles = 144;  // cq entries per cell: 9 fields x 16 quadrature points
// so: solution_old (velocity) or nullptr
void asm_cell_state(hipStream_t s, const AsmMesh &M, const double *su, const double *sp, const double *so, double *cq);
// stokes != 0: the Stokes phase of the reference (assemble_system(.., computing_stokes = true)): no convective
// part in the matrix, no residual in the right-hand side (only the outlet term and the Dirichlet values)
void asm_d0(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, double *out);
void asm_F_rows(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, const double *d0,
                const int *rowptr, double *val);
void asm_rhs_u(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, double p_out, int stokes,
               const double *d0, const double *bc, double *rhs, double *x0);
void asm_rhs_p(hipStream_t s, const AsmMesh &M, const double *cq, int stokes, double *rhs);
// y = jacobian(0,0) x without reading the block: the operator asm_F_rows assembles, applied from cq.
// x: owned entries and ghost tail ([n_unodes] and the rest of cell_u's numbering, two doubles per node); d0: device
// pointer to the Dirichlet diagonal of that assembly; wk: kMatfreeCellDoubles per cell; y: owned rows.  Two launches.
constexpr int kMatfreeCellDoubles = 32;  // the cell's share of its 16 node rows, both components
void asm_matfree_F(hipStream_t s, const AsmMesh &M, const double *cq, double nu, double inv_dt, int stokes, const double *d0,
                   const double *x_own, const double *x_ghost, double *wk, double *y);
double asm_matfree_F_bytes(const AsmMesh &M, int stokes);   // bytes the two kernels move for one product

// ---- consumers of the solution: forces over boundary id 10, output patches ----
// su / sp: the resident `solution` [owned | ghost].  slots: 2 doubles per (face, Gauss point) — 4 points per Q3/Q2 face,
// 2 per P2/P1 edge; out2: (drag, lift) of the handed-over faces, the slots added in a fixed order by one workgroup.
// ftab: nsp_face_tables (672 doubles).  Two launches, no atomics.
void forces_faces(hipStream_t s, const AsmMesh &M, long n_faces, const int *face_cell, const unsigned char *face_side,
                  const double *ftab, const double *su, const double *sp, double nu, double *slots, double *out2);
// (u_x, u_y) [8 per cell] and p [4 per cell] at the four vertices of the listed cells: the bits of the state
void state_patches(hipStream_t s, const AsmMesh &M, long n, const int *cells, const double *su, const double *sp, double *vel,
                   double *prs);
// The VTU record in file layout: for the listed cells and pt = l (s + 1) + k, s = subdivisions in 1..4,
// (u_x, u_y, +0.0) into vel3 and p into prs.  s = 1: the bits of the state at the vertices; s > 1: the sums over the
// cell's 16 nodes / 9 DoFs with wu[(s+1)^2][16], wp[(s+1)^2][9], n increasing, one accumulator.  One launch, no atomics.
void state_record(hipStream_t s, const AsmMesh &M, long n_cells, int subdivisions, const int *cells, const double *wu,
                  const double *wp, const double *su, const double *sp, double *vel3, double *prs);
// Vorticity d_x u_y - d_y u_x and divergence d_x u_x + d_y u_y at the same points: four sums over the cell's 16
// nodes with dx[(s+1)^2][16], dy[(s+1)^2][16], n increasing, one accumulator each.  vort / div: n_cells (s+1)^2 doubles, or
// null for a field that is not wanted.  One launch, no atomics.
void record_fields(hipStream_t s, const AsmMesh &M, long n_cells, int subdivisions, const int *cells, const double *dx,
                   const double *dy, const double *su, double *vort, double *div);

// ---- P2/P1 on triangles (general cells; the reference's -M path) ----
struct SimplexMesh {  // device pointers
  long n_cells, n_blocks;
  int n_unodes, n_pdofs;
  long pos00;               // position of entry (0,0) in the scalar CSR of block (0,0); -1: another rank owns global DoF 0
  // several ranks: n_unodes / n_pdofs are the OWNED counts; the cells' ids run on into the ghost tail of the
  // state vectors [owned | ghost], every list below is over owned nodes / DoFs / rows
  const int *cell_u;        // [n_cells][6] velocity node ids (vertices, then edge midpoints (0,1), (1,2), (2,0))
  const int *cell_p;        // [n_cells][3]
  const double *grad_lam;   // [n_cells][3][2] gradients of the barycentric coordinates
  const double *area;       // [n_cells]
  const int *blk_ptr;       // [n_blocks + 1] per 2x2 node block of (0,0): its cells ...
  const int *blk_ent;       //   ... as cell * 36 + local row node * 6 + local column node
  const long *blk_pos0, *blk_pos1;   // position of the block's first entry in the node's first / second scalar row
  const int *node_ptr, *node_ent;    // per velocity node: cell * 6 + local node
  const int *vert_ptr, *vert_ent;    // per pressure DoF: cell * 3 + local vertex
  const double *outlet_w;   // [2 n_unodes] int phi_n n_c over the outlet (id 8) edges
  const unsigned char *dirichlet;    // per velocity DoF
};
// One assembly in two halves, the sum of d0 over the ranks between them (the rank owning global DoF 0 writes
// |val[pos00]|, the others 0).  simplex_assemble_blocks: the 2x2 node blocks of (0,0) and d0; simplex_assemble_rows: the
// Dirichlet rows and the two right-hand sides, which read d0.
void simplex_assemble_blocks(hipStream_t s, const SimplexMesh &M, const double *su, double nu, double inv_dt, int stokes,
                             double *val, double *d0);
void simplex_assemble_rows(hipStream_t s, const SimplexMesh &M, const double *su, const double *sp, const double *so, double nu,
                           double inv_dt, double p_out, int stokes, const int *rowptr, const int *col, double *val,
                           const double *d0, const double *bc, double *rhs_u, double *rhs_p, double *x0_u, double *x0_p);

// forces over the id-10 edges: edge_cell, edge_local (the cell's local edge 0-2), edge_nl = (nx, ny, length) per edge
void forces_edges(hipStream_t s, const SimplexMesh &M, long n_edges, const int *edge_cell, const unsigned char *edge_local,
                  const double *edge_nl, const double *su, const double *sp, double nu, double *slots, double *out2);
// the record of the mesh's vertices: the first n_points velocity nodes and pressure DoFs, (u_x, u_y, +0.0) and p
void simplex_record(hipStream_t s, long n_points, const double *su, const double *sp, double *vel3, double *prs);
// vorticity and divergence at those vertices: the area-weighted average over the vertex's cells (vert_ptr / vert_ent, list
// order) of the cell's own value at the vertex; vort / div may be null.  One launch, one thread per vertex
void simplex_record_fields(hipStream_t s, const SimplexMesh &M, long n_points, const double *su, double *vort, double *div);
// the record of listed points (nsk_record_set_points): per point a velocity node and a pressure DoF of the state
// [owned | ghost]; the bits of the state.  One launch, one thread per point
void simplex_record_points(hipStream_t s, long n_points, const int *u_node, const int *p_dof, const double *su, const double *sp,
                           double *vel3, double *prs);

}  // namespace nsk
