// nsk_capi_assembly.cpp — the device-assembly group of include/nsk.h: cell data, Newton state, nsk_assemble, the consumers
// of the solution (forces, output patches, the VTU record) and nsk_time_assemble.  Kernels: nsk_assembly_kernels.hip.
#include <algorithm>

#include <omp.h>
#include "nsk_handle.hpp"

extern "C" {

// ------------------------------------------------------------------ device assembly + Newton state
int nsk_assembly_set_cells(nsk_handle h, int64_t n_cells, const int32_t *cell_u_nodes, const int32_t *cell_p_dofs,
                           const uint8_t *cell_flags, const double *tables944, int32_t cell_of_dof0) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  if (n_cells <= 0 || !cell_u_nodes || !cell_p_dofs || !cell_flags || !tables944) throw Error(-60, "nsk_assembly_set_cells: bad arguments");
  Csr &F = h->blk[NSK_BLK_F];
  const int nu = h->n_u(), np = h->n_p();
  if (nu % 2 || h->sp[0].ng % 2) throw Error(-61, "assembly needs both velocity components of every node");
  const int n_nodes = nu / 2, n_nodes_all = (nu + h->sp[0].ng) / 2, n_p_all = np + h->sp[1].ng;
  if (cell_of_dof0 >= n_cells) throw Error(-60, "nsk_assembly_set_cells: cell_of_dof0 out of range");
  std::vector<int> node_cells((size_t)n_nodes * 4, -1), pdof_cells((size_t)np * 4, -1), cnt_u((size_t)n_nodes, 0), cnt_p((size_t)np, 0);
  for (int64_t c = 0; c < n_cells; ++c) {
    for (int n = 0; n < 16; ++n) {
      const int node = cell_u_nodes[c * 16 + n];
      if (node < 0 || node >= n_nodes_all) throw Error(-62, "assembly: velocity node id out of range");
      if (node < n_nodes) {
        if (cnt_u[node] >= 4) throw Error(-63, "assembly: more than 4 cells touch one velocity node");
        node_cells[(size_t)node * 4 + cnt_u[node]++] = (int)(c * 16 + n);
      }
    }
    for (int m = 0; m < 9; ++m) {
      const int d = cell_p_dofs[c * 9 + m];
      if (d < 0 || d >= n_p_all) throw Error(-62, "assembly: pressure DoF id out of range");
      if (d < np) {
        if (cnt_p[d] >= 4) throw Error(-63, "assembly: more than 4 cells touch one pressure DoF");
        pdof_cells[(size_t)d * 4 + cnt_p[d]++] = (int)(c * 9 + m);
      }
    }
  }
  // where each (row node, cell, column node) block lives in the node's rows of jacobian(0,0)
  std::vector<unsigned char> node_off((size_t)n_nodes * 64, 0);
  std::vector<int> node_self((size_t)n_nodes, 0);
  bool ok = true;
#pragma omp parallel for schedule(static) reduction(&& : ok)
  for (int r = 0; r < n_nodes; ++r) {
    const int a0 = F.h_rowptr[2 * r], a1 = F.h_rowptr[2 * r + 1], a2 = F.h_rowptr[2 * r + 2];
    if (cnt_u[r] == 0 || a1 - a0 != a2 - a1 || (a1 - a0) % 2 || (a1 - a0) / 2 > 49) { ok = false; continue; }
    auto find = [&](int node) {
      for (int k = a0; k + 1 < a1; k += 2)
        if (F.h_col[k] == 2 * node && F.h_col[k + 1] == 2 * node + 1) return (k - a0) / 2;
      return -1;
    };
    const int self = find(r);
    if (self < 0) { ok = false; continue; }
    node_self[r] = self;
    for (int k = 0; k < cnt_u[r]; ++k) {
      const int64_t cell = node_cells[(size_t)r * 4 + k] / 16;
      for (int m = 0; m < 16; ++m) {
        const int off = find(cell_u_nodes[cell * 16 + m]);
        if (off < 0) { ok = false; break; }
        node_off[(size_t)r * 64 + k * 16 + m] = (unsigned char)off;
      }
    }
  }
  if (!ok) throw Error(-64, "assembly: a cell couples DoFs that are not in the sparsity pattern of block (0,0)");
  for (int d = 0; d < np; ++d)
    if (cnt_p[d] == 0) throw Error(-64, "assembly: an owned pressure DoF belongs to no cell");
  // reference-cell tables + the state-independent element matrices K (viscosity) and M3 (mass)
  std::vector<double> tab(1456);
  std::copy(tables944, tables944 + 944, tab.begin());
  const double *phi = tables944, *dpx = tables944 + 256, *dpy = tables944 + 512, *jxw = tables944 + 912;
  for (int n = 0; n < 16; ++n)
    for (int m = 0; m < 16; ++m) {
      double kk = 0.0, mm = 0.0;
      for (int q = 0; q < 16; ++q) {
        kk += jxw[q] * (dpx[n * 16 + q] * dpx[m * 16 + q] + dpy[n * 16 + q] * dpy[m * 16 + q]);
        mm += jxw[q] * phi[n * 16 + q] * phi[m * 16 + q];
      }
      tab[944 + n * 16 + m] = kk;
      tab[1200 + n * 16 + m] = mm;
    }
  auto &A = h->asmd;
  hipStream_t s = h->s();
  A.n_cells = (long)n_cells;
  A.cell_of_dof0 = cell_of_dof0;
  A.cell_u.upload(cell_u_nodes, (size_t)n_cells * 16, s);
  A.cell_p.upload(cell_p_dofs, (size_t)n_cells * 9, s);
  A.cell_flags.upload(cell_flags, (size_t)n_cells, s);
  A.node_cells.upload(node_cells, s);
  A.node_self.upload(node_self, s);
  A.node_off.upload(node_off, s);
  A.pdof_cells.upload(pdof_cells, s);
  A.tables.upload(tab, s);
  A.cq.alloc((size_t)n_cells * kAsmCellDoubles);
  A.mf_wk.alloc((size_t)n_cells * kMatfreeCellDoubles);
  A.d0.alloc(1);
  A.mf_valid = false;   // (cq of another mesh)
  A.forces_set = false;   // (faces index the cells of another mesh)
  A.record_set = false;   // (so does the record's list)
  A.rec_grad_set = false;
  A.rec_points_set = false;
  if (!A.sol_u) {
    A.sol_u = h->pool_u.get(true); A.eval_u = h->pool_u.get(true); A.old_u = h->pool_u.get(true);
    A.sol_p = h->pool_p.get(true); A.eval_p = h->pool_p.get(true);
  }
  h->ctx.sync();
  A.ready = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_assembly_set_dirichlet(nsk_handle h, const uint8_t *dirichlet_u, const double *bc_u) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  if (!dirichlet_u) throw Error(-60, "nsk_assembly_set_dirichlet: bad arguments");
  for (int r = 0; r + 1 < h->n_u(); r += 2)
    if ((dirichlet_u[r] != 0) != (dirichlet_u[r + 1] != 0)) throw Error(-65, "assembly: Dirichlet flags must cover both components of a node");
  h->asmd.dirichlet.upload(dirichlet_u, (size_t)h->n_u(), h->s());
  h->asmd.mf_valid = false;   // (rows of F were cleared under other flags)
  h->asmd.have_bc = bc_u != nullptr;
  if (bc_u) h->asmd.bc.upload(bc_u, (size_t)h->n_u(), h->s());
  h->ctx.sync();
  h->asmd.dirichlet_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_state_set(nsk_handle h, const double *u_owned, const double *p_owned) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-66, "call nsk_assembly_set_cells first");
  NSK_HIP(hipMemcpyAsync(A.sol_u, u_owned, sizeof(double) * (size_t)h->n_u(), hipMemcpyHostToDevice, h->s()));
  NSK_HIP(hipMemcpyAsync(A.sol_p, p_owned, sizeof(double) * (size_t)h->n_p(), hipMemcpyHostToDevice, h->s()));
  h->halo(0, h->pool_u.view(A.sol_u));   // solution = solution_owned: refresh the ghost entries
  h->halo(1, h->pool_p.view(A.sol_p));
  h->ctx.sync();
  A.state_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_state_get(nsk_handle h, double *u_owned, double *p_owned) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.state_set) throw Error(-66, "no state on the device");
  NSK_HIP(hipMemcpyAsync(u_owned, A.sol_u, sizeof(double) * (size_t)h->n_u(), hipMemcpyDeviceToHost, h->s()));
  NSK_HIP(hipMemcpyAsync(p_owned, A.sol_p, sizeof(double) * (size_t)h->n_p(), hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_state_save(nsk_handle h) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.state_set) throw Error(-66, "no state on the device");
  vec_copy(h->s(), h->n_u(), A.sol_u, A.eval_u);
  vec_copy(h->s(), h->n_p(), A.sol_p, A.eval_p);
  return 0;
  NSK_CATCH(h)
}

int nsk_state_save_old(nsk_handle h) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.state_set) throw Error(-66, "no state on the device");
  // solution_old = solution (NSSolver.cpp:813), ghost entries included
  vec_copy(h->s(), h->n_u() + h->sp[0].ng, A.sol_u, A.old_u);
  A.have_old = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_state_update(nsk_handle h, double alpha) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.state_set) throw Error(-66, "no state on the device");
  // solution_owned = evaluation_point; solution_owned.add(alpha, delta_owned); solution = solution_owned
  vec_copy(h->s(), h->n_u(), A.eval_u, A.sol_u);
  vec_copy(h->s(), h->n_p(), A.eval_p, A.sol_p);
  // (P2/P1: an assembly since the solve has overwritten x_b; the result is in the copy made there)
  const double *delta = (A.simplex && A.sx_delta_valid) ? A.sx_delta : h->x_b;
  vec_axpy(h->s(), h->n_u(), sref(alpha), delta, A.sol_u);
  vec_axpy(h->s(), h->n_p(), sref(alpha), delta + h->n_u(), A.sol_p);
  h->halo(0, h->pool_u.view(A.sol_u));
  h->halo(1, h->pool_p.view(A.sol_p));
  return 0;
  NSK_CATCH(h)
}

int nsk_assembly_set_simplex(nsk_handle h, int64_t n_cells, const int32_t *cell_u_nodes, const int32_t *cell_p_dofs,
                             const double *grad_lambda, const double *area, int64_t n_blocks, const int32_t *blk_ptr,
                             const int32_t *blk_ent, const int64_t *blk_pos0, const int64_t *blk_pos1,
                             const int32_t *node_ptr, const int32_t *node_ent, const int32_t *vert_ptr,
                             const int32_t *vert_ent, const double *outlet_w, int64_t pos00) {
  NSK_TRY_DEV(h)
  Csr &F = h->blk[NSK_BLK_F];
  if (!F.present) throw Error(-63, "hand the blocks over before the assembly data");
  const bool several = h->ctx.comm.nranks > 1;
  // several ranks: the cells' ids run on into the ghost tail of the state vectors [owned | ghost] (VecPool), whole nodes
  if (several && h->sp[0].ng % 2) throw Error(-65, "nsk_assembly_set_simplex: the ghost velocity DoFs must be whole nodes");
  h->ensure_pools();
  const int nun = h->n_u() / 2, np = h->n_p();
  const int nun_all = several ? nun + h->sp[0].ng / 2 : nun, np_all = several ? np + h->sp[1].ng : np;
  if (n_cells <= 0 || n_blocks <= 0 || pos00 >= F.nnz) throw Error(-64, "nsk_assembly_set_simplex: bad sizes");
  // pos00 = -1: another rank owns global DoF 0 (its |entry (0,0)| reaches this one in nsk_assemble's sum over the ranks)
  if (pos00 < (several ? -1 : 0)) throw Error(-64, "nsk_assembly_set_simplex: bad sizes (pos00 = -1 needs several ranks)");
  // shapes the kernels index with: checked on the host before anything is launched
  for (int64_t k = 0; k < 6 * n_cells; ++k)
    if (cell_u_nodes[k] < 0 || cell_u_nodes[k] >= nun_all) throw Error(-64, "simplex assembly: velocity node id out of range");
  for (int64_t k = 0; k < 3 * n_cells; ++k)
    if (cell_p_dofs[k] < 0 || cell_p_dofs[k] >= np_all) throw Error(-64, "simplex assembly: pressure DoF id out of range");
  if (blk_ptr[0] != 0 || node_ptr[0] != 0 || vert_ptr[0] != 0) throw Error(-64, "simplex assembly: lists must start at 0");
  for (int64_t b = 0; b < n_blocks; ++b) {
    if (blk_ptr[b + 1] < blk_ptr[b]) throw Error(-64, "simplex assembly: block list not ascending");
    if (blk_pos0[b] < 0 || blk_pos0[b] + 1 >= F.nnz || blk_pos1[b] < 0 || blk_pos1[b] + 1 >= F.nnz)
      throw Error(-64, "simplex assembly: block position outside block (0,0)");
  }
  for (int i = 0; i < nun; ++i)
    if (node_ptr[i + 1] < node_ptr[i]) throw Error(-64, "simplex assembly: node list not ascending");
  for (int i = 0; i < np; ++i)
    if (vert_ptr[i + 1] < vert_ptr[i]) throw Error(-64, "simplex assembly: vertex list not ascending");
  for (int k = 0; k < blk_ptr[n_blocks]; ++k)
    if (blk_ent[k] < 0 || blk_ent[k] / 36 >= n_cells) throw Error(-64, "simplex assembly: block entry names no cell");
  for (int k = 0; k < node_ptr[nun]; ++k)
    if (node_ent[k] < 0 || node_ent[k] / 6 >= n_cells) throw Error(-64, "simplex assembly: node entry names no cell");
  for (int k = 0; k < vert_ptr[np]; ++k)
    if (vert_ent[k] < 0 || vert_ent[k] / 3 >= n_cells) throw Error(-64, "simplex assembly: vertex entry names no cell");
  auto &A = h->asmd;
  hipStream_t s = h->s();
  A.n_cells = (long)n_cells;
  A.sx_blocks = (long)n_blocks;
  A.sx_pos00 = (long)pos00;
  A.cell_u.upload(cell_u_nodes, (size_t)n_cells * 6, s);
  A.cell_p.upload(cell_p_dofs, (size_t)n_cells * 3, s);
  A.sx_grad.upload(grad_lambda, (size_t)n_cells * 6, s);
  A.sx_area.upload(area, (size_t)n_cells, s);
  A.sx_blk_ptr.upload(blk_ptr, (size_t)n_blocks + 1, s);
  A.sx_blk_ent.upload(blk_ent, (size_t)blk_ptr[n_blocks], s);
  std::vector<long> p0(blk_pos0, blk_pos0 + n_blocks), p1(blk_pos1, blk_pos1 + n_blocks);
  A.sx_pos0.upload(p0, s);
  A.sx_pos1.upload(p1, s);
  A.sx_node_ptr.upload(node_ptr, (size_t)nun + 1, s);
  A.sx_node_ent.upload(node_ent, (size_t)node_ptr[nun], s);
  A.sx_vert_ptr.upload(vert_ptr, (size_t)np + 1, s);
  A.sx_vert_ent.upload(vert_ent, (size_t)vert_ptr[np], s);
  A.sx_outlet.upload(outlet_w, (size_t)h->n_u(), s);
  if (!A.sol_u) {
    A.sol_u = h->pool_u.get(true); A.eval_u = h->pool_u.get(true); A.old_u = h->pool_u.get(true);
    A.sol_p = h->pool_p.get(true); A.eval_p = h->pool_p.get(true);
  }
  h->ctx.sync();
  A.mf_valid = false;
  A.forces_set = false;   // (edges index the cells of another mesh)
  A.record_set = false;
  A.rec_grad_set = false;
  A.rec_points_set = false;   // (the points name nodes of another numbering)
  A.sx_delta_valid = false;
  A.rec_out.release();
  A.simplex = true;
  A.ready = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_assemble(nsk_handle h, int stokes, double nu, double inv_dt, double p_out, int inhomogeneous_bc,
                 double *residual_norm) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready || !A.dirichlet_set || !A.state_set) throw Error(-66, "nsk_assemble needs cells, Dirichlet flags and a state");
  if (!(nu > 0.0)) throw Error(-60, "nsk_assemble: nu must be positive");
  // (a hierarchy still pending here was requested for a solve that never applied it: it is built from the values the
  //  block holds when it is first applied — nsk.h, nsk_setup_preconditioner — here as after nsk_update_values)
  if (inhomogeneous_bc && !A.have_bc) throw Error(-60, "nsk_assemble: no boundary values were given");
  Csr &F = h->blk[NSK_BLK_F];
  hipStream_t s = h->s();
  const double t0 = wall_ms();
  const SlotLease sl(h->ctx, 3);
  if (A.simplex) {   // P2/P1 triangles: general cells (nsk_assembly_kernels.hip, second half)
    const SimplexMesh SM{A.n_cells, A.sx_blocks, h->n_u() / 2, h->n_p(), A.sx_pos00, A.cell_u.p, A.cell_p.p, A.sx_grad.p,
                         A.sx_area.p, A.sx_blk_ptr.p, A.sx_blk_ent.p, A.sx_pos0.p, A.sx_pos1.p, A.sx_node_ptr.p,
                         A.sx_node_ent.p, A.sx_vert_ptr.p, A.sx_vert_ent.p, A.sx_outlet.p, A.dirichlet.p};
    simplex_assemble_blocks(s, SM, A.sol_u, nu, inv_dt, stokes != 0, F.val.p, h->ctx.slot(sl));
    // the Dirichlet diagonal, as in the Q3/Q2 branch below: the rank owning global DoF 0 wrote it, the others 0
    if (h->ctx.comm.nranks > 1) h->ctx.comm.allreduce_sum(h->ctx.slot(sl), 1, s);
    if (A.x_is_result) {   // the rows below write the next initial guess over it: keep delta_owned for nsk_state_update
      if (!A.sx_delta) A.sx_delta = h->pool_b.get(false);
      vec_copy(s, h->N(), h->x_b, A.sx_delta);
      A.sx_delta_valid = true;
      A.x_is_result = false;
    }
    simplex_assemble_rows(s, SM, A.sol_u, A.sol_p, (A.have_old && inv_dt != 0.0) ? A.old_u : nullptr, nu, inv_dt, p_out,
                          stokes != 0, F.rowptr.p, F.col.p, F.val.p, h->ctx.slot(sl), inhomogeneous_bc ? A.bc.p : nullptr,
                          h->rhs_b, h->rhs_b + h->n_u(), h->x_b, h->x_b + h->n_u());
    ++F.values_version;
    F.refresh_blocked(s);
    h->ctx.norm2(h->N(), h->rhs_b, sl + 1);
    const double nrm = h->ctx.read_slots(sl + 2, 1)[0];
    if (residual_norm) *residual_norm = nrm;
    A.assemble_ms = wall_ms() - t0;
    return 0;
  }
  const AsmMesh M = h->asm_view();
  A.mf_valid = false;
  asm_cell_state(s, M, A.sol_u, A.sol_p, A.have_old ? A.old_u : nullptr, A.cq.p);
  stokes = stokes != 0;
  asm_d0(s, M, A.cq.p, nu, inv_dt, stokes, h->ctx.slot(sl));
  h->ctx.comm.allreduce_sum(h->ctx.slot(sl), 1, s);   // the rank owning global DoF 0 wrote it, the others 0
  vec_copy(s, 1, h->ctx.slot(sl), A.d0.p);            // (the slot is handed out again; the matrix-free F reads this copy)
  asm_F_rows(s, M, A.cq.p, nu, inv_dt, stokes, h->ctx.slot(sl), F.rowptr.p, F.val.p);
  ++F.values_version;
  A.mf_valid = true;   // F.val and cq: one state, these parameters
  A.mf_nu = nu; A.mf_inv_dt = inv_dt; A.mf_stokes = stokes;
  F.refresh_blocked(s);
  // the time term of the residual needs solution_old (nsk_state_save_old); without one it is left out
  asm_rhs_u(s, M, A.cq.p, nu, A.have_old ? inv_dt : 0.0, p_out, stokes, h->ctx.slot(sl),
            inhomogeneous_bc ? A.bc.p : nullptr, h->rhs_b, h->x_b);
  asm_rhs_p(s, M, A.cq.p, stokes, h->rhs_b + h->n_u());
  h->ctx.norm2(h->N(), h->rhs_b, sl + 1);
  const double nrm = h->ctx.read_slots(sl + 2, 1)[0];
  if (residual_norm) *residual_norm = nrm;
  A.assemble_ms = wall_ms() - t0;
  return 0;
  NSK_CATCH_ABORT(h)
}

// ------------------------------------------------------------------ consumers of the solution: forces, output patches
int nsk_forces_set_faces(nsk_handle h, int64_t n_faces, const int32_t *face_cell, const uint8_t *face_side,
                         const double *tables672) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_forces_set_faces: no cells on the handle (call nsk_assembly_set_cells first)");
  if (A.simplex) throw Error(-71, "nsk_forces_set_faces: the handle holds P2/P1 triangles (nsk_forces_set_edges)");
  if (n_faces < 0 || !tables672 || (n_faces > 0 && (!face_cell || !face_side))) throw Error(-60, "nsk_forces_set_faces: bad arguments");
  // what the kernel indexes with: checked on the host before anything is launched
  for (int64_t f = 0; f < n_faces; ++f) {
    if (face_cell[f] < 0 || face_cell[f] >= A.n_cells) throw Error(-72, "nsk_forces_set_faces: cell index out of range");
    if (face_side[f] > 3) throw Error(-72, "nsk_forces_set_faces: side out of range");
  }
  hipStream_t s = h->s();
  A.face_cell.upload(face_cell, (size_t)n_faces, s);
  A.face_side.upload(face_side, (size_t)n_faces, s);
  A.face_tab.upload(tables672, 672, s);
  A.force_slots.alloc((size_t)std::max<int64_t>(1, n_faces * 8));
  A.force_out.alloc(4);
  h->ctx.sync();
  A.n_faces = (long)n_faces;
  A.forces_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_forces_set_edges(nsk_handle h, int64_t n_edges, const int32_t *edge_cell, const uint8_t *edge_local,
                         const double *edge_nl) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_forces_set_edges: no cells on the handle (call nsk_assembly_set_simplex first)");
  if (!A.simplex) throw Error(-71, "nsk_forces_set_edges: the handle holds Q3/Q2 cells (nsk_forces_set_faces)");
  if (n_edges < 0 || (n_edges > 0 && (!edge_cell || !edge_local || !edge_nl))) throw Error(-60, "nsk_forces_set_edges: bad arguments");
  for (int64_t e = 0; e < n_edges; ++e) {
    if (edge_cell[e] < 0 || edge_cell[e] >= A.n_cells) throw Error(-72, "nsk_forces_set_edges: cell index out of range");
    if (edge_local[e] > 2) throw Error(-72, "nsk_forces_set_edges: local edge out of range");
  }
  hipStream_t s = h->s();
  A.face_cell.upload(edge_cell, (size_t)n_edges, s);
  A.face_side.upload(edge_local, (size_t)n_edges, s);
  A.face_tab.upload(edge_nl, (size_t)n_edges * 3, s);
  A.force_slots.alloc((size_t)std::max<int64_t>(1, n_edges * 4));
  A.force_out.alloc(4);
  h->ctx.sync();
  A.n_faces = (long)n_edges;
  A.forces_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_forces(nsk_handle h, double nu, double *drag_lift, double *local_drag_lift) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_forces: no cells on the handle");
  if (!A.forces_set) throw Error(-69, A.simplex ? "nsk_forces: no edges handed over (nsk_forces_set_edges)"
                                                : "nsk_forces: no faces handed over (nsk_forces_set_faces)");
  if (!A.state_set) throw Error(-73, "nsk_forces: no state on the device");
  if (!drag_lift) throw Error(-60, "nsk_forces: bad arguments");
  hipStream_t s = h->s();
  double *out = A.force_out.p;   // [0, 1] this rank's share, [2, 3] the sum over the ranks
  if (A.simplex) {
    const SimplexMesh SM{A.n_cells, A.sx_blocks, h->n_u() / 2, h->n_p(), A.sx_pos00, A.cell_u.p, A.cell_p.p, A.sx_grad.p,
                         A.sx_area.p, A.sx_blk_ptr.p, A.sx_blk_ent.p, A.sx_pos0.p, A.sx_pos1.p, A.sx_node_ptr.p,
                         A.sx_node_ent.p, A.sx_vert_ptr.p, A.sx_vert_ent.p, A.sx_outlet.p, A.dirichlet.p};
    forces_edges(s, SM, A.n_faces, A.face_cell.p, A.face_side.p, A.face_tab.p, A.sol_u, A.sol_p, nu, A.force_slots.p, out);
  } else {
    forces_faces(s, h->asm_view(), A.n_faces, A.face_cell.p, A.face_side.p, A.face_tab.p, A.sol_u, A.sol_p, nu,
                 A.force_slots.p, out);
  }
  vec_copy(s, 2, out, out + 2);
  h->ctx.comm.allreduce_sum(out + 2, 2, s);   // Utilities::MPI::sum (NSSolverStationary.cpp:895-896)
  double host[4];
  NSK_HIP(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, s));
  h->ctx.sync();
  drag_lift[0] = host[2]; drag_lift[1] = host[3];
  if (local_drag_lift) { local_drag_lift[0] = host[0]; local_drag_lift[1] = host[1]; }
  return 0;
  NSK_CATCH_ABORT(h)
}

int nsk_state_get_patches(nsk_handle h, int64_t n, const int32_t *cells, double *vel, double *prs) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_state_get_patches: no cells on the handle (call nsk_assembly_set_cells first)");
  if (A.simplex) throw Error(-71, "nsk_state_get_patches: the handle holds P2/P1 triangles");
  if (!A.state_set) throw Error(-73, "nsk_state_get_patches: no state on the device");
  if (n < 0 || (n > 0 && (!cells || !vel || !prs))) throw Error(-60, "nsk_state_get_patches: bad arguments");
  for (int64_t c = 0; c < n; ++c)
    if (cells[c] < 0 || cells[c] >= A.n_cells) throw Error(-72, "nsk_state_get_patches: cell index out of range");
  if (n == 0) return 0;
  hipStream_t s = h->s();
  DBuf<int> dc;
  DBuf<double> dv;
  dc.upload(cells, (size_t)n, s);
  dv.alloc((size_t)n * 12);
  state_patches(s, h->asm_view(), (long)n, dc.p, A.sol_u, A.sol_p, dv.p, dv.p + (size_t)n * 8);
  NSK_HIP(hipMemcpyAsync(vel, dv.p, sizeof(double) * (size_t)n * 8, hipMemcpyDeviceToHost, s));
  NSK_HIP(hipMemcpyAsync(prs, dv.p + (size_t)n * 8, sizeof(double) * (size_t)n * 4, hipMemcpyDeviceToHost, s));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_record_set_cells(nsk_handle h, int64_t n_cells, const int32_t *cells, int subdivisions, const double *w_u,
                         const double *w_p) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_record_set_cells: no cells on the handle (call nsk_assembly_set_cells first)");
  if (A.simplex) throw Error(-71, "nsk_record_set_cells: the handle holds P2/P1 triangles (their record is the mesh's vertices)");
  if (subdivisions < 1 || subdivisions > 4) throw Error(-60, "nsk_record_set_cells: subdivisions outside 1..4");
  if (n_cells < 0 || (n_cells > 0 && !cells) || (subdivisions > 1 && (!w_u || !w_p)))
    throw Error(-60, "nsk_record_set_cells: bad arguments");
  const int64_t ppc = (int64_t)(subdivisions + 1) * (subdivisions + 1);
  if (n_cells > INT64_MAX / (4 * ppc * (int64_t)sizeof(double))) throw Error(-60, "nsk_record_set_cells: bad arguments");
  // what the kernel indexes with: checked on the host before anything is launched
  for (int64_t c = 0; c < n_cells; ++c)
    if (cells[c] < 0 || cells[c] >= A.n_cells) throw Error(-72, "nsk_record_set_cells: cell index out of range");
  hipStream_t s = h->s();
  A.record_set = false;
  A.rec_grad_set = false;   // (tables of another list's subdivisions)
  A.rec_cell.upload(cells, (size_t)n_cells, s);
  if (subdivisions > 1) {
    A.rec_wu.upload(w_u, (size_t)ppc * 16, s);
    A.rec_wp.upload(w_p, (size_t)ppc * 9, s);
  } else {
    A.rec_wu.release();
    A.rec_wp.release();
  }
  A.rec_out.alloc((size_t)std::max<int64_t>(1, n_cells * ppc * 4));
  h->ctx.sync();
  A.rec_cells = (long)n_cells;
  A.rec_sub = subdivisions;
  A.record_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_record_set_points(nsk_handle h, int64_t n_points, const int32_t *u_node, const int32_t *p_dof) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_record_set_points: no cells on the handle (call nsk_assembly_set_simplex first)");
  if (!A.simplex) throw Error(-71, "nsk_record_set_points: the handle holds Q3/Q2 cells (nsk_record_set_cells)");
  if (n_points < 0 || (n_points > 0 && (!u_node || !p_dof)) || n_points > INT64_MAX / (4 * (int64_t)sizeof(double)))
    throw Error(-60, "nsk_record_set_points: bad arguments");
  // what the kernel indexes with: checked on the host before anything is launched.  The state is [owned | ghost]
  const int64_t nun_all = (h->n_u() + h->sp[0].ng) / 2, np_all = (int64_t)h->n_p() + h->sp[1].ng;
  for (int64_t k = 0; k < n_points; ++k) {
    if (u_node[k] < 0 || u_node[k] >= nun_all) throw Error(-72, "nsk_record_set_points: velocity node id out of range");
    if (p_dof[k] < 0 || p_dof[k] >= np_all) throw Error(-72, "nsk_record_set_points: pressure DoF id out of range");
  }
  hipStream_t s = h->s();
  A.rec_points_set = false;
  A.rec_unode.upload(u_node, (size_t)n_points, s);
  A.rec_pdof.upload(p_dof, (size_t)n_points, s);
  A.rec_out.alloc((size_t)std::max<int64_t>(1, n_points * 4));
  h->ctx.sync();
  A.rec_points = (long)n_points;
  A.rec_points_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_state_get_record(nsk_handle h, int64_t n_points, double *vel3, double *prs) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_state_get_record: no cells on the handle");
  if (!A.simplex && !A.record_set) throw Error(-69, "nsk_state_get_record: no record list handed over (nsk_record_set_cells)");
  if (!A.state_set) throw Error(-73, "nsk_state_get_record: no state on the device");
  const bool listed = A.simplex && A.rec_points_set;
  const int64_t want = listed ? (int64_t)A.rec_points
                              : A.simplex ? (int64_t)h->n_p() : (int64_t)A.rec_cells * (A.rec_sub + 1) * (A.rec_sub + 1);
  if (n_points != want || (n_points > 0 && (!vel3 || !prs)))
    throw Error(-60, "nsk_state_get_record: bad arguments (n_points is not the record's number of points)");
  if (n_points == 0) return 0;
  hipStream_t s = h->s();
  if (listed) {   // the listed points of a P2/P1 handle (nsk_record_set_points): one rank's piece, ghost vertices included
    if (A.rec_out.n != (size_t)n_points * 4) A.rec_out.alloc((size_t)n_points * 4);
    simplex_record_points(s, (long)n_points, A.rec_unode.p, A.rec_pdof.p, A.sol_u, A.sol_p, A.rec_out.p,
                          A.rec_out.p + (size_t)n_points * 3);
  } else if (A.simplex) {
    // the vertices are the first n_p velocity nodes (simplex.py's numbering); one rank: the state is [owned]
    if (h->ctx.comm.nranks > 1 || 2 * n_points > (int64_t)h->n_u())
      throw Error(-60, "nsk_state_get_record: the P2/P1 record covers one rank with the vertices numbered first");
    if (A.rec_out.n != (size_t)n_points * 4) A.rec_out.alloc((size_t)n_points * 4);
    simplex_record(s, (long)n_points, A.sol_u, A.sol_p, A.rec_out.p, A.rec_out.p + (size_t)n_points * 3);
  } else {
    state_record(s, h->asm_view(), A.rec_cells, A.rec_sub, A.rec_cell.p, A.rec_wu.p, A.rec_wp.p, A.sol_u, A.sol_p, A.rec_out.p,
                 A.rec_out.p + (size_t)n_points * 3);
  }
  NSK_HIP(hipMemcpyAsync(vel3, A.rec_out.p, sizeof(double) * (size_t)n_points * 3, hipMemcpyDeviceToHost, s));
  NSK_HIP(hipMemcpyAsync(prs, A.rec_out.p + (size_t)n_points * 3, sizeof(double) * (size_t)n_points, hipMemcpyDeviceToHost, s));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_record_set_gradient(nsk_handle h, int subdivisions, const double *d_x, const double *d_y) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready) throw Error(-69, "nsk_record_set_gradient: no cells on the handle (call nsk_assembly_set_cells first)");
  if (A.simplex) throw Error(-71, "nsk_record_set_gradient: the handle holds P2/P1 triangles (their fields need no tables)");
  if (!A.record_set) throw Error(-69, "nsk_record_set_gradient: no record list handed over (nsk_record_set_cells)");
  if (subdivisions != A.rec_sub) throw Error(-60, "nsk_record_set_gradient: subdivisions differ from the record's");
  if (!d_x || !d_y) throw Error(-60, "nsk_record_set_gradient: bad arguments");
  const size_t ppc = (size_t)(subdivisions + 1) * (subdivisions + 1);
  hipStream_t s = h->s();
  A.rec_grad_set = false;
  A.rec_dx.upload(d_x, ppc * 16, s);
  A.rec_dy.upload(d_y, ppc * 16, s);
  A.rec_fout.alloc(std::max<size_t>(1, (size_t)A.rec_cells * ppc * 2));
  h->ctx.sync();
  A.rec_grad_set = true;
  return 0;
  NSK_CATCH(h)
}

int nsk_state_get_record_fields(nsk_handle h, int64_t n_points, int fields, double *out) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (fields <= 0 || (fields & ~(NSK_FIELD_VORTICITY | NSK_FIELD_DIVERGENCE)))
    throw Error(-60, "nsk_state_get_record_fields: fields must be a non-empty mask of vorticity (1) and divergence (2)");
  if (!A.ready) throw Error(-69, "nsk_state_get_record_fields: no cells on the handle");
  if (!A.simplex && !A.record_set)
    throw Error(-69, "nsk_state_get_record_fields: no record list handed over (nsk_record_set_cells)");
  if (!A.state_set) throw Error(-73, "nsk_state_get_record_fields: no state on the device");
  if (A.simplex && A.rec_points_set)
    throw Error(-71, "nsk_state_get_record_fields: a point list is in force (a rank's piece sees only its own cells of a vertex)");
  const int64_t want = A.simplex ? (int64_t)h->n_p() : (int64_t)A.rec_cells * (A.rec_sub + 1) * (A.rec_sub + 1);
  if (n_points != want || (n_points > 0 && !out))
    throw Error(-60, "nsk_state_get_record_fields: bad arguments (n_points is not the record's number of points)");
  if (!A.simplex && !A.rec_grad_set)
    throw Error(-69, "nsk_state_get_record_fields: no gradient tables handed over (nsk_record_set_gradient)");
  if (A.simplex && (h->ctx.comm.nranks > 1 || 2 * n_points > (int64_t)h->n_u()))
    throw Error(-60, "nsk_state_get_record_fields: the P2/P1 record covers one rank with the vertices numbered first");
  if (n_points == 0) return 0;
  hipStream_t s = h->s();
  const bool wv = fields & NSK_FIELD_VORTICITY, wd = fields & NSK_FIELD_DIVERGENCE;
  if (A.simplex && A.rec_fout.n != (size_t)n_points * 2) A.rec_fout.alloc((size_t)n_points * 2);
  double *dv = wv ? A.rec_fout.p : nullptr, *dd = wd ? A.rec_fout.p + (size_t)n_points : nullptr;
  if (A.simplex) {
    const SimplexMesh SM{A.n_cells, A.sx_blocks, h->n_u() / 2, h->n_p(), A.sx_pos00, A.cell_u.p, A.cell_p.p, A.sx_grad.p,
                         A.sx_area.p, A.sx_blk_ptr.p, A.sx_blk_ent.p, A.sx_pos0.p, A.sx_pos1.p, A.sx_node_ptr.p,
                         A.sx_node_ent.p, A.sx_vert_ptr.p, A.sx_vert_ent.p, A.sx_outlet.p, A.dirichlet.p};
    simplex_record_fields(s, SM, (long)n_points, A.sol_u, dv, dd);
  } else {
    record_fields(s, h->asm_view(), A.rec_cells, A.rec_sub, A.rec_cell.p, A.rec_dx.p, A.rec_dy.p, A.sol_u, dv, dd);
  }
  double *o = out;   // vorticity first
  if (wv) { NSK_HIP(hipMemcpyAsync(o, dv, sizeof(double) * (size_t)n_points, hipMemcpyDeviceToHost, s)); o += n_points; }
  if (wd) NSK_HIP(hipMemcpyAsync(o, dd, sizeof(double) * (size_t)n_points, hipMemcpyDeviceToHost, s));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_scale_values(nsk_handle h, int blk, double factor) {
  NSK_TRY_DEV(h)
  if (blk < 0 || blk > NSK_BLK_S || !h->blk[blk].present) throw Error(-52, "nsk_scale_values: no such block");
  Csr &A = h->blk[blk];
  vec_scale(h->s(), (int)A.nnz, sref(factor), A.val.p);
  if (blk == NSK_BLK_MP) ++h->mp_values_version;
  if (blk == NSK_BLK_F) h->asmd.mf_valid = false;
  ++A.values_version;
  A.refresh_blocked(h->s());
  return 0;
  NSK_CATCH(h)
}

int nsk_download_rhs(nsk_handle h, double *ru, double *rp) {
  NSK_TRY_DEV(h)
  h->ensure_pools();
  NSK_HIP(hipMemcpyAsync(ru, h->rhs_b, sizeof(double) * (size_t)h->n_u(), hipMemcpyDeviceToHost, h->s()));
  NSK_HIP(hipMemcpyAsync(rp, h->rhs_b + h->n_u(), sizeof(double) * (size_t)h->n_p(), hipMemcpyDeviceToHost, h->s()));
  h->ctx.sync();
  return 0;
  NSK_CATCH(h)
}

int nsk_time_assemble(nsk_handle h, double nu, double inv_dt, int reps, double *avg_ms) {
  NSK_TRY_DEV(h)
  auto &A = h->asmd;
  if (!A.ready || !A.dirichlet_set || !A.state_set || reps <= 0) throw Error(-66, "nsk_time_assemble: nothing to time");
  Csr &F = h->blk[NSK_BLK_F];
  hipStream_t s = h->s();
  const AsmMesh M = h->asm_view();
  const SlotLease sl(h->ctx, 1);
  const Event e0, e1;
  auto once = [&]() {
    asm_cell_state(s, M, A.sol_u, A.sol_p, A.have_old ? A.old_u : nullptr, A.cq.p);
    asm_d0(s, M, A.cq.p, nu, inv_dt, 0, h->ctx.slot(sl));
    vec_copy(s, 1, h->ctx.slot(sl), A.d0.p);
    asm_F_rows(s, M, A.cq.p, nu, inv_dt, 0, h->ctx.slot(sl), F.rowptr.p, F.val.p);
    ++F.values_version;
    A.mf_valid = true;
    A.mf_nu = nu; A.mf_inv_dt = inv_dt; A.mf_stokes = 0;
    F.refresh_blocked(s);
    asm_rhs_u(s, M, A.cq.p, nu, A.have_old ? inv_dt : 0.0, 1.0, 0, h->ctx.slot(sl), nullptr, h->rhs_b, h->x_b);
    asm_rhs_p(s, M, A.cq.p, 0, h->rhs_b + h->n_u());
  };
  once();
  NSK_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < reps; ++i) once();
  NSK_HIP(hipEventRecord(e1, s));
  NSK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  NSK_HIP(hipEventElapsedTime(&ms, e0, e1));
  if (avg_ms) *avg_ms = ms / reps;
  return 0;
  NSK_CATCH(h)
}

}  // extern "C"
