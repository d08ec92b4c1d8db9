#!/usr/bin/env python3
"""`-M` on two rank threads of one GPU: solve_newton() with the host-assembly backend (newton.MultiRankSimplexBackend) against
the rank-local device path of NSK_DEVICE_ASSEMBLY=1 (cli._gmsh_rank_main's set-up: simplex.device_rank_handoff,
newton.DeviceBackend with halo plans), alternated `--rounds` times on a structured triangulation of the empty channel
(DESIGN 5w).

Per run: wall time of solve_newton, the number of assemblies and solves, and the wall time per assembly split into
assembly (host: simplex.assemble; device: nsk_assemble and the two nsk_scale_values), hand-over (host only:
simplex.local_problem per rank, nsk_update_values per block, nsk_upload_system) and per solve (set-up, solve, and on the
host path the download and gather of the solution); then one report (forces and one VTU piece per rank, ASCII).  The
device path's figures are rank 0's: the ranks run in step.
"""
import argparse, os, subprocess, sys, tempfile, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from navier_stokes_solver_amd import gmsh as G, newton as N, partition as PT, simplex as SX, solver as S

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="200,40", help="cells of the lattice, two triangles each")
ap.add_argument("--re", type=float, default=30.0)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--ranks", type=int, default=2)
ap.add_argument("--tol", type=float, default=1e-8)
ap.add_argument("--source", default="", help="what to print as the source where the tree is no git checkout")
a = ap.parse_args()
nx, ny = (int(v) for v in a.mesh.split(","))
here = os.path.dirname(os.path.abspath(__file__))
sha = a.source or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=here).stdout.strip() or "unknown"
print(f"source: {sha}\nlattice {nx}x{ny}, {a.ranks} rank threads, Re {a.re:g}, FGMRES + aSIMPLE to {a.tol:g}", flush=True)


def channel(nx, ny, L=2.2, H=0.41):
    xs, ys = np.linspace(0, L, nx + 1), np.linspace(0, H, ny + 1)
    nodes = np.array([[x, y] for x in xs for y in ys])
    idx = lambda i, j: i * (ny + 1) + j    # noqa: E731
    tris, lines, ids = [], [], []
    for i in range(nx):
        for j in range(ny):
            p, q, r, s = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tris += [(p, q, r), (p, r, s)] if (i + j) % 2 == 0 else [(p, q, s), (q, r, s)]
    for i in range(nx):
        lines += [(idx(i, 0), idx(i + 1, 0)), (idx(i, ny), idx(i + 1, ny))]; ids += [6, 6]
    for j in range(ny):
        lines += [(idx(0, j), idx(0, j + 1)), (idx(nx, j), idx(nx, j + 1))]; ids += [7, 8]
    return G.TriMesh(nodes, np.array(tris), np.array(lines), np.array(ids))


t0 = time.time()
space = SX.build_space(channel(nx, ny))
lay = SX.rank_layout(space, a.ranks)
print(f"{len(space.cell_u)} triangles, {space.n_u} + {space.n_p} DoFs; space and layout in {time.time() - t0:.2f} s", flush=True)
out_dir = tempfile.mkdtemp(prefix="nsk_simplex_ranks_")
quiet = lambda *_a, **_k: None    # noqa: E731


class Clock:
    def __init__(self):
        self.t, self.n = {}, {}

    def wrap(self, key, fn):
        def timed(*args, **kw):
            t = time.perf_counter()
            try:
                return fn(*args, **kw)
            finally:
                self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t
                self.n[key] = self.n.get(key, 0) + 1
        return timed


def line(tag, wall, clk, report):
    na, ns = clk.n["assemble"], clk.n["solve"]
    prod = clk.t.get("producer", 0.0)
    asm = prod if prod else clk.t["assemble"]
    hand = clk.t["assemble"] - prod if prod else 0.0
    print(f"{tag}: solve_newton {wall:.2f} s; {na} assemblies, {ns} solves; per assembly: assembly {1e3 * asm / na:.2f} ms, "
          f"hand-over {1e3 * hand / na:.2f} ms; per solve {1e3 * clk.t['solve'] / ns:.2f} ms; one report {1e3 * report:.2f} ms", flush=True)


def run_host():
    clk = Clock()
    be = N.MultiRankSimplexBackend(space, a.ranks, S.FGMRES, S.ASIMPLE, a.tol, S.local_group_id(a.ranks, on_stream=True))
    real = SX.assemble
    SX.assemble = clk.wrap("producer", real)
    try:
        be.assemble, be.solve = clk.wrap("assemble", be.assemble), clk.wrap("solve", be.solve)
        t = time.perf_counter()
        N.solve_newton(be, a.re, log=quiet)
        wall = time.perf_counter() - t
        t = time.perf_counter()
        u, p = be.solution()
        be.lift_drag(1.0 / a.re)
        for r in range(a.ranks):
            SX.write_vtu(os.path.join(out_dir, f"host.{r}.vtu"), space, u, p, cells=np.nonzero(lay.cell_rank == r)[0])
        line("host assembly  ", wall, clk, time.perf_counter() - t)
    finally:
        SX.assemble = real
        be.close()


def run_device():
    first = SX.assemble(space, 0.1, mode=0, inlet_bc=1, U=0.1)
    uid = S.local_group_id(a.ranks, on_stream=True)
    parts = [SX.local_problem(first, lay, r) for r in range(a.ranks)]
    plans = [{S.SPACE_U: PT.build_halo_plan(r, lay.u_ranges, [q.ghost_u for q in parts]),
              S.SPACE_P: PT.build_halo_plan(r, lay.p_ranges, [q.ghost_p for q in parts])} for r in range(a.ranks)]
    res, errs = [None] * a.ranks, []

    def rank(r):
        try:
            q = parts[r]
            q.simplex = SX.device_rank_handoff(space, lay, r, q)
            ls = S.LinearSolver(r, a.ranks, 0, uid)
            try:
                ls.set_option(S.OPT_TRI_ORDERING, S.ORDER_MULTICOLOR)
                be = N.DeviceBackend(ls, q, S.FGMRES, S.ASIMPLE, a.tol, plan=plans[r])
                ls.set_force_edges_rank(space, lay, r, q.simplex)
                xy, tris, un, pd = SX.record_points_rank(space, lay, r, q.simplex)
                ls.set_record_points(un, pd)
                clk = Clock()
                be.assemble, be.solve = clk.wrap("assemble", be.assemble), clk.wrap("solve", be.solve)
                t = time.perf_counter()
                N.solve_newton(be, a.re, log=quiet)
                wall = time.perf_counter() - t
                t = time.perf_counter()
                ls.forces(1.0 / a.re)
                vel3, prs = ls.state_record(n_points=len(un))
                SX.write_vtu_points(os.path.join(out_dir, f"device.{r}.vtu"), xy, tris, vel3[:, 0], vel3[:, 1], prs)
                res[r] = (wall, clk, time.perf_counter() - t)
            finally:
                ls.close()
        except Exception as e:  # noqa: BLE001
            errs.append((r, repr(e)))
            S.abort_local_group(uid)

    th = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(a.ranks)]
    [t.start() for t in th]
    [t.join(3000) for t in th]
    if errs:
        raise RuntimeError(f"rank failures: {errs}")
    line("device assembly", *res[0])


for k in range(a.rounds):
    run_host()
    run_device()
