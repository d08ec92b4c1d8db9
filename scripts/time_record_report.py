#!/usr/bin/env python3
"""Cost of one driver report with the ASCII record against NSK_VTU_FORMAT=binary on one mesh.

One handle, one process, a smooth state: `cli._report` with the ASCII writer (the parent's path: nsk_state_get_patches and
%.12g formatting) and with the binary record (nsk_state_get_record into the file image, one write), alternated `--rounds`
times; wall time ending after the files are closed, file sizes, the one-time cost of building the writer
(nsk_record_set_cells and the file image), and nsk_state_get_record alone.  `--subdivisions S`: one more binary report with
S x S patches per cell.
"""
import argparse, contextlib, io, os, subprocess, sys, tempfile, time, types
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from navier_stokes_solver_amd import cli, problem as P, solver as S

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="600,200")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--subdivisions", type=int, default=0, help="also one binary report with S x S patches per cell")
ap.add_argument("--reps", type=int, default=20, help="calls of nsk_state_get_record timed alone")
ap.add_argument("--source", default="", help="what to print as the source where the tree is no git checkout")
a = ap.parse_args()
nx, ny = (int(v) for v in a.mesh.split(","))
here = os.path.dirname(os.path.abspath(__file__))
sha = a.source or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=here).stdout.strip() or "unknown"
print(f"source: {sha}\nmesh {nx}x{ny}", flush=True)

t0 = time.time()
pr = P.generate(nx, ny, nu=0.1, mode=0, state=0, inlet_bc=1)
print(f"cells {len(pr.cell_flags)}, obstacle faces {len(pr.face_cell)}; hand-off produced in {time.time() - t0:.2f} s", flush=True)
ls = S.LinearSolver()
ls.set_problem(pr)
ls.set_assembly(pr, bc_u=pr.x0_u)
x, y = pr.support_u[0::2, 0], pr.support_u[0::2, 1]
u = np.zeros(pr.n_u)
u[0::2], u[1::2] = 4.0 * y * (0.41 - y) / 0.41 ** 2 * (1.0 + 0.1 * np.sin(3.0 * x)), 0.05 * np.sin(2.0 * x) * np.cos(5.0 * y)
ls.state_set(u, (2.2 - pr.support_p[:, 0]) * (1.0 + 0.2 * pr.support_p[:, 1]))
ls.set_forces(pr)
backend = types.SimpleNamespace(ls=ls)
out_dir = tempfile.mkdtemp(prefix="nsk_record_")
os.environ["NSK_OUTPUT_DIR"] = out_dir
os.environ.pop("NSK_HOST_POSTPROCESS", None)


def report(record, name):
    text = io.StringIO()
    t = time.time()
    with contextlib.redirect_stdout(text):
        cli._report(backend, nx, ny, 0.001, 1.0, name, 0, None, pr=pr, record=record)
    dt = time.time() - t
    size = os.path.getsize(os.path.join(out_dir, f"{name}_0.0.vtu"))
    coeff = "; ".join(ln for ln in text.getvalue().splitlines() if "coefficient" in ln)
    return dt, size, coeff


def build(s):
    t = time.time()
    rec = cli._make_record(ls, pr, dict(vtu_format="binary", vtu_subdivisions=s))
    return rec, time.time() - t


rec, t_build = build(1)
print(f"building the writer (nsk_record_set_cells + the file image, {len(rec.image)} bytes): {t_build:.3f} s", flush=True)
for r in range(a.rounds):
    dt, size, coeff = report(None, "ascii")
    print(f"round {r} ascii  report: {dt:8.3f} s   (piece {size} bytes; {coeff})", flush=True)
    dt, size, coeff = report(rec, "binary")
    print(f"round {r} binary report: {dt:8.3f} s   (piece {size} bytes; {coeff})", flush=True)
ls.state_record(vel3=rec.vel3, prs=rec.prs)
t = time.time()
for _ in range(a.reps):
    ls.state_record(vel3=rec.vel3, prs=rec.prs)
print(f"nsk_state_get_record of {rec.n_points} points alone: {(time.time() - t) / a.reps * 1e3:.2f} ms per call (wall, {a.reps} calls: "
      f"one launch + two downloads into the file image)", flush=True)
if a.subdivisions > 1:
    s = a.subdivisions
    rec, t_build = build(s)
    print(f"s = {s}: building the writer ({len(rec.image)} bytes): {t_build:.3f} s", flush=True)
    dt, size, coeff = report(rec, f"binary_s{s}")
    print(f"s = {s} binary report: {dt:8.3f} s   (piece {size} bytes, {rec.n_points} points, {rec.n_cells} cells; {coeff})", flush=True)
    ls.state_record(vel3=rec.vel3, prs=rec.prs)
    t = time.time()
    for _ in range(a.reps):
        ls.state_record(vel3=rec.vel3, prs=rec.prs)
    print(f"s = {s}: nsk_state_get_record of {rec.n_points} points alone: {(time.time() - t) / a.reps * 1e3:.2f} ms per call", flush=True)
ls.close()
for f in os.listdir(out_dir):
    os.remove(os.path.join(out_dir, f))
os.rmdir(out_dir)
