#!/usr/bin/env python3
"""Matrix-free F against the assembled inner product of F (NSK_OPT_INNER_MATRIX_FREE_F) on one mesh.

One handle, one process: after one nsk_assemble and a set-up (stationary aSIMPLE, option off), device time of
nsk_time_op 56 (the two matrix-free kernels) against op 50 (the inner solves' SpMV of the assembled F), alternated twice,
with the bytes each moves per product.  With --driver, also one `StationaryNSSolver -m nx,ny -r 30 -p 2` Newton solve per
setting of NSK_INNER_MATRIX_FREE_F: off, on, off, on (wall time of the child process and its last lines).  Run with
NSK_INNER_MATRIX_FREE_F unset: it would override the handle's option.
"""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navier_stokes_solver_amd import problem as P, solver as S

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="1200,400")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=2, help="times the pair (op 50, op 56) is taken, order alternating")
ap.add_argument("--driver", action="store_true", help="also time the stationary driver with the switch off, on, off, on")
ap.add_argument("--driver-timeout", type=int, default=600)
a = ap.parse_args()
if os.environ.get("NSK_INNER_MATRIX_FREE_F"):
    sys.exit("unset NSK_INNER_MATRIX_FREE_F: it overrides the option of the handle")
nx, ny = (int(v) for v in a.mesh.split(","))
sha = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True,
                     cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or "unknown"
out = {"source": sha, "mesh": [nx, ny], "reps": a.reps, "rounds": a.rounds}

t0 = time.time()
pr = P.generate(nx, ny, nu=1 / 30.0, mode=1, state=1)
print(f"{nx}x{ny}: n_u {pr.n_u}, n_p {pr.n_p}, nnz(F) {pr.F.nnz}, cells {len(pr.cell_flags)}, generated in {time.time() - t0:.1f} s",
      flush=True)
ls = S.LinearSolver()
ls.set_option(S.OPT_TRI_ORDERING, 1)
ls.set_problem(pr)
ls.set_assembly(pr)
ls.state_set(pr.x0_u * 0.0, pr.x0_p * 0.0)
ls.assemble(1 / 30.0, 0.0, 1.0)
ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
assert ls.inner_matrix_free() == 0 and ls.inner_value_bytes(S.BLK_F) == 8
ops = {S.TIMEOP_INNER_SPMV + S.BLK_F: "assembled inner SpMV F (op 50)", S.TIMEOP_MATFREE_F: "matrix-free F (op 56)"}
samples, fmt = {op: [] for op in ops}, {}
for r in range(a.rounds):
    for op in (list(ops) if r % 2 == 0 else list(ops)[::-1]):
        ms, by = ls.time_op(op, a.reps)
        samples[op].append(ms)
        fmt[op] = by
out["ops"] = {}
for op, nm in ops.items():
    v = sorted(samples[op])
    ms, gb = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), fmt[op] / 1e9
    print(f"{nm}: {ms:.4f} ms (rounds {', '.join(f'{x:.4f}' for x in samples[op])}), {gb:.3f} GB, {gb / ms * 1e3:.0f} GB/s", flush=True)
    out["ops"][nm] = dict(ms=ms, rounds=samples[op], GB=gb, GBps=gb / ms * 1e3)
a50, a56 = (out["ops"][ops[k]]["ms"] for k in ops)
print(f"matrix-free / assembled time: {a56 / a50:.3f}", flush=True)
out["matrix_free_over_assembled"] = a56 / a50
ls.close()

if a.driver:
    exe = os.path.join(os.path.dirname(os.path.abspath(S.__file__)), "bin", "StationaryNSSolver")
    out["driver"] = []
    for sw in ("0", "1", "0", "1"):
        env = dict(os.environ, NSK_INNER_MATRIX_FREE_F=sw)
        t0 = time.time()
        p = subprocess.run([exe, "-m", f"{nx},{ny}", "-r", "30", "-p", "2"], env=env, capture_output=True, text=True,
                           timeout=a.driver_timeout)
        wall = time.time() - t0
        tail = [l for l in p.stdout.splitlines() if l.strip()][-4:]
        said = any("NSK_INNER_MATRIX_FREE_F=1" in l for l in p.stdout.splitlines())
        print(f"StationaryNSSolver -m {nx},{ny} -r 30 -p 2, NSK_INNER_MATRIX_FREE_F={sw}: exit {p.returncode}, {wall:.1f} s wall, "
              f"driver line {'printed' if said else 'absent'}", flush=True)
        for l in tail:
            print("    " + l, flush=True)
        out["driver"].append(dict(switch=int(sw), exit=p.returncode, wall_s=wall, line=said, tail=tail))
        if p.returncode != 0:
            print(p.stderr[-2000:], flush=True)
            break
print(json.dumps(out))
