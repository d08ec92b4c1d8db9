#!/usr/bin/env python3
"""fp64 against fp32 values of the inner solves' matrices (NSK_OPT_INNER_MATRIX_PRECISION) on one mesh.

Two handles in one process, one per precision, on the same hand-off (stationary aSIMPLE): device time of the inner SpMVs
of F and S (nsk_time_op 50 / 55, alternated between the handles over several rounds), the bytes the stored format streams
per launch, device memory taken by each handle's set-up, and the inner iteration counts and time per outer step of a
short FGMRES run from the bench's initial state.  Run with NSK_INNER_MATRIX_PRECISION unset (it would override both
handles).  The factors stay fp64 in both handles (NSK_FACTOR_PRECISION must be unset too).
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navier_stokes_solver_amd import problem as P, solver as S

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="1200,400")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=5, help="outer FGMRES iterations for the inner iteration counts")
a = ap.parse_args()
if os.environ.get("NSK_INNER_MATRIX_PRECISION"):
    sys.exit("unset NSK_INNER_MATRIX_PRECISION: it overrides the option of both handles")
if os.environ.get("NSK_FACTOR_PRECISION"):
    sys.exit("unset NSK_FACTOR_PRECISION: both handles are meant to keep fp64 factors")
nx, ny = (int(v) for v in a.mesh.split(","))


def free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


t0 = time.time()
pr = P.generate(nx, ny, nu=1 / 90.0, mode=1, state=1)
print(f"{nx}x{ny}: n_u {pr.n_u}, n_p {pr.n_p}, nnz(F) {pr.F.nnz}, generated in {time.time() - t0:.1f} s", flush=True)
hs, mem = {}, {}
for bits in (64, 32):
    before = free_bytes()
    ls = S.LinearSolver()
    ls.set_option(S.OPT_TRI_ORDERING, 1)
    ls.set_option(S.OPT_INNER_MATRIX_PRECISION, bits)
    ls.set_problem(pr)
    ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
    mem[bits] = (before - free_bytes()) / 1e9
    hs[bits] = ls
    print(f"fp{bits}: inner value bytes F {ls.inner_value_bytes(S.BLK_F)}, S {ls.inner_value_bytes(S.BLK_S)}; "
          f"device memory of the handle after set-up {mem[bits]:.2f} GB", flush=True)

ops = {S.TIMEOP_INNER_SPMV + S.BLK_F: "inner SpMV F", S.TIMEOP_INNER_SPMV + S.BLK_S: "inner SpMV S"}
prof = {S.TIMEOP_INNER_SPMV + S.BLK_F: S.BLK_F, S.TIMEOP_INNER_SPMV + S.BLK_S: S.BLK_S}   # sampled in the solve as SpMV ops
samples = {(bits, op): [] for bits in hs for op in ops}
fmt = {}
for r in range(a.rounds):
    for bits in ((64, 32) if r % 2 == 0 else (32, 64)):
        for op in ops:
            ms, by = hs[bits].time_op(op, a.reps)
            samples[(bits, op)].append(ms)
            fmt[(bits, op)] = by
# inner iteration counts, and the format bytes nsk_profile_read reports for the SpMVs sampled inside the solve (with the
# fused J x every sampled F and S launch is an inner one: they must equal what time_op reported)
its = {}
for bits, ls in hs.items():
    for op in ops:
        ls.profile_begin(prof[op], 64)
    ls.setup_preconditioner(S.ASIMPLE, S.STATIONARY, 0.5)
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    ls.reset_stats()
    n_out, res, rc = ls.solve_resident(1, 0.0, a.steps)   # FGMRES
    st = ls.stats()
    for op in ops:
        sampled = ls.profile_read(prof[op])
        assert sampled[4] == fmt[(bits, op)], (bits, op, sampled[4], fmt[(bits, op)])
        print(f"fp{bits} {ops[op]} sampled in the solve: {sampled[0]:.4f} ms over {sampled[1]} launches", flush=True)
    ls.profile_end()
    outer = max(1, st["outer_iters"])
    its[bits] = dict(outer=st["outer_iters"], inner_u_per_outer=st["inner_u_its"] / outer,
                     inner_p_per_outer=st["inner_p_its"] / outer, solve_ms_per_outer=st["solve_ms"] / outer)

out = {"mesh": [nx, ny], "reps": a.reps, "rounds": a.rounds, "memory_GB": {str(b): mem[b] for b in mem}, "iterations": {}, "applies": {}}
for bits in hs:
    print(f"fp{bits}: {its[bits]['outer']} outer steps, inner u {its[bits]['inner_u_per_outer']:.2f} / p "
          f"{its[bits]['inner_p_per_outer']:.2f} per outer step, {its[bits]['solve_ms_per_outer']:.1f} ms per outer step")
    out["iterations"][str(bits)] = its[bits]
for op, nm in ops.items():
    for bits in hs:
        v = sorted(samples[(bits, op)])
        ms = v[len(v) // 2]
        gb = fmt[(bits, op)] / 1e9
        print(f"{nm} fp{bits}: median {ms:.4f} ms (rounds {', '.join(f'{x:.4f}' for x in samples[(bits, op)])}), "
              f"format {gb:.3f} GB, {gb / ms * 1e3:.0f} GB/s")
        out["applies"][f"{nm} fp{bits}"] = dict(ms=ms, rounds=samples[(bits, op)], format_GB=gb, GBps=gb / ms * 1e3)
    print(f"{nm}: fp32 / fp64 time {out['applies'][f'{nm} fp32']['ms'] / out['applies'][f'{nm} fp64']['ms']:.3f}")
print(json.dumps(out))
for ls in hs.values():
    ls.close()
