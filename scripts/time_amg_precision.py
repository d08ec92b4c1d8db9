#!/usr/bin/env python3
"""fp64 against fp32 storage of the velocity AMG's V-cycle operators (NSK_OPT_AMG_PRECISION) on one mesh.

Two handles in one process, one per precision, on the same hand-off (stationary blockTriangular): device time of one
V-cycle (nsk_time_op 57: bytes of the stored formats; op 20: the algorithmic CSR bytes), alternated between the handles
over several rounds; per level the rows and the entries of A, P and R with the bytes their values take at 8 and at 4
bytes; device memory taken by each handle once the hierarchy stands; and outer / inner iteration counts, V-cycles per
F-solve and time per outer step of a short FGMRES run from the bench's initial state.  Run with NSK_AMG_PRECISION unset
(it would override both handles); NSK_INNER_MATRIX_PRECISION / NSK_FACTOR_PRECISION unset too (both handles keep those
at 64).
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navier_stokes_solver_amd import problem as P, solver as S

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="1200,400")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=5, help="outer FGMRES iterations for the iteration counts")
a = ap.parse_args()
for v in ("NSK_AMG_PRECISION", "NSK_INNER_MATRIX_PRECISION", "NSK_FACTOR_PRECISION"):
    if os.environ.get(v):
        sys.exit(f"unset {v}: it overrides the options of both handles")
nx, ny = (int(v) for v in a.mesh.split(","))


def free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def level_entries(ls):
    """[(rows, nnz A, nnz P, nnz R)] of shard 0 (nsk_internal.h: nsk_debug_amg_level, size queries only)."""
    f = ls.L.nsk_debug_amg_level
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    lv = ls.amg_levels()
    out = []
    for l, (rows, nnz, _) in enumerate(lv):
        last = l == len(lv) - 1
        out.append((rows, nnz, 0 if last else f(ls.h, 0, l, 1, None, None, None, None), 0 if last else f(ls.h, 0, l, 2, None, None, None, None)))
    return out


t0 = time.time()
pr = P.generate(nx, ny, nu=1 / 90.0, mode=1, state=1)
print(f"{nx}x{ny}: n_u {pr.n_u}, n_p {pr.n_p}, nnz(F) {pr.F.nnz}, generated in {time.time() - t0:.1f} s", flush=True)
hs, mem = {}, {}
for bits in (64, 32):
    before = free_bytes()
    ls = S.LinearSolver()
    ls.set_option(S.OPT_TRI_ORDERING, 1)
    ls.set_option(S.OPT_AMG_PRECISION, bits)
    ls.set_problem(pr)
    ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY, 0.5)
    vb = ls.amg_value_bytes()      # (builds the hierarchy)
    mem[bits] = (before - free_bytes()) / 1e9
    hs[bits] = ls
    print(f"fp{bits}: AMG value bytes {vb}, inner value bytes F {ls.inner_value_bytes(S.BLK_F)}; device memory of the handle "
          f"with its hierarchy {mem[bits]:.2f} GB", flush=True)

lev = level_entries(hs[32])
own = 0
print("level  rows        nnz A        nnz P        nnz R    values at 8 B / 4 B (GB; level 0's A is F itself: 4 B is its 2x2 copy)")
for l, (rows, za, zp, zr) in enumerate(lev):
    tot = za + zp + zr
    own += (0 if l == 0 else za) + zp + zr
    print(f"{l:5d} {rows:9d} {za:12d} {zp:12d} {zr:12d}    {8 * tot / 1e9:.3f} / {4 * tot / 1e9:.3f}")
print(f"the hierarchy's own operators (all but level 0's A): {own} values: {8 * own / 1e9:.3f} GB in double, {4 * own / 1e9:.3f} GB "
      f"more as fp32 copies beside them, {4 * own / 1e9:.3f} GB in all if the double values were released", flush=True)

ops = {57: "V-cycle (format bytes)", 20: "V-cycle (algorithmic bytes)"}
samples = {(bits, op): [] for bits in hs for op in ops}
fmt = {}
for r in range(a.rounds):
    for bits in ((64, 32) if r % 2 == 0 else (32, 64)):
        for op in ops:
            ms, by = hs[bits].time_op(op, a.reps)
            samples[(bits, op)].append(ms)
            fmt[(bits, op)] = by

its = {}
for bits, ls in hs.items():
    ls.setup_preconditioner(S.BLOCK_TRIANGULAR, S.STATIONARY, 0.5)
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    ls.amg_value_bytes()           # (the hierarchy again, outside the timed solve)
    ls.reset_stats()
    n_out, res, rc = ls.solve_resident(1, 0.0, a.steps)   # FGMRES
    st = ls.stats()
    outer = max(1, st["outer_iters"])
    its[bits] = dict(outer=st["outer_iters"], v_cycles_per_f_solve=st["inner_u_its"] / outer,
                     inner_p_per_outer=st["inner_p_its"] / outer, solve_ms_per_outer=st["solve_ms"] / outer, residual=res)

out = {"mesh": [nx, ny], "reps": a.reps, "rounds": a.rounds, "memory_GB": {str(b): mem[b] for b in mem},
       "levels": lev, "iterations": {}, "applies": {}}
for bits in hs:
    print(f"fp{bits}: {its[bits]['outer']} outer steps, {its[bits]['v_cycles_per_f_solve']:.2f} V-cycles per F-solve, inner p "
          f"{its[bits]['inner_p_per_outer']:.2f} per outer step, {its[bits]['solve_ms_per_outer']:.1f} ms per outer step, "
          f"residual {its[bits]['residual']:.6e}")
    out["iterations"][str(bits)] = its[bits]
for op, nm in ops.items():
    for bits in hs:
        v = sorted(samples[(bits, op)])
        ms = v[len(v) // 2]
        gb = fmt[(bits, op)] / 1e9
        print(f"{nm} fp{bits}: median {ms:.4f} ms (rounds {', '.join(f'{x:.4f}' for x in samples[(bits, op)])}), "
              f"{gb:.3f} GB, {gb / ms * 1e3:.0f} GB/s")
        out["applies"][f"{nm} fp{bits}"] = dict(ms=ms, rounds=samples[(bits, op)], GB=gb, GBps=gb / ms * 1e3)
    print(f"{nm}: fp32 / fp64 time {out['applies'][f'{nm} fp32']['ms'] / out['applies'][f'{nm} fp64']['ms']:.3f}")
print(json.dumps(out))
for ls in hs.values():
    ls.close()
