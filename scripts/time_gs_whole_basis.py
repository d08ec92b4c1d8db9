#!/usr/bin/env python3
"""Device time of the fused Gram-Schmidt sweeps over a whole basis of 30 velocity-sized vectors and of the cycle-end
update of 29 terms (nsk_time_op 35 / 36 / 37), for NSK_IOPT_GS_ONE_LAUNCH = 0 (chunks of eight; one vec_axpy per term),
2 (at most 16 vectors per launch) and 1 (one launch).  usage: time_gs_whole_basis.py [NX,NY] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navier_stokes_solver_amd import problem as P, solver as S
nx, ny = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1200,400").split(","))
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
pr = P.generate(nx, ny, nu=1 / 90.0)
ls = S.LinearSolver()
ls.set_problem(pr)
for rnd in range(2):   # twice: the second round shows what the first one's order did
    for mode, what in ((0, "chunks of 8"), (2, "16 per launch"), (1, "one launch")):
        ls.set_option(S.IOPT_GS_ONE_LAUNCH, mode)
        for op, nm in ((35, "coefficients m=30"), (36, "update+norm m=30"), (37, "x += sum, 29 terms")):
            ms, by = ls.time_op(op, reps)
            print(f"round {rnd} {what:14s} {nm:20s} {1e3 * ms:8.1f} us  {by / 1e6:8.1f} MB  {by / 1e9 / (ms / 1e3) / 1e3:6.2f} TB/s", flush=True)
ls.close()
