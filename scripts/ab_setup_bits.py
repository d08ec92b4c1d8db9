#!/usr/bin/env python3
"""Does another build of the library set up the same preconditioners?  One line per set-up, to be compared with `diff`.

The library comes from NSK_HIP_LIBRARY (solver.library_path).  ONE handle on the 60x20 mesh runs a fixed sequence of
set-ups — every preconditioner, the opt-in switches of the set-up on and back off — and after each one K outer FGMRES
iterations from the same initial guess (tolerance 0, as bench.py limits its steps).  A line holds the sha256 of the solution
bytes and of the residual history, the counters of those K steps and what the getters report of the set-up.  Then one child
process per environment override, that variable alone set to its non-default value, runs the one set-up it acts on and
prints the same line.  Children run one after the other, after the parent has closed its handle.

  NSK_HIP_LIBRARY=/path/to/other/libnsk_hip.so python3 scripts/ab_setup_bits.py > other.log
  python3 scripts/ab_setup_bits.py > this.log && diff other.log this.log

Run it with none of the eight variables set.  A stage whose line differs between two runs of ONE library is not
deterministic and says nothing about two.
"""
import argparse
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from navier_stokes_solver_amd import problem as P, solver as S  # noqa: E402

K = 4
NU = 0.01
DEFAULTS = {S.OPT_FACTOR_PRECISION: 64, S.OPT_INNER_MATRIX_PRECISION: 64, S.OPT_INNER_BASIS_PRECISION: 64,
            S.OPT_AMG_PRECISION: 64, S.OPT_INNER_MATRIX_FREE_F: 0, S.OPT_SCHUR_AMG: 0, S.OPT_ASIMPLE_VELOCITY_AMG: 0}
# (label, type, variant, options on top of the defaults, needs nsk_assemble first)
STAGES = [
    ("aSIMPLE/stationary defaults", 2, 0, {}, False),
    ("aSIMPLE/stationary SCHUR_AMG", 2, 0, {S.OPT_SCHUR_AMG: 1}, False),
    ("aSIMPLE/stationary SCHUR_AMG+ASIMPLE_VELOCITY_AMG+AMG_PRECISION=32", 2, 0,
     {S.OPT_SCHUR_AMG: 1, S.OPT_ASIMPLE_VELOCITY_AMG: 1, S.OPT_AMG_PRECISION: 32}, False),
    ("aSIMPLE/stationary defaults again (ILU(F) comes back)", 2, 0, {}, False),
    ("blockTriangular/stationary defaults", 1, 0, {}, False),
    ("blockTriangular/stationary AMG_PRECISION=32", 1, 0, {S.OPT_AMG_PRECISION: 32}, False),
    ("blockTriangular/unsteady defaults", 1, 1, {}, False),
    ("blockDiagonal/stationary defaults", 0, 0, {}, False),
    ("blockDiagonal/unsteady defaults", 0, 1, {}, False),
    ("aSIMPLE/unsteady defaults", 2, 1, {}, False),
    ("aSIMPLE/stationary FACTOR+INNER_MATRIX+INNER_BASIS_PRECISION=32", 2, 0,
     {S.OPT_FACTOR_PRECISION: 32, S.OPT_INNER_MATRIX_PRECISION: 32, S.OPT_INNER_BASIS_PRECISION: 32}, False),
    ("blockTriangular/stationary INNER_MATRIX_FREE_F after nsk_assemble", 1, 0, {S.OPT_INNER_MATRIX_FREE_F: 1}, True),
]
# variable -> (its non-default value, the stage it acts on)
CHILDREN = {
    "NSK_FACTOR_PRECISION": ("32", ("aSIMPLE/stationary", 2, 0, {}, False)),
    "NSK_INNER_MATRIX_PRECISION": ("32", ("aSIMPLE/stationary", 2, 0, {}, False)),
    "NSK_INNER_BASIS_PRECISION": ("32", ("aSIMPLE/stationary", 2, 0, {}, False)),
    "NSK_AMG_PRECISION": ("32", ("blockTriangular/stationary", 1, 0, {}, False)),
    "NSK_INNER_MATRIX_FREE_F": ("1", ("blockTriangular/stationary after nsk_assemble", 1, 0, {}, True)),
    "NSK_SCHUR_AMG": ("1", ("aSIMPLE/stationary", 2, 0, {}, False)),
    "NSK_ASIMPLE_VELOCITY_AMG": ("1", ("aSIMPLE/stationary", 2, 0, {}, False)),
    "NSK_AMG_FUSED_CHEBY": ("0", ("aSIMPLE/stationary ASIMPLE_VELOCITY_AMG", 2, 0, {S.OPT_ASIMPLE_VELOCITY_AMG: 1}, False)),
}


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def handle():
    pr = P.generate(60, 20, nu=NU, mode=1, state=1)
    ls = S.LinearSolver()
    ls.set_problem(pr)
    return pr, ls


def run_stage(ls, pr, stage):
    label, type_, variant, options, assembled = stage
    if assembled:   # block (0,0) from the device assembly: what the matrix-free product needs (and keeps)
        ls.set_assembly(pr)
        ls.state_set(pr.x0_u * 0.0, pr.x0_p * 0.0)
        ls.assemble(NU, 0.0, 1.0)
    for opt, value in {**DEFAULTS, **options}.items():
        ls.set_option(opt, value)
    ls.setup_preconditioner(type_, variant, 0.5)
    ls.reset_stats()
    ls.upload_system(pr.rhs_u, pr.rhs_p, pr.x0_u, pr.x0_p)
    its, _, rc = ls.solve_resident(S.FGMRES, 0.0, K)
    xu, xp = ls.download_solution()
    st = ls.stats()
    fields = [("x", sha(xu)[:32] + sha(xp)[:32]), ("history", sha(ls.history())[:32]), ("rc", rc), ("outer", its),
              ("inner_u", st["inner_u_its"]), ("inner_p", st["inner_p_its"]), ("prec_applies", st["prec_applies"]),
              ("tri_bytes", f"{ls.tri_value_bytes(S.TRI_VELOCITY)}/{ls.tri_value_bytes(S.TRI_PRESSURE)}"),
              ("inner_bytes_F_Mp_S", "/".join(str(ls.inner_value_bytes(b)) for b in (S.BLK_F, S.BLK_MP, S.BLK_S))),
              ("basis_bytes", ls.inner_basis_bytes()), ("amg_bytes", ls.amg_value_bytes()),
              ("amg_levels", len(ls.amg_levels())), ("schur_amg_levels", len(ls.schur_amg_info())),
              ("matrix_free", ls.inner_matrix_free())]
    return f"{label}: " + " ".join(f"{k}={v}" for k, v in fields)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=sorted(CHILDREN), help="(internal) run the one stage of that variable and print its line")
    a = ap.parse_args()
    if a.child:
        pr, ls = handle()
        print(f"{a.child}={CHILDREN[a.child][0]} " + run_stage(ls, pr, CHILDREN[a.child][1]), flush=True)
        ls.close()
        return
    left = [n for n in CHILDREN if os.environ.get(n) is not None]
    if left:
        sys.exit("unset " + ", ".join(left) + ": the environment overrides the options of every handle")
    pr, ls = handle()
    for stage in STAGES:
        print(run_stage(ls, pr, stage), flush=True)
    ls.close()
    for name, (value, _) in CHILDREN.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env={**os.environ, name: value},
                           stdout=subprocess.PIPE, text=True, timeout=120)
        if r.returncode != 0:
            sys.exit(f"the child of {name} ended with status {r.returncode}")   # (nothing more is started on the device)
        print(r.stdout, end="", flush=True)


if __name__ == "__main__":
    main()
