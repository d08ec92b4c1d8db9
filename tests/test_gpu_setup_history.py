"""A handle with a history sets up like a fresh one.

The property: after nsk_setup_preconditioner a handle behaves bit for bit like a fresh handle that was given the same final
block values, the same final options and that one set-up — whatever the first handle did before.  H::setup keeps analyses,
the factor of M_p, the Schur pattern, row runs, blocked and fp32 copies, 16-bit offsets, two hierarchies and the state of
stationary aSIMPLE between set-ups; a copy that is stale does not fail a solve, it gives a slightly different
preconditioner.  So nothing here looks at residuals: fingerprints (tests/setup_fingerprint.py) are compared with
np.array_equal, and the relations of group 5 are exact in floating point (scaling by a power of two).

Groups: 0 control (two fresh handles agree: without it an inequality says nothing), 1 a closed walk over all 36 transitions
between the six preconditioners, 2 options on and back off, 3 every writer of a block followed by a set-up, 4 writers
without a set-up (the products, not the preconditioner), 5 exact relations, 6 two ranks.  Everything at 16 x 10, under two
option bases: D the defaults (tiny factors: the walker), K multicolour ordering with NSK_IOPT_TINY_BYTES = 0 and
NSK_OPT_TRI_SYNC_FREE = 2 (stream and single-launch kernels, 16-bit offsets, blocked velocity factor, colour-ordered
working vector).  Options change only directly before a set-up.
"""
import contextlib
import dataclasses
import hashlib
import importlib.util
import os
import threading
import time

import numpy as np
import pytest

from navier_stokes_solver_amd import partition as PT
from navier_stokes_solver_amd import problem as P
from navier_stokes_solver_amd import solver as S
from tests import setup_fingerprint as FP
from tests import spmv_reference as M
from tests.util import CASES, problem

pytestmark = pytest.mark.gpu

U = M.U
PAIRS = [(t, v) for t in (S.BLOCK_DIAGONAL, S.BLOCK_TRIANGULAR, S.ASIMPLE) for v in (S.STATIONARY, S.UNSTEADY)]
PAIR_IDS = {(0, 0): "bD-stat", (0, 1): "bD-unst", (1, 0): "bT-stat", (1, 1): "bT-unst", (2, 0): "aS-stat", (2, 1): "aS-unst"}
BASES = {"D": {}, "K": {S.OPT_TRI_ORDERING: 1, S.IOPT_TINY_BYTES: 0, S.OPT_TRI_SYNC_FREE: 2}}
BLOCK_NAME = {S.BLK_F: "F", S.BLK_BT: "Bt", S.BLK_B: "B", S.BLK_MP: "Mp"}
pair_param = pytest.mark.parametrize("target", PAIRS, ids=[PAIR_IDS[p] for p in PAIRS])
base_param = pytest.mark.parametrize("base", sorted(BASES))


def _children():
    """CHILDREN of scripts/ab_setup_bits.py: the set-up's environment variables (read once per process)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "ab_setup_bits.py")
    spec = importlib.util.spec_from_file_location("ab_setup_bits", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CHILDREN


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    print(f"\nmodule wall time {time.time() - t0:.1f} s, {len(_FRESH)} fresh fingerprints (each built twice)")


def case_of(target):
    """ns16; the unsteady variants on the matrix with the mass term"""
    return problem("ns16" if target[1] == S.STATIONARY else "unsteady16")


# ------------------------------------------------------------------ fresh fingerprints, cached; the control
_FRESH = {}


def _asm_key(assemble):
    if assemble is None:
        return None
    h = hashlib.sha256(np.concatenate(assemble["state"]).tobytes()).hexdigest()
    return (h, assemble["nu"], assemble["inv_dt"], bool(assemble.get("timed")))


def fresh_fp(pr, options, target, assemble=None):
    """The fingerprint of a fresh handle, cached per (values, options, target).  The control: it is built twice, and the two
    must agree — a stage that is not deterministic says nothing about histories."""
    key = (FP.values_key(pr), tuple(sorted(options.items())), target, _asm_key(assemble))
    if key not in _FRESH:
        a = FP.fresh(pr, options, *target, assemble=assemble)
        b = FP.fresh(pr, options, *target, assemble=assemble)
        FP.assert_same(a, b, f"control: two fresh handles, {PAIR_IDS[target]}, options {options}")
        _FRESH[key] = a
    return _FRESH[key]


@contextlib.contextmanager
def handle(pr, options):
    ls = S.LinearSolver()
    try:
        FP.set_options(ls, options)
        ls.set_problem(pr)
        yield ls
    finally:
        ls.close()


def setup_fp(ls, pr, target):
    ls.setup_preconditioner(*target, FP.ALPHA)
    return FP.fingerprint(ls, pr)


# ------------------------------------------------------------------ 0. control
@base_param
@pair_param
def test_control_two_fresh_handles_agree(target, base):
    fp = fresh_fp(case_of(target), BASES[base], target)
    names = [k for k, _ in fp]
    assert "solution u" in names and "precond_vmult u" in names and len(dict(fp)["history"]) == FP.OUTER_STEPS + 1


# ------------------------------------------------------------------ 1. walk over the preconditioners
def euler_circuit(n):
    """A closed walk over every edge of the complete directed graph on n vertices, self-loops included (Hierholzer)."""
    out = {v: list(range(n)) for v in range(n)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop(0))
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


@base_param
def test_walk_over_all_transitions_between_the_preconditioners(base):
    """37 set-ups on one handle: every (type, variant) after every other and after itself.  Self-loops take the "held"
    paths; the others ILU <-> SGS on one analysis, mass_ordering changes, S's factor coming and going.  A second round
    must leave the pools as the first did."""
    walk = euler_circuit(len(PAIRS))
    assert len(walk) == 37 and walk[0] == walk[-1]
    assert len({(a, b) for a, b in zip(walk, walk[1:])}) == 36
    pr = problem("unsteady16")
    opts = BASES[base]
    with handle(pr, opts) as ls:
        counts = []
        for rnd in (1, 2):
            for k, v in enumerate(walk):
                want = fresh_fp(pr, opts, PAIRS[v])
                got = setup_fp(ls, pr, PAIRS[v])
                prev = PAIR_IDS[PAIRS[walk[k - 1]]] if k else ("nothing" if rnd == 1 else PAIR_IDS[PAIRS[walk[-1]]])
                FP.assert_same(got, want, f"round {rnd}, set-up {k}: {PAIR_IDS[PAIRS[v]]} after {prev}")
            counts.append(ls.pool_counts())
        assert counts[0] == counts[1], f"a cycle of set-ups grows the pools: {counts}"


# ------------------------------------------------------------------ 2. options on and back off
def run_states(pr, base, target, const, states, assemble=None):
    """One handle through `states` (option dicts, set directly before each set-up, cumulative); after every set-up the
    fingerprint equals the one of a fresh handle with the options as they then stand."""
    opts = {**BASES[base], **const}
    cur = dict(opts)
    with handle(pr, opts) as ls:
        if assemble is not None:
            FP.run_assembly(ls, pr, assemble)
        for k, st in enumerate(states):
            cur.update(st)
            want = fresh_fp(pr, dict(cur), target, assemble)
            FP.set_options(ls, st)
            got = setup_fp(ls, pr, target)
            FP.assert_same(got, want, f"set-up {k} of {[list(s.items()) for s in states]} on {PAIR_IDS[target]}")


AS, BT_ = (S.ASIMPLE, S.STATIONARY), (S.BLOCK_TRIANGULAR, S.STATIONARY)
# name: (environment variable, target, options held throughout, on, off, after an assembly)
TOGGLES = {
    "factor_precision": ("NSK_FACTOR_PRECISION", AS, {}, {S.OPT_FACTOR_PRECISION: 32}, {S.OPT_FACTOR_PRECISION: 64}, False),
    "inner_matrix_precision": ("NSK_INNER_MATRIX_PRECISION", AS, {}, {S.OPT_INNER_MATRIX_PRECISION: 32},
                               {S.OPT_INNER_MATRIX_PRECISION: 64}, False),
    "inner_basis_precision": ("NSK_INNER_BASIS_PRECISION", AS, {}, {S.OPT_INNER_BASIS_PRECISION: 32},
                              {S.OPT_INNER_BASIS_PRECISION: 64}, False),
    "amg_precision": ("NSK_AMG_PRECISION", BT_, {S.OPT_VELOCITY_AMG: 1}, {S.OPT_AMG_PRECISION: 32}, {S.OPT_AMG_PRECISION: 64}, False),
    "schur_amg": ("NSK_SCHUR_AMG", AS, {}, {S.OPT_SCHUR_AMG: 1}, {S.OPT_SCHUR_AMG: 0}, False),
    "asimple_velocity_amg": ("NSK_ASIMPLE_VELOCITY_AMG", AS, {}, {S.OPT_ASIMPLE_VELOCITY_AMG: 1}, {S.OPT_ASIMPLE_VELOCITY_AMG: 0}, False),
    "amg_fused_cheby": ("NSK_AMG_FUSED_CHEBY", AS, {S.OPT_ASIMPLE_VELOCITY_AMG: 1}, {S.IOPT_AMG_FUSED_CHEBY: 0},
                        {S.IOPT_AMG_FUSED_CHEBY: -1}, False),
    "matrix_free_f": ("NSK_INNER_MATRIX_FREE_F", BT_, {}, {S.OPT_INNER_MATRIX_FREE_F: 1}, {S.OPT_INNER_MATRIX_FREE_F: 0}, True),
}


def _skip_if_overridden(*variables):
    children = _children()
    for v in variables:
        assert v in children, f"{v} is not among the set-up's environment variables of scripts/ab_setup_bits.py"
        if os.environ.get(v) is not None:
            pytest.skip(f"{v} is set: it overrides the option of every handle of this process, so the option cannot be toggled")


def other_state(pr):
    """Another state and viscosity than the hand-off's to assemble F about"""
    return dict(state=(0.3 * FP.seeded(pr.n_u, 7), FP.seeded(pr.n_p, 8)), nu=1.0 / 50.0, inv_dt=pr.params["inv_dt"])


@base_param
@pytest.mark.parametrize("name", sorted(TOGGLES))
def test_option_on_off_on(name, base):
    var, target, const, on, off, assembled = TOGGLES[name]
    _skip_if_overridden(var)
    pr = case_of(target)
    run_states(pr, base, target, const, [on, off, on], other_state(pr) if assembled else None)


IM32, IM64 = {S.OPT_INNER_MATRIX_PRECISION: 32}, {S.OPT_INNER_MATRIX_PRECISION: 64}
AMG32, AMG64 = {S.OPT_AMG_PRECISION: 32}, {S.OPT_AMG_PRECISION: 64}
# the fp32 copies of F (of S) serve the inner products and the V-cycle's level 0: one goes, the other stays
SHARED = {
    "F, blockTriangular, inner matrix off": (BT_, {S.OPT_VELOCITY_AMG: 1}, [{**IM32, **AMG32}, IM64, IM32]),
    "F, blockTriangular, AMG precision off": (BT_, {S.OPT_VELOCITY_AMG: 1}, [{**IM32, **AMG32}, AMG64, AMG32]),
    "F, aSIMPLE, inner matrix off": (AS, {S.OPT_ASIMPLE_VELOCITY_AMG: 1}, [{**IM32, **AMG32}, IM64, IM32]),
    "F, aSIMPLE, AMG precision off": (AS, {S.OPT_ASIMPLE_VELOCITY_AMG: 1}, [{**IM32, **AMG32}, AMG64, AMG32]),
    "S, inner matrix off": (AS, {S.OPT_SCHUR_AMG: 1}, [{**IM32, **AMG32}, IM64, IM32]),
    "S, AMG precision off": (AS, {S.OPT_SCHUR_AMG: 1}, [{**IM32, **AMG32}, AMG64, AMG32]),
}


@base_param
@pytest.mark.parametrize("name", sorted(SHARED))
def test_options_that_share_storage(name, base):
    _skip_if_overridden("NSK_INNER_MATRIX_PRECISION", "NSK_AMG_PRECISION", "NSK_SCHUR_AMG", "NSK_ASIMPLE_VELOCITY_AMG")
    target, const, states = SHARED[name]
    run_states(case_of(target), base, target, const, states)


@base_param
@pytest.mark.parametrize("target", [AS, (S.BLOCK_DIAGONAL, S.STATIONARY), (S.ASIMPLE, S.UNSTEADY)],
                         ids=["aS-stat", "bD-stat", "aS-unst"])
def test_factor_precision_with_the_sync_free_mode(target, base):
    """The fp32 halves of the factors are reallocated by numeric(); the single-launch kernels keep more of them"""
    _skip_if_overridden("NSK_FACTOR_PRECISION")
    f32, f64 = {S.OPT_FACTOR_PRECISION: 32}, {S.OPT_FACTOR_PRECISION: 64}
    sf2, sf0 = {S.OPT_TRI_SYNC_FREE: 2}, {S.OPT_TRI_SYNC_FREE: 0}
    run_states(case_of(target), base, target, {}, [{**f32, **sf2}, sf0, sf2, f64, sf0, f32])


# value -> other value -> back
ANALYSIS = {
    "tri_ordering": (S.OPT_TRI_ORDERING, [0, 1, 0]),
    "subdomains": (S.OPT_SUBDOMAINS, [1, 3, 1]),
    "line_groups": (S.OPT_TRI_LINE_GROUPS, [0, 1, 0]),
    "sync_free": (S.OPT_TRI_SYNC_FREE, [0, 1, 2, 0, 2, 1, 0]),
    "x_layout": (S.IOPT_TRI_X_LAYOUT, [1, 0, 1]),
    "bsr_velocity": (S.OPT_BSR_VELOCITY, [1, 0, 1]),
    "stream_kernels": (S.OPT_STREAM_KERNELS, [1, 0, 1]),
    "index16": (S.IOPT_INDEX16, [1, 0, 1]),
    "host_analysis": (S.IOPT_HOST_ANALYSIS, [0, 1, 0]),
    "mass_ordering": (S.OPT_MASS_ORDERING, [-1, 1, 0, -1]),
}


@base_param
@pair_param
@pytest.mark.parametrize("name", sorted(ANALYSIS))
def test_analysis_option_there_and_back(name, target, base):
    opt, values = ANALYSIS[name]
    run_states(case_of(target), base, target, {}, [{opt: v} for v in values])


# ------------------------------------------------------------------ 3. writers, then a set-up
def block_of(pr, blk):
    return {S.BLK_F: pr.F, S.BLK_BT: pr.Bt, S.BLK_B: pr.B, S.BLK_MP: pr.Mp, S.BLK_BT_GHOST: pr.Bt_ghost}[blk]


def new_values(m, seed):
    """val * (1 + 0.25 u), u uniform in [-1, 1] and drawn once per row.  (Drawn per entry the 25 % make F indefinite, and
    the inner FGMRES on F under the V-cycle of stationary blockTriangular, which may take 10^7 iterations, does not end.
    One factor per row keeps the signs and the row-relative sizes every preconditioner here is built on, and still
    changes every stored value, each row by another factor.)"""
    return m.val * (1.0 + 0.25 * np.repeat(FP.seeded(m.rows, seed), np.diff(m.rowptr.astype(np.int64))))


def write(ls, pr, blk, writer):
    """One writer of block values; returns the assembly a fresh handle has to repeat (None: it is handed the values)"""
    m = block_of(pr, blk)
    if writer == "update_values":
        ls.update_values(blk, new_values(m, 40 + blk))
    elif writer == "scale_values":
        ls.scale_values(blk, 0.7)
    elif writer == "set_block":
        ls.set_block(blk, P.CsrBlock(rows=m.rows, cols=m.cols, rowptr=m.rowptr, col=m.col, val=new_values(m, 40 + blk)))
    else:
        assert blk == S.BLK_F and writer in ("assemble", "time_assemble")
        asm = dict(other_state(pr), timed=writer == "time_assemble")
        FP.run_assembly(ls, pr, asm)
        return asm
    return None


WRITES = [(S.BLK_F, w, t) for w in ("update_values", "scale_values", "set_block", "assemble", "time_assemble") for t in PAIRS] + \
         [(b, w, t) for b in (S.BLK_B, S.BLK_BT) for w in ("update_values", "scale_values", "set_block")
          for t in PAIRS if t[0] == S.ASIMPLE] + \
         [(S.BLK_MP, w, t) for w in ("update_values", "scale_values", "set_block") for t in PAIRS if t[0] != S.ASIMPLE]


@base_param
@pytest.mark.parametrize("blk,writer,target", WRITES, ids=[f"{BLOCK_NAME[b]}-{w}-{PAIR_IDS[t]}" for b, w, t in WRITES])
def test_writer_then_setup(blk, writer, target, base):
    """Set up, fingerprint (forces every lazy build), write, set up again: as a fresh handle on the final values.  B and Bt:
    S must follow; M_p: the kept factor must not survive."""
    pr = case_of(target)
    opts = BASES[base]
    with handle(pr, opts) as ls:
        FP.assert_same(setup_fp(ls, pr, target), fresh_fp(pr, opts, target), "before the write")
        asm = write(ls, pr, blk, writer)
        final = pr if asm is not None else FP.problem_from_handle(ls, pr)
        assert asm is not None or not np.array_equal(block_of(final, blk).val, block_of(pr, blk).val)
        want = fresh_fp(final, opts, target, asm)
        got = setup_fp(ls, pr, target)
        FP.assert_same(got, want, f"{writer}({BLOCK_NAME[blk]}), then {PAIR_IDS[target]}")
        assert FP.first_difference(want, fresh_fp(pr, opts, target)) is not None, "the write changes nothing the fingerprint sees"


@base_param
@pytest.mark.parametrize("writer", ["update_values", "scale_values", "set_block"])
def test_a_writer_of_f_ends_the_matrix_free_product(writer, base):
    """NSK_OPT_INNER_MATRIX_FREE_F multiplies by the F of the last nsk_assemble; every other writer of F ends that, and the
    next set-up multiplies by the block as a fresh handle that was handed the values does"""
    _skip_if_overridden("NSK_INNER_MATRIX_FREE_F")
    pr = problem("ns16")
    opts = {**BASES[base], S.OPT_INNER_MATRIX_FREE_F: 1}
    with handle(pr, opts) as ls:
        FP.run_assembly(ls, pr, other_state(pr))
        assert dict(setup_fp(ls, pr, BT_))["inner_matrix_free"] == 1
        write(ls, pr, S.BLK_F, writer)
        final = FP.problem_from_handle(ls, pr)
        want = fresh_fp(final, opts, BT_)
        assert dict(want)["inner_matrix_free"] == 0
        FP.assert_same(setup_fp(ls, pr, BT_), want, f"assemble, {writer}(F), then blockTriangular")


@base_param
@pair_param
def test_the_device_backends_sequence_between_two_setups(target, base):
    """newton.DeviceBackend at a continuation level: pressure_mass rescaled by nu_0 / nu_1, block (1,0) negated"""
    pr = case_of(target)
    opts = BASES[base]
    with handle(pr, opts) as ls:
        setup_fp(ls, pr, target)
        ls.scale_values(S.BLK_MP, (1.0 / 90.0) / (1.0 / 110.0))
        ls.scale_values(S.BLK_B, -1.0)
        final = FP.problem_from_handle(ls, pr)
        assert np.array_equal(final.B.val, -pr.B.val)
        FP.assert_same(setup_fp(ls, pr, target), fresh_fp(final, opts, target), f"scaled M_p and -B, then {PAIR_IDS[target]}")


@base_param
@pair_param
def test_setup_twice_with_nothing_written(target, base):
    """The factor of M_p and the analyses are kept: the bits are the same"""
    pr = case_of(target)
    opts = BASES[base]
    want = fresh_fp(pr, opts, target)
    with handle(pr, opts) as ls:
        FP.assert_same(setup_fp(ls, pr, target), want, "first set-up")
        FP.assert_same(setup_fp(ls, pr, target), want, "second set-up")
        ls.setup_preconditioner(*target, FP.ALPHA)       # and a set-up nothing was asked of in between
        FP.assert_same(setup_fp(ls, pr, target), want, "fourth set-up")


def renumbered(pr):
    """The problem with its velocity nodes in reverse order: F2 = P F P^T, Bt2 = P Bt, B2 = B P^T — same sizes, other patterns"""
    import scipy.sparse as sp
    n = pr.n_u
    i = np.arange(n)
    new = 2 * (n // 2 - 1 - i // 2) + i % 2          # new id of old DoF i: components kept together

    def csr(m, rows, cols):                          # (through COO: a sparse product would drop the stored zeros)
        c = m.to_scipy().tocoo()
        r = sp.csr_matrix((c.data, (rows(c.row), cols(c.col))), shape=c.shape)
        r.sort_indices()
        assert r.nnz == m.nnz
        return P.CsrBlock(rows=m.rows, cols=m.cols, rowptr=r.indptr.astype(np.int32), col=r.indices.astype(np.int32), val=r.data)

    same = lambda a: a  # noqa: E731
    perm = lambda a: new[a]  # noqa: E731

    def vec(v):
        out = np.empty_like(v)
        out[new] = v
        return out

    return dataclasses.replace(pr, F=csr(pr.F, perm, perm), Bt=csr(pr.Bt, perm, same), B=csr(pr.B, same, perm),
                               rhs_u=vec(pr.rhs_u), x0_u=vec(pr.x0_u), support_u=vec(pr.support_u), dirichlet_u=vec(pr.dirichlet_u))


@base_param
def test_a_second_hand_off_with_another_pattern(base):
    pr = problem("ns16")
    pr2 = renumbered(pr)
    assert not np.array_equal(pr2.F.col, pr.F.col) and not np.array_equal(pr2.Bt.rowptr, pr.Bt.rowptr)
    opts = BASES[base]
    bd = (S.BLOCK_DIAGONAL, S.STATIONARY)
    with handle(pr, opts) as ls:
        setup_fp(ls, pr, AS)
        setup_fp(ls, pr, bd)
        for space, xy in ((S.SPACE_U, pr2.support_u), (S.SPACE_P, pr2.support_p)):   # (the partition stays: same sizes)
            ls.set_support_points(space, xy)
        for blk in (S.BLK_F, S.BLK_BT, S.BLK_B, S.BLK_MP):
            ls.set_block(blk, block_of(pr2, blk))
        FP.assert_same(setup_fp(ls, pr2, AS), fresh_fp(pr2, opts, AS), "aSIMPLE on the second pattern")
        FP.assert_same(setup_fp(ls, pr2, bd), fresh_fp(pr2, opts, bd), "blockDiagonal on the second pattern")


# ------------------------------------------------------------------ 4. writers without a set-up
COMBOS = [(f, b, s) for f in (0, 1) for b in (0, 1) for s in (0, 1)]


def products(ls, pr, blk):
    """The products that read the written block: nsk_spmv, nsk_jacobian_vmult under every combination of its three options,
    the inner products of F and M_p.  (The three options are put back to 1: no set-up follows.)"""
    m = block_of(pr, blk)
    n_own = pr.n_u if blk in (S.BLK_F, S.BLK_B) else pr.n_p
    assert m.cols == n_own
    out = [("spmv", ls.spmv(blk, FP.seeded(n_own, 800)))]
    xu, xp = FP.seeded(pr.n_u, 801), FP.seeded(pr.n_p, 802)
    for f, b, s in COMBOS:
        FP.set_options(ls, {S.OPT_FUSE_BLOCK_ROW: f, S.OPT_BSR_VELOCITY: b, S.OPT_STREAM_KERNELS: s})
        out.append((f"jacobian_vmult fuse {f} bsr {b} stream {s}", np.concatenate(ls.jacobian_vmult(xu, xp))))
    FP.set_options(ls, {S.OPT_FUSE_BLOCK_ROW: 1, S.OPT_BSR_VELOCITY: 1, S.OPT_STREAM_KERNELS: 1})
    out.append(("inner_spmv(F)", ls.inner_spmv(S.BLK_F, xu)))
    out.append(("inner_spmv(M_p)", ls.inner_spmv(S.BLK_MP, xp)))
    return out


_SUMS = {}


def row_sums(m, x, fp32=False):
    """Exact row sums (tests/spmv_reference.py) of a block of a LocalProblem on one rank, cached per values"""
    key = (hashlib.sha256(m.val.tobytes() + x.tobytes()).hexdigest(), fp32)
    if key not in _SUMS:
        _SUMS[key] = M.exact_row_sums(M.Csr(m.rows, m.cols, m.rowptr, m.col, m.val), x, np.zeros(0), fp32=fp32)
    return _SUMS[key]


def most_roundings(m, Cc):
    """The largest count of tests/spmv_reference.roundings over the kernel forms a block with Cc columns per node can take
    (csr_vector at the block's lanes per row, stream, blocked; the blocked forms with L // Cc blocks per row, which is what
    Csr::build_blocked finds on these node-structured blocks): the bound of whichever form the rule picked holds under it.
    So this bound is looser than the one of the form the dispatch takes — it stays at rounding level and says that the
    product is one of the NEW values.  What catches a single stale value is the bit-equality with the fresh handle."""
    A = M.Csr(m.rows, m.cols, m.rowptr, m.col, m.val)
    L = A.row_len
    d = np.maximum(M.roundings("csrv", L, lpr=M.pick_lpr(A)), M.roundings("stream", L))
    return np.maximum(d, M.roundings(f"blk_c{Cc}", L // Cc))


def check_bounds(got, final, blk, f32):
    """f32: the names of the inner products that read fp32 copies"""
    # every product against the exact row sums of the NEW values, within the row-wise bound of the SpMV kernel tests
    got = dict(got)
    cc = {S.BLK_F: 2, S.BLK_BT: 1, S.BLK_B: 2, S.BLK_MP: 1}
    n_own = final.n_u if blk in (S.BLK_F, S.BLK_B) else final.n_p
    m = block_of(final, blk)
    s, a = row_sums(m, FP.seeded(n_own, 800))
    M_within(got["spmv"], s, M.gamma(most_roundings(m, cc[blk])) * a + U * np.abs(s), f"spmv({BLOCK_NAME[blk]})")
    xu, xp = FP.seeded(final.n_u, 801), FP.seeded(final.n_p, 802)
    (sa, aa), (sb, ab), (sB, aB) = row_sums(final.F, xu), row_sums(final.Bt, xp), row_sums(final.B, xu)
    want_u = sa + sb
    d = np.maximum(most_roundings(final.F, 2), most_roundings(final.Bt, 1))
    lf, lb = np.diff(final.F.rowptr.astype(np.int64)), np.diff(final.Bt.rowptr.astype(np.int64))
    d = np.maximum(d, np.maximum(M.roundings("blk_fused", lf // 2, lb), M.roundings("stream2", lf, lb)))
    tol_u = M.gamma(d) * (aa + ab) + 2 * U * (np.abs(sa) + np.abs(sb) + np.abs(want_u))
    tol_p = M.gamma(most_roundings(final.B, 2)) * aB + U * np.abs(sB)
    for f, b, st in COMBOS:
        k = f"jacobian_vmult fuse {f} bsr {b} stream {st}"
        M_within(got[k], np.concatenate([want_u, sB]), np.concatenate([tol_u, tol_p]), k)
    for name, mm, x, c in (("inner_spmv(F)", final.F, xu, 2), ("inner_spmv(M_p)", final.Mp, xp, 1)):
        s, a = row_sums(mm, x, fp32=name in f32)       # fp32: the new values rounded to float first
        M_within(got[name], s, M.gamma(most_roundings(mm, c)) * a + U * np.abs(s), f"{name}, fp32 values {name in f32}")


def M_within(got, want, tol, what):
    err = np.abs(np.asarray(got) - want)
    bad = np.nonzero(~(err <= tol))[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} rows outside the bound, first {bad[:8].tolist()}, error / bound "
                           f"{(err[bad[:8]] / np.maximum(tol[bad[:8]], 1e-300)).tolist()}")


UNSET_WRITES = [(S.BLK_F, w) for w in ("update_values", "scale_values", "set_block", "assemble", "time_assemble")] + \
               [(b, w) for b in (S.BLK_BT, S.BLK_B, S.BLK_MP) for w in ("update_values", "scale_values", "set_block")]


@base_param
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("blk,writer", UNSET_WRITES, ids=[f"{BLOCK_NAME[b]}-{w}" for b, w in UNSET_WRITES])
def test_writer_without_a_setup_reaches_every_product(blk, writer, precision, base):
    """The preconditioner is documented as stale after a write without a set-up and is not asserted; the products are: each
    equals the same product of a fresh handle that holds the new values, and meets the kernels' row-wise bound against
    the exact row sums of the new values."""
    if precision == 32:
        _skip_if_overridden("NSK_INNER_MATRIX_PRECISION")
    pr = problem("ns16")
    opts = {**BASES[base], S.OPT_INNER_MATRIX_PRECISION: precision}
    inner = {S.BLK_F: "inner_spmv(F)", S.BLK_MP: "inner_spmv(M_p)"}
    f32 = set(inner.values()) if precision == 32 else set()
    with handle(pr, opts) as ls:
        setup_fp(ls, pr, BT_)
        assert ls.inner_value_bytes(S.BLK_F) == ls.inner_value_bytes(S.BLK_MP) == precision // 8
        before = products(ls, pr, blk)              # every lazy plan and copy exists
        asm = write(ls, pr, blk, writer)
        got = products(ls, pr, blk)
        final = FP.problem_from_handle(ls, pr)
        width = {b: ls.inner_value_bytes(b) for b in inner}

    def fresh_products(options):
        with handle(pr if asm is not None else final, options) as ref:
            if asm is not None:
                FP.run_assembly(ref, pr, asm)
                assert np.array_equal(ref.get_block(S.BLK_F)[2], final.F.val), "two device assemblies of one state differ"
            ref.setup_preconditioner(*BT_, FP.ALPHA)
            return products(ref, pr, blk)

    want = fresh_products(opts)
    if writer == "set_block" and precision == 32 and blk in inner:
        # Narrowed.  include/nsk.h, NSK_OPT_INNER_MATRIX_PRECISION: "nsk_set_block_csr of F or M_p hands over a pattern and
        # drops that block's copy: until the next set-up the inner product of that block reads the double values
        # (nsk_inner_value_bytes: 8), and the next set-up converts again"
        assert width[blk] == 8 and width[S.BLK_MP if blk == S.BLK_F else S.BLK_F] == 4
        f32.discard(inner[blk])
        want64 = dict(fresh_products({**opts, S.OPT_INNER_MATRIX_PRECISION: 64}))
        want = [(k, want64[k] if k == inner[blk] else v) for k, v in want]
    else:
        assert all(w == precision // 8 for w in width.values()), width
    FP.assert_same(got, want, f"{writer}({BLOCK_NAME[blk]}) without a set-up, inner matrices in fp{precision}")
    assert FP.first_difference(got, before) is not None
    check_bounds(got, final, blk, f32)


# ------------------------------------------------------------------ 5. exact relations
def assert_normal(v, f32, what):
    """No entry that is not zero leaves the normal range of the format it is stored in, with a factor 2^8 to spare"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    a = a[a != 0]
    tiny, huge = (np.finfo(np.float32) if f32 else np.finfo(np.float64)).tiny, (np.finfo(np.float32) if f32 else np.finfo(np.float64)).max
    assert np.all(np.isfinite(a)) and (a.size == 0 or (a.min() > 256.0 * float(tiny) and a.max() < float(huge) / 256.0)), what


def bits(fp, *names):
    d = dict(fp)
    return [d[n] for n in names]


PRS = ["tri_apply(pressure, b0)", "tri_apply(pressure, b1)"]
VEL = ["tri_apply(velocity, b0)", "tri_apply(velocity, b1)"]


@base_param
@pytest.mark.parametrize("factor_bits", [64, 32])
@pytest.mark.parametrize("target", [p for p in PAIRS if p[0] != S.ASIMPLE], ids=[PAIR_IDS[p] for p in PAIRS if p[0] != S.ASIMPLE])
def test_half_the_pressure_mass_doubles_its_factors_solution(target, factor_bits, base):
    """ILU(0) and SGS of c A: the same L, c U — exact for a power of two, also with fp32 off-diagonals"""
    if factor_bits == 32:
        _skip_if_overridden("NSK_FACTOR_PRECISION")
    pr = case_of(target)
    with handle(pr, {**BASES[base], S.OPT_FACTOR_PRECISION: factor_bits}) as ls:
        one = bits(setup_fp(ls, pr, target), *PRS)
        ls.scale_values(S.BLK_MP, 0.5)
        assert_normal(ls.get_block(S.BLK_MP)[2], factor_bits == 32, "M_p / 2")
        two = bits(setup_fp(ls, pr, target), *PRS)
    for a, b in zip(one, two):
        assert_normal(a, False, "tri_apply(pressure)")
        assert np.array_equal(b, 2.0 * a) and np.any(a != 0)


@base_param
@pytest.mark.parametrize("factor_bits", [64, 32])
@pytest.mark.parametrize("target", [(0, 0), (0, 1), (1, 1), (2, 0), (2, 1)], ids=lambda t: PAIR_IDS[t])
def test_twice_f_halves_its_factors_solution(target, factor_bits, base):
    """SGS (blockDiagonal, stationary) and ILU(0) of 2 F, with fp64 and fp32 off-diagonals.  Under aSIMPLE S = B D^-1 Bt
    halves exactly, and with fp64 factors the solution of S's factor doubles.  (Not asserted of S's factor with fp32
    off-diagonals: S at 16 x 10 holds entries near 3e-38, what cancellation leaves of structural zeros — below the normal
    range of fp32, where halving does not commute with the rounding to float.)"""
    if factor_bits == 32:
        _skip_if_overridden("NSK_FACTOR_PRECISION")
    pr = case_of(target)
    asimple = target[0] == S.ASIMPLE
    names = VEL + (["get_block(S) values"] + (PRS if factor_bits == 64 else []) if asimple else [])
    scale = {**{n: 0.5 for n in VEL}, "get_block(S) values": 0.5, **{n: 2.0 for n in PRS}}
    with handle(pr, {**BASES[base], S.OPT_FACTOR_PRECISION: factor_bits}) as ls:
        one = bits(setup_fp(ls, pr, target), *names)
        ls.scale_values(S.BLK_F, 2.0)
        assert_normal(ls.get_block(S.BLK_F)[2], factor_bits == 32, "2 F")
        two = bits(setup_fp(ls, pr, target), *names)
    for n, a, b in zip(names, one, two):
        assert_normal(a, False, n)
        assert_normal(b, False, n)
        assert np.array_equal(b, scale[n] * a) and np.any(a != 0), n


@base_param
@pytest.mark.parametrize("blk,factor", [(S.BLK_B, -1.0), (S.BLK_BT, 4.0)], ids=["minus-B", "4-Bt"])
@pytest.mark.parametrize("variant", [S.STATIONARY, S.UNSTEADY], ids=["stat", "unst"])
def test_s_follows_b_and_bt_exactly(variant, blk, factor, base):
    target = (S.ASIMPLE, variant)
    pr = case_of(target)
    with handle(pr, BASES[base]) as ls:
        one = bits(setup_fp(ls, pr, target), "get_block(S) values")[0]
        ls.scale_values(blk, factor)
        two = bits(setup_fp(ls, pr, target), "get_block(S) values")[0]
    assert_normal(one, False, "S")
    assert np.array_equal(two, factor * one) and np.any(one != 0)


# ------------------------------------------------------------------ 6. two ranks
@base_param
def test_two_ranks_with_a_history(base):
    """aSIMPLE, three writers (one of them of the imported rows of Bt), blockTriangular, aSIMPLE again on two rank threads
    in lockstep: each rank as a fresh pair of handles — the ghosts of D^-1 and the imported Bt rows in S included."""
    world, case = 2, CASES["ns16"]
    parts = [P.generate(**case, nranks=world, rank=r) for r in range(world)]
    plans = [{S.SPACE_U: PT.build_halo_plan(r, parts[0].u_ranges, [p.ghost_u for p in parts]),
              S.SPACE_P: PT.build_halo_plan(r, parts[0].p_ranges, [p.ghost_p for p in parts])} for r in range(world)]
    opts = BASES[base]

    def group(body):
        uid = S.local_group_id(world, True)
        errs, out = [], [None] * world

        def run(r):
            try:
                out[r] = body(r, uid)
            except Exception as e:  # noqa: BLE001
                errs.append((r, repr(e)))
                S.abort_local_group(uid)

        th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
        [t.start() for t in th]
        [t.join(120) for t in th]
        if any(t.is_alive() for t in th):
            S.abort_local_group(uid)
            [t.join(30) for t in th]
        assert not any(t.is_alive() for t in th), "rank threads still blocked"
        assert not errs, errs
        return out

    def history(r, uid):
        p = parts[r]
        ls = S.LinearSolver(r, world, 0, uid)
        try:
            FP.set_options(ls, opts)
            ls.set_problem(p, plans[r])
            ls.setup_preconditioner(*AS, FP.ALPHA)
            first = FP.fingerprint(ls, p, r)
            ls.scale_values(S.BLK_B, -1.0)
            ls.scale_values(S.BLK_F, 0.7)
            ls.update_values(S.BLK_BT_GHOST, new_values(p.Bt_ghost, 60 + r))
            ls.setup_preconditioner(*BT_, FP.ALPHA)
            FP.fingerprint(ls, p, r)
            final = FP.problem_from_handle(ls, p)
            ls.setup_preconditioner(*AS, FP.ALPHA)
            return first, FP.fingerprint(ls, p, r), final
        finally:
            ls.close()

    hist = group(history)
    finals = [h[2] for h in hist]
    assert all(len(p.ghost_u) and p.Bt_ghost.nnz for p in parts)
    fresh = [group(lambda r, uid: FP.fresh(finals[r], opts, *AS, rank=r, nranks=world, uid=uid, plan=plans[r])) for _ in (0, 1)]
    for r in range(world):
        FP.assert_same(fresh[0][r], fresh[1][r], f"control: two fresh pairs of handles, rank {r}")
        FP.assert_same(hist[r][1], fresh[0][r], f"rank {r} after the history")
        assert FP.first_difference(hist[r][0], hist[r][1]) is not None
