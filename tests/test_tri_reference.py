"""The reference of the triangular-solve kernel tests (tests/tri_reference.py), checked on the CPU:

* against the oracle's ILU(0) / SGS (oracle.Tri) on the golden problems and on irregular patterns: its exported factor
  meets the exact-defect bound, its apply the residual bounds;
* a plain double solve meets its own bounds with room to spare, the exact rational solve has residual zero;
* ONE wrong entry — its contribution removed, the vector read at a neighbouring column, the value of the other half
  used — breaks the bound (and, on integer inputs, the equality) ON THE ROW CONCERNED, for every pattern of the list, in
  both halves and both kinds; one update left out of the factorisation breaks the defect bound at that position.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import tri_reference as T
from tests.util import problem

ILU, SGS = 0, 1
PATTERNS = ["n2", "n63", "n129", "irregular", "nonsymmetric", "stair", "stair_nonsymmetric", "stair_lower", "stair_upper",
            "lattice", "nodes", "nodes_stair", "odd_nodes"]


def _pattern(name):
    p = T.pattern(name)
    return p if isinstance(p, tuple) else (p, None)


def _permuted(name, vals, sub_off=None, natural=False):
    """(matrix, P) in the ordering the analysis chooses (line groups of three on the lattice)."""
    A0, xy = _pattern(name)
    A = T.values(A0, vals)
    perm = np.arange(A.n_rows) if natural else T.multicolour_perm(A, sub_off, name.startswith("nodes"), xy, 3 if xy is not None else 1)[0]
    return A, T.Permuted(A, perm.astype(np.int64), T.keep_mask(A, sub_off))


def _rhs(n, seed=0):
    return np.random.default_rng(900 + seed).uniform(-1.0, 1.0, n)


# ------------------------------------------------------------------ against the oracle
def _oracle_case(A, kind, perm, sub_off, what):
    from oracle import oracle as O
    tri = O.Tri(O.CsrHolder(A.rowptr, A.col, A.val, A.n_rows, A.n_cols), kind=kind, shard_off=sub_off, perm=perm)
    rp, col, val = tri.export()
    P = T.Permuted(A, np.arange(A.n_rows) if perm is None else np.asarray(perm, dtype=np.int64), T.keep_mask(A, sub_off))
    assert np.array_equal(rp, P.rp) and np.array_equal(col, P.col), f"{what}: the permuted pattern differs from the oracle's"
    a = P.values(A.val)
    if kind == ILU:
        E, B, _ = T.ilu0_defect(P, a, val)
        assert np.all(E <= B), (what, np.nonzero(~(E <= B))[0][:5])
        assert np.array_equal(T.ilu0_float(P, a), val), f"{what}: the double model of ILU(0) has other bits than the oracle"
    else:
        assert np.array_equal(val, a)
    b = _rhs(A.n_rows)
    x = tri.apply(b)
    assert T.check_solution(P, val, kind, b, x, "walker") == [], what      # (b - sum) / d: the walker's count
    assert np.abs(T.model_apply(P, val, kind, b) - x).max() <= 1e-12 * np.abs(x).max(), what


@pytest.mark.parametrize("kind", [ILU, SGS])
@pytest.mark.parametrize("name", ["stokes16", "ns16", "unsteady16"])
def test_reference_agrees_with_the_oracle_on_the_golden_problems(name, kind):
    from tests import spmv_reference as M
    pr = problem(name)
    for blk, tag in ((pr.F, "F"), (pr.Mp, "Mp")):
        A = M.Csr(blk.rows, blk.cols, blk.rowptr, blk.col, blk.val, blk.cols, f"{name}:{tag}")
        _oracle_case(A, kind, None, None, f"{name} {tag} natural")
        if kind == SGS or tag == "Mp":       # (the exact defect of F's wide rows costs seconds: one ordering is enough)
            perm = T.multicolour_perm(A, None, tag == "F")[0]
            _oracle_case(A, kind, perm, None, f"{name} {tag} multicolour")
    n = pr.Mp.rows
    A = M.Csr(n, n, pr.Mp.rowptr, pr.Mp.col, pr.Mp.val, n, f"{name}:Mp")
    offs = [0, n // 3, n // 3, n]
    _oracle_case(A, kind, T.multicolour_perm(A, offs)[0], offs, f"{name} Mp, sub-domains with an empty one")


@pytest.mark.parametrize("kind", [ILU, SGS])
@pytest.mark.parametrize("name", ["irregular", "nonsymmetric", "stair", "lattice", "nodes"])
def test_reference_agrees_with_the_oracle_on_irregular_patterns(name, kind):
    A, P = _permuted(name, "real")
    _oracle_case(A, kind, P.perm, None, name)
    if name == "irregular":
        offs = [0, 700, 700, 1501, 2300]
        _oracle_case(A, kind, T.multicolour_perm(A, offs)[0], offs, f"{name}, sub-domains")


# ------------------------------------------------------------------ the bounds hold for a correct solve, with room
@pytest.mark.parametrize("name", PATTERNS)
def test_a_double_solve_meets_its_bounds_with_room(name):
    A, P = _permuted(name, "real")
    a = P.values(A.val)
    f = T.ilu0_float(P, a)
    E, B, m = T.ilu0_defect(P, a, f)
    assert np.all(E <= B)
    assert np.all(E[m == 0] == 0.0)                      # copies are exact
    many = m >= 8                                        # worst-case bounds of many roundings are far from attained
    assert not many.any() or np.all(E[many] <= 0.5 * B[many])
    b = _rhs(A.n_rows, 1)
    for kind, fv in ((ILU, f), (SGS, a)):
        for fh in (fv, T.round_halves_f32(P, fv, block2=name.startswith("nodes"))):
            x = T.model_apply(P, fh, kind, b)
            for path in ("walker", "sf_scalar"):
                res, bound = T.residual_composed(P, fh, kind, b, x, path)
                assert np.all(res <= 0.5 * bound), (name, kind, path, float((res / np.maximum(bound, 1e-300)).max()))
                alone = T.residual_alone(P, fh, kind, b, x, path)
                assert (alone is not None) == (not P.n_lower.any() or not P.n_upper.any())
                if alone is not None:
                    assert np.all(alone[0] <= 0.5 * alone[1]), (name, kind, path)


def test_the_exact_rational_solve_has_residual_zero_where_it_is_a_double():
    """Integer data: the exact solution is representable, the residuals of both forms must be exactly 0."""
    for name in ("stair", "stair_lower", "stair_upper", "nonsymmetric"):
        A, P = _permuted(name, "int")
        a = P.values(A.val)
        b = T.integer_problem(P, a)
        x, big = T.int_solve(P, a, b)
        assert big < 2 ** 20
        res, bound = T.residual_composed(P, a, SGS, b, x, "ring")
        assert np.all(res == 0.0) and np.all(bound > 0.0)
        alone = T.residual_alone(P, a, SGS, b, x, "ring")
        assert alone is None or np.all(alone[0] == 0.0)
        assert np.array_equal(T.model_apply(P, a, SGS, b), x)


def test_exact_arithmetic_helper():
    v = np.array([1.0, -0.75, 2.0 ** -60, 3.0e7, 0.0, 5e-324])
    (q,), S = T.to_ints(v)
    assert [Fraction(t, 1 << S) for t in q] == [Fraction(float(t)) for t in v]
    assert T._to_float(q[1], S) == -0.75 and T._to_float(0, 5) == 0.0


# ------------------------------------------------------------------ one wrong entry is caught on its row
def _entries(P, seed):
    """One strict-lower and one strict-upper entry of P whose rows hold at least two entries in that half where there
    are such rows (the 'swap' mutation then reads another column of the same row)."""
    rng = np.random.default_rng(seed)
    out = []
    for cnt, lo in ((P.n_lower, P.rp[:-1]), (P.n_upper, P.diag + 1)):
        rows = np.nonzero(cnt >= 2)[0]
        if len(rows) == 0:
            rows = np.nonzero(cnt >= 1)[0]
        if len(rows):
            i = int(rows[rng.integers(len(rows))])
            out.append((i, int(lo[i] + rng.integers(cnt[i]))))
    return out


@pytest.mark.parametrize("kind", [ILU, SGS])
@pytest.mark.parametrize("name", PATTERNS)
def test_one_wrong_entry_breaks_the_bound_on_its_row(name, kind):
    A, P = _permuted(name, "real")
    a = P.values(A.val)
    f = T.ilu0_float(P, a) if kind == ILU else a
    b = _rhs(A.n_rows, 2)
    assert T.check_solution(P, f, kind, b, T.model_apply(P, f, kind, b), "sf_scalar") == []
    seen = 0
    for i, k in _entries(P, 5):
        for what in ("drop", "swap", "other_half"):
            x = T.model_apply(P, f, kind, b, (what, k))
            bad = T.check_solution(P, f, kind, b, x, "sf_scalar")
            assert i in [r for r, _, _, _ in bad], f"{name} {what} entry {k} of row {i}: rows reported {[r for r, _, _, _ in bad][:8]}"
            seen += 1
    assert seen >= 3 or name == "n2"


@pytest.mark.parametrize("name", PATTERNS)
def test_one_wrong_entry_breaks_the_integer_equality_on_its_row(name):
    A, P = _permuted(name, "int")
    a = P.values(A.val).copy()
    a[(a == 0.0)] = 2.0                       # a stored zero hides its entry: here every entry counts
    b = T.integer_problem(P, a)
    want, _ = T.int_solve(P, a, b)
    xs = np.empty(P.n)
    xs[P.perm] = np.arange(P.n)
    for i, k in _entries(P, 6):
        for what in ("drop", "swap"):
            x = T.model_apply(P, a, SGS, b, (what, k))
            wrong = np.nonzero(x != want)[0]
            if what == "swap" and len(wrong) == 0:
                continue                      # the neighbouring column held the same integer
            assert int(P.perm[i]) in wrong.tolist(), (name, what, i, k)


@pytest.mark.parametrize("name", ["n63", "irregular", "nonsymmetric", "stair", "lattice", "nodes"])
def test_an_update_left_out_of_the_factorisation_breaks_the_defect_bound_there(name):
    A, P = _permuted(name, "real")
    a = P.values(A.val)
    # the first update of the factorisation: (k, t) with t in row i updated by the lower entry k
    hit = None
    for i in range(P.n):
        where = {int(P.col[q]): q for q in range(P.rp[i], P.rp[i + 1])}
        for k in range(P.rp[i], P.diag[i]):
            c = int(P.col[k])
            for m in range(P.diag[c] + 1, P.rp[c + 1]):
                t = where.get(int(P.col[m]))
                if t is not None and t > k:
                    hit = (k, t)
                    break
            if hit:
                break
        if hit:
            break
    assert hit is not None
    f = T.ilu0_float(P, a, skip=hit)
    E, B, _ = T.ilu0_defect(P, a, f)
    assert not E[hit[1]] <= B[hit[1]]


def test_sub_domains_drop_the_cross_entries_and_nothing_else():
    A0, _ = _pattern("irregular")
    offs = [0, 700, 700, 1501, 2300]
    keep = T.keep_mask(A0, offs)
    r, c = A0.row_ids, A0.col
    shard = np.searchsorted(np.array(offs[1:]), np.arange(A0.n_rows), side="right")
    assert np.array_equal(keep, shard[r] == shard[c]) and 0 < (~keep).sum() < A0.nnz
    P = T.Permuted(A0, T.multicolour_perm(A0, offs)[0], keep)
    assert P.nnz == keep.sum() and np.array_equal(np.sort(P.src), np.nonzero(keep)[0])


def test_staircase_patterns_have_the_colours_they_promise():
    for name in ("stair", "stair_nonsymmetric", "stair_lower", "stair_upper", "nodes_stair"):
        A = T.pattern(name)
        perm, info = T.multicolour_perm(A, None, name.startswith("nodes"))
        assert np.array_equal(perm, np.arange(A.n_rows)) and info[0] == len(A.layers) - 1, name
    A = T.pattern("stair")
    P = T.Permuted(A, np.arange(A.n_rows))
    f = A.layers
    assert P.n_lower[f[6]:f[7]].sum() == 2048 and f[7] - f[6] == 32 and f[5] - f[4] == 64 and f[6] - f[5] == 65
    assert f[2] - f[1] == 1 and not P.n_lower[:f[1]].any() and not P.n_upper[f[8]:].any()
    xy_pat, xy = T.pattern("lattice")
    for group in (2, 3):
        assert T.multicolour_perm(xy_pat, None, False, xy, group)[1][1] == group
