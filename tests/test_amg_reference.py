"""The reference of the AMG set-up kernel tests (tests/amg_reference.py), checked on the CPU:

* its full aggregation model against the oracle's aggregates (default threshold, full diagonal) and against the numpy
  statement of DESIGN.md 5a on every case matrix;
* transpose and A B against SciPy: same pattern, values within nnz_row 2^-52 |A||B|;
* a chained level — aggregates, weights, smoothed prolongator, transpose, A P, R (A P) — gives the oracle's level 1;
* every listed mutation of the model is caught, on a named row, by at least one case;
* every case set holds the rows it is named for, so that a GPU test cannot pass by having nothing to check.
"""
import numpy as np
import pytest

from tests import amg_reference as R
from tests.util import problem

u64 = np.uint64


def _oracle_amg(A):
    from oracle import oracle as O
    return O.Amg(O.CsrHolder(A.rp, A.col, A.val, A.n_rows, A.n_cols))


def _first_bad(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return -1
    bad = np.flatnonzero(a != b)
    return None if len(bad) == 0 else int(bad[0])


# ------------------------------------------------------------------ against the oracle and the numpy statement
@pytest.mark.parametrize("name", R.GRAPH_CASES)
def test_aggregation_model_equals_the_numpy_statement(name):
    A = R.case(name)
    r = R.aggregate(A)
    assert _first_bad(r.agg, R.aggregate_numpy(A.scipy())) is None, name
    assert r.nc == int(r.agg.max()) + 1 and np.all((r.agg == -2) == (r.key0 == 0))
    assert np.all(r.agg != -1), "every row with a strong connection ends in an aggregate"


@pytest.mark.parametrize("name", R.FULL_DIAGONAL)
def test_aggregation_model_equals_the_oracle(name):
    A = R.case(name)
    M = _oracle_amg(A)
    agg = M.aggregates(0)
    assert agg is not None
    assert _first_bad(R.aggregate(A).agg, agg) is None, name


def test_aggregation_model_equals_the_oracle_on_the_velocity_block():
    pr = problem("ns16")
    A = R.Mat(pr.F.rows, pr.F.cols, pr.F.rowptr, pr.F.col, pr.F.val, "ns16:F")
    assert _first_bad(R.aggregate(A).agg, _oracle_amg(A).aggregates(0)) is None


# ------------------------------------------------------------------ against SciPy
@pytest.mark.parametrize("width", R.WIDTHS)
def test_product_against_scipy(width):
    A, B = R.product_a(width), R.product_b()
    C = R.product(A, B)
    Sa, Sb = A.scipy(), B.scipy()
    S = (Sa @ Sb).tocsr()
    # scipy drops nothing structurally; exact cancellations stay as stored zeros in both
    mag = (abs(Sa) @ abs(Sb)).tocsr()
    mag.sort_indices()
    S.sort_indices()
    assert np.array_equal(mag.indptr, C.rp) and np.array_equal(mag.indices, C.col)
    nnz_row = np.repeat(A.lens, C.lens)
    Sd = np.asarray(S[C.row, C.col]).ravel()
    assert np.all(np.abs(C.val - Sd) <= nnz_row * 2.0 ** -52 * mag.data), width


def test_transpose_against_scipy():
    A = R.transpose_case()
    T = R.transpose(A)
    S = A.scipy().T.tocsr()
    S.sort_indices()
    assert np.array_equal(T.rp, S.indptr) and np.array_equal(T.col, S.indices) and np.array_equal(R.bits(T.val), R.bits(S.data))
    P = R.prolongator(*R.prolong_case(40))
    T = R.transpose(P)
    S = P.scipy().T.tocsr()
    S.sort_indices()
    assert np.array_equal(T.rp, S.indptr) and np.array_equal(T.col, S.indices) and np.array_equal(R.bits(T.val), R.bits(S.data))


# ------------------------------------------------------------------ a chained level
def chained_level(A, lam):
    r = R.aggregate(A)
    _, dinv = R.diag(A)
    P = R.prolongator(A, r.agg, r.pw, dinv, (4.0 / 3.0) / lam)
    Rt = R.transpose(P)
    AP = R.product(A, P)
    return r, P, Rt, AP, R.product(Rt, AP)


@pytest.mark.parametrize("name", ["lap40", "directed", "ns16"])
def test_a_chained_level_gives_the_oracles_level_one(name):
    if name == "ns16":
        pr = problem("ns16")
        A = R.Mat(pr.F.rows, pr.F.cols, pr.F.rowptr, pr.F.col, pr.F.val, "ns16:F")
    else:
        A = R.case(name)
    lv = _oracle_amg(A).levels()
    assert len(lv) >= 2 and lv[0][0] == A.n_rows
    r, P, Rt, AP, C = chained_level(A, lv[0][2])
    assert (C.n_rows, C.nnz) == (lv[1][0], lv[1][1]), (name, C.n_rows, C.nnz, lv[1])
    assert r.nc == lv[1][0]


# ------------------------------------------------------------------ mutations of the model
def _ties_strength(mutate=None):
    A, t = R.ties()
    return A, R.strength(A, R.diag(A)[0], t, mutate)


def test_mutation_strength_with_greater_or_equal_is_caught():
    A, good = _ties_strength()
    _, bad = _ties_strength("ge")
    k = _first_bad(good[0], bad[0])
    assert k is not None and (int(A.row[k]), int(A.col[k])) == (0, 1)        # v^2 == t2 ad_i ad_j exactly
    assert _first_bad(good[1], bad[1]) is not None and _first_bad(good[3], bad[3]) == 0   # flag words; row 0 leaves -2


def test_mutation_product_of_the_diagonals_first_is_caught():
    A, t = R.ties_order()
    ad = R.diag(A)[0]
    good, bad = R.strength(A, ad, t), R.strength(A, ad, t, "product_first")
    k = _first_bad(good[0], bad[0])
    assert k is not None and (int(A.row[k]), int(A.col[k])) == (0, 1)
    assert good[4] == 3 and bad[4] == 0


def _tie_join(mutate=None):
    A, where = R.float_ties()
    strong, key, agg = R.float_ties_join_inputs(A)
    return A, where, R.join(A, strong, key, 1, agg, np.full(A.n_rows, -9, np.int32), mutate)


def test_mutation_last_equal_weight_wins_is_caught():
    A, where, good = _tie_join()
    _, _, bad = _tie_join("last")
    for r, k1, k2 in where:
        assert good[r] == 1000 + A.col[A.rp[r] + min(k1, k2)], r            # the first in the row
        assert bad[r] == 1000 + A.col[A.rp[r] + max(k1, k2)], r
    assert _first_bad(good, bad) == 0


def test_mutation_weights_compared_as_doubles_is_caught():
    A, where, good = _tie_join()
    _, _, bad = _tie_join("double")
    differs = [r for r, _, _ in where if good[r] != bad[r]]
    assert differs == [r for r, _, _ in where if r % 2 == 1]                # the rows with the larger double second


@pytest.mark.parametrize("name", ["lap40", "directed"])
def test_mutation_pass_b_on_the_live_array_is_caught(name):
    A = R.case(name)
    good, bad = R.aggregate(A), R.aggregate(A, mutate="live")
    assert np.array_equal(good.agg_a, bad.agg_a)
    k = _first_bad(good.agg, bad.agg)
    assert k is not None and good.agg_a[k] == -1, k                         # a pass-B row


def test_mutation_roots_numbered_by_key_is_caught():
    A = R.case("lap40")
    good, bad = R.aggregate(A), R.aggregate(A, mutate="by_key")
    k = _first_bad(good.agg_roots, bad.agg_roots)
    assert k is not None and R.state(good.key)[k] == 2


@pytest.mark.parametrize("name", ["lap40", "directed"])
def test_mutation_stale_pull_one_value_is_caught(name):
    A = R.case(name)
    good = R.aggregate(A)
    bad = R.aggregate(A, mutate="stale_pull1", max_rounds=len(good.und) + 1)
    rounds = [r for r, (a, b) in enumerate(zip(good.keys, bad.keys)) if not np.array_equal(a, b)]
    assert rounds and good.stamped[rounds[0]], (name, rounds)               # first seen in a stamped round
    assert _first_bad(good.keys[rounds[0]], bad.keys[rounds[0]]) is not None


def test_mutation_reversed_sum_order_is_caught():
    A, B = R.product_a(63), R.product_b()
    good, bad = R.product(A, B), R.product(A, B, mutate="reverse")
    assert np.array_equal(good.col, bad.col)
    row = next(i for i in range(A.n_rows) if A.lens[i] == 4 and np.array_equal(A.val[A.rp[i]:A.rp[i + 1]], R.ORDER_TERMS))
    k = int(good.rp[row]) + int(np.flatnonzero(good.col[good.rp[row]:good.rp[row + 1]] == 7)[0])
    assert good.val[k] == 2.0 ** -53 and bad.val[k] == 2.0 ** -52


@pytest.mark.parametrize("order", ["reversed", "random"])
def test_mutation_sort_tail_ignored_is_caught(order):
    A = R.sort_case(order)
    good, bad = R.rows_sort(A), R.rows_sort(A, mutate="no_tail")
    k = _first_bad(good[0], bad[0])
    long_rows = np.flatnonzero(A.lens > R.SORT_STAGE)
    assert k is not None and np.searchsorted(A.rp, k, side="right") - 1 == long_rows[0]
    for i in np.flatnonzero(A.lens <= R.SORT_STAGE):
        assert np.array_equal(good[0][A.rp[i]:A.rp[i + 1]], bad[0][A.rp[i]:A.rp[i + 1]])


def test_mutation_scan_without_the_carry_is_caught():
    n = R.SCAN_SIZES[-1]
    x = R.scan_input(n)
    good, bad = R.scan(x)[0], R.scan(x, mutate="drop_carry")[0]
    assert _first_bad(good, bad) == R.SCAN_CHUNK * 1024                     # the first element of the second trip
    for m in R.SCAN_SIZES[:-1]:
        assert np.array_equal(R.scan(R.scan_input(m))[0], R.scan(R.scan_input(m), mutate="drop_carry")[0])


def test_mutation_block_fill_with_global_columns_is_caught():
    A = R.block_case()
    for r0, r1 in R.BLOCK_RANGES:
        good, bad = R.block(A, r0, r1), R.block(A, r0, r1, mutate="global_columns")
        assert np.array_equal(good[0], bad[0])
        assert (_first_bad(good[1], bad[1]) is None) == (r0 == 0), r0


# ------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("n", [300, 255, 256, 257])
def test_lengths_cases_hold_every_row_they_are_named_for(n):
    A = R.case(f"lengths{n}")
    assert n % 256 != 0 or n == 256
    assert set(R.LENGTHS) <= set(A.lens.tolist())
    pos = np.full(n, -1)
    on = np.flatnonzero(A.col == A.row)
    pos[A.row[on]] = on - A.rp[A.row[on]]
    assert np.any(pos == 0) and np.any((pos == A.lens - 1) & (A.lens > 1)) and np.any(pos >= 16) and np.any((pos < 0) & (A.lens > 0))
    ad, dinv = R.diag(A)
    d = np.zeros(n)
    d[A.row[on]] = A.val[on]
    zero = (pos >= 0) & (d == 0.0)
    assert np.any(zero & ~np.signbit(d)) and np.any(zero & np.signbit(d)) and np.any(d < 0)
    assert np.all(dinv[zero] == 1.0) and np.all(dinv[pos < 0] == 1.0) and np.all(ad[pos < 0] == 0.0) and not np.any(np.signbit(ad))
    strong = R.strength(A, ad, R.THRESHOLD)[0]
    off = A.col != A.row
    assert strong[off].any() and (~strong[off]).any()


def test_ties_hold_equality_one_ulp_either_side_and_one_direction():
    A, (strong, fw, key, agg, und) = _ties_strength()
    ad = R.diag(A)[0]
    lhs, rhs = A.val * A.val, (0.25 * ad[A.row]) * ad[A.col]
    off = A.col != A.row
    assert np.any(off & (lhs == rhs)) and np.any(off & (lhs == np.nextafter(rhs, np.inf))) and np.any(off & (lhs == np.nextafter(rhs, -np.inf)))
    S = {(int(i), int(j)) for i, j, s in zip(A.row, A.col, strong) if s}
    assert (4, 5) in S and (5, 4) not in S
    assert agg[0] == -2 and key[0] == 0 and agg[3] == -2 and A.lens[3] == 2 and und == 5


@pytest.mark.parametrize("name", ["lap40", "directed", "path700"])
def test_rounds_of_the_cases(name):
    r = R.aggregate(R.case(name))
    want = {"lap40": [1600, 523, 114, 10], "path700": [700, 134, 5], "directed": [1441, 507, 197, 44, 7]}[name]
    assert r.und == want
    assert (not r.stamped[0]) and all(r.stamped[1:]) and len(r.stamped) >= 2     # one unstamped round, the rest stamped
    assert int((r.agg_a == -1).sum()) > 0, "pass B is not empty"
    if name == "lap40":
        assert r.nc == 239 and int((r.agg_a == -1).sum()) == 439
    if name == "directed":
        assert int((r.key0 == 0).sum()) == 59 and len(r.und) == 5
        S = {(int(i), int(j)) for i, j, s in zip(R.case(name).row, R.case(name).col, r.strong) if s}
        assert any((j, i) not in S for i, j in S), "the strength graph is directed"


def test_float_tie_rows_exist():
    A, where = R.float_ties()
    assert len(where) == 2 * len(R.TIE_PAIRS)
    kinds = set()
    for r, k1, k2 in where:
        a, b = abs(A.val[A.rp[r] + k1]), abs(A.val[A.rp[r] + k2])
        assert a != b and np.float32(a) == np.float32(b) and {a, b} == {R.TIE_LO, R.TIE_HI}
        assert (a > b) == (r % 2 == 0)
        others = np.delete(np.abs(A.val[A.rp[r]:A.rp[r + 1]]), [0, k1, k2])
        assert np.all(others.astype(np.float32) < np.float32(a))
        kinds.add(("same step" if k1 // 16 == k2 // 16 else "other step", "same group" if k1 // 64 == k2 // 64 else "other group"))
        assert k1 % 16 != k2 % 16 or k1 // 16 != k2 // 16
    assert {("same step", "same group"), ("other step", "same group"), ("other step", "other group")} <= kinds


@pytest.mark.parametrize("width", R.WIDTHS)
def test_product_rows_hold_exactly_the_named_widths(width):
    A, B = R.product_a(width), R.product_b()
    C = R.product(A, B)
    assert C.lens[0] == width == C.lens.max()
    assert R.tier_for(width) == {63: 0, 64: 0, 65: 1, 127: 1, 128: 1, 129: 2, 511: 2, 512: 2, 513: 3}[width]
    assert set(B.lens.tolist()) >= set(R.B_LENGTHS)
    used = set(B.lens[A.col].tolist())
    assert used >= {ln for ln in R.B_LENGTHS if ln <= width}
    want = {0, 1} | {m for L in (8, 16, 64) for m in (L, L + 1, 4 * L, 4 * L + 1) if m <= width}
    assert want <= set(A.lens.tolist()), sorted(want - set(A.lens.tolist()))
    assert all(len(set(B.col[B.rp[j]:B.rp[j + 1]].tolist())) == B.lens[j] for j in range(B.n_rows))


def test_the_widest_product_case_holds_every_length_of_a_row_of_a():
    assert {0, 1, 8, 9, 32, 33, 16, 17, 64, 65, 256, 257} <= set(R.product_a(512).lens.tolist())


@pytest.mark.parametrize("modulus", R.PROLONG_MODULI)
def test_prolongator_cases(modulus):
    A, agg, pw, dinv, c = R.prolong_case(modulus)
    P = R.prolongator(A, agg, pw, dinv, c)
    tier = R.PROLONG_MODULI.index(modulus)
    assert R.tier_for(int(P.lens.max())) == tier
    assert A.lens.max() == 600 and all(np.any(A.lens > s) for s in R.TIER_SLOTS)       # rows longer than every tier's staging
    i = 46
    assert A.lens[i] == 1 and agg[i] == modulus and agg[A.col[A.rp[i]]] != modulus and A.col[A.rp[i]] != i
    assert P.lens[i] == (2 if agg[A.col[A.rp[i]]] >= 0 else 1)
    assert np.any((agg == -2) & (A.lens > 0)) and np.any(agg[A.col] == -2)
    k = int(P.rp[i]) + int(np.flatnonzero(P.col[P.rp[i]:P.rp[i + 1]] == modulus)[0])
    assert P.val[k] == pw[modulus]                                                        # the identity part alone


@pytest.mark.parametrize("order", ["reversed", "random"])
def test_sort_cases(order):
    A = R.sort_case(order)
    assert A.lens.tolist() == R.SORT_LENGTHS
    col, val = R.rows_sort(A)
    for i in range(A.n_rows):
        c = col[A.rp[i]:A.rp[i + 1]]
        assert np.all(np.diff(c) > 0)
        assert np.array_equal(val[A.rp[i]:A.rp[i + 1]], c + i / 16.0)
        if A.lens[i] > 1:
            assert not np.array_equal(A.col[A.rp[i]:A.rp[i + 1]], c)


def test_transpose_case():
    A = R.transpose_case()
    hit = np.bincount(A.col, minlength=A.n_cols)
    assert A.n_rows != A.n_cols and np.any(A.lens == 0) and np.any(hit == 0) and hit[5] == (A.lens > 0).sum() > 64


def test_scan_and_block_cases():
    assert R.SCAN_SIZES[-1] > R.SCAN_CHUNK * 1024 and 0 in R.SCAN_SIZES
    x = R.scan_cap_input(2 ** 32)
    assert np.all(x == 2 ** 20) and R.scan(x)[1] == 2 ** 32
    assert R.scan(R.scan_cap_input(R.SCAN_CAP))[1] == R.SCAN_CAP and R.scan(R.scan_cap_input(R.SCAN_CAP + 1))[1] == R.SCAN_CAP + 1
    A = R.block_case()
    for r0, r1 in R.BLOCK_RANGES:
        assert r1 < A.n_rows
        rp, col, val = R.block(A, r0, r1)
        lens = np.diff(rp)
        assert np.any((lens == 0) & (A.lens[r0:r1] > 0)) and np.any(A.lens[r0:r1] == 0)
    assert {r0 for r0, _ in R.BLOCK_RANGES} == {0, 1, 300}


def test_start_vector_is_the_oracles():
    x = R.start_vector(1000)
    assert x[0] == -0.5 and np.all((x >= -0.5) & (x < 0.5)) and len(np.unique(x)) > 900
