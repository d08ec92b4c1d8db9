"""The host side of the SpMV kernel tests (tests/spmv_reference.py) on its own: the exact row sums against scipy and
exact rationals, the promised properties of the pattern generators, and the Python model of the plan builders against
the properties the GPU tests expect of the plans — so that a failure on the GPU is not a wrong expectation."""
from fractions import Fraction

import numpy as np
import pytest

from tests import spmv_reference as M


def _small(seed=3, fp=True):
    A = M.from_lengths([0, 3, 1, 0, 7, 2, 40, 0], 60, seed, n_own=50, ghost_lens=[1, 0, 0, 0, 2, 0, 3, 0])
    return M.real_values(A, seed) if fp else M.int_values(A, seed)


def test_exact_row_sums_against_fractions_and_scipy():
    A = _small()
    xo, xg = M.real_x(A, 1)
    s, a = M.exact_row_sums(A, xo, xg)
    x = np.concatenate([xo, xg])
    for i in range(A.n_rows):
        terms = [Fraction(float(A.val[k])) * Fraction(float(x[A.col[k]])) for k in range(A.rowptr[i], A.rowptr[i + 1])]
        exact = sum(terms, Fraction(0))
        assert Fraction(float(s[i])) == Fraction(float(exact)), i          # float(Fraction) rounds correctly
        assert abs(Fraction(float(a[i])) - sum(map(abs, terms))) <= Fraction(M.U) * 64 * sum(map(abs, terms))
    assert np.allclose(s, A.to_scipy() @ x, rtol=1e-13, atol=1e-15)
    assert s[0] != 0 and s[3] == 0 and s[7] == 0      # a row of ghost entries only; empty rows give an exact zero


def test_fp32_reference_is_the_sum_over_rounded_values():
    A = _small()
    xo, xg = M.real_x(A, 1)
    s32, _ = M.exact_row_sums(A, xo, xg, fp32=True)
    B = A.with_values(A.val.astype(np.float32).astype(np.float64))
    s, _ = M.exact_row_sums(B, xo, xg)
    assert np.array_equal(s, s32)
    assert not np.array_equal(s32, M.exact_row_sums(A, xo, xg)[0])


def test_int_row_sums_and_operands():
    A = _small(fp=False)
    xo, xg = M.int_x(A)
    assert np.all(np.abs(A.val) <= 8) and np.all(A.val != 0) and np.all(A.val == np.rint(A.val))
    assert np.all(np.abs(xo) <= 16) and np.all(xo != 0) and np.all(np.abs(xg) <= 16) and np.all(xg != 0)
    assert len(set(xo[:31])) == 31
    s = M.int_row_sums(A, xo, xg)
    assert np.array_equal(s, np.rint(A.to_scipy() @ np.concatenate([xo, xg])).astype(np.int64))
    # all of it is exact in fp32 as well
    assert np.array_equal(A.val.astype(np.float32).astype(np.float64), A.val)


def test_modes_and_epilogue_round_once_per_operation():
    s = np.array([1.0, 2.0 ** -60, 3.0])
    y, z = np.array([1.0, 1.0, 1.0]), np.array([2.0, 2.0, 2.0])
    assert np.array_equal(M.apply_mode(s, 0, y, z), s)
    assert np.array_equal(M.apply_mode(s, 1, y, None), y + s) and np.array_equal(M.apply_mode(s, 1, y, z), z + s)
    assert np.array_equal(M.apply_mode(s, 2, y, z), z - s)
    d, dinv = np.array([3.0, 3.0, 3.0]), np.array([1 / 3.0] * 3)
    assert np.array_equal(M.epilogue(s, y, d, dinv), ((y * d) - s) * dinv)


def test_rounding_counts():
    assert M.roundings("stream", 0) == 3 and M.roundings("stream", 4) == 3 and M.roundings("stream", 5) == 4
    assert M.roundings("stream", 2048) == 1 + 511 + 2
    assert M.roundings("csrv", 9, lpr=4) == 3 + 2 and M.roundings("csrv", 64, lpr=64) == 1 + 6
    assert M.roundings("blk_c2", 8) == 2 + 1 + 2 and M.roundings("blk_c1", 8) == 1 + 1 + 2
    assert M.roundings("stream2", 8, 4) == 1 + 2 + 2 and M.roundings("blk_fused", 0, 9) == 2 + 2 + 2


# ------------------------------------------------------------------ generators
@pytest.fixture(scope="module")
def scalar():
    return M.scalar_patterns()


@pytest.fixture(scope="module")
def blocks():
    return M.block_patterns()


@pytest.fixture(scope="module")
def pairs():
    return M.pair_patterns()


def _valid(A):
    assert A.columns_sorted(), A.name
    assert A.nnz == 0 or (A.col.min() >= 0 and A.col.max() < A.n_cols), A.name
    assert np.all(np.diff(A.rowptr) >= 0)


def test_every_pattern_is_a_valid_sorted_csr(scalar, blocks, pairs):
    for A in scalar.values():
        _valid(A)
    for _, _, A in blocks.values():
        _valid(A)
    for A, B in pairs.values():
        _valid(A)
        _valid(B)
        assert A.n_rows == B.n_rows
    assert max(A.nnz for A in scalar.values()) <= 2.2e5


def test_scalar_pattern_promises(scalar):
    L = {k: A.row_len for k, A in scalar.items()}
    assert np.all(L["empty_start"][:5] == 0) and L["empty_start"][5] > 0
    assert np.all(L["empty_middle"][300:303] == 0) and L["empty_last"][-1] == 0 and L["empty_last"][-2] > 0
    assert np.all(L["empty_64"][100:164] == 0) and L["empty_64"][164] > 0 and L["empty_64"][99] > 0
    assert np.all(L["empty_65"][100:165] == 0) and np.all(L["empty_65_last"][-65:] == 0)
    assert scalar["nnz0"].nnz == 0
    assert L["row_2048"].max() == 2048 and L["row_2049"].max() == 2049 and L["row_6144"].max() == 6144
    assert set(L["len_1_2"]) == {1, 2} and set(L["len_1"]) == {1}
    for mean, lpr in ((3, 4), (12, 8), (60, 16), (150, 32), (300, 64)):
        assert M.pick_lpr(scalar[f"geom_{mean}"]) == lpr, mean
    assert np.all(scalar["even"].rowptr % 2 == 0)
    assert np.all(scalar["odd_after_0"].rowptr[1:] % 2 == 1)
    assert scalar["odd_after_0"].nnz == scalar["even"].nnz + 1


def test_run_ends_fall_on_both_residues(scalar):
    for name, want in (("ends_even", {0}), ("ends_alternate", {0, 1})):
        A = scalar[name]
        p = M.stream_plan(A)
        ends = {int(A.rowptr[r]) % 2 for r in p["rb"][1:]}
        assert ends == want, (name, ends)
        assert p["rb"][-1] == A.n_rows and A.rowptr[p["rb"][-1]] == A.nnz and A.row_len[-1] > 0
    A, B = scalar["ends_alternate"], scalar["ends_alternate_plus_1"]
    assert {A.nnz % 2, B.nnz % 2} == {0, 1}        # the last run ends on the last entry of the arrays, at either residue
    last = set()
    for X in (A, B):
        p = M.stream_plan(X)
        assert p["vec"] == 3
        last.add((int(X.rowptr[p["rb"][-1]]) - int(X.rowptr[p["rb"][-2]])) % 2)
    assert last == {0, 1}     # the last run of one ends with a whole pair at the arrays' end, the other's with an odd entry


def test_ghost_pattern_promises(scalar):
    p = M.stream_plan(scalar["ghost_edges"])
    assert M.find_interior(scalar["ghost_edges"]) == (40, 670) and p["int_b1"] > p["int_b0"] > 0
    assert p["int_b1"] < len(p["rb"]) - 1
    assert 40 in p["rb"] and 670 in p["rb"]         # the plan is cut at the interior range
    q = M.stream_plan(scalar["ghost_every_row"])
    assert M.find_interior(scalar["ghost_every_row"]) == (0, 0) and q["int_b0"] == q["int_b1"] == 0
    assert scalar["ghost_only"].n_own == 0 and scalar["ghost_only"].col.min() >= 0
    assert M.find_interior(scalar["ghost_one_row_interior_first"]) == (0, 699)


def test_stream_plan_model_properties(scalar):
    for name, A in scalar.items():
        p = M.stream_plan(A)
        if A.row_len.max(initial=0) > M.K_STREAM_NNZ:
            assert not p["ok"], name
            continue
        rb = p["rb"]
        assert p["ok"] and rb[0] == 0 and rb[-1] == A.n_rows and all(b > a for a, b in zip(rb, rb[1:]))
        assert p["rows"] <= M.K_STREAM_ROWS and p["entries"] <= M.K_STREAM_NNZ
        i0, i1 = M.find_interior(A)
        cuts = {c for c in (i0, i1) if 0 < c < A.n_rows and i1 > i0}
        for a, b in zip(rb, rb[1:-1] + [None]):   # greedy: a run that stops short of both caps stops at a cut or the end
            if b is None:
                continue
            nxt = int(A.rowptr[b + 1] - A.rowptr[a])
            assert b - a == M.K_STREAM_ROWS or nxt > M.K_STREAM_NNZ or b in cuts, (name, a, b)
    assert not M.stream_plan(scalar["row_2049"])["ok"] and not M.stream_plan(scalar["row_6144"])["ok"]
    assert M.stream_plan(scalar["row_2048"])["entries"] == 2048
    assert M.stream_plan(scalar["len_1_2"])["rows"] == 64 and M.stream_plan(scalar["len_1_2"])["entries"] == 96
    p = M.stream_plan(scalar["empty_65_last"])
    k = p["rb"]
    A = scalar["empty_65_last"]
    assert A.rowptr[k[-2]] == A.nnz                 # the last run holds no entry at all
    assert M.stream_plan(scalar["even"])["vec"] == 2 and M.stream_plan(scalar["odd_after_0"])["vec"] == 3
    assert M.stream_plan(scalar["nnz0"])["entries"] == 0 and M.stream_plan(scalar["nnz0"])["vec"] == 2


def test_row_cap_of_the_model():
    rp = np.arange(0, 201)
    assert M.build_rowblocks(rp, None, 200, 2048) == [0, 64, 128, 192, 200]
    assert M.build_rowblocks(rp, None, 200, 2048, row_cap=65) == [0, 65, 130, 195, 200]
    assert M.build_rowblocks(rp, None, 200, 2048, cuts=[10, 100]) == [0, 10, 74, 100, 164, 200]
    assert M.build_rowblocks(rp * 100, None, 200, 2048)[:3] == [0, 20, 40]
    assert M.build_rowblocks(rp * 100, rp * 100, 200, 2048)[:3] == [0, 10, 20]
    assert M.build_rowblocks(rp * 2049, None, 200, 2048) is None


def test_block_pattern_promises(blocks):
    for name, (Rr, Cc, A) in blocks.items():
        p = M.blocked_plan(A, Rr, Cc)
        t = f"blk{Rr}x{Cc}_"
        what = name[len(t):]
        if what in ("broken", f"row_{M.K_BLK_MAX + 1}"):
            assert not p["ok"], name
            if what == "broken":
                assert M.blocked_rowptr(A, Rr, Cc) is None
            else:
                assert np.diff(M.blocked_rowptr(A, Rr, Cc)).max() == M.K_BLK_MAX + 1
            continue
        assert p["ok"], name
        assert p["brp"][-1] * Rr * Cc == A.nnz and p["entries"] <= M.K_BLK_MAX and p["rows"] <= M.K_STREAM_ROWS
        if what == f"row_{M.K_BLK_MAX}":
            assert p["entries"] == M.K_BLK_MAX
        if what == "empty_tail":      # runs without a block behind the last block of the matrix
            assert sum(p["brp"][a] == p["brp"][-1] for a in p["rb"][:-1]) >= 1
        if what == "nnz0":
            assert A.nnz == 0 and len(p["rb"]) == 3
        if what == "mixed":
            assert any(p["brp"][a] == p["brp"][b] for a, b in zip(p["rb"], p["rb"][1:]))   # a whole run of empty block rows
        if what == "ghost_edges":
            assert p["int_b1"] > p["int_b0"] > 0 and p["int_b1"] < len(p["rb"]) - 1
        if what == "ghost_every_row":
            assert p["int_b0"] == p["int_b1"] == 0
    # a wrong block shape is refused as well
    assert not M.blocked_plan(blocks["blk2x1_mixed"][2], 2, 2)["ok"]
    assert not M.blocked_plan(blocks["blk1x2_mixed"][2], 2, 2)["ok"]


def test_pair_pattern_promises(pairs):
    for name, (A, B) in pairs.items():
        assert np.all(A.rowptr % 2 == 0), name
        for blocked in (False, True):
            p = M.fused_plan(A, B, blocked)
            if name == "pair_over_cap" and blocked:
                assert not p["ok"] and p["reason"] == 4
                continue
            assert p["ok"], (name, blocked)
            rb, ra, rbp = p["rb"], p["ra"], p["rb2"]
            ea = np.array([ra[b] - ra[a] for a, b in zip(rb, rb[1:])])
            eb = np.array([rbp[b] - rbp[a] for a, b in zip(rb, rb[1:])])
            assert np.all(ea + eb <= (M.K_BLK_MAX if blocked else M.K_STREAM_NNZ))
            if name == "pair_ghost_both":
                assert A.n_own < A.n_cols and B.n_own < B.n_cols and np.any(A.col >= A.n_own) and np.any(B.col >= B.n_own)
                assert A.n_cols - A.n_own != B.n_cols - B.n_own
            if name == "pair_B_empty_runs":
                assert np.any((eb == 0) & (ea > 0))
            if name == "pair_A_empty_runs":
                assert np.any((ea == 0) & (eb > 0))
            if name == "pair_both_empty_tail":
                assert ea[-1] == 0 and eb[-1] == 0
            if name == "pair_caps" and blocked:
                assert np.any((ea == M.K_BLK_MAX) & (eb == 0)) and np.any((eb == M.K_BLK_MAX) & (ea == 0))
                assert np.any((ea + eb == M.K_BLK_MAX) & (ea > 0) & (eb > 0))
            if name == "pair_caps" and not blocked:
                assert np.any((ea == M.K_STREAM_NNZ) & (eb == 0))


def test_symmetric_with_diagonal():
    A = M.symmetric_with_diagonal(M.from_lengths(M.geometric_lengths(200, 5, 1, cap=40), 200, 2))
    _valid(A)
    S = A.with_values(np.ones(A.nnz)).to_scipy()
    assert (S != S.T).nnz == 0 and np.all(S.diagonal() == 1)


def test_big_and_generator_anchors_are_valid():
    A = M.from_lengths(M.geometric_lengths(5000, 8, 1, cap=900), 1 << 14, 2)
    _valid(A)
    for name, Rr, Cc, A in M.generator_blocks(60, 20):
        _valid(A)
        assert M.blocked_plan(A, Rr, Cc)["ok"], name
        assert M.stream_plan(A)["ok"], name
