"""The host references of tests/test_gpu_krylov_kernels.py, checked without a GPU: the exact dot product against rational
arithmetic, and the two Gram-Schmidt references against each other on the basis the GPU test uses."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import krylov_reference as R


def _fraction_dot(x, y):
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(x, y)), Fraction(0))


def _wide_range(n, seed):
    """Entries from ~1e-300 to ~1e300 with random signs, paired so that every product stays inside the exact domain."""
    rng = np.random.default_rng(seed)
    ex = rng.integers(-996, 996, n)
    ey = np.clip(rng.integers(-960, 1000, n) - ex, -996, 995)
    ey = np.where(ex + ey < -950, -950 - ex, ey)
    x = rng.uniform(1.0, 2.0, n) * np.exp2(ex.astype(float)) * rng.choice([-1.0, 1.0], n)
    y = rng.uniform(1.0, 2.0, n) * np.exp2(ey.astype(float)) * rng.choice([-1.0, 1.0], n)
    return x, y


def test_two_product_is_exact():
    x, y = _wide_range(2000, 1)
    p, e = R.two_product(x, y)
    for a, b, pp, ee in zip(x, y, p, e):
        assert Fraction(float(pp)) + Fraction(float(ee)) == Fraction(float(a)) * Fraction(float(b))


@pytest.mark.parametrize("seed", range(6))
def test_exact_dot_is_correctly_rounded_over_a_wide_range(seed):
    x, y = _wide_range(64 + 37 * seed, seed)
    assert R.exact_dot(x, y) == float(_fraction_dot(x, y))


def test_exact_dot_cancellation():
    """Sums that cancel to exactly zero, and to a remainder far below every product (np.dot gets neither)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(500) * np.exp2(rng.integers(-300, 300, 500).astype(float))
    y = rng.standard_normal(500)
    xx, yy = np.concatenate([x, x]), np.concatenate([y, -y])
    assert R.exact_dot(xx, yy) == 0.0
    tiny = 3.0 * 2.0 ** -700
    x3, y3 = np.append(xx, tiny), np.append(yy, 1.0)
    assert R.exact_dot(x3[::-1], y3[::-1]) == tiny
    assert R.exact_dot([1e300, 1.0, -1e300], [1.0, 1e-280, 1.0]) == 1e-280
    # a sum whose correct rounding needs every bit of the error terms
    a = np.array([1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0])
    b = np.array([1.0 + 2.0 ** -52, 1.0 + 2.0 ** -53, 1.0])
    assert R.exact_dot(a, b) == float(_fraction_dot(a, b))


def test_exact_dot_refuses_inputs_it_cannot_split():
    with pytest.raises(ValueError):
        R.exact_dot([1e305], [1e-10])
    with pytest.raises(ValueError):
        R.exact_dot([1e-200], [1e-200])


def test_exact_dot_of_integers_matches_int64():
    n = 100_000
    x = np.ones(n)
    y = np.arange(1, n + 1, dtype=np.float64)
    assert R.exact_dot(x, y) == float(np.arange(1, n + 1, dtype=np.int64).sum())


@pytest.mark.parametrize("m", [2, 7, 17])
def test_mgs_and_cgs_references_differ_on_the_nearly_parallel_basis(m):
    n = 4097
    w, V = R.nearly_parallel_case(n, m)
    hm, wm, nm = R.mgs(w, V)
    hc, wc, nc = R.cgs(w, V)
    assert hm[0] == hc[0]
    # every later coefficient differs at O(1)
    assert np.all(np.abs(hm[1:] - hc[1:]) > 1.0)
    # MGS leaves w orthogonal to the last basis vector, CGS does not come close
    assert abs(R.exact_dot(wm, V[-1])) < 1e-10 * np.linalg.norm(w)
    assert abs(R.exact_dot(wc, V[-1])) > 1e-2 * np.linalg.norm(w)


def test_gram_schmidt_references_agree_on_an_orthonormal_basis():
    n, m = 2049, 9
    V = R.orthonormal_basis(n, m)
    w = np.random.default_rng(6).standard_normal(n)
    hm, wm, nm = R.mgs(w, V)
    hc, wc, nc = R.cgs(w, V)
    assert np.allclose(hm, hc, rtol=0, atol=1e-13 * np.linalg.norm(w))
    q, r = R.pythagoras(hc, R.exact_dot(w, w))
    assert abs(q - nc) <= 1e-12 * R.exact_dot(w, w)
    assert r == math.sqrt(q)
    assert R.pythagoras([2.0], 3.0) == (0.0, 0.0)   # a negative difference clamps to 0


def test_cg_scalars_reference():
    sc = [4.0, 2.0, 9.0, 0.0, 0.0, 0.0, 0.0]
    assert list(R.cg_fused_scalars(sc, 1)[3:]) == [4.0, 2.0, 0.0, 3.0]
    sc = [1.0, 3.0, 16.0, 2.0, 0.5, 0.0, 0.0]
    out = R.cg_fused_scalars(sc, 0)
    beta = 1.0 / 2.0
    assert out[5] == beta and out[4] == 1.0 / (3.0 - beta * 1.0 / 0.5) and out[6] == 4.0


def test_cheby_reference_ignores_w_when_c1_is_zero():
    w = np.array([np.nan, np.inf, 1.0])
    wn, xn = R.cheby_step(0.0, 2.0, np.ones(3), np.array([1.0, 2.0, 3.0]), w, np.zeros(3), 0)
    assert np.array_equal(wn, [2.0, 4.0, 6.0]) and np.array_equal(xn, wn)
