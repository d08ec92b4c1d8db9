"""The host references of tests/krylov_f32_reference.py, checked without a GPU.

A model of the two kernels that follows csrc/nsk_kernels.hip operation by operation — the quads of a thread trip after
trip, one fused multiply-add per entry (formed exactly with rationals and rounded once), the tail entries on thread 0 of
workgroup 0, reduce_finish's shuffles, wavefront sums and last-workgroup fold — is held against the exact sums: it must
sit inside the bounds the module counts, and reproduce integer data exactly.  So a bound that was counted too tight, or a
reference that is not exact, fails here before any GPU test uses it."""
from fractions import Fraction

import numpy as np
import pytest

from tests import krylov_f32_reference as F
from tests import krylov_reference as R


def fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))   # int / int division rounds correctly


def wave_sum(v):
    """subwave_sum<64> as lane 0 sees it: v += shfl_down(v, off) for off = 32 .. 1."""
    v = np.array(v, dtype=np.float64)
    off = 32
    while off:
        v[:64 - off] = v[:64 - off] + v[off:64]
        off //= 2
    return v[0]


def block_sum(vals):
    """1024 per-thread values -> the workgroup's partial: 16 wavefront sums added in order from 0.0."""
    s = 0.0
    for wv in range(F.THREADS // 64):
        s += wave_sum(vals[64 * wv:64 * wv + 64])
    return s


def model_dot(w, v):
    """multi_dot_f32_kernel + reduce_finish for one accumulator."""
    n = len(w)
    G, nq = F.grid_quads(n), n >> 2
    partials = []
    for b in range(G):
        acc = np.zeros(F.THREADS)
        for t in range(F.THREADS):
            i, a = b * F.THREADS + t, 0.0
            while i < nq:
                for e in range(4 * i, 4 * i + 4):
                    a = fma(w[e], v[e], a)
                i += G * F.THREADS
            if b == 0 and t == 0:
                for e in range(n & ~3, n):
                    a = fma(w[e], v[e], a)
            acc[t] = a
        partials.append(block_sum(acc))
    last = np.zeros(F.THREADS)
    last[:G] = 0.0 + np.array(partials)
    return block_sum(last)


def model_axpy(w, V, h):
    out = np.array(w, dtype=np.float64)
    for e in range(len(out)):
        for hk, v in zip(h, V):
            out[e] = fma(-hk, v[e], out[e])
    return out


def random_case(n, m, seed):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n)
    V = [rng.standard_normal(n).astype(np.float32).astype(np.float64) for _ in range(m)]
    return w, V


def test_grid_trips_and_depth_at_the_sizes_the_gpu_tests_use():
    assert [F.grid_quads(n) for n in (1, 3, 4, 16384, 16388, 4_194_304, 8_575_417)] == [1, 1, 1, 1, 2, 256, 256]
    assert [F.trips(n) for n in (1, 4, 4096, 4100, 20_001, 1 << 20, 4_194_304, 4_194_308, 8_575_417)] == \
        [0, 1, 1, 2, 3, 4, 4, 5, 9]
    assert F.depth(8_575_417) == 84 and F.depth(3) == 48


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1001, 4100, 20_001])
def test_the_kernel_model_sits_inside_the_counted_bound(n):
    w, V = random_case(n, 2, 100 + n)
    for v in V + [w]:                      # w itself: the w.w rider and the norm
        s, want = model_dot(w, v), R.exact_dot(w, v)
        assert abs(s - want) <= F.dot_bound(n, w, v), (n, s, want)
    if n > 100:                            # (the model does round: the check above is not vacuous)
        errs = [abs(model_dot(w, v) - R.exact_dot(w, v)) for v in V]
        assert max(errs) > 0.0


@pytest.mark.parametrize("n", [3, 1000, 4099, 16_390])
def test_integer_data_is_reproduced_exactly(n):
    rng = np.random.default_rng(n)
    w = rng.integers(-1000, 1001, n).astype(np.float64)
    V = [rng.integers(-1000, 1001, n).astype(np.float64) for _ in range(3)]
    assert all(F.is_f32(v) for v in V)
    for v in V + [w]:
        assert model_dot(w, v) == float(F.int_dot(w, v)) == R.exact_dot(w, v)
    h = [3.0, -2.0, 5.0]
    want = w - sum(hk * v for hk, v in zip(h, V))
    ref, scale = F.axpy(w, V, h)
    assert np.array_equal(ref, want) and np.array_equal(model_axpy(w, V, h), want)
    assert np.array_equal(scale, np.abs(w) + sum(abs(hk) * np.abs(v) for hk, v in zip(h, V)))


@pytest.mark.parametrize("m", [1, 8, 30])
def test_the_update_model_sits_inside_the_counted_bound(m):
    w, V = random_case(257, m, 7 * m)
    h = [0.5 - 0.03 * k for k in range(m)]
    ref, scale = F.axpy(w, V, h)
    got = model_axpy(w, V, h)
    assert np.all(np.abs(got - ref) <= F.axpy_bound(m, scale))
    exact = [float(Fraction(float(w[e])) - sum(Fraction(hk) * Fraction(float(v[e])) for hk, v in zip(h, V)))
             for e in range(len(w))]
    assert np.all(np.abs(ref - np.array(exact)) <= R.U * scale)      # the reference rounds once


def test_normalise_rounds_to_nearest_even_and_widens_exactly():
    x = np.array([1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, -1.0 - 2.0 ** -24,
                  1e-40, 0.0, 3.0e38])
    y, v, vw = F.normalise(x, 1.0)
    assert np.array_equal(y, x)
    assert v.dtype == np.float32 and vw.dtype == np.float64
    want = [1.0, 1.0, 1.0 + 2.0 ** -22, 1.0 + 2.0 ** -23, -1.0, float(np.float32(1e-40)), 0.0, float(np.float32(3.0e38))]
    assert np.array_equal(vw, np.array(want)) and np.array_equal(v.astype(np.float64), vw)
    y, v, vw = F.normalise(np.array([1.0, 2.0, 3.0]), 3.0)
    assert np.array_equal(y, (1.0 / 3.0) * np.array([1.0, 2.0, 3.0]))    # the scalar first, then one product per entry
    assert np.array_equal(F.round_f32(y), vw) and F.is_f32(vw) and not F.is_f32(y)


def test_launch_counts_of_the_three_settings():
    assert [F.launches(1, m) for m in (1, 8, 9, 30, 32)] == [1, 1, 1, 1, 1]
    assert [F.launches(2, m) for m in (1, 16, 17, 30, 32)] == [1, 1, 2, 2, 2]
    assert [F.launches(0, m) for m in (1, 8, 9, 16, 17, 30)] == [1, 1, 2, 2, 3, 4]
    # the rider takes a spare output of the last piece, else a launch of its own
    assert [F.launches(0, m, True) for m in (7, 8, 15, 16, 30)] == [1, 2, 2, 3, 4]
    assert [F.launches(1, m, True) for m in (1, 30, 31, 32)] == [1, 1, 1, 2]


def test_the_column_reference_agrees_between_its_two_norms():
    n, m = 2000, 6
    V = [F.round_f32(v) for v in R.orthonormal_basis(n, m)]
    w = np.random.default_rng(5).standard_normal(n)
    h1, w1, _, q1, n1 = F.cgs_f32(w, V, one_red=False)
    h2, w2, _, q2, n2 = F.cgs_f32(w, V, one_red=True)
    assert np.array_equal(h1, h2) and np.array_equal(w1, w2)
    # V is orthonormal to fp32 rounding only (~6e-8 per pair): Pythagoras and the direct norm agree to that
    assert abs(q1 - q2) <= 1e-5 * q1 and abs(n1 - n2) <= 1e-5 * n1
