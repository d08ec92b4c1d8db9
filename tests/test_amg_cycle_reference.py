"""The NumPy restatement of the V-cycle (tests/amg_cycle_reference.py), pinned on the CPU:

* closed form: on a two-level hierarchy of a 1-D Laplacian (n = 12, aggregates of three, dense coarse inverse) it is held
  against x1 = S(b, 0); x2 = x1 + P Ac^-1 R (b - A x1); x = S(b, x2) formed with dense np.longdouble matrices, within a
  running bound of the double roundings of the few dozen operations involved;
* against the oracle: oracle.Amg.apply on the same Laplacian and on problem("ns16").F, the level operators from
  tests/amg_reference.py's own aggregate / prolongator / product / transpose (level sizes asserted first), to 1e-11 — the
  figure tests/test_gpu_parity.py::test_amg_vcycle_matches_oracle holds the device to.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import amg_cycle_reference as V
from tests.util import problem

LD = np.longdouble
U = 2.0 ** -53


def _laplace1d(n):
    return sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()


def _two_level():
    n = 12
    A = _laplace1d(n)
    dinv = 1.0 / A.diagonal()
    lam = 1.1 * float(np.max(np.abs(np.linalg.eigvals((dinv[:, None] * A.toarray())))))
    agg = np.arange(n) // 3
    Phat = sp.csr_matrix((np.full(n, 1.0 / np.sqrt(3.0)), (np.arange(n), agg)), shape=(n, 4))
    P = (Phat - sp.diags((V.OMEGA / lam) * dinv) @ (A @ Phat)).tocsr()
    R = P.T.tocsr()
    Ac = (R @ A @ P).toarray()
    return [V.Level(A, dinv, lam, P, R), V.Level(sp.csr_matrix(Ac), 1.0 / np.diag(Ac), 1.0, inv=np.linalg.inv(Ac))]


class Tracked:
    """A longdouble vector with a bound on what the double computation of it may be off by: every double operation adds
    its rounding on the magnitudes it sees, |x| + err, and carries the errors of its operands along."""

    def __init__(self, v, err=None):
        self.v = np.asarray(v, dtype=LD)
        self.err = np.zeros(len(self.v), dtype=LD) if err is None else err

    @property
    def mag(self):
        return np.abs(self.v) + self.err


def _mv(M, x):
    """y = M x, rows of at most m entries: m products and m - 1 additions, gamma_m on |M| |x|."""
    Md = np.asarray(M, dtype=LD)
    m = int(np.max(np.count_nonzero(Md, axis=1)))
    g = m * U / (1 - m * U)
    aM = np.abs(Md)
    return Tracked(Md @ x.v, aM @ x.err + g * (aM @ x.mag))


def _lin(terms):
    """sum_k c_k .* v_k with coefficients exact in longdouble (their double counterparts are off by at most 8 roundings each:
    a handful of divisions and products, Amg::cheby), one rounding per product and per addition."""
    v = sum(np.asarray(c, dtype=LD) * t.v for c, t in terms)
    mag = sum(np.abs(np.asarray(c, dtype=LD)) * t.mag for c, t in terms)
    err = sum(np.abs(np.asarray(c, dtype=LD)) * t.err for c, t in terms)
    ops = 8 + 3 + len(terms)
    return Tracked(v, err + ops * U * mag)


def _closed_form(levels, b):
    L, C = levels
    A, P, R = (np.asarray(M.toarray(), dtype=LD) for M in (L.A, L.P, L.R))
    dinv = np.asarray(L.dinv, dtype=LD)
    c0, c1, c2 = V.cheby_coefficients(LD(L.lam))
    one = LD(1)
    bt = Tracked(b)

    def S(x):
        if x is None:
            w = _lin([(c0 * dinv, bt)])
            x = w
        else:
            r = _lin([(one, bt), (-one, _mv(A, x))])
            w = _lin([(c0 * dinv, r)])
            x = _lin([(one, x), (one, w)])
        r = _lin([(one, bt), (-one, _mv(A, x))])
        w = _lin([(c1, w), (c2 * dinv, r)])
        return _lin([(one, x), (one, w)])

    x1 = S(None)
    r = _lin([(one, bt), (-one, _mv(A, x1))])
    xc = _mv(C.inv, _mv(R, r))
    x2 = _lin([(one, x1), (one, _mv(P, xc))])
    return S(x2)


def test_two_level_cycle_equals_the_closed_form():
    levels = _two_level()
    assert levels[0].P.shape == (12, 4) and levels[1].inv.shape == (4, 4)
    rng = np.random.default_rng(5)
    for trial in range(4):
        b = rng.standard_normal(12)
        x = V.vcycle(levels, b)
        ref = _closed_form(levels, b)
        diff = np.abs(np.asarray(x, dtype=LD) - ref.v)
        assert np.all(diff <= ref.err), (trial, float(np.max(diff / ref.err)))
        # the bound is one of roundings: it pins the cycle harder than the 1e-11 the comparison with the oracle holds
        assert float(np.max(ref.err)) < 1e-11 * float(np.max(np.abs(ref.v)))
        # and the cycle is a useful preconditioner (the criterion the device test holds: 0.8)
        assert np.linalg.norm(b - levels[0].A @ x) < 0.8 * np.linalg.norm(b)


def test_a_wrong_cycle_leaves_the_bound():
    """The bound tells cycles apart: without the second smoother step of the post-smoothing the result is far outside."""
    levels = _two_level()
    b = np.random.default_rng(6).standard_normal(12)
    ref = _closed_form(levels, b)
    L = levels[0]
    x = V.cheby(L, b)
    x = x + L.P @ (levels[1].inv @ (L.R @ (b - L.A @ x)))
    c0 = V.cheby_coefficients(L.lam)[0]
    x = x + c0 * L.dinv * (b - L.A @ x)
    assert np.any(np.abs(np.asarray(x, dtype=LD) - ref.v) > 1e6 * ref.err)


def _oracle_apply(A, b):
    from oracle import oracle as O
    A = A.tocsr()
    A.sort_indices()
    M = O.Amg(O.CsrHolder(A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, A.shape[0], A.shape[1]))
    return M.levels(), M.apply(b)


@pytest.mark.parametrize("name", ["laplace1d", "ns16"])
def test_cycle_matches_the_oracle(name):
    A = _laplace1d(600) if name == "laplace1d" else problem("ns16").F.to_scipy()
    levels = V.build(A)
    b = np.random.default_rng(77).standard_normal(A.shape[0])
    olev, xo = _oracle_apply(A, b)
    assert [(L.n, L.A.nnz) for L in levels] == [(r, z) for r, z, _ in olev], "the reference set-up reproduces the oracle's levels"
    assert len(levels) >= 2
    for L, (_, _, olam) in zip(levels, olev):
        assert abs(L.lam - olam) <= 1e-12 * olam
    x = V.vcycle(levels, b)
    assert np.linalg.norm(x - xo) <= 1e-11 * np.linalg.norm(xo)
