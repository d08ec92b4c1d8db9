"""NumPy / SciPy restatement of the velocity AMG's V-cycle (csrc/nsk_amg.cpp: Amg::vcycle, Amg::cheby) on GIVEN level
operators — the cycle alone, whoever built the hierarchy (the device through nsk_debug_amg_level, the functions of
tests/amg_reference.py, a hierarchy written down by hand).

A level is `Level(A, dinv, lam, P, R, inv)`: A, P, R scipy CSR in double (P, R None on the last level), dinv the inverse
diagonal, lam the eigenvalue estimate the smoother uses, inv the dense inverse of the last level (None: it is smoothed
twice instead, as the library does above 2 048 rows).

    smoother S(b, x), degree-2 Chebyshev in D^-1 A on [lam / 20, lam]  (Amg::cheby):
        theta = (lam + lam / 20) / 2, delta = (lam - lam / 20) / 2, sigma = theta / delta, rho = 1 / sigma
        zero guess:  w = (1 / theta) dinv .* b ;            x = w
        otherwise:   w = (1 / theta) dinv .* (b - A x) ;    x = x + w
        rho' = 1 / (2 sigma - rho)
        w = (rho' rho) w + (2 rho' / delta) dinv .* (b - A x) ;  x = x + w
    cycle(l, b)  (Amg::vcycle):
        last level:  x = inv b, or x = S(b, S(b, 0))
        else:        x = S(b, 0) ; r = b - A x ; x_c = cycle(l + 1, R r) ; x = x + P x_c ; x = S(b, x)

`rounded(levels)` gives the same hierarchy with the values of every A, P and R rounded through float32 — what
NSK_OPT_AMG_PRECISION = 32 stores; dinv, lam and inv stay as they are.  `build(A)` is the set-up itself from the exact
functions of tests/amg_reference.py (power iteration included), for the comparison with the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

CHEBY_ALPHA = 20.0
COARSE_MAX = 128
DENSE_LIMIT = 2048
MAX_LEVELS = 10
OMEGA = 4.0 / 3.0
EIG_ITS = 10
EIG_BOOST = 1.1


@dataclass
class Level:
    A: object
    dinv: np.ndarray
    lam: float
    P: Optional[object] = None
    R: Optional[object] = None
    inv: Optional[np.ndarray] = None

    @property
    def n(self):
        return self.A.shape[0]


def cheby_coefficients(lam):
    """(1 / theta, rho' rho, 2 rho' / delta) with the operations of Amg::cheby, in the type of lam."""
    lmax, lmin = lam, lam / CHEBY_ALPHA
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    rho_new = 1.0 / (2.0 * sigma - rho)
    return 1.0 / theta, rho_new * rho, 2.0 * rho_new / delta


def cheby(L, b, x=None):
    """S(b, x); x None: the zero guess (x is never read)."""
    c0, c1, c2 = cheby_coefficients(float(L.lam))
    if x is None:
        w = c0 * L.dinv * b
        x = w.copy()
    else:
        w = c0 * L.dinv * (b - L.A @ x)
        x = x + w
    w = c1 * w + c2 * L.dinv * (b - L.A @ x)
    return x + w


def vcycle(levels, b, l=0):
    L = levels[l]
    b = np.asarray(b, dtype=np.float64)
    if L.P is None:
        if L.inv is not None:
            return L.inv @ b
        return cheby(L, b, cheby(L, b))
    x = cheby(L, b)
    r = b - L.A @ x
    xc = vcycle(levels, L.R @ r, l + 1)
    x = x + L.P @ xc
    return cheby(L, b, x)


def apply_shards(shards, offsets, b):
    """The block-Jacobi application over diagonal shards: shards[k] the levels of rows offsets[k] .. offsets[k + 1]."""
    x = np.zeros(len(b))
    for k, levels in enumerate(shards):
        x[offsets[k]:offsets[k + 1]] = vcycle(levels, b[offsets[k]:offsets[k + 1]])
    return x


def _round32(M):
    if M is None:
        return None
    M = M.copy()
    with np.errstate(over="ignore"):
        M.data = M.data.astype(np.float32).astype(np.float64)
    return M


def rounded(levels):
    return [Level(_round32(L.A), L.dinv, L.lam, _round32(L.P), _round32(L.R), L.inv) for L in levels]


def estimate_lambda(A, dinv):
    """1.1 x |(D^-1 A)^k x0| / |(D^-1 A)^(k-1) x0| after ten steps from the set-up's start vector."""
    from tests.amg_reference import start_vector
    x = start_vector(A.shape[0])
    x = x / np.sqrt(x @ x)
    nrm = 0.0
    for _ in range(EIG_ITS):
        y = dinv * (A @ x)
        nrm = np.sqrt(y @ y)
        x = y / nrm
    return EIG_BOOST * nrm


def build(A):
    """The hierarchy under the scipy matrix A with the set-up's rules (nsk_amg.cpp: Amg::build) and the exact functions of
    tests/amg_reference.py; the dense inverse from numpy."""
    from tests import amg_reference as R
    levels = []
    M = R.from_scipy(A)
    for l in range(MAX_LEVELS + 1):
        As = M.scipy()
        n = M.n_rows
        ad, dinv = R.diag(M)
        lam = estimate_lambda(As, dinv)
        nc = 0
        if n > COARSE_MAX and l + 1 < MAX_LEVELS:
            G = R.aggregate(M, ad)
            nc = G.nc
        if nc <= 0 or nc >= n:
            levels.append(Level(As, dinv, lam, inv=np.linalg.inv(As.toarray()) if n <= DENSE_LIMIT else None))
            return levels
        P = R.prolongator(M, G.agg, G.pw, dinv, OMEGA / lam)
        Rt = R.transpose(P)
        Ac = R.product(Rt, R.product(M, P))
        levels.append(Level(As, dinv, lam, P.scipy(), Rt.scipy()))
        M = Ac
    raise AssertionError("more levels than the set-up allows")
