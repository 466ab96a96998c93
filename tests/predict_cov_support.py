"""The predictor's joint covariance and draws restated on the CPU (TEST INFRASTRUCTURE ONLY).

K from tests/fisher_support.kernel_ref, a Cholesky factorisation and triangular solves with scipy -- never the device's
K, L or R:  V_ref = (L^-1 K_s)^T [m, n],  Sigma_ref = K_ss - V^T V [m, m'].  Inputs are those of tests/predict_support
(the same seeds, so mu_ref and var_ref of predict_support.case_reference belong to the same points).  On these inputs
the triangular route here and the explicit-inverse route (K_ss - K_s^T inv(K) K_s) agree to <= 9.5e-13 (LIN: 3.6e-10):
the reference sits at <= 4 % of the 1e-8 bar.
"""
import functools

import numpy as np
import scipy.linalg as sla

from tests import fisher_support as fs
from tests import predict_support as ps

EPS = float(np.finfo(np.float64).eps)


def _k(name, a, b):
    tree, hyp, d, scaled, mode = ps.CASES[name]
    return fs.kernel_ref(tree, hyp, a, b, scaled, False, mode or "SIGMOID")


@functools.lru_cache(maxsize=None)
def train_factor(name, n, noise=ps.NOISE):
    """(x, y, L) of a case at n: the training set of predict_support.case_reference and the host Cholesky factor."""
    d = ps.CASES[name][2]
    x, y, _ = ps.inputs(n, 1, d, 1000 + 7 * n)
    L = sla.cholesky(_k(name, x, x) + noise * np.eye(n), lower=True)
    for a in (x, y, L):
        a.setflags(write=False)
    return x, y, L


def vt_ref(name, n, xs):
    """V_ref = (L^-1 K_s)^T [m, n]"""
    x, _, L = train_factor(name, n)
    return sla.solve_triangular(L, _k(name, x, xs), lower=True).T


def cov_ref(name, n, xa, xb=None):
    """Sigma_ref [ma, mb] between xa and xb (xb None: xa with itself)"""
    va = vt_ref(name, n, xa)
    vb = va if xb is None else vt_ref(name, n, xb)
    return _k(name, xa, xa if xb is None else xb) - va @ vb.T


@functools.lru_cache(maxsize=None)
def case_reference(name, n, m):
    """(x, y, x_new, V_ref, Sigma_ref, mu_ref, var_ref) of a case at (n, m), computed once and frozen."""
    x, y, xs, mu, var = ps.case_reference(name, n, m)
    V, S = vt_ref(name, n, xs), cov_ref(name, n, xs)
    for a in (V, S):
        a.setflags(write=False)
    return x, y, xs, V, S, mu, var


def draws_ref(name, n, m, z, add):
    """mu_ref + chol(Sigma_ref + add I) z [m, columns of z]; add = jitter (latent) or noise + jitter"""
    _, _, _, _, S, mu, _ = case_reference(name, n, m)
    return mu[:, None] + sla.cholesky(S + add * np.eye(m), lower=True) @ z
