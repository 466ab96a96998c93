"""The fitted predictor restated on the CPU (TEST INFRASTRUCTURE ONLY).

``posterior_ref``: K from tests/fisher_support.kernel_ref (every leaf and the change-point tree), a Cholesky
factorisation and triangular solves with numpy / scipy, k(x*, x*) from the kernel itself -- never the device's K, L
or R.  Inputs as the predictor's tests draw them: x ~ U[0, 10]^d, x_new ~ U[-1, 11]^d, noise 0.05, length scales
0.7 .. 1.3, so cond(K + noise I) <= 5e3 up to n = 333 and the two host routes (triangular solve here, the explicit
inverse of oracle.posterior) agree to <= 4e-14 in mu and var: the reference sits far inside the 1e-8 bar.
"""
import functools

import numpy as np
import scipy.linalg as sla

from tests import fisher_support as fs

NOISE = 0.05
BAR = 1e-8   # |got - ref| <= 1e-8 max(1, max|ref|) for mu and diag Sigma

# name -> (tree, hyperparameter list, d, scaled, change-point mode)
CASES = {
    "SE": (("SE", {}), [0.9], 1, False, None),
    "MAT52_scaled": (("MAT52", {}), [1.1, 1.6], 1, True, None),
    "RQ": (("RQ", {}), [0.8, 1.3], 1, False, None),
    "ADD(SE,PER)": (("ADD", [("SE", {}), ("PER", {})]), [0.7, 1.2, 2.5], 1, False, None),
    "MUL(SE,PER)": (("MUL", [("SE", {}), ("PER", {})]), [1.3, 1.0, 3.0], 1, False, None),
    "SE_ARD@3": (("SE", {"ard": True}), [[0.8, 1.0, 1.3]], 3, False, None),
    "LIN": (("LIN", {}), [[4.0]], 1, False, None),
    # (scaled leaves with different signal variances: k(x, x) = w_0(x)^2 sg_0 + w_1(x)^2 sg_1 steps from 1 to 2.5 at 5)
    "CP(SE,SE)": (("CP", [("SE", {}), ("SE", {})]), [5.0, 0.8, 1.0, 1.2, 2.5], 1, True, "SIGMOID"),
}
ORACLE_CASES = ("SE", "MAT52_scaled", "ADD(SE,PER)", "MUL(SE,PER)", "SE_ARD@3")   # plain SE / MAT / PER trees
NONSTATIONARY = ("LIN", "CP(SE,SE)")


def inputs(n, m, d, seed):
    """(x [n, d], y [n], x_new [m, d]); the training set depends on (n, d, seed) only, not on m"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 10.0, (n, d))
    y = np.sin(0.9 * x.sum(1)) + 0.3 * np.cos(2.1 * x[:, 0]) + 0.1 * rng.standard_normal(n)
    xs = np.random.default_rng(seed + 100003 * m).uniform(-1.0, 11.0, (m, d))
    return x, y, xs


def bar(ref):
    return BAR * max(1.0, float(np.max(np.abs(ref))))


def posterior_ref(tree, hyp, noise, x, y, xs, scaled=False, mode=None):
    """(mu [m], var [m]) of the latent posterior at xs."""
    md = mode or "SIGMOID"
    n = len(x)
    K = fs.kernel_ref(tree, hyp, x, x, scaled, False, md) + noise * np.eye(n)
    Ks = fs.kernel_ref(tree, hyp, x, xs, scaled, False, md)               # [n, m]
    kdiag = np.diag(fs.kernel_ref(tree, hyp, xs, xs, scaled, False, md))  # k(x*, x*) per point
    L = sla.cholesky(K, lower=True)
    alpha = sla.cho_solve((L, True), np.asarray(y, dtype=np.float64))
    V = sla.solve_triangular(L, Ks, lower=True)
    return Ks.T @ alpha, kdiag - np.sum(V * V, axis=0)


@functools.lru_cache(maxsize=None)
def case_reference(name, n, m, noise=NOISE):
    """(x, y, x_new, mu_ref, var_ref) of a case at (n, m), computed once and frozen."""
    tree, hyp, d, scaled, mode = CASES[name]
    x, y, xs = inputs(n, m, d, 1000 + 7 * n)
    mu, var = posterior_ref(tree, hyp, noise, x, y, xs, scaled, mode)
    for a in (x, y, xs, mu, var):
        a.setflags(write=False)
    return x, y, xs, mu, var


def log_density_ref(y_new, mean, var_with_noise):
    r = np.asarray(y_new, dtype=np.float64).reshape(-1) - mean
    return float(np.mean(-0.5 * (np.log(2.0 * np.pi) + np.log(var_with_noise) + r * r / var_with_noise)))
