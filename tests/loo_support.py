"""Restatement of leave-one-out cross-validation and its gradient (CPU, fp64) for the LOO tests.

K = k(X, X) + s2 I, alpha = K^-1 y, d_i = (K^-1)_ii; the prediction of point i from the other n - 1 points is
mu_i = y_i - alpha_i / d_i with variance 1 / d_i (Rasmussen & Williams 5.4.2).  Two losses f = sum_i phi(alpha_i, d_i):
    LPD  phi = 1/2 log 2 pi - 1/2 log d + alpha^2 / (2 d)    (minus the LOO log predictive density, minus R&W eq. 5.13)
    MSE  phi = (alpha / d)^2 / n
Three routes:
- ``loo_autodiff``: torch reverse mode through the whole expression -- the reference value and gradient;
- ``loo_formula``: the cotangent the device forms, G = -1/2 (alpha u^T + u alpha^T) - K^-1 diag(phi_d) K^-1 with
  u = K^-1 phi_alpha, contracted with dK / d theta (and tr G for the noise);
- ``loo_refits``: n explicit fits on n - 1 points each, the definition itself.
Gradients are flat vectors over the hyperparameter entries in list order, the noise last.  Under the project's scaled
flag every leaf of a tree carries a signal variance.
"""
import math

import numpy as np
import torch

from tests import mse_support as ms

F64 = torch.float64
LPD, MSE = 0, 1          # GPK_LOO_LPD / GPK_LOO_MSE
VALUE_REL = ms.VALUE_REL
GRAD_TOL = ms.GRAD_TOL
PRED_TOL = 1e-8          # |mu - mu_ref| <= 1e-8 max(1, |mu_ref|_max), the same for the variances
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)

SE, PER = ("SE", {}), ("PER", {})
# name: (tree, hyperparameter list, d, scaled)
PROGRAMS = {
    "SE": (SE, [0.3], 1, False),
    "ADD_SE_PER_scaled": (("ADD", [SE, PER]), [0.3, 2.0, 0.9, 0.5, 1.5], 1, True),
    "MUL_SE_PER": (("MUL", [SE, PER]), [0.5, 0.8, 0.6], 1, False),
    "SE_ard_d3": (("SE", {"ard": True}), [[0.4, 0.7, 1.1]], 3, False),
}


def _operands(hyp, noise, x, y):
    params = [torch.tensor(np.asarray(h, dtype=np.float64), dtype=F64, requires_grad=True) for h in hyp]
    nz = torch.tensor(float(noise), dtype=F64, requires_grad=True)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return params, nz, t(x), t(y).reshape(-1, 1)


def _phi(loss, alpha, d):
    """(phi, phi_alpha, phi_d) per point."""
    n = alpha.shape[0]
    if loss == LPD:
        return (HALF_LOG_2PI - 0.5 * torch.log(d) + alpha * alpha / (2.0 * d), alpha / d,
                -1.0 / (2.0 * d) - alpha * alpha / (2.0 * d * d))
    if loss == MSE:
        return (alpha / d) ** 2 / n, 2.0 * alpha / (n * d * d), -2.0 * alpha * alpha / (n * d ** 3)
    raise ValueError(loss)


def loo_autodiff(tree, hyp, noise, x, y, loss, scaled=False):
    """(f, g, mu [n], var [n]): the reference by torch reverse mode through K^-1."""
    params, nz, X, Y = _operands(hyp, noise, x, y)
    K = ms.kmat(tree, params, X, X, scaled) + nz * torch.eye(X.shape[0], dtype=F64)
    Kinv = torch.cholesky_inverse(torch.linalg.cholesky(K))
    alpha = (Kinv @ Y).reshape(-1)
    d = torch.diagonal(Kinv)
    f = torch.sum(_phi(loss, alpha, d)[0])
    grads = torch.autograd.grad(f, params + [nz], allow_unused=True)
    mu = (Y.reshape(-1) - alpha / d).detach().numpy()
    return float(f.detach()), ms._flat(params + [nz], grads), mu, (1.0 / d).detach().numpy()


def loo_formula(tree, hyp, noise, x, y, loss, scaled=False):
    """(f, g): the device's formula, sum_ij G_ij dK_ij / d theta with G built from K^-1, alpha, phi_alpha, phi_d."""
    params, nz, X, Y = _operands(hyp, noise, x, y)
    K = ms.kmat(tree, params, X, X, scaled) + nz * torch.eye(X.shape[0], dtype=F64)
    with torch.no_grad():
        Kinv = torch.cholesky_inverse(torch.linalg.cholesky(K))
        alpha = (Kinv @ Y).reshape(-1)
        d = torch.diagonal(Kinv)
        phi, pa, pd = _phi(loss, alpha, d)
        u = Kinv @ pa
        G = -0.5 * (torch.outer(alpha, u) + torch.outer(u, alpha)) - Kinv @ torch.diag(pd) @ Kinv
    leaves = params + [nz]
    grads = torch.autograd.grad(torch.sum(K * G), leaves, allow_unused=True)
    return float(torch.sum(phi)), ms._flat(leaves, grads)


def loo_refits(tree, hyp, noise, x, y, loss, scaled=False):
    """(f, mu [n], var [n]) from n explicit refits: point i predicted by the GP fitted to the other n - 1 points
    (predictive variance including the noise)."""
    params, nz, X, Y = _operands(hyp, noise, x, y)
    n = X.shape[0]
    mu, var = np.zeros(n), np.zeros(n)
    with torch.no_grad():
        K = ms.kmat(tree, params, X, X, scaled) + nz * torch.eye(n, dtype=F64)
        for i in range(n):
            keep = [j for j in range(n) if j != i]
            if not keep:
                mu[i], var[i] = 0.0, float(K[i, i])
                continue
            Kk = K[keep][:, keep]
            ks = K[keep, i].reshape(-1, 1)
            L = torch.linalg.cholesky(Kk)
            mu[i] = float((ks.T @ torch.cholesky_solve(Y[keep], L))[0, 0])
            var[i] = float(K[i, i] - (ks.T @ torch.cholesky_solve(ks, L))[0, 0])
    r = np.asarray(Y).reshape(-1) - mu
    if loss == LPD:
        f = float(np.sum(HALF_LOG_2PI + 0.5 * np.log(var) + r * r / (2.0 * var)))
    else:
        f = float(np.mean(r * r))
    return f, mu, var


def nlml(tree, hyp, noise, x, y, scaled=False):
    """-LML of the same model (the n = 1 known answer: f_LPD equals it)."""
    params, nz, X, Y = _operands(hyp, noise, x, y)
    with torch.no_grad():
        K = ms.kmat(tree, params, X, X, scaled) + nz * torch.eye(X.shape[0], dtype=F64)
        L = torch.linalg.cholesky(K)
        fit = float((Y.T @ torch.cholesky_solve(Y, L))[0, 0])
        return 0.5 * fit + float(torch.sum(torch.log(torch.diagonal(L)))) + X.shape[0] * HALF_LOG_2PI


def grad_bar(g_ref):
    return GRAD_TOL * max(1.0, float(np.max(np.abs(g_ref))))


def assert_value_close(f, f_ref, what="loo"):
    rel = abs(f - f_ref) / abs(f_ref)
    print("%s value %.12e ref %.12e rel %.2e" % (what, f, f_ref, rel))
    assert rel <= VALUE_REL, (f, f_ref)


def assert_grad_close(g, g_ref, what="loo"):
    g, g_ref = np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(g_ref, dtype=np.float64).reshape(-1)
    assert g.shape == g_ref.shape
    err = float(np.max(np.abs(g - g_ref)))
    print("%s gradient: max |g - g_ref| = %.3e, bar %.3e, |g_ref|max %.3e" % (what, err, grad_bar(g_ref),
                                                                              float(np.max(np.abs(g_ref)))))
    assert err <= grad_bar(g_ref), (g, g_ref)


def assert_pred_close(v, v_ref, what):
    v, v_ref = np.asarray(v, dtype=np.float64).reshape(-1), np.asarray(v_ref, dtype=np.float64).reshape(-1)
    assert v.shape == v_ref.shape
    bar = PRED_TOL * max(1.0, float(np.max(np.abs(v_ref))))
    err = float(np.max(np.abs(v - v_ref)))
    print("%s: max abs error %.3e, bar %.3e" % (what, err, bar))
    assert err <= bar


def inputs(n, d, seed, amplitude=3.0):
    """n points uniform in [0, 1]^d (sorted along the first axis for d = 1), smooth targets plus a little noise."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    if d == 1:
        x = np.sort(x, axis=0)
    fun = amplitude * (np.sin(5.0 * x.sum(axis=1)) + 0.5 * np.cos(11.0 * x[:, 0]))
    return x, fun + 0.3 * rng.standard_normal(n)


def flat(hyp):
    return np.concatenate([np.atleast_1d(np.asarray(h, dtype=np.float64)).reshape(-1) for h in hyp])


# ----------------------------------------------------------------------------------------- the fitter's problem
FIT_START_SEED = 2


def fit_problem():
    """(x [96, 1], y [96]): the training part of tests/mse_support.fit_problem (one draw of an SE prior, length scale
    0.12, plus noise 0.05, over a grid of 96 points)."""
    x, y, _, _ = ms.fit_problem()
    return x, y


def objective(tree, x, y, loss, scaled=False):
    """v [n_hyp + 1] -> (f, g) of the reference; (inf, NaN) where K + noise I is not positive definite."""
    def fn(v):
        try:
            f, g, _, _ = loo_autodiff(tree, list(v[:-1]), v[-1], x, y, loss, scaled)
            if not np.isfinite(f):
                raise ValueError
            return f, g
        except Exception:
            return np.inf, np.full(len(v), np.nan)
    return fn
