"""Restatement of the held-out mean squared error and its gradient (CPU, fp64) for the MSE tests.

f = mean((K_s^T (K + s2 I)^-1 y - y*)^2).  Two routes to its gradient:
- ``mse_autodiff``: torch reverse mode through the whole expression -- the reference gradient, built from
  oracle.gp_autodiff.kernel_matrix_t (LIN / RQ leaves and change-point trees: the differentiable restatements of
  lin_support, rq_support and cp_support, which the oracle does not know);
- ``mse_formula``: the formula the device implements, with r = mu - y*, alpha = K^-1 y, q = K^-1 K_s r:
      d f / d theta = (2/m) [ sum_it alpha_i r_t dK_s,it - sum_ij q_i alpha_j dK_ij ],  d f / d s2 = -(2/m) q^T alpha,
  the two sums returned separately as well (the K_s term and the K term), so that a test can assert its bar sees each.
Gradients are flat vectors over the hyperparameter entries in list order, the noise last.
"""
import numpy as np
import torch

from oracle import gp_autodiff as ad
from tests import cp_support, lin_support, rq_support

F64 = torch.float64
VALUE_REL = 1e-8   # value bar: rel < 1e-8 against oracle.gp_oracle.mse (test_gpu_strategies / test_gpu_segmented)
GRAD_TOL = 1e-7    # gradient bar: |g - g_ref| <= 1e-7 max(1, |g_ref|_max) at noise >= 1e-2 (test_gpu_grad)


def n_entries(tree, scaled=False):
    """hyperparameter list entries of a tree (LIN: its offset vector is one entry)."""
    op, arg = tree
    if op in ("ADD", "MUL"):
        return sum(n_entries(c, scaled) for c in arg)
    if op == "CP":
        return cp_support.n_entries(tree, scaled, 1)
    base = {"LIN": 1, "RQ": 2, "PER": 2}.get(op, 1)
    return base + (1 if scaled else 0)


def has_op(tree, name):
    op, arg = tree
    return op == name or (op in ("ADD", "MUL", "CP") and any(has_op(c, name) for c in arg))


def kmat(tree, params, A, B, scaled=False, mode="INDICATOR"):
    """The kernel program as a differentiable torch matrix [len(A), len(B)]."""
    op, arg = tree
    if has_op(tree, "CP"):
        return cp_support.cp_torch(tree, list(params), A, B, mode, scaled)
    if op in ("ADD", "MUL"):
        idx, res = 0, None
        for c in arg:
            k = n_entries(c, scaled)
            m = kmat(c, params[idx:idx + k], A, B, scaled, mode)
            idx += k
            res = m if res is None else (res + m if op == "ADD" else res * m)
        return res
    if op == "LIN":
        return lin_support.lin_torch(list(params), A, B, scaled)
    if op == "RQ":
        return rq_support.rq_torch(list(params), A, B, scaled)
    return ad.kernel_matrix_t(tree, list(params), A, B, scaled)


def _operands(hyp, noise, x, y, xs, ys):
    params = [torch.tensor(np.asarray(h, dtype=np.float64), dtype=F64, requires_grad=True) for h in hyp]
    nz = torch.tensor(float(noise), dtype=F64, requires_grad=True)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    return params, nz, t(x), t(y).reshape(-1, 1), t(xs), t(ys).reshape(-1, 1)


def _flat(params, grads):
    parts = [np.zeros(p.numel()) if g is None else g.detach().numpy().reshape(-1) for p, g in zip(params, grads)]
    return np.concatenate(parts) if parts else np.zeros(0)


def mse_autodiff(tree, hyp, noise, x, y, xs, ys, scaled=False, mode="INDICATOR"):
    """(f, g): the reference value and gradient (noise last) by torch reverse mode."""
    params, nz, X, Y, Xs, Ys = _operands(hyp, noise, x, y, xs, ys)
    K = kmat(tree, params, X, X, scaled, mode) + nz * torch.eye(X.shape[0], dtype=F64)
    Ks = kmat(tree, params, X, Xs, scaled, mode)
    L = torch.linalg.cholesky(K)
    alpha = torch.cholesky_solve(Y, L)
    f = torch.mean((Ks.T @ alpha - Ys) ** 2)
    grads = torch.autograd.grad(f, params + [nz], allow_unused=True)
    return float(f.detach()), _flat(params + [nz], grads)


def mse_formula(tree, hyp, noise, x, y, xs, ys, scaled=False, mode="INDICATOR"):
    """(f, g, g_K, g_Ks): the device's formula; g = g_K + g_Ks (the noise entry lives in g_K)."""
    params, nz, X, Y, Xs, Ys = _operands(hyp, noise, x, y, xs, ys)
    m = Xs.shape[0]
    K = kmat(tree, params, X, X, scaled, mode) + nz * torch.eye(X.shape[0], dtype=F64)
    Ks = kmat(tree, params, X, Xs, scaled, mode)
    with torch.no_grad():
        L = torch.linalg.cholesky(K)
        z = torch.linalg.solve_triangular(L, Y, upper=False)
        V = torch.linalg.solve_triangular(L, Ks, upper=False).T        # K_s^T L^-T
        r = V @ z - Ys
        alpha = torch.linalg.solve_triangular(L.T, z, upper=True)
        q = torch.linalg.solve_triangular(L.T, V.T @ r, upper=True)
        f = float(torch.mean(r * r))
    leaves = params + [nz]
    gK = torch.autograd.grad(torch.sum(K * (q @ alpha.T)), leaves, allow_unused=True)
    gKs = torch.autograd.grad(torch.sum(Ks * (alpha @ r.T)), leaves, allow_unused=True)
    g_k = -(2.0 / m) * _flat(leaves, gK)
    g_ks = (2.0 / m) * _flat(leaves, gKs)
    return f, g_k + g_ks, g_k, g_ks


def grad_bar(g_ref):
    return GRAD_TOL * max(1.0, float(np.max(np.abs(g_ref))))


def assert_terms_visible(g_ref, g_k, g_ks):
    """On the reference alone: dropping (or mis-signing) the K term, the K_s term or the noise partial moves the
    gradient by more than 100 x the bar, so the bar can see each of them."""
    bar = grad_bar(g_ref)
    assert float(np.max(np.abs(g_k[:-1]))) > 100.0 * bar, ("K term below the bar's sight", g_k, bar)
    assert float(np.max(np.abs(g_ks))) > 100.0 * bar, ("K_s term below the bar's sight", g_ks, bar)
    assert abs(float(g_ref[-1])) > 100.0 * bar, ("noise partial below the bar's sight", g_ref[-1], bar)


def assert_grad_close(g, g_ref):
    g, g_ref = np.asarray(g, dtype=np.float64).reshape(-1), np.asarray(g_ref, dtype=np.float64).reshape(-1)
    assert g.shape == g_ref.shape
    err = float(np.max(np.abs(g - g_ref)))
    print("mse gradient: max |g - g_ref| = %.3e, bar %.3e, |g_ref|max %.3e" % (err, grad_bar(g_ref),
                                                                               float(np.max(np.abs(g_ref)))))
    assert err <= grad_bar(g_ref), (g, g_ref)


def inputs(n, m, d, seed, amplitude=10.0):
    """n training and m test points, uniform in [0, 1]^d, targets of amplitude ~10 (so the MSE's gradient is far above
    the bar away from the optimum) with a little noise."""
    rng = np.random.default_rng(seed)
    x, xs = rng.uniform(0.0, 1.0, (n, d)), rng.uniform(0.0, 1.0, (m, d))
    fun = lambda p: amplitude * (np.sin(5.0 * p.sum(axis=1)) + 0.5 * np.cos(11.0 * p[:, 0]))
    return x, fun(x) + 0.3 * rng.standard_normal(n), xs, fun(xs) + 0.3 * rng.standard_normal(m)


def projected_gradient_inf(x, g, lo, hi):
    """Infinity norm of the projected gradient of a box-constrained minimiser (SciPy's L-BFGS-B criterion):
    x - clip(x - g, lo, hi)."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    return float(np.max(np.abs(x - np.clip(x - g, lo, hi))))


# ----------------------------------------------------------------------------------------- the fitter's problems
FIT_N, FIT_M = 96, 32          # training and test points of the end-to-end fit
FIT_HYP, FIT_NOISE = [0.12], 0.05   # the SE length scale and the noise the targets are drawn with
FIT_TARGET_SEED = 11
KF_N, KF_RATIO, KF_SPLIT_SEED = 103, 0.25, 4   # four folds of CrossValidation.get_data_inputs: 26, 26, 26, 25 held out


def fit_problem():
    """(x [96, 1], y [96], xs [32, 1], ys [32]): one draw of an SE prior plus noise over 96 grid points and 32 uniform
    test points."""
    rng = np.random.default_rng(FIT_TARGET_SEED)
    x = np.linspace(0.0, 1.0, FIT_N).reshape(-1, 1)
    xs = np.sort(rng.uniform(0.0, 1.0, FIT_M)).reshape(-1, 1)
    xa = np.concatenate([x, xs])
    K = ad.kernel_matrix_t(("SE", {}), [torch.tensor(FIT_HYP[0], dtype=F64)], torch.as_tensor(xa),
                           torch.as_tensor(xa)).numpy() + FIT_NOISE * np.eye(len(xa))
    ya = np.linalg.cholesky(K) @ rng.standard_normal(len(xa))
    return x, ya[:FIT_N], xs, ya[FIT_N:]


def kfold_problem():
    """(x [103, 1], y [103]) of the k-fold fit: the same prior on a grid of 103 points."""
    rng = np.random.default_rng(FIT_TARGET_SEED + 1)
    x = np.linspace(0.0, 1.0, KF_N).reshape(-1, 1)
    K = ad.kernel_matrix_t(("SE", {}), [torch.tensor(FIT_HYP[0], dtype=F64)], torch.as_tensor(x),
                           torch.as_tensor(x)).numpy() + FIT_NOISE * np.eye(KF_N)
    return x, np.linalg.cholesky(K) @ rng.standard_normal(KF_N)


def kfold_arrays(x, y):
    """[(x_train, y_train, x_test, y_test)] of CrossValidation.get_data_inputs(.., KF_RATIO) under numpy's global
    generator seeded with KF_SPLIT_SEED (oracle.gp_oracle.cv_folds draws the same indices)."""
    from oracle import gp_oracle as o
    np.random.seed(KF_SPLIT_SEED)
    return [(x[tr], y[tr], x[te], y[te]) for tr, te in o.cv_folds(len(x), KF_RATIO)]


def objective(tree, folds):
    """v [n_hyp + 1] -> (mean over the folds of the reference MSE, its gradient); (inf, NaN) where a fold's
    K + noise I is not positive definite.  One fold: the held-out MSE itself."""
    def fn(v):
        try:
            f_sum, g_sum = 0.0, np.zeros(len(v))
            for k, (x, y, xs, ys) in enumerate(folds):
                f, g = mse_autodiff(tree, list(v[:-1]), v[-1], x, y, xs, ys)
                if not np.isfinite(f):
                    raise ValueError
                f_sum, g_sum = (f, g) if k == 0 else (f_sum + f, g_sum + g)
            return f_sum / len(folds), g_sum / len(folds)
        except Exception:
            return np.inf, np.full(len(v), np.nan)
    return fn
