"""Change-point trees for the tests: a numpy reference, a differentiable torch restatement and inputs that exercise
the transition zones.

TEST INFRASTRUCTURE ONLY.  Tree form: ``("CP", [child, ...])`` beside the oracle's ("ADD" | "MUL", [...]) and leaves;
its hyperparameter list is ``[cp_0 .. cp_{C-1}, hyp(child_0), .., hyp(child_C)]`` (K/Operators.py:445-476).  Children
with a LIN leaf need the ``lin_oracle`` fixture of tests/lin_support.py (the oracle modules learn the leaf there).

Reference (paths relative to gpbasics/): K/Operators.py:379-408 (the masks), :410-476 (the operator),
    K = sum_i K_i * prev_i * ind_i ind_i'^T,  prev_0 = 1,  prev_{i+1} = (1 - ind_i)(1 - ind_i')^T
-- only the complement of the PREVIOUS change point enters, not a running product."""
import math

import numpy as np
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests.lin_support import make_kernel as _make_leaf_kernel

F64 = torch.float64
MODES = ("INDICATOR", "SIGMOID", "APPROX_INDICATOR")
# offsets around every change point: inside the SIGMOID transition (0.01 wide: tanh leaves +-1 for |cp - x| <~ 0.048,
# and is visibly between them for |cp - x| <~ 0.005), on it, and just outside
CP_OFFSETS = (-0.004, -0.0015, -0.0004, 0.0, 0.0007, 0.002, 0.005)


def set_mode(mode: str):
    gp.p_cp_operator_type = gp.ChangePointOperatorType[mode]


def cp_inputs(n, seed, cps, m=0):
    """n uniform points in [0, 1] (unsorted), the first 7 per change point replaced by cp + CP_OFFSETS; a target with
    a different regime per segment; m uniform test points (the first 7 per change point placed likewise)."""
    rng = np.random.default_rng(seed)

    def points(count):
        x = rng.uniform(0.0, 1.0, count)
        at = 0
        for cp in cps:
            for off in CP_OFFSETS:
                if at < count:
                    x[at] = cp + off
                    at += 1
        return x[rng.permutation(count)].reshape(-1, 1)

    x = points(n)
    seg = np.searchsorted(np.sort(np.asarray(cps, dtype=np.float64)), x[:, 0])
    y = np.sin((6.0 + 5.0 * seg) * x[:, 0]) + 0.4 * seg + 0.05 * rng.standard_normal(n)
    xs = points(m) if m else None
    return x, y, xs


def n_entries(tree, scaled=False, dim=1):
    """hyperparameter list entries of a tree with CP nodes"""
    op, arg = tree
    if op == "CP":
        return len(arg) - 1 + sum(n_entries(c, scaled, dim) for c in arg)
    if op in ("ADD", "MUL"):
        return sum(n_entries(c, scaled, dim) for c in arg)
    return o.n_hyp(tree, scaled, dim)


def has_cp(tree):
    op, arg = tree
    return op == "CP" or (op in ("ADD", "MUL") and any(has_cp(c) for c in arg))


def cp_numpy(tree, hyp, x, x_, mode, scaled=False):
    """The reference matrix: oracle.gp_oracle.change_point_matrix at every CP node (its children plain oracle trees),
    ADD / MUL above it folded left."""
    op, arg = tree
    if op == "CP":
        ncp = len(arg) - 1
        cps = [float(np.asarray(c)) for c in hyp[:ncp]]
        hyps, idx = [], ncp
        for c in arg:
            k = n_entries(c, scaled, x.shape[1])
            hyps.append(list(hyp[idx:idx + k]))
            idx += k
        assert idx == len(hyp) and not any(has_cp(c) for c in arg)
        return o.change_point_matrix(arg, hyps, cps, x, x_, mode, scaled)
    if op in ("ADD", "MUL") and has_cp(tree):
        idx, res = 0, None
        for c in arg:
            k = n_entries(c, scaled, x.shape[1])
            m = cp_numpy(c, hyp[idx:idx + k], x, x_, mode, scaled)
            idx += k
            res = m if res is None else (res + m if op == "ADD" else res * m)
        return res
    return o.kernel_matrix(tree, list(hyp), x, x_, scaled)


def ind_torch(x, cp, mode):
    """K/Operators.py:379-400 on a 1-D tensor of points."""
    if mode == "SIGMOID":
        return 0.5 * (1 + torch.tanh((cp - x) / 0.0025))
    if mode == "APPROX_INDICATOR":
        return 1.0 / (1.0 + torch.exp(-100.0 * (x - cp)))
    return (x < cp).to(F64)                                          # tf.less: no gradient


def cp_torch(tree, params, x, x_, mode, scaled=False):
    """K as a differentiable fp64 torch tensor (CPU): params the hyperparameter list as tensors, x / x_ [n, 1] / [m, 1]
    tensors.  The separable form sum_i w_i(x) w_i(y) K_i with w_i = (1 - ind_{i-1}) ind_i."""
    op, arg = tree
    if op == "CP":
        ncp = len(arg) - 1
        idx, res = ncp, None
        xv, xv_ = x[:, 0], x_[:, 0]
        for i, c in enumerate(arg):
            k = n_entries(c, scaled, 1)
            Ki = cp_torch(c, params[idx:idx + k], x, x_, mode, scaled)
            idx += k
            w, w_ = torch.ones_like(xv), torch.ones_like(xv_)
            if i > 0:
                w, w_ = 1.0 - ind_torch(xv, params[i - 1], mode), 1.0 - ind_torch(xv_, params[i - 1], mode)
            if i < ncp:
                w, w_ = w * ind_torch(xv, params[i], mode), w_ * ind_torch(xv_, params[i], mode)
            term = Ki * (w[:, None] * w_[None, :])
            res = term if res is None else res + term
        return res
    if op in ("ADD", "MUL") and has_cp(tree):
        idx, res = 0, None
        for c in arg:
            k = n_entries(c, scaled, 1)
            m = cp_torch(c, params[idx:idx + k], x, x_, mode, scaled)
            idx += k
            res = m if res is None else (res + m if op == "ADD" else res * m)
        return res
    return ad.kernel_matrix_t(tree, list(params), x, x_, scaled)


def as_params(hyp, requires_grad=True):
    return [torch.tensor(np.asarray(h, dtype=np.float64), dtype=F64, requires_grad=requires_grad) for h in hyp]


def nlml_torch(K, y, noise):
    """-LML through torch.linalg.cholesky (M/LogLikelihood.py:26-48), differentiable."""
    n = K.shape[0]
    Y = torch.as_tensor(np.asarray(y, dtype=np.float64)).reshape(-1, 1)
    L = torch.linalg.cholesky(K + noise * torch.eye(n, dtype=F64))
    z = torch.linalg.solve_triangular(L, Y, upper=False)
    fit = (z.T @ z)[0, 0]
    logdet = 2.0 * torch.sum(torch.log(torch.diagonal(L)))
    return 0.5 * fit + 0.5 * logdet + 0.5 * n * math.log(2.0 * math.pi)


def cp_nlml_and_grad(tree, hyp, noise, x, y, mode, scaled=False):
    """(-LML, flat gradient over the hyperparameter entries, d / d noise) by autograd on the CPU; a parameter the
    value does not depend on (the change points under the hard mask) gets 0."""
    params = as_params(hyp)
    nz = torch.tensor(float(noise), dtype=F64, requires_grad=True)
    X = torch.as_tensor(np.asarray(x, dtype=np.float64))
    nl = nlml_torch(cp_torch(tree, params, X, X, mode, scaled), y, nz)
    grads = torch.autograd.grad(nl, params + [nz], allow_unused=True)
    flat = [np.zeros(p.numel()) if g is None else g.numpy().reshape(-1) for p, g in zip(params, grads[:-1])]
    return float(nl.detach()), np.concatenate(flat), float(grads[-1])


def cp_posterior(tree, hyp, noise, x, y, xs, mode, scaled=False):
    """Posterior mean and variance diagonal at xs from the restatement (numpy Cholesky)."""
    params = as_params(hyp, False)
    X, Xs = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(xs, dtype=np.float64))
    K = cp_torch(tree, params, X, X, mode, scaled).numpy() + noise * np.eye(len(x))
    Ks = cp_torch(tree, params, X, Xs, mode, scaled).numpy()
    Kss = cp_torch(tree, params, Xs, Xs, mode, scaled).numpy()
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, np.asarray(y, dtype=np.float64)))
    V = np.linalg.solve(L, Ks)
    return Ks.T @ alpha, np.diag(Kss) - np.sum(V * V, axis=0)


def make_kernel(tree, hyp, dim=1):
    """The package's kernel object of a tree with CP nodes; the operator's initial change points are those of hyp."""
    op, arg = tree
    if op == "CP":
        ncp = len(arg) - 1
        kids, idx = [], ncp
        for c in arg:
            k = n_entries(c, gp.p_scaled_base_kernel, dim)
            kids.append(make_kernel(c, hyp[idx:idx + k], dim))
            idx += k
        return ops.ChangePointOperator(dim, kids, [torch.tensor(float(np.asarray(c)), dtype=F64) for c in hyp[:ncp]])
    if op in ("ADD", "MUL") and has_cp(tree):
        kids, idx = [], 0
        for c in arg:
            k = n_entries(c, gp.p_scaled_base_kernel, dim)
            kids.append(make_kernel(c, hyp[idx:idx + k], dim))
            idx += k
        return (ops.AdditionOperator if op == "ADD" else ops.MultiplicationOperator)(dim, kids)
    return _make_leaf_kernel(tree, dim)
