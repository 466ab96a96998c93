"""Derivative matrices and Fisher information restated on the CPU (TEST INFRASTRUCTURE ONLY).

``jacobian_ref``: torch.autograd.functional.jacobian over the oracle's differentiable kernel program
(oracle/gp_autodiff.py; LIN / RQ leaves and CP nodes through lin_torch, rq_torch, cp_torch) -- the planes
d K(x, x_) / d theta_p in the flat DFS order of the device.  ``fisher_ref``: F_pq = 1/2 tr(K^-1 D_p K^-1 D_q) with
numpy solves, the identity plane for the noise last.
"""
import numpy as np
import torch

from oracle import gp_autodiff as ad
from tests import cp_support as cs
from tests.lin_support import lin_torch
from tests.rq_support import rq_torch

F64 = torch.float64


def n_entries(tree, scaled):
    """hyperparameter list entries of a tree (an ARD vector is one entry)"""
    op, arg = tree
    if op == "CP":
        return len(arg) - 1 + sum(n_entries(c, scaled) for c in arg)
    if op in ("ADD", "MUL"):
        return sum(n_entries(c, scaled) for c in arg)
    return {"PER": 2, "RQ": 2}.get(op, 1) + (1 if scaled else 0)


def kernel_t(tree, params, x, x_, scaled=False, expanded=False, mode="SIGMOID"):
    """K(x, x_) as a differentiable fp64 torch tensor: gp_autodiff's program, with the LIN / RQ leaves and CP nodes of
    the *_support restatements."""
    op, arg = tree
    if op == "CP":
        return cs.cp_torch(tree, list(params), x, x_, mode, scaled)
    if op in ("ADD", "MUL"):
        idx, res = 0, None
        for child in arg:
            k = n_entries(child, scaled)
            m = kernel_t(child, params[idx:idx + k], x, x_, scaled, expanded, mode)
            idx += k
            res = m if res is None else (res + m if op == "ADD" else res * m)
        return res
    if op == "LIN":
        return lin_torch(params, x, x_, scaled)
    if op == "RQ":
        return rq_torch(params, x, x_, scaled)
    if not expanded:
        return ad.kernel_matrix_t(tree, list(params), x, x_, scaled)
    return ad._base(op, arg, params, x, x_, scaled, True)


def as_params(hyp):
    return [torch.tensor(np.asarray(h, dtype=np.float64), dtype=F64) for h in hyp]


def kernel_ref(tree, hyp, x, x_, scaled=False, expanded=False, mode="SIGMOID"):
    X, X_ = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(x_, dtype=np.float64))
    return kernel_t(tree, as_params(hyp), X, X_, scaled, expanded, mode).numpy()


def jacobian_ref(tree, hyp, x, x_, scaled=False, expanded=False, mode="SIGMOID"):
    """[n_hyp, n, m] numpy: plane p = d K / d (flat hyperparameter p).  A parameter K does not depend on (a change
    point of the hard mask) gets a plane of zeros."""
    params = tuple(as_params(hyp))
    X, X_ = torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(x_, dtype=np.float64))
    jac = torch.autograd.functional.jacobian(
        lambda *p: kernel_t(tree, list(p), X, X_, scaled, expanded, mode), params, vectorize=True,
        strategy="forward-mode")
    planes = []
    for j, p in zip(jac, params):   # [n, m, *p.shape] -> [numel, n, m]
        planes.append(j.reshape(j.shape[0], j.shape[1], -1).permute(2, 0, 1))
    return torch.cat(planes, dim=0).numpy()


def fisher_ref(K_noised, planes):
    """[P + 1, P + 1]: 1/2 tr(K^-1 D_p K^-1 D_q) over ``planes`` [P, n, n] and the identity (the noise, last)."""
    K = np.asarray(K_noised, dtype=np.float64)
    n = K.shape[0]
    D = list(np.asarray(planes, dtype=np.float64).reshape(-1, n, n)) + [np.eye(n)]
    T = [np.linalg.solve(K, d) for d in D]
    F = np.empty((len(T), len(T)))
    for p in range(len(T)):
        for q in range(p, len(T)):
            F[p, q] = F[q, p] = 0.5 * float(np.sum(T[p] * T[q].T))
    return F
