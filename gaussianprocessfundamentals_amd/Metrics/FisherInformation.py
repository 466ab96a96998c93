"""Fisher information of the hyperparameters as a model-comparison score (no counterpart upstream, whose only
parameter-aware score is BIC, which counts the parameters instead of measuring them).

With K = k(X, X) + noise I the Fisher information of (hyperparameters in DFS order, noise) is
F_pq = 1/2 tr(K^-1 d_pK K^-1 d_qK), d_noise K = I: the expected Hessian of -LML, computed on the device from the
identity-augmented factorisation the gradient already runs (engine.InverseFactorization.fisher -> gpk_fisher).
``LaplaceEvidence`` is the Fisher-Laplace approximation of minus the log evidence at a fitted point,

    -LML + 1/2 log det F_free - (P_free / 2) log 2 pi        (minimise convention, like BIC)

over the parameters that are free: every kernel hyperparameter, and the noise when p_optimize_noise is on.

Exact, CHOLESKY_BASED, fp64, one DataInput.  F does not depend on y: any mean function is fine.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch

from .. import global_parameters as global_param
from . import MatrixHandlingTypes as mht
from .Metrics import AbstractMetric, MetricType

global_param.ensure_init()

LOG_2PI = math.log(2.0 * math.pi)


def free_log_determinant(fisher: np.ndarray, free: Sequence[int]) -> float:
    """log det of F restricted to the positions ``free`` by an unpivoted Cholesky on the host ((P + 1)^2 work).
    Raises ValueError naming the offending positions when the restriction is not positive definite: those whose own
    information F_pp is not positive (e.g. a change point of the hard INDICATOR mask, whose derivative is zero), else
    the position whose pivot fails (a parameter the earlier ones determine)."""
    free = [int(p) for p in free]
    F = np.asarray(fisher, dtype=np.float64)[np.ix_(free, free)]
    if not np.all(np.isfinite(F)):
        raise ValueError("the Fisher information is not finite (K + noise I not positive definite?)")
    bad = [free[i] for i in range(len(free)) if not F[i, i] > 0.0]
    if bad:
        raise ValueError("the Fisher information of the free parameters is not positive definite: no information "
                         "about parameter position(s) %s" % bad)
    L = np.zeros_like(F)
    logdet = 0.0
    for j in range(len(free)):
        piv = F[j, j] - float(np.dot(L[j, :j], L[j, :j]))
        # (a pivot lost to rounding counts as zero: eps times the diagonal entry it was subtracted from)
        if not piv > len(free) * np.finfo(np.float64).eps * F[j, j]:
            raise ValueError("the Fisher information of the free parameters is not positive definite: parameter "
                             "position(s) %s are determined by the ones before" % [free[j]])
        L[j, j] = math.sqrt(piv)
        L[j + 1:, j] = (F[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        logdet += math.log(piv)
    return logdet


def laplace_evidence(neg_lml, fisher: np.ndarray, free: Sequence[int]):
    """-LML + 1/2 log det F_free - (P_free / 2) log 2 pi (``neg_lml``: a float or a tensor, returned in kind)."""
    return neg_lml + (0.5 * free_log_determinant(fisher, free) - 0.5 * len(free) * LOG_2PI)


class LaplaceEvidence(AbstractMetric):
    def __init__(self, data_input, covariance_matrix, local_approx=mht.MatrixApproximations.NONE,
                 numerical_matrix_handling=mht.NumericalMatrixHandlingType.CHOLESKY_BASED, subset_size: int = None):
        from ..DataHandling.DataInput import BatchDataInput, DataInput
        name = type(self).__name__
        if local_approx is not mht.MatrixApproximations.NONE:
            raise NotImplementedError("%s: approximation %s is not supported" % (name, local_approx.name))
        if numerical_matrix_handling is not mht.NumericalMatrixHandlingType.CHOLESKY_BASED:
            raise NotImplementedError("%s: matrix handling %s is not supported (CHOLESKY_BASED)"
                                      % (name, numerical_matrix_handling.name))
        if isinstance(data_input, BatchDataInput):
            raise NotImplementedError("%s: BatchDataInput is not supported" % name)
        if not isinstance(data_input, DataInput):
            raise NotImplementedError("%s: data input %s is not supported (DataInput)"
                                      % (name, type(data_input).__name__))
        self.data_input = data_input
        self.covariance_matrix = covariance_matrix
        self.covariance_matrix.set_data_input(data_input)
        self.local_approx = local_approx
        self.numerical_matrix_handling = numerical_matrix_handling
        self.subset_size = subset_size
        self.type = MetricType.LL

    def _evaluate(self, hyper_parameter: List, noise):
        """(-LML [1] device, F [P + 1, P + 1] device) from ONE identity-augmented factorisation."""
        f = self.covariance_matrix.inverse_factorization(hyper_parameter, noise, gradient=False)
        return f.nlml(), f.fisher()[0]

    def get_fisher_information(self, hyper_parameter: List, noise) -> torch.Tensor:
        return self._evaluate(hyper_parameter, noise)[1]

    def get_metric(self, hyper_parameter: List, noise, indices=None) -> torch.Tensor:
        nl, F = self._evaluate(hyper_parameter, noise)
        n_par = int(F.shape[0])
        free = list(range(n_par - 1)) + ([n_par - 1] if global_param.p_optimize_noise else [])
        return laplace_evidence(nl.reshape(1, 1), F.cpu().numpy(), free)
