"""Leave-one-out cross-validation as a metric (Rasmussen & Williams 5.4.2; no counterpart upstream, whose
Metrics/CrossValidation.py approximates it with k random folds and k factorisations).

With K = k(X, X) + noise I, alpha = K^-1 y and d_i = (K^-1)_ii the prediction of point i from the other n - 1 points
is mu_i = y_i - alpha_i / d_i with variance 1 / d_i: all n refits are an O(n) read-out of the identity-augmented
factorisation the -LML gradient already runs (engine.InverseFactorization -> gpk_loo_grad).  ``loss``:

  MetricType.LL   minus the LOO log predictive density, sum_i [1/2 log 2 pi + 1/2 log sigma_i^2 + (y_i - mu_i)^2 /
                  (2 sigma_i^2)] (minus R&W eq. 5.13; minimise convention, summed like -LML)
  MetricType.MSE  the LOO mean squared error, mean_i (y_i - mu_i)^2

Exact, CHOLESKY_BASED, fp64, one DataInput.  A mean function is honoured through the detrended targets.
"""
from __future__ import annotations

from typing import List

import torch

from .. import _native as nat
from .. import engine
from .. import global_parameters as global_param
from ..Statistics.CovarianceMatrix import noise_vector
from . import MatrixHandlingTypes as mht
from .LogLikelihood import _split_like
from .Metrics import AbstractMetric, MetricType

global_param.ensure_init()

LOSS_CODES = {MetricType.LL: nat.LOO_LPD, MetricType.MSE: nat.LOO_MSE}


def loss_code(loss: MetricType, owner: str) -> int:
    if loss not in LOSS_CODES:
        raise NotImplementedError("%s: loss %s is not supported (LL: log predictive density, MSE)"
                                  % (owner, getattr(loss, "name", loss)))
    return LOSS_CODES[loss]


class LeaveOneOut(AbstractMetric):
    def __init__(self, data_input, covariance_matrix, local_approx=mht.MatrixApproximations.NONE,
                 numerical_matrix_handling=mht.NumericalMatrixHandlingType.CHOLESKY_BASED, subset_size: int = None,
                 loss: MetricType = MetricType.LL):
        from ..DataHandling.DataInput import BatchDataInput, DataInput
        name = type(self).__name__
        self.loss_code = loss_code(loss, name)
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
        self.type = loss
        self._fact = None

    def _run(self, hyper_parameter: List, noise, gradient: bool):
        """One gpk_loo_grad on the detrended targets; the factorisation object (and its workspace) is kept."""
        di = self.data_input
        kernel = self.covariance_matrix.kernel
        x = engine.as_device_f64(di.data_x_train).contiguous()
        n, d = int(x.shape[0]), int(x.shape[1])
        y = engine.as_device_f64(di.get_detrended_y_train()).reshape(1, n).contiguous()
        kd = engine.kernel_descriptor(kernel, d)
        hyp = engine.pack_hyper_parameter(hyper_parameter, kd.n_hyp)
        if self._fact is None or (self._fact.n, self._fact.d) != (n, d):
            self._fact = engine.InverseFactorization(n, d, 1, torch.float64)
        self._fact.run_loo(self.loss_code, kd, hyp, 0, noise_vector(noise), 0, x, 0, y, 0, gradient=gradient)
        kernel._record_hyper_parameter(list(hyper_parameter))
        return kd, self._fact.loo_results()

    def get_metric(self, hyper_parameter: List, noise, indices=None) -> torch.Tensor:
        _, (f, _, _, _) = self._run(hyper_parameter, noise, False)
        return f.reshape(1, 1)

    def get_metric_and_gradient(self, hyper_parameter: List, noise):
        """(f [1, 1], [d f / d h for h in hyper_parameter] (each shaped like h), d f / d noise); +inf and NaN when
        K + noise I is not positive definite."""
        kd, (f, g, _, _) = self._run(hyper_parameter, noise, True)
        return f.reshape(1, 1), _split_like(g[0, :kd.n_hyp], hyper_parameter), g[0, kd.n_hyp]

    def get_gradients(self, hyper_parameter: List, noise, reset: bool = True) -> torch.Tensor:
        """d f / d(hyperparameters) as one flat vector in DFS order (as LogLikelihood.get_gradients)."""
        _, grads, _ = self.get_metric_and_gradient(hyper_parameter, noise)
        return torch.cat([g.reshape(-1) for g in grads]) if grads else torch.zeros(0, dtype=torch.float64)

    def get_predictions(self, hyper_parameter: List, noise):
        """(mu [n], var [n]): every training point predicted from the others; the mean function's value at the point is
        added back to mu, var includes the noise."""
        _, (_, _, mu, var) = self._run(hyper_parameter, noise, False)
        di = self.data_input
        mean = (engine.as_device_f64(di.data_y_train).reshape(-1)
                - engine.as_device_f64(di.get_detrended_y_train()).reshape(-1))
        return mu[0] + mean, var[0].clone()
