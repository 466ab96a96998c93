"""Mean squared error of the posterior mean on the test set (gpbasics/Metrics/MeanSquaredError.py:14-81).

``get_posterior_mu`` (mu = K_s^T alpha, :33-42) comes from ONE device factorisation of the
augmented matrix with the test points as extra rows; the blockwise form factors every segment
together in one ragged batch.  MSE = mean((mu - detrended y_test)^2).
"""
from __future__ import annotations

from typing import List

import torch

from .. import engine
from .. import global_parameters as global_param
from ..Statistics.CovarianceMatrix import noise_vector
from .LogLikelihood import _split_like, blockwise_hyper_parameter_offset
from .Metrics import AbstractMetric, Metric, MetricType

global_param.ensure_init()


class AbstractMSE(Metric):
    pass


def posterior_mu(kernel, hyper_parameter: List, noise, data_input) -> torch.Tensor:
    """mu = K_s^T alpha for one DataInput, [n_test] (MeanSquaredError.py:33-42)."""
    x, xt = data_input.data_x_train, data_input.data_x_test
    n, d, m = int(x.shape[0]), int(x.shape[1]), int(xt.shape[0])
    y = data_input.get_detrended_y_train().reshape(1, n).to(torch.float64).contiguous()
    f = engine.AugmentedFactorization(n, d, m, 1, global_param.p_dtype)
    kd = engine.kernel_descriptor(kernel, d)
    hyp = engine.pack_hyper_parameter(hyper_parameter, kd.n_hyp)
    f.run(kd, hyp, 0, noise_vector(noise), 0, x.contiguous(), 0, y, 0, Xs=xt.contiguous(), xs_bstride=0)
    kernel._record_hyper_parameter(list(hyper_parameter))
    f.check_info()
    return f.posterior_mu(0).clone()


class MeanSquaredError(AbstractMSE):
    def __init__(self, data_input, covariance_matrix, aux_gp, local_approx, numerical_matrix_handling,
                 subset_size: int = None):
        super().__init__(data_input, covariance_matrix, MetricType.MSE, local_approx, numerical_matrix_handling,
                         subset_size)
        self.aux_gp = aux_gp

    def get_metric(self, hyper_parameter: List, noise, indices=None) -> torch.Tensor:
        self.aux_gp.reset()
        self.covariance_matrix.reset()
        mu = self.get_posterior_mu(hyper_parameter, noise, indices).reshape(-1, 1)
        yt = self.data_input.get_detrended_y_test().reshape(-1, 1).to(torch.float64)
        return torch.mean((mu - yt) ** 2)

    def get_metric_and_gradient(self, hyper_parameter: List, noise):
        """(mse, [d mse / d h for h in hyper_parameter] (each shaped like h), d mse / d noise): the gradient the
        reference's tape takes through get_metric, from ONE device factorisation with the test points as extra rows
        and one tile pass with two rank-one weights (gpk_mse_grad; no inverse is formed).  The targets are the
        detrended ones, so a fixed mean function is honoured.  +inf and NaN when K + noise I is not positive
        definite.  Exact, CHOLESKY_BASED MSE of a DataInput only."""
        from ..DataHandling.DataInput import BatchDataInput, DataInput
        from . import MatrixHandlingTypes as mht
        name = type(self).__name__
        if self.local_approx is not mht.MatrixApproximations.NONE:
            raise NotImplementedError("%s.get_metric_and_gradient: approximation %s is not supported"
                                      % (name, self.local_approx.name))
        if self.numerical_matrix_handling is not mht.NumericalMatrixHandlingType.CHOLESKY_BASED:
            raise NotImplementedError("%s.get_metric_and_gradient: matrix handling %s is not supported "
                                      "(CHOLESKY_BASED)" % (name, self.numerical_matrix_handling.name))
        di = self.data_input
        if isinstance(di, BatchDataInput) or not isinstance(di, DataInput):
            raise NotImplementedError("%s.get_metric_and_gradient: data input %s is not supported (DataInput)"
                                      % (name, type(di).__name__))
        self.aux_gp.reset()
        self.covariance_matrix.reset()
        kernel = self.covariance_matrix.kernel
        x, xt = di.data_x_train, di.data_x_test
        n, d, m = int(x.shape[0]), int(x.shape[1]), int(xt.shape[0])
        if m < 1:
            raise NotImplementedError("%s.get_metric_and_gradient: the data input has no test points" % name)
        y = di.get_detrended_y_train().reshape(1, n).to(torch.float64).contiguous()
        yt = di.get_detrended_y_test().reshape(1, m).to(torch.float64).contiguous()
        kd = engine.kernel_descriptor(kernel, d)
        hyp = engine.pack_hyper_parameter(hyper_parameter, kd.n_hyp)
        f = engine.AugmentedFactorization(n, d, m, 1, torch.float64)
        f.run_mse(kd, hyp, 0, noise_vector(noise), 0, engine.as_device_f64(x).contiguous(), 0,
                  engine.as_device_f64(y), 0, engine.as_device_f64(xt).contiguous(), 0, engine.as_device_f64(yt), 0)
        kernel._record_hyper_parameter(list(hyper_parameter))
        g = f.mse_grad()[0]
        return f.mse()[0], _split_like(g[:kd.n_hyp], hyper_parameter), g[kd.n_hyp]

    def get_gradients(self, hyper_parameter: List, noise, reset: bool = True) -> torch.Tensor:
        """Metrics.py:31: d mse / d(hyperparameters) as one flat vector in DFS order (as LogLikelihood.get_gradients)."""
        _, grads, _ = self.get_metric_and_gradient(hyper_parameter, noise)
        return torch.cat([g.reshape(-1) for g in grads]) if grads else torch.zeros(0, dtype=torch.float64)

    def get_posterior_mu(self, hyper_parameter: List, noise, indices=None):
        """K_s^T alpha (MeanSquaredError.py:33-42).  CHOLESKY_BASED: one augmented factorisation with
        the test rows; the other handlings: their alpha (Metrics.get_alpha) and one device GEMV."""
        from .. import engine
        from . import MatrixHandlingTypes as mht
        if self.numerical_matrix_handling is mht.NumericalMatrixHandlingType.CHOLESKY_BASED:
            return posterior_mu(self.covariance_matrix.kernel, hyper_parameter, noise, self.data_input)
        alpha = self.get_alpha(hyper_parameter, noise, None, indices)
        ks_t = self.covariance_matrix.get_K_s(hyper_parameter).transpose(0, 1).contiguous()
        return engine.gemv(ks_t, alpha.reshape(-1)).reshape(-1)


class BlockwiseMeanSquaredError(AbstractMetric):
    def __init__(self, _gp, local_approx, numerical_matrix_handling, subset_size: int = None):
        self.local_approx = local_approx
        self.numerical_matrix_handling = numerical_matrix_handling
        self.subset_size = subset_size
        self.aux_gp = _gp.aux
        self._gp = _gp
        self.data_input = _gp.data_input

    def get_metric(self, hyper_parameter: List, noise, indices=None) -> torch.Tensor:
        """Per-segment posterior means (hyperparameters sliced from offset 0, the reference's
        quirk, see blockwise_hyper_parameter_offset) against the segments' detrended test targets,
        both concatenated in segment order (MeanSquaredError.py:63-81)."""
        from ..Statistics.Auxiliary import segment_posterior_mu
        index = blockwise_hyper_parameter_offset(self._gp)
        kernels, slices, dis = [], [], []
        for sub in self._gp.constituent_gps:
            kern = sub.covariance_matrix.kernel
            nh = kern.get_number_of_hyper_parameter()
            kernels.append(kern)
            slices.append(list(hyper_parameter[index:index + nh]))
            dis.append(sub.data_input)
            index += nh
        mu = segment_posterior_mu(kernels, slices, dis, noise).reshape(-1, 1)
        yt = torch.cat([d.get_detrended_y_test().reshape(-1, 1).to(torch.float64) for d in dis], dim=0)
        return torch.mean((mu - yt) ** 2)
