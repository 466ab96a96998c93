"""A fitted GP as a predictor: factor once, then stream new points (build extension).

``GaussianProcess.predict`` and the posterior read-outs of Statistics/Auxiliary.py carry the test points of the
DataInput through the factorisation as extra rows, so every new set of points costs a new n^3 factorisation and a
matrix of (n_pad + m + 1)^2 doubles.  :class:`PosteriorPredictor` runs ONE identity-augmented factorisation
(engine.InverseFactorization: L^-T in the extra rows, -alpha in the corner's y row) and keeps it; every later
:meth:`predict` is one pass of gpk_predict over the new points, linear in their number, in a bounded workspace, with
the latent variance per point.  The formulas are the reference's (gpbasics/Statistics/Auxiliary.py:57-93):
mu = K_s^T alpha, var = diag(K_ss) - |inv(L) K_s|^2 column-wise.  The joint posterior comes from the same factor
(DESIGN 28): :meth:`covariance` is K_ss - V^T V between new points (gpk_predict_vt + gpk_predict_cov), :meth:`sample`
draws functions from it like get_n_posterior_functions (gpbasics/Statistics/GaussianProcess.py:97-110).
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from .. import engine
from .. import global_parameters as global_param
from ..DataHandling.DataInput import BatchDataInput
from ..MeanFunctionBasics import BaseMeanFunctions as bmf
from .CovarianceMatrix import noise_vector

global_param.ensure_init()


class PosteriorPredictor:
    """The posterior of ``kernel`` (hyperparameters ``hyper_parameter``, noise ``noise``) over the training data of
    ``data_input``, with the mean function ``mean_function`` at ``mean_function_hyper_param`` taken off the targets.
    Construction factors once (fp64) and raises engine.CholeskyError if K + noise I is not positive definite."""

    def __init__(self, kernel, hyper_parameter: List, noise, mean_function, mean_function_hyper_param: Optional[List],
                 data_input, max_rows: Optional[int] = None):
        if isinstance(data_input, BatchDataInput) or data_input.data_x_train.dim() != 2:
            raise NotImplementedError("PosteriorPredictor: BatchDataInput is not supported")
        self.kernel, self.mean_function = kernel, mean_function
        self.hyper_parameter = list(hyper_parameter)
        self.mean_function_hyper_param = mean_function_hyper_param
        self.max_rows = max_rows
        x = engine.as_device_f64(data_input.data_x_train).contiguous()
        n, d = int(x.shape[0]), int(x.shape[1])
        self.n, self.d = n, d
        y = engine.as_device_f64(data_input.data_y_train).reshape(n)
        if not self._zero_mean():
            y = engine.mean_vector(mean_function, mean_function_hyper_param, x, y)
        kd = engine.kernel_descriptor(kernel, d)
        hyp = engine.pack_hyper_parameter(self.hyper_parameter, kd.n_hyp)
        self.noise = noise_vector(noise)
        f = engine.InverseFactorization(n, d, 1, torch.float64)
        f.run(kd, hyp, 0, self.noise, 0, x, 0, y.reshape(1, n).contiguous(), 0, gradient=False)
        f.check_info()
        self.factorization = f

    def _zero_mean(self) -> bool:
        return self.mean_function is None or isinstance(self.mean_function, bmf.ZeroMeanFunction)

    def _points(self, x_new) -> torch.Tensor:
        x_new = engine.as_device_f64(x_new)
        if x_new.dim() != 2 or int(x_new.shape[1]) != self.d or int(x_new.shape[0]) < 1:
            raise ValueError("x_new must be [m >= 1, %d], got %s" % (self.d, tuple(x_new.shape)))
        return x_new.contiguous()

    def _mean(self, x_new: torch.Tensor) -> torch.Tensor:
        if self._zero_mean():
            return torch.zeros(int(x_new.shape[0]), dtype=torch.float64, device=x_new.device)
        return engine.mean_vector(self.mean_function, self.mean_function_hyper_param, x_new)

    def predict(self, x_new, return_var: bool = False, include_noise: bool = False):
        """(mean + mu, mean, mu), each [m] on the device, like GaussianProcess.predict; with ``return_var`` a fourth
        entry: the posterior variance per point (latent; + noise with ``include_noise``)."""
        x_new = self._points(x_new)
        mu, var = self.factorization.predict(x_new, want_var=return_var, max_rows=self.max_rows)
        mean = self._mean(x_new)
        if not return_var:
            return mean + mu, mean, mu
        if include_noise:
            var = var + self.noise
        return mean + mu, mean, mu, var

    # -- the joint posterior: covariance between new points and function draws -----------------------
    def covariance(self, x_new, x_other=None, include_noise: bool = False) -> torch.Tensor:
        """The latent posterior covariance K_ss - V^T V between new points (Auxiliary.py:83-93, get_posterior_var),
        from the kept factorisation: [m, m] of ``x_new`` with itself, symmetric bit for bit, or [m, m'] between
        ``x_new`` and ``x_other``.  ``include_noise`` adds noise I (the covariance of observations at the points); it
        has no meaning between two different sets of points."""
        if include_noise and x_other is not None:
            raise ValueError("include_noise adds noise I to the covariance of one set of points with itself: "
                             "not with x_other")
        x_new = self._points(x_new)
        if x_other is not None:
            return self.factorization.predict_cov(x_new, self._points(x_other))
        sigma = self.factorization.predict_cov(x_new)
        if include_noise:
            engine.add_diagonal(sigma, float(self.noise[0]))
        return sigma

    def draw_factor(self, x_new, include_noise: bool = False):
        """(mean + mu [m], L [m, m]) that :meth:`sample` draws from: L the lower Cholesky factor of
        Sigma [+ noise I] + p_cov_matrix_jitter I on the device (engine.DenseFactorization; engine.CholeskyError if it
        is not positive definite).  Keep it to draw again at the same points without factoring again."""
        x_new = self._points(x_new)
        total = self.predict(x_new)[0]
        sigma = self.covariance(x_new, include_noise=include_noise)
        f = engine.DenseFactorization(int(x_new.shape[0]))
        f.run(sigma, float(torch.as_tensor(global_param.p_cov_matrix_jitter)))
        f.check_info()
        return total, f.cholesky(0).to(torch.float64).contiguous()

    def sample(self, x_new, n_draws: int, generator=None, include_noise: bool = False, z=None) -> torch.Tensor:
        """``n_draws`` posterior function draws at the new points, [m, n_draws] like get_n_posterior_functions
        (GaussianProcess.py:97-110): mean + mu + chol(Sigma [+ noise I] + p_cov_matrix_jitter I) z, with
        z ~ N(0, 1) [m, n_draws] from ``torch.randn`` on the device with ``generator`` unless ``z`` is given.
        ``include_noise`` draws observations instead of latent function values."""
        n_draws = int(n_draws)
        if n_draws < 1:
            raise ValueError("n_draws must be >= 1")
        if z is not None:   # (checked before anything reaches the device)
            z = z if isinstance(z, torch.Tensor) else torch.as_tensor(z)
            m_given = int(len(x_new))
            if tuple(z.shape) != (m_given, n_draws):
                raise ValueError("z must be [%d, %d], got %s" % (m_given, n_draws, tuple(z.shape)))
        x_new = self._points(x_new)
        m = int(x_new.shape[0])
        if z is not None:
            z = engine.as_device_f64(z)
        total, L = self.draw_factor(x_new, include_noise)
        if z is None:
            z = torch.randn((m, n_draws), dtype=torch.float64, device=L.device, generator=generator)
        return engine.dgemm(L, z, beta=1.0, C=total.reshape(-1, 1).expand(m, n_draws).contiguous())

    def log_predictive_density(self, x_new, y_new) -> torch.Tensor:
        """Mean over the points of log N(y_new; mean + mu, var + noise) (rank 0, device)."""
        total, _, _, var = self.predict(x_new, return_var=True, include_noise=True)
        y = engine.as_device_f64(y_new).reshape(-1)
        if y.numel() != total.numel():
            raise ValueError("%d targets for %d points" % (y.numel(), total.numel()))
        r = y - total
        return torch.mean(-0.5 * (math.log(2.0 * math.pi) + torch.log(var) + r * r / var))
