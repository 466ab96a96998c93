"""Hyperparameter fitters (gpbasics/Optimizer/Fitter.py).

``Fitter`` / ``GradientFitter`` keep the reference's constructor (:20-41): the GP receives the data input and the
metric comes from ``get_metric_by_type``.  The reference's own ``fit`` implementations are a one-step variational SGD
(:51-170, restated for SKC elsewhere) and a SciPy wrapper that cannot be constructed; neither is provided.

``DeviceLbfgsFitter`` is the fitter this engine was built for: ``n_starts`` restarts of a bound-projected L-BFGS
advance in lockstep.  Every iteration is ONE batched value + gradient factorisation
(sweep.native_batched_value_and_gradient -> gpk_nlml_grad) followed by ONE gpk_fit_step launch that runs every
restart's update, bound projection, line-search decision and convergence test on the device
(engine.LbfgsState); the host reads the status words back once per ``check_every`` iterations and nothing else.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from .. import _native as nat
from .. import global_parameters as global_param
from ..DataHandling.DataInput import BatchDataInput, DataInput
from ..Metrics import Auxiliary as met_aux
from ..Metrics import MatrixHandlingTypes as mht
from ..Metrics import Metrics as met
from . import FitterType as ft

global_param.ensure_init()


class Fitter:
    def __init__(self, data_input, gaussian_process, metric_type: met.MetricType, fitter_type: ft.FitterType,
                 from_distribution: bool, local_approx: mht.GlobalApproximationsType,
                 numerical_matrix_handling: mht.NumericalMatrixHandlingType, subset_size: int = None):
        self._gp = gaussian_process
        if isinstance(data_input, list):
            # k-fold: one metric per fold over a copy of the GP (Fitter.py:27-33)
            self.metric = []
            for fold in data_input:
                copied = self._gp.copy()
                copied.set_data_input(fold)
                self.metric.append(met_aux.get_metric_by_type(metric_type, copied, local_approx,
                                                              numerical_matrix_handling, subset_size))
        else:
            self._gp.set_data_input(data_input)
            self.metric = met_aux.get_metric_by_type(metric_type, self._gp, local_approx, numerical_matrix_handling,
                                                     subset_size)
        self.data_input = data_input
        self.type = fitter_type
        self.from_distribution = bool(from_distribution)

    def fit(self) -> Tuple:
        """(pre-fit metric, post-fit metric, last hyperparameter list, noise, indices) (Fitter.py:43-44: no body)."""
        return None


class GradientFitter(Fitter):
    pass


def pack_bounds(kernel, xrange, n: int, bounded: bool, optimize_noise: bool):
    """(lo, hi) float lists of the n_hyp + 1 optimised values, the noise last.  Bounded: the kernel's
    get_hyper_parameter_bounds (one pair per scalar hyperparameter, a pair of an ARD entry repeated over its values;
    their +-inf entries kept) and [p_cov_matrix_jitter, inf) for the noise; unbounded: +-inf.  Without
    ``optimize_noise`` the noise slot is pinned, lo = hi = p_cov_matrix_jitter, whatever ``bounded``."""
    jitter = float(torch.as_tensor(global_param.p_cov_matrix_jitter))
    dims = kernel.get_hyper_parameter_dimensionalities()
    lo: List[float] = []
    hi: List[float] = []
    if bounded:
        bounds = kernel.get_hyper_parameter_bounds(xrange, n)
        if len(bounds) != len(dims):
            raise ValueError("the kernel gives %d bounds for %d hyperparameters" % (len(bounds), len(dims)))
        for (b_lo, b_hi), dim in zip(bounds, dims):
            k = max(1, int(math.prod(dim)))
            lo += [float(torch.as_tensor(b_lo))] * k
            hi += [float(torch.as_tensor(b_hi))] * k
    else:
        k = sum(max(1, int(math.prod(dim))) for dim in dims)
        lo, hi = [-math.inf] * k, [math.inf] * k
    if optimize_noise:
        lo.append(jitter if bounded else -math.inf)
        hi.append(math.inf)
    else:
        lo.append(jitter)
        hi.append(jitter)
    return lo, hi


def split_winner(flat: torch.Tensor, dimensionalities: List[list]) -> List[torch.Tensor]:
    """The hyperparameter list of a flat DFS-ordered vector: entry i takes prod(dimensionalities[i]) values from the
    running offset (the reference's deserialize_hyper_parameter slices every entry from 0 for scalars: not used)."""
    out, off = [], 0
    for dim in dimensionalities:
        k = max(1, int(math.prod(dim)))
        out.append(flat[off:off + k].reshape(list(dim)).clone())
        off += k
    if off != flat.numel():
        raise ValueError("%d values for hyperparameters of %d values" % (flat.numel(), off))
    return out


def _flatten(hyper_parameter: List) -> List[float]:
    vals: List[float] = []
    for h in hyper_parameter:
        vals += [float(v) for v in torch.as_tensor(h, dtype=torch.float64).reshape(-1).tolist()]
    return vals


class DeviceLbfgsFitter(GradientFitter):
    """Multi-start L-BFGS on the device for the exact, Cholesky-based LL / BIC of a DataInput.

    BIC is 2 LL + a constant for a fixed kernel, so both minimise -LML; pre- and post-fit metrics are the metric's
    own ``get_metric``.  Start 0 is ``kernel.get_default_hyper_parameter(xrange, n, from_distribution)``, starts 1..
    are drawn with from_distribution=True under ``generator`` (a CPU torch.Generator; None: torch's global one).
    ``bounded`` None follows p_check_hyper_parameters.  After ``fit``, ``report`` holds one
    (f, status name, iterations) per start, ``points`` their accepted points, ``winner`` the index of the returned
    one, ``steps`` the gpk_fit_step launches and ``status_reads`` the host reads of the status words."""

    def __init__(self, data_input, gaussian_process, metric_type: met.MetricType, fitter_type: ft.FitterType,
                 from_distribution: bool, local_approx: mht.GlobalApproximationsType,
                 numerical_matrix_handling: mht.NumericalMatrixHandlingType, subset_size: int = None, *,
                 n_starts: int = 8, history: int = 8, max_iter: int = 200, gtol: float = 1e-5, ftol: float = 1e-9,
                 check_every: int = 8, generator: Optional[torch.Generator] = None, bounded: Optional[bool] = None):
        self._check_supported(data_input, gaussian_process, metric_type, local_approx, numerical_matrix_handling)
        if int(n_starts) < 1 or int(check_every) < 1:
            raise ValueError("n_starts and check_every must be >= 1")
        if not 1 <= int(history) <= nat.FIT_MAX_HISTORY:
            raise ValueError("history must be in [1, %d]" % nat.FIT_MAX_HISTORY)
        super().__init__(data_input, gaussian_process, metric_type, fitter_type, from_distribution, local_approx,
                         numerical_matrix_handling, subset_size)
        self.n_starts, self.history, self.max_iter = int(n_starts), int(history), int(max_iter)
        self.gtol, self.ftol, self.check_every = float(gtol), float(ftol), int(check_every)
        self.generator = generator
        self.bounded = bounded
        self.report: List[tuple] = []
        self.steps = 0
        self.status_reads = 0

    # -- what the class accepts (the k-fold sibling overrides the data-input part, the MSE siblings the metric) ----
    _METRICS = (met.MetricType.LL, met.MetricType.BIC)

    @classmethod
    def _check_data_input(cls, data_input):
        name = cls.__name__
        if isinstance(data_input, list):
            raise NotImplementedError("%s: a list of data inputs (k-fold) is not supported" % name)
        if isinstance(data_input, BatchDataInput):
            raise NotImplementedError("%s: BatchDataInput is not supported" % name)
        if not isinstance(data_input, DataInput):
            raise NotImplementedError("%s: data input %s is not supported" % (name, type(data_input).__name__))
        return [data_input]

    @classmethod
    def _check_supported(cls, data_input, gaussian_process, metric_type, local_approx, numerical_matrix_handling):
        name = cls.__name__
        inputs = cls._check_data_input(data_input)
        if metric_type not in cls._METRICS:
            raise NotImplementedError("%s: metric %s is not supported (%s)"
                                      % (name, metric_type.name, ", ".join(t.name for t in cls._METRICS)))
        if local_approx is not mht.MatrixApproximations.NONE:
            raise NotImplementedError("%s: approximation %s is not supported" % (name, local_approx.name))
        if numerical_matrix_handling is not mht.NumericalMatrixHandlingType.CHOLESKY_BASED:
            raise NotImplementedError("%s: matrix handling %s is not supported (CHOLESKY_BASED)"
                                      % (name, numerical_matrix_handling.name))
        from ..MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
        for owner in inputs + [gaussian_process]:
            mean_function = getattr(owner, "mean_function", None)
            if mean_function is not None and not isinstance(mean_function, ZeroMeanFunction):
                raise NotImplementedError("%s: fitting with the non-zero mean function %s (its "
                                          "hyperparameters) is not supported" % (name, type(mean_function).__name__))

    # -- hooks of the shared loop: the data behind xrange / n, the batched evaluator, the reported metric ----
    def _reference_input(self):
        """The data input whose get_x_range() / n_train size the defaults and the bounds."""
        return self.data_input

    def _evaluator(self, kernel):
        """f(cands [S, n_hyp + 1], settle=False) -> (f [S], g [S, n_hyp + 1], info [S]) with .n_par."""
        from .. import sweep
        di = self.data_input
        return sweep.native_batched_value_and_gradient(kernel, di.data_x_train, di.get_detrended_y_train())

    def _metric_value(self, hyper_parameter, noise):
        return self.metric.get_metric(hyper_parameter, noise)

    # -- pieces (host only) ---------------------------------------------------------------------
    def _kernel(self):
        return self._gp.covariance_matrix.kernel

    def starts(self) -> torch.Tensor:
        """[n_starts, n_hyp + 1] host tensor: hyperparameters in DFS order, then the noise p_cov_matrix_jitter."""
        kernel = self._kernel()
        ref = self._reference_input()
        xrange, n = ref.get_x_range(), ref.n_train
        jitter = float(torch.as_tensor(global_param.p_cov_matrix_jitter))
        rows = [_flatten(kernel.get_default_hyper_parameter(xrange, n, self.from_distribution)) + [jitter]]
        if self.n_starts > 1:
            if self.generator is not None:
                # the kernels draw from torch's global generator: run them on the caller's stream of numbers
                with torch.random.fork_rng(devices=[]):
                    torch.set_rng_state(self.generator.get_state())
                    for _ in range(1, self.n_starts):
                        rows.append(_flatten(kernel.get_default_hyper_parameter(xrange, n, True)) + [jitter])
                    self.generator.set_state(torch.get_rng_state())
            else:
                for _ in range(1, self.n_starts):
                    rows.append(_flatten(kernel.get_default_hyper_parameter(xrange, n, True)) + [jitter])
        return torch.tensor(rows, dtype=torch.float64)

    def bounds(self):
        bounded = bool(global_param.p_check_hyper_parameters) if self.bounded is None else bool(self.bounded)
        ref = self._reference_input()
        return pack_bounds(self._kernel(), ref.get_x_range(), ref.n_train, bounded,
                           bool(global_param.p_optimize_noise))

    # -- the fit ------------------------------------------------------------------------------------
    def fit(self) -> Tuple:
        from .. import engine
        kernel = self._kernel()
        dims = kernel.get_hyper_parameter_dimensionalities()
        x0 = self.starts()
        lo, hi = self.bounds()
        n_par = int(x0.shape[1])
        pre_fit_metric = self._metric_value(split_winner(x0[0, :-1], dims), x0[0, -1].clone())

        evaluate = self._evaluator(kernel)
        if evaluate.n_par != n_par:
            raise ValueError("the kernel's device program has %d hyperparameters, its defaults %d"
                             % (evaluate.n_par - 1, n_par - 1))
        state = engine.LbfgsState(x0, torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64),
                                  history=self.history, max_iter=self.max_iter, gtol=self.gtol, ftol=self.ftol)
        # every restart needs at most max_iter accepted steps, each after at most max_backtracks + 1 trials, twice
        # (one steepest-descent restart per search) -- the loop ends long before on the status words
        limit = 2 * self.max_iter * (state.opts.max_backtracks + 2) + 2
        self.status_reads = 0
        status = None
        for k in range(limit):
            check = (k + 1) % self.check_every == 0
            # the first evaluation (a timed-out persistent run must not read as BAD_START) and the ones the status
            # read waits for anyway are verified; in between a timeout is a failed trial, i.e. one more backtrack
            f, g, info = evaluate(state.x_trial, settle=check or k == 0)
            state.step(f, g, info)
            if check:
                status = state.status.cpu()   # the planned host synchronisation
                self.status_reads += 1
                if not bool((status == nat.FIT_RUNNING).any()):
                    break
        self.steps = state.steps
        x, fx, _, iters = state.current()
        x, fx, iters, status = x.cpu(), fx.cpu(), iters.cpu(), state.status.cpu()
        self.report = [(float(fx[b]), nat.FIT_STATUS_NAMES[int(status[b])] if 0 <= int(status[b]) < 6 else "INVALID",
                        int(iters[b])) for b in range(self.n_starts)]
        ok = torch.isfinite(fx) & (status != nat.FIT_BAD_START) & (status >= 0)
        if not bool(ok.any()):
            raise RuntimeError("%s: no start has a finite objective (%s)" % (type(self).__name__, self.report))
        winner = int(torch.argmin(torch.where(ok, fx, torch.full_like(fx, math.inf))))
        self.winner = winner
        self.points = x            # [n_starts, n_hyp + 1]: every start's accepted point (host), the noise last
        hyper_parameter = split_winner(x[winner, :-1], dims)
        noise = x[winner, -1].clone()
        kernel.set_last_hyper_parameter(hyper_parameter)
        kernel.set_noise(noise)
        last = kernel.get_last_hyper_parameter()
        post_fit_metric = self._metric_value(last, kernel.get_noise())
        # (get_metric records its argument in the kernel, SURVEY Q9: the same list)
        return pre_fit_metric, post_fit_metric, kernel.get_last_hyper_parameter(), kernel.get_noise(), None

    # -- after the fit: how well the data determine the point -----------------------------------------
    _FISHER_OBJECTIVE = True   # the objective is -LML of one DataInput: its Fisher information is the fit's curvature

    def _require_fisher_objective(self, what: str) -> None:
        if not self._FISHER_OBJECTIVE:
            raise NotImplementedError("%s.%s: the objective of this fitter is not -LML of one data input, so the Fisher "
                                      "information of the likelihood is not the curvature of what was fitted"
                                      % (type(self).__name__, what))
        if getattr(self, "points", None) is None:
            raise RuntimeError("%s.%s: fit() first" % (type(self).__name__, what))

    def fisher_information(self) -> torch.Tensor:
        """F [n_hyp + 1, n_hyp + 1] (device) at the winning point of the last ``fit``: hyperparameters in DFS order,
        the noise last, from one B = 1 identity-augmented factorisation (engine.InverseFactorization.fisher)."""
        self._require_fisher_objective("fisher_information")
        from .. import engine
        di = self.data_input
        x = engine.as_device_f64(di.data_x_train).contiguous()
        n, d = int(x.shape[0]), int(x.shape[1])
        y = engine.as_device_f64(di.get_detrended_y_train()).reshape(1, n).contiguous()
        kd = engine.kernel_descriptor(self._kernel(), d)
        point = engine.host_f64_to_device([float(v) for v in self.points[self.winner]])
        f = engine.InverseFactorization(n, d, 1, torch.float64)
        f.run(kd, point[:-1], 0, point[-1:], 0, x, 0, y, 0, gradient=False)
        return f.fisher()[0]

    def standard_errors(self) -> torch.Tensor:
        """[n_hyp + 1] host tensor: sqrt(diag(F_free^-1)) of the winning point, scattered back to every position
        (:func:`standard_errors_from_fisher`).  NaN for a parameter that is pinned (lo == hi, e.g. the noise when
        p_optimize_noise is off) or sits on a bound; inf for a free parameter the data say nothing about."""
        self._require_fisher_objective("standard_errors")
        lo, hi = self.bounds()
        point = [float(v) for v in self.points[self.winner]]
        free = [lo[i] < point[i] < hi[i] for i in range(len(point))]
        return standard_errors_from_fisher(self.fisher_information().cpu(), free)


    # -- after the fit: the model at new points --------------------------------------------------------
    def predictor(self):
        """A :class:`Statistics.Predictor.PosteriorPredictor` at the winning point of the last ``fit``: kernel
        hyperparameters and noise from ``points[winner]``, one B = 1 identity-augmented factorisation of the training
        data; ``predictor().predict(x_new, return_var=True)`` then streams any new points through it."""
        name = type(self).__name__
        if isinstance(self.data_input, list):
            raise NotImplementedError("%s.predictor: the folds are a list of data inputs, there is no single "
                                      "training set to predict from" % name)
        if getattr(self, "points", None) is None:
            raise RuntimeError("%s.predictor: fit() first" % name)
        from ..Statistics.Predictor import PosteriorPredictor
        kernel = self._kernel()
        point = self.points[self.winner]
        hyper_parameter = split_winner(point[:-1], kernel.get_hyper_parameter_dimensionalities())
        mean_function = self._gp.mean_function
        mean_hyp = mean_function.get_last_hyper_parameter()
        if mean_hyp is None:
            mean_hyp = mean_function.get_default_hyper_parameter()
        return PosteriorPredictor(kernel, hyper_parameter, point[-1].clone(), mean_function, mean_hyp, self.data_input)


def standard_errors_from_fisher(fisher, free) -> torch.Tensor:
    """sqrt(diag(F_free^-1)) scattered to all positions (host, fp64): NaN where ``free`` is false, inf for a free
    parameter whose row of F is zero (no information), the inverse taken over the remaining ones."""
    import numpy as np
    F = np.asarray(torch.as_tensor(fisher, dtype=torch.float64).cpu())
    out = np.full(F.shape[0], np.nan)
    idx = [i for i in range(F.shape[0]) if free[i]]
    blind = [i for i in idx if not np.any(F[i, idx] != 0.0)]
    out[blind] = np.inf
    rest = [i for i in idx if i not in blind]
    if rest:
        try:
            var = np.diag(np.linalg.inv(F[np.ix_(rest, rest)]))
            out[rest] = np.where(var >= 0.0, np.sqrt(np.abs(var)), np.nan)
        except np.linalg.LinAlgError:   # (exactly singular among parameters that each have information)
            out[rest] = np.inf
    return torch.from_numpy(out)


class DeviceKfoldLbfgsFitter(DeviceLbfgsFitter):
    """:class:`DeviceLbfgsFitter` for a k-fold list of DataInputs: the objective is the mean of the folds' -LML
    (the reference's opt_kfold / opt_optimize_noise_kfold, Fitter.py:97-102), evaluated for every start and fold as
    ONE ragged identity-augmented batch per iteration (sweep.native_kfold_value_and_gradient -> gpk_grad_ragged): folds
    of Metrics/CrossValidation.get_data_inputs differ in n_train whenever n is not divisible.  The constructor arguments
    are the sibling's; ``data_input`` is the list.  xrange and n of the defaults and bounds come from fold 0, as
    upstream (Fitter.py:64-66); the pre- and post-fit metrics are the mean of the folds' ``get_metric``."""

    _FISHER_OBJECTIVE = False

    @classmethod
    def _check_data_input(cls, data_input):
        name = cls.__name__
        if not isinstance(data_input, list) or not data_input:
            raise NotImplementedError("%s: data_input must be a non-empty list of DataInputs (the folds); a single "
                                      "data input is DeviceLbfgsFitter's" % name)
        for fold in data_input:
            if isinstance(fold, BatchDataInput):
                raise NotImplementedError("%s: BatchDataInput folds are not supported" % name)
            if not isinstance(fold, DataInput):
                raise NotImplementedError("%s: fold of type %s is not supported" % (name, type(fold).__name__))
            if int(fold.n_train) < 1:
                raise NotImplementedError("%s: a fold without training points is not supported" % name)
        return list(data_input)

    def _reference_input(self):
        return self.data_input[0]

    def _evaluator(self, kernel):
        from .. import sweep
        return sweep.native_kfold_value_and_gradient(
            kernel, [(di.data_x_train, di.get_detrended_y_train()) for di in self.data_input])

    def _metric_value(self, hyper_parameter, noise):
        values = [m.get_metric(hyper_parameter, noise).reshape(1, 1) for m in self.metric]
        return torch.mean(torch.stack(values), dim=0)


def _check_has_test_points(name: str, data_input) -> None:
    x_test = getattr(data_input, "data_x_test", None)
    if x_test is None or int(x_test.shape[0]) < 1:
        raise NotImplementedError("%s: a data input without test points is not supported (the MSE is measured on "
                                  "them)" % name)


class DeviceMseLbfgsFitter(DeviceLbfgsFitter):
    """:class:`DeviceLbfgsFitter` for the exact, Cholesky-based held-out MSE of a DataInput with test data: the loop,
    starts, bounds and report are the sibling's; every iteration's evaluation is ONE batched factorisation with the
    test points as extra rows plus the MSE gradient pass (sweep.native_batched_mse_value_and_gradient ->
    gpk_mse_grad).  Pre- and post-fit metrics are MeanSquaredError.get_metric.  With a scaled kernel and an optimised
    noise the MSE is invariant along (sg, noise) -> (c sg, c noise): the minimiser is a ray, compare objective values."""

    _FISHER_OBJECTIVE = False

    _METRICS = (met.MetricType.MSE,)

    @classmethod
    def _check_data_input(cls, data_input):
        inputs = super()._check_data_input(data_input)
        _check_has_test_points(cls.__name__, inputs[0])
        return inputs

    def _evaluator(self, kernel):
        from .. import sweep
        di = self.data_input
        return sweep.native_batched_mse_value_and_gradient(kernel, di.data_x_train, di.get_detrended_y_train(),
                                                           di.data_x_test, di.get_detrended_y_test())


class DeviceKfoldMseLbfgsFitter(DeviceKfoldLbfgsFitter):
    """:class:`DeviceKfoldLbfgsFitter` for the mean of the folds' held-out MSE -- what CrossValidation(metric_type=MSE)
    evaluates -- for every start and fold as ONE ragged batch per iteration
    (sweep.native_kfold_mse_value_and_gradient -> gpk_mse_grad with n_dev / m_dev).  ``data_input`` is the list of
    folds, e.g. CrossValidation.get_data_inputs; every fold needs test points."""

    _METRICS = (met.MetricType.MSE,)

    @classmethod
    def _check_data_input(cls, data_input):
        folds = super()._check_data_input(data_input)
        for fold in folds:
            _check_has_test_points(cls.__name__, fold)
        return folds

    def _evaluator(self, kernel):
        from .. import sweep
        return sweep.native_kfold_mse_value_and_gradient(
            kernel, [(di.data_x_train, di.get_detrended_y_train(), di.data_x_test, di.get_detrended_y_test())
                     for di in self.data_input])


class DeviceLooLbfgsFitter(DeviceLbfgsFitter):
    """:class:`DeviceLbfgsFitter` for the exact leave-one-out objective of a DataInput (Metrics/LeaveOneOut.py):
    ``metric_type`` LL fits by minus the LOO log predictive density, MSE by the LOO mean squared error.  The loop,
    starts, bounds and report are the sibling's; every iteration's evaluation is ONE batched identity-augmented
    factorisation plus the LOO pass (sweep.native_batched_loo_value_and_gradient -> gpk_loo_grad).  Pre- and post-fit
    metrics are LeaveOneOut.get_metric.  The LOO-MSE is invariant under K -> c K: with a scaled kernel and an optimised
    noise its minimiser is a ray, compare objective values (or pin the noise)."""

    _FISHER_OBJECTIVE = False

    _METRICS = (met.MetricType.LL, met.MetricType.MSE)

    def __init__(self, data_input, gaussian_process, metric_type: met.MetricType, fitter_type: ft.FitterType,
                 from_distribution: bool, local_approx: mht.GlobalApproximationsType,
                 numerical_matrix_handling: mht.NumericalMatrixHandlingType, subset_size: int = None, **kwargs):
        super().__init__(data_input, gaussian_process, metric_type, fitter_type, from_distribution, local_approx,
                         numerical_matrix_handling, subset_size, **kwargs)
        from ..Metrics.LeaveOneOut import LeaveOneOut
        self.metric = LeaveOneOut(data_input, self._gp.covariance_matrix, local_approx, numerical_matrix_handling,
                                  subset_size, loss=metric_type)

    def _evaluator(self, kernel):
        from .. import sweep
        di = self.data_input
        return sweep.native_batched_loo_value_and_gradient(kernel, di.data_x_train, di.get_detrended_y_train(),
                                                           self.metric.loss_code)
