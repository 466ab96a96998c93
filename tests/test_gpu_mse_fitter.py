"""DeviceMseLbfgsFitter / DeviceKfoldMseLbfgsFitter end to end on the MI355X against SciPy's L-BFGS-B on the
restatement of tests/mse_support.py.

N = 96 training and 32 test points (k-fold: four folds of n = 103), D = 1, targets drawn from an SE prior (length
scale 0.12) plus noise 0.05, the unscaled SE kernel, 8 starts, bounded, the noise optimised (from its lower bound 1e-3)
and pinned (at 0.05).  The MSE has several local minima here and, with a free noise, its minimiser sits far from the
drawn noise: objective values are compared, never points.
"""
import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import CrossValidation as cv
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import (DeviceKfoldMseLbfgsFitter, DeviceMseLbfgsFitter,
                                                              pack_bounds)
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import mse_support as ms
from tests.test_gpu_fitter import E2E_FTOL, e2e_jitter, e2e_scipy

pytestmark = pytest.mark.gpu

SE = ("SE", {})
START_SEED = 2   # SciPy's L-BFGS-B converges from all 8 starts in the four cases below (checked on the CPU)
GTOL = 1e-5
# the largest device_best - scipy_best measured on the MI355X over the four cases (DESIGN.md section 23 lists them);
# the bar is twice it, and never below the floor ftol max(1, |f|) -- the form of tests/test_gpu_fitter.py
MSE_MEASURED_GAP = 3.981e-13   # (single input, noise pinned; the other three: -6.211e-13, 6.251e-14, 4.885e-15)


@pytest.fixture
def flags():
    gp.init(0)
    jitter = gp.p_cov_matrix_jitter
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False
    gp.p_cov_matrix_jitter = jitter


def _data_input(x, y, xs, ys):
    di = DataInput(x, y.reshape(-1, 1), xs, ys.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    return di


def _run(kfold, optimize_noise):
    gp.p_optimize_noise = optimize_noise
    gp.p_cov_matrix_jitter = torch.tensor(e2e_jitter(optimize_noise), dtype=torch.float64)
    kernel = bk.SquaredExponentialKernel(1)
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    if kfold:
        x, y = ms.kfold_problem()
        folds = ms.kfold_arrays(x, y)
        np.random.seed(ms.KF_SPLIT_SEED)
        data = cv.get_data_inputs(_data_input(x, y, x, y), ms.KF_RATIO)
        for di, (xt, yt, xs, ys) in zip(data, folds):   # the folds the restatement sees are the package's
            di.set_mean_function(ZeroMeanFunction(1))
            assert np.array_equal(di.data_x_train.cpu().numpy(), xt) and np.array_equal(di.data_x_test.cpu().numpy(), xs)
        assert len(data) == 4 and len({int(d.n_train) for d in data}) == 2
        cls, ref = DeviceKfoldMseLbfgsFitter, data[0]
    else:
        folds = [ms.fit_problem()]
        data = _data_input(*folds[0])
        cls, ref = DeviceMseLbfgsFitter, data
    fitter = cls(data, g, MetricType.MSE, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                 mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=8, gtol=GTOL, ftol=E2E_FTOL,
                 generator=torch.Generator().manual_seed(START_SEED), bounded=True)
    x0 = fitter.starts().numpy()
    fitter.generator = torch.Generator().manual_seed(START_SEED)
    lo, hi = (np.array(v) for v in pack_bounds(kernel, ref.get_x_range(), ref.n_train, True, optimize_noise))
    return fitter, kernel, x0, lo, hi, ms.objective(SE, folds)


@pytest.mark.parametrize("optimize_noise", [True, False])
@pytest.mark.parametrize("kfold", [False, True])
def test_mse_fit_end_to_end(kfold, optimize_noise, flags):
    """Every start's accepted objective does not exceed its start's (both re-evaluated by the restatement); post-fit
    MSE <= pre-fit MSE; the winner against SciPy's best from the same starts (measured bar, below); CONVERGED_G
    members pass gtol + the gradient bar in the restatement's projected gradient."""
    fitter, kernel, x0, lo, hi, fn = _run(kfold, optimize_noise)
    pre, post, hyp, noise, indices = fitter.fit()
    print("kfold", kfold, "noise optimised", optimize_noise, "report", fitter.report, "steps", fitter.steps)
    assert indices is None and float(post) <= float(pre)
    assert fitter.status_reads == fitter.steps // fitter.check_every
    again = fitter._metric_value(kernel.get_last_hyper_parameter(), kernel.get_noise())
    assert torch.equal(torch.as_tensor(again).reshape(-1), torch.as_tensor(post).reshape(-1))
    if not optimize_noise:
        assert float(noise) == e2e_jitter(False)
    status = [r[1] for r in fitter.report]
    fdev = np.array([r[0] for r in fitter.report])
    pts = fitter.points.numpy()
    w = fitter.winner
    assert fdev[w] == np.min(fdev[np.isfinite(fdev)])
    assert np.all(pts >= lo) and np.all(pts <= hi)
    start = np.minimum(np.maximum(x0, lo), hi)
    for b in range(8):
        fb, gb = fn(pts[b])
        f0, _ = fn(start[b])
        assert abs(fb - fdev[b]) <= ms.VALUE_REL * abs(fb)          # the device's value is the restatement's
        assert fb <= f0, (b, fb, f0)                                 # accepted steps never went up
        if status[b] == "CONVERGED_G":
            pg = ms.projected_gradient_inf(pts[b], gb, lo, hi)
            bar = GTOL + ms.grad_bar(gb)
            print("  start %d %s projected gradient %.3e (bar %.3e) f %.12e" % (b, status[b], pg, bar, fb))
            assert pg <= bar, (b, pg, bar)
    device_best, _ = fn(pts[w])
    assert abs(float(post) - device_best) <= ms.VALUE_REL * device_best
    ref = e2e_scipy(fn, x0, lo, hi)
    assert all(c for _, _, c in ref)
    scipy_best = min(f for f, _, _ in ref)
    gap = device_best - scipy_best
    floor = E2E_FTOL * max(1.0, abs(scipy_best))
    print("kfold", kfold, "noise optimised", optimize_noise, "device_best - scipy_best = %.3e (floor %.3e)" % (gap, floor))
    assert gap <= max(2 * MSE_MEASURED_GAP, floor)
