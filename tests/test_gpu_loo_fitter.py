"""DeviceLooLbfgsFitter end to end on the MI355X against SciPy's L-BFGS-B on the restatement of tests/loo_support.py.

N = 96, D = 1, the data of the SE case of tests/test_gpu_fitter.py (targets drawn from an SE prior, length scale 0.12,
plus noise 0.05), the unscaled SE kernel, 8 starts, bounded.  Cases: the log predictive density with the noise
optimised (from its lower bound 1e-3) and pinned (at 0.05); the LOO mean squared error with the noise optimised (the
kernel is unscaled, so the MSE has no flat direction).  Objective values are compared, never points.

The bar on device_best - scipy_best is twice the larger of ftol max(1, |f|) and the spread (max - min) of SciPy's own
converged minima over the same 8 starts: a measurement on the reference alone, taken in the test.  It means something
because SciPy converges from every start to one and the same minimiser here (asserted; checked on the CPU for
START_SEED before the device ran), so the spread is SciPy's own scatter at that point.
"""
import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceLooLbfgsFitter, pack_bounds
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import loo_support as ls
from tests import mse_support as ms
from tests.test_gpu_fitter import E2E_FTOL, E2E_NOISE, _x, e2e_jitter, e2e_scipy, e2e_targets

pytestmark = pytest.mark.gpu

START_SEED = ls.FIT_START_SEED   # SciPy's L-BFGS-B converges from all 8 starts in the three cases (checked on the CPU)
GTOL = 1e-5
CASES = [(MetricType.LL, ls.LPD, True), (MetricType.LL, ls.LPD, False), (MetricType.MSE, ls.MSE, True)]


@pytest.fixture
def flags():
    gp.init(0)
    jitter = gp.p_cov_matrix_jitter
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False
    gp.p_cov_matrix_jitter = jitter


@pytest.mark.parametrize("metric_type,loss,optimize_noise", CASES)
def test_loo_fit_end_to_end(metric_type, loss, optimize_noise, flags):
    """Every start's accepted objective does not exceed its start's (both re-evaluated by the restatement); post-fit
    metric <= pre-fit metric and equal to LeaveOneOut.get_metric at the returned point; the winner against SciPy's best
    from the same starts (the bar of the module docstring); CONVERGED_G members pass gtol + the gradient bar in the
    restatement's projected gradient."""
    gp.p_optimize_noise = optimize_noise
    gp.p_cov_matrix_jitter = torch.tensor(e2e_jitter(optimize_noise), dtype=torch.float64)
    x, y = _x(), e2e_targets("SE", E2E_NOISE)
    assert x.shape == (96, 1)
    kernel = bk.SquaredExponentialKernel(1)
    di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    fitter = DeviceLooLbfgsFitter(di, g, metric_type, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                                  mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=8, gtol=GTOL, ftol=E2E_FTOL,
                                  generator=torch.Generator().manual_seed(START_SEED), bounded=True)
    x0 = fitter.starts().numpy()
    fitter.generator = torch.Generator().manual_seed(START_SEED)
    lo, hi = (np.array(v) for v in pack_bounds(kernel, di.get_x_range(), di.n_train, True, optimize_noise))
    fn = ls.objective(ls.SE, x, y, loss)

    pre, post, hyp, noise, indices = fitter.fit()
    print(metric_type.name, "noise optimised", optimize_noise, "report", fitter.report, "steps", fitter.steps)
    assert indices is None and pre.shape == (1, 1) and post.shape == (1, 1) and float(post) <= float(pre)
    assert fitter.status_reads == fitter.steps // fitter.check_every
    again = fitter.metric.get_metric(kernel.get_last_hyper_parameter(), kernel.get_noise())
    assert abs(float(again) - float(post)) <= 1e-12 * abs(float(post))
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
        assert abs(fb - fdev[b]) <= ls.VALUE_REL * abs(fb)          # the device's value is the restatement's
        assert fb <= f0, (b, fb, f0)                                 # accepted steps never went up
        if status[b] == "CONVERGED_G":
            pg = ms.projected_gradient_inf(pts[b], gb, lo, hi)
            bar = GTOL + ls.grad_bar(gb)
            print("  start %d %s projected gradient %.3e (bar %.3e) f %.12e" % (b, status[b], pg, bar, fb))
            assert pg <= bar, (b, pg, bar)
    device_best, _ = fn(pts[w])
    assert abs(float(post) - device_best) <= ls.VALUE_REL * abs(device_best)

    ref = e2e_scipy(fn, x0, lo, hi)
    assert all(c for _, _, c in ref)
    minima = np.array([f for f, _, _ in ref])
    points = np.array([p for _, p, _ in ref])
    k = int(np.argmin(minima))
    assert np.max(np.abs(points - points[k])) <= 1e-3        # one minimiser from every start: the spread is SciPy's scatter
    scipy_best, spread = float(minima[k]), float(np.max(minima) - np.min(minima))
    floor = E2E_FTOL * max(1.0, abs(scipy_best))
    gap = device_best - scipy_best
    print(metric_type.name, "noise optimised", optimize_noise,
          "device_best - scipy_best = %.3e (SciPy's spread %.3e, floor %.3e)" % (gap, spread, floor))
    assert gap <= 2.0 * max(floor, spread)
