"""The k-fold problems of tests/test_gpu_ragged_grad.py and tests/test_ragged_grad_host.py: folds, the oracle's mean
-LML over them, the fitter's construction and SciPy's runs on the oracle (host only; no GPU needed to import this).

The end-to-end construction is the one of tests/test_gpu_fitter.py: N = 96 points on [0, 1], targets drawn from an SE
prior (length scale 0.12, noise 0.05), 8 starts, bounded, the two noise settings and the tolerances of its e2e cases."""
import numpy as np
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceKfoldLbfgsFitter, pack_bounds
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests.test_gpu_fitter import E2E_FTOL, E2E_NOISE, N_E2E, e2e_jitter, e2e_scipy

SE = ("SE", {})
KF_HYP = [0.12]                # the length scale the targets are drawn with (the SE case of tests/test_gpu_fitter.py)
KF_TEST_SIZES = (30, 32, 34)   # held-out points of the three folds of N = 96: 66, 64 and 62 training points
KF_TARGET_SEED = 11
KF_SPLIT_SEED = 4
KF_START_SEED = 2              # SciPy's L-BFGS-B converges from every start under both noise settings
                               # (tests/test_ragged_grad_host.py checks that with the oracle alone)


def split(n, test_sizes, seed):
    """[(sorted training indices, sorted held-out indices)]: consecutive blocks of one seeded permutation are held
    out, fold by fold (the scheme of Metrics/CrossValidation.get_data_inputs with blocks of the given sizes)."""
    perm = np.random.default_rng(seed).permutation(n)
    out, at = [], 0
    for k in test_sizes:
        te = np.sort(perm[at:at + k])
        tr = np.sort(np.concatenate([perm[:at], perm[at + k:]]))
        out.append((tr, te))
        at += k
    return out


def fold_arrays(x, y, test_sizes, seed):
    """[(x_train, y_train, x_test, y_test)] as numpy arrays."""
    return [(x[tr], y[tr], x[te], y[te]) for tr, te in split(len(x), test_sizes, seed)]


def oracle_mean(tree, folds, scaled=False, expanded=False):
    """v [n_hyp + 1] -> (mean over the folds of the oracle's -LML, its gradient [n_hyp + 1]); (inf, NaN) where a fold's
    K + noise I is not positive definite.  The folds are added in fold order and divided by their number."""
    def fn(v):
        try:
            f_sum, g_sum = 0.0, np.zeros(len(v))
            for k, (xt, yt, _, _) in enumerate(folds):
                f, gh, gn = ad.nlml_and_grad(tree, list(v[:-1]), v[-1], xt, yt, scaled, expanded)
                if not np.isfinite(f):
                    raise ValueError
                g = np.array([float(a) for a in gh] + [gn], dtype=np.float64)
                f_sum, g_sum = (f, g) if k == 0 else (f_sum + f, g_sum + g)
            return f_sum / len(folds), g_sum / len(folds)
        except Exception:
            return np.inf, np.full(len(v), np.nan)
    return fn


def e2e_problem():
    """(x [96, 1], y [96], folds as arrays): the SE targets of the fitter's e2e cases split into three unequal folds."""
    x = np.linspace(0.0, 1.0, N_E2E).reshape(-1, 1)
    K = o.kernel_matrix(SE, KF_HYP, x, x) + E2E_NOISE * np.eye(N_E2E)
    y = np.linalg.cholesky(K) @ np.random.default_rng(KF_TARGET_SEED).standard_normal(N_E2E)
    return x, y, fold_arrays(x, y, KF_TEST_SIZES, KF_SPLIT_SEED)


def data_inputs(folds):
    out = []
    for xt, yt, xs, ys in folds:
        di = DataInput(xt, yt.reshape(-1, 1), xs, ys.reshape(-1, 1))
        di.set_mean_function(ZeroMeanFunction(xt.shape[1]))
        out.append(di)
    return out


def e2e_fitter(folds, optimize_noise, seed=KF_START_SEED, cls=DeviceKfoldLbfgsFitter):
    """(fitter, kernel, x0 [8, 2], lo, hi) with the global flags of the e2e cases set (the caller restores them)."""
    gp.p_optimize_noise = optimize_noise
    gp.p_cov_matrix_jitter = torch.tensor(e2e_jitter(optimize_noise), dtype=torch.float64)
    kernel = bk.SquaredExponentialKernel(1)
    dis = data_inputs(folds)
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    fitter = cls(dis, g, MetricType.LL, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                 mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=8, ftol=E2E_FTOL,
                 generator=torch.Generator().manual_seed(seed), bounded=True)
    x0 = fitter.starts().numpy()
    fitter.generator = torch.Generator().manual_seed(seed)
    lo, hi = (np.array(v) for v in pack_bounds(kernel, dis[0].get_x_range(), dis[0].n_train, True, optimize_noise))
    return fitter, kernel, x0, lo, hi


def scipy_runs(folds, x0, lo, hi):
    """SciPy's L-BFGS-B on the oracle's mean -LML from every start: [(f, x, converged)]."""
    return e2e_scipy(oracle_mean(SE, folds), x0, lo, hi)
