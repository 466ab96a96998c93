"""Host side of the multi-start L-BFGS fitter (no GPU): the Optimizer package's contracts, bounds / noise packing,
gpk_fit_state_bytes, and the numpy restatement of the state machine (tests/fit_support.py) on its own."""
import ctypes
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _build, _native
from gaussianprocessfundamentals_amd.DataHandling.DataInput import BatchDataInput, DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as kop
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import LinearMeanFunction, ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer import Fitter as fitter_mod
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceLbfgsFitter, Fitter, GradientFitter
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import fit_support as fs

NONE, CHOL = mht.MatrixApproximations.NONE, mht.NumericalMatrixHandlingType.CHOLESKY_BASED


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_library()


@pytest.fixture(autouse=True)
def _flags():
    gp.init(0)
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False


def _problem(kernel=None, mean=None, n=24):
    x = np.linspace(0.0, 1.0, n).reshape(-1, 1)
    y = np.sin(6 * x)
    di = DataInput(x, y, x, y)
    di.set_mean_function(mean or ZeroMeanFunction(1))
    g = GaussianProcess(kernel or bk.SquaredExponentialKernel(1), mean or ZeroMeanFunction(1))
    return di, g


def _make(di, g, metric=MetricType.LL, approx=NONE, handling=CHOL, **kw):
    return DeviceLbfgsFitter(di, g, metric, FitterType.GRADIENT, False, approx, handling, **kw)


# ------------------------------------------------------------------------------------------------ the package
def test_fitter_type_values():
    assert FitterType.GRADIENT.value == (0,)       # the reference's trailing comma
    assert FitterType.NON_GRADIENT.value == 1
    assert issubclass(DeviceLbfgsFitter, GradientFitter) and issubclass(GradientFitter, Fitter)


def test_base_fitter_sets_up_the_metric():
    di, g = _problem()
    f = GradientFitter(di, g, MetricType.BIC, FitterType.GRADIENT, True, NONE, CHOL)
    assert g.data_input is di and f.data_input is di and f.type is FitterType.GRADIENT and f.from_distribution
    assert f.metric.type is MetricType.BIC if hasattr(f.metric, "type") else True
    assert f.fit() is None


def test_supported_combinations_construct():
    di, g = _problem()
    for metric in (MetricType.LL, MetricType.BIC):
        f = _make(di, g, metric)
        assert (f.n_starts, f.history, f.max_iter, f.gtol, f.ftol, f.check_every) == (8, 8, 200, 1e-5, 1e-9, 8)
        assert f.generator is None and f.bounded is None


@pytest.mark.parametrize("what", ["MSE", "BatchDataInput", "k-fold", "BASIC_NYSTROEM", "SKI", "SKC_LOWER_BOUND",
                                  "SOD_RANDOM", "STRICT_INVERSE", "LINEAR_CONJUGATE_GRADIENT", "LinearMeanFunction"])
def test_unsupported_combinations_are_named(what):
    di, g = _problem()
    kw = {}
    if what == "MSE":
        kw["metric"] = MetricType.MSE
    elif what == "BatchDataInput":
        x = np.linspace(0, 1, 16).reshape(2, 8, 1)
        di = BatchDataInput(x, np.sin(x), None, None, test_ratio=0)
    elif what == "k-fold":
        di = [di, di]
    elif what in ("BASIC_NYSTROEM", "SKI", "SKC_LOWER_BOUND"):
        kw["approx"] = mht.MatrixApproximations[what]
    elif what == "SOD_RANDOM":
        kw["approx"] = mht.SubsetOfDataApproaches.SOD_RANDOM
    elif what in ("STRICT_INVERSE", "LINEAR_CONJUGATE_GRADIENT"):
        kw["handling"] = mht.NumericalMatrixHandlingType[what]
    else:
        di, g = _problem(mean=LinearMeanFunction(1))
    with pytest.raises(NotImplementedError, match=what):
        _make(di, g, **kw)


# ------------------------------------------------------------------------------------ bounds, noise, winner
def _add_kernel():
    return kop.AdditionOperator(2, [bk.SquaredExponentialKernel(2, ard=True), bk.PeriodicKernel(2)])


def test_bounds_and_noise_packing():
    k = _add_kernel()
    xr, n = [[0.0, 2.0], [0.0, 2.0]], 40
    jit = float(gp.p_cov_matrix_jitter)
    kb = k.get_hyper_parameter_bounds(xr, n)          # SE l (one pair for the ARD vector), PER l, PER p
    assert len(kb) == 3
    # bounded, noise optimised: the ARD pair repeated over its two values, then PER's, then [jitter, inf)
    lo, hi = fitter_mod.pack_bounds(k, xr, n, True, True)
    assert lo == [float(kb[0][0])] * 2 + [float(kb[1][0]), float(kb[2][0]), jit]
    assert hi == [float(kb[0][1])] * 2 + [float(kb[1][1]), float(kb[2][1]), math.inf]
    # bounded, noise pinned
    lo, hi = fitter_mod.pack_bounds(k, xr, n, True, False)
    assert lo[-1] == hi[-1] == jit and lo[:-1] == [float(kb[0][0])] * 2 + [float(kb[1][0]), float(kb[2][0])]
    # unbounded: +-inf everywhere, the noise free below as well -- or pinned
    lo, hi = fitter_mod.pack_bounds(k, xr, n, False, True)
    assert lo == [-math.inf] * 5 and hi == [math.inf] * 5
    lo, hi = fitter_mod.pack_bounds(k, xr, n, False, False)
    assert lo == [-math.inf] * 4 + [jit] and hi == [math.inf] * 4 + [jit]
    # a scaled kernel's signal variance keeps its +inf upper bound
    gp.p_scaled_base_kernel = True
    try:
        lo, hi = fitter_mod.pack_bounds(bk.SquaredExponentialKernel(1), [[0.0, 1.0]], 10, True, True)
        assert hi[1] == math.inf and lo[1] == 100 * jit and len(lo) == 3
    finally:
        gp.p_scaled_base_kernel = False


def test_bounded_follows_the_global_flag():
    di, g = _problem()
    f = _make(di, g)
    assert f.bounds()[0][0] == -math.inf
    gp.p_check_hyper_parameters = True
    assert f.bounds()[0][0] == float(g.kernel.get_hyper_parameter_bounds(di.get_x_range(), di.n_train)[0][0])
    assert _make(di, g, bounded=False).bounds()[0][0] == -math.inf
    gp.p_optimize_noise = True
    lo, hi = f.bounds()
    assert lo[-1] == float(gp.p_cov_matrix_jitter) and hi[-1] == math.inf


def test_winner_split_offsets():
    k = _add_kernel()
    dims = k.get_hyper_parameter_dimensionalities()
    assert dims == [[2], [], []]
    flat = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    parts = fitter_mod.split_winner(flat, dims)
    assert [p.shape for p in parts] == [torch.Size([2]), torch.Size([]), torch.Size([])]
    assert parts[0].tolist() == [1.0, 2.0] and float(parts[1]) == 3.0 and float(parts[2]) == 4.0
    k.set_last_hyper_parameter(parts)
    assert [torch.as_tensor(h).reshape(-1).tolist() for h in k.get_last_hyper_parameter()] == [[1.0, 2.0], [3.0], [4.0]]
    with pytest.raises(ValueError):
        fitter_mod.split_winner(torch.zeros(5, dtype=torch.float64), dims)


def test_starts_are_seeded_and_start_zero_is_the_default():
    di, g = _problem(kop.AdditionOperator(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1)]))
    gen = torch.Generator().manual_seed(5)
    a = _make(di, g, n_starts=6, generator=gen).starts()
    b = _make(di, g, n_starts=6, generator=torch.Generator().manual_seed(5)).starts()
    assert a.shape == (6, 4) and torch.equal(a, b)
    width = di.get_x_range()[0][1] - di.get_x_range()[0][0]
    assert a[0].tolist() == [width / 10.0] * 3 + [float(gp.p_cov_matrix_jitter)]
    assert len({tuple(r.tolist()) for r in a}) == 6
    # the generator advanced: the next draw differs
    assert not torch.equal(_make(di, g, n_starts=6, generator=gen).starts()[1:], a[1:])


# ----------------------------------------------------------------------------------------- gpk_fit_state_bytes
def test_state_bytes_layout_and_monotone(lib):
    base = _native.fit_state_bytes(3, 2, _native.GpkFitOpts(m=4))
    assert base == 2 * 8 * (_native.FIT_HEADER + 5 * 3 + 4 + 2 * 4 * 3)
    assert _native.fit_state_bytes(4, 2, _native.GpkFitOpts(m=4)) > base
    assert _native.fit_state_bytes(3, 2, _native.GpkFitOpts(m=5)) > base
    assert _native.fit_state_bytes(3, 3, _native.GpkFitOpts(m=4)) > base
    assert _native.fit_state_bytes(3, 2) == _native.fit_state_bytes(3, 2, _native.GpkFitOpts())   # NULL: the defaults
    assert _native.fit_state_bytes(65, 1, _native.GpkFitOpts(m=16)) > 0
    assert ctypes.sizeof(_native.GpkFitOpts) == 4 * 4 + 3 * 8


@pytest.mark.parametrize("n_par,m,batch,word", [(0, 8, 1, "n_par"), (66, 8, 1, "n_par"), (3, 0, 1, "m (history)"),
                                                (3, 17, 1, "m (history)"), (3, 8, 0, "batch")])
def test_state_bytes_rejects(lib, n_par, m, batch, word):
    assert _native.fit_state_bytes(n_par, batch, _native.GpkFitOpts(m=m)) == 0
    err = _native.last_error()
    assert "invalid argument" in err and word in err


def test_fit_calls_reject_bad_arguments_before_any_device_work(lib):
    """Argument errors are found on the host (no GPU here): negative return, the argument named."""
    o = _native.GpkFitOpts()
    P = ctypes.c_void_p
    one = P(8)  # (never dereferenced: every call below fails its checks first)
    assert lib.gpk_fit_init(3, 2, ctypes.byref(o), one, 2, one, one, one, one, 3, None) == -5
    assert "x0_stride" in _native.last_error()
    assert lib.gpk_fit_init(3, 2, ctypes.byref(o), one, 3, one, one, one, one, 2, None) == -10
    assert lib.gpk_fit_step(3, 2, ctypes.byref(o), one, 0, one, 3, None, one, one, 3, one, None) == -5
    assert lib.gpk_fit_step(3, 2, ctypes.byref(o), one, 1, one, 2, None, one, one, 3, one, None) == -7
    assert "g_stride" in _native.last_error()
    assert lib.gpk_fit_step(66, 2, ctypes.byref(o), one, 1, one, 66, None, one, one, 66, one, None) == -1
    assert lib.gpk_fit_step(3, 2, ctypes.byref(_native.GpkFitOpts(m=17)), one, 1, one, 3, None, one, one, 3, one,
                            None) == -3
    assert lib.gpk_fit_current(3, 0, one, one, 3, one, one, 3, one, None) == -2
    assert lib.gpk_fit_current(3, 1, one, one, 2, one, one, 3, one, None) == -5


def test_library_without_fit_entries_still_loads(lib):
    class Old:
        gpk_abi_version = None
    assert _native.fit_supported(lib) and not _native.fit_supported(Old())


# ----------------------------------------------------------------------------- the restatement on its own
INF3 = np.full(3, np.inf)


def test_restatement_isotropic_quadratic_terminates():
    """H = c I, 3-D: the steepest-descent step is followed by a quasi-Newton step whose scaling
    gamma = s^T y / y^T y = 1 / c is the exact inverse Hessian, so the minimiser is reached (to rounding) within
    n_par + 2 accepted steps.  (That count is a property of exact line searches in general; with Armijo unit steps
    it holds for H = c I only -- rotated quadratics of condition 1.5 .. 10 take 6 .. 10 accepted steps, measured with
    this restatement, and are checked for convergence below, not for a step count.)"""
    xs = np.array([0.3, -0.2, 0.5])
    ft = fs.NumpyFitter(np.array([[2.0, 1.0, -1.0], [0.3, -0.2, 0.6], [-5.0, 4.0, 3.0]]), -INF3, INF3, fs.Opts(ftol=0.0))
    fs.drive(ft, fs.diag_quadratic(np.full(3, 7.0), xs))
    x, f, g, it = ft.current()
    assert np.all(ft.status == fs.CONVERGED_G) and np.all(it <= 3 + 2)
    assert np.abs(x - xs).max() <= 1e-5 / 7.0


def test_restatement_rotated_quadratic_converges():
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    A = Q @ np.diag([1.0, 3.0, 10.0]) @ Q.T
    xs = np.array([0.3, -0.2, 0.5])
    ft = fs.NumpyFitter(rng.standard_normal((4, 3)), -INF3, INF3, fs.Opts(ftol=0.0))
    fvals = []
    fs.drive(ft, fs.quadratic(A, xs), on_step=lambda k, F: fvals.append(F.current()[1].copy()))
    x, f, g, it = ft.current()
    assert np.all(ft.status == fs.CONVERGED_G)
    # |g|_inf <= gtol and g = A (x - x*): |x - x*|_inf <= |x - x*|_2 <= |g|_2 / lambda_min <= sqrt(3) gtol / 1
    assert np.abs(x - xs).max() <= math.sqrt(3) * 1e-5
    assert np.all(np.diff(np.array(fvals)[1:], axis=0) <= 0)      # accepted f never increases


def test_restatement_box_and_pinned_coordinate():
    xs = np.array([2.0, -3.0, 0.25, 0.7])
    lo = np.array([-1.0, -1.0, -1.0, 0.4])
    hi = np.array([1.0, 1.0, 1.0, 0.4])             # the last coordinate is pinned
    ft = fs.NumpyFitter(np.array([[0.0, 0.0, 0.0, 9.0], [0.9, -0.9, 0.9, -9.0]]), lo, hi, fs.Opts(ftol=0.0))
    seen = []
    fs.drive(ft, fs.diag_quadratic(np.array([1.0, 4.0, 2.0, 1.0]), xs), on_step=lambda k, F: seen.append(F.x_trial))
    seen = np.array(seen)
    assert np.all(seen >= lo) and np.all(seen <= hi)
    assert np.all(seen[:, :, 3] == 0.4)
    x = ft.current()[0]
    assert np.all(x[:, 0] == 1.0) and np.all(x[:, 1] == -1.0) and np.all(x[:, 3] == 0.4)   # the active face
    assert np.abs(x[:, 2] - 0.25).max() <= 1e-5 / 2.0
    assert np.all(ft.status == fs.CONVERGED_G)


def test_restatement_failed_trials_and_bad_start():
    wall = 0.5
    inner = fs.pseudo_huber([0.45, 0.0])

    def walled(X):
        f, g, _ = inner(X)
        bad = np.atleast_2d(X)[:, 0] > wall
        return np.where(bad, np.inf, f), np.where(bad[:, None], np.nan, g), bad.astype(np.int32)
    ft = fs.NumpyFitter(np.array([[-30.0, 2.0], [0.9, 0.0], [-50.0, 5.0]]), -np.full(2, np.inf), np.full(2, np.inf),
                        fs.Opts())
    crossed = []
    fs.drive(ft, walled, on_step=lambda k, F: crossed.append(F.x_trial[:, 0] > wall))
    assert ft.status[1] == fs.BAD_START and np.all(ft.status[[0, 2]] == fs.CONVERGED_G)
    assert np.all(np.any(np.array(crossed)[:, [0, 2]], axis=0))      # the far starts overshoot across the wall
    assert np.abs(ft.current()[0][[0, 2]] - [0.45, 0.0]).max() <= 2e-5


def test_two_loop_matches_dense_bfgs_inverse():
    """The two-loop recursion is the product with the BFGS inverse built from gamma I by the same pairs."""
    rng = np.random.default_rng(1)
    n = 5
    A = np.diag(fs.log_spaced(50.0, n))
    pairs = []
    for _ in range(4):
        s = rng.standard_normal(n)
        pairs.append((s, A @ s))
    s, y = pairs[-1]
    H = (np.dot(s, y) / np.dot(y, y)) * np.eye(n)
    for s, y in pairs:
        rho = 1.0 / np.dot(s, y)
        V = np.eye(n) - rho * np.outer(y, s)
        H = V.T @ H @ V + rho * np.outer(s, s)
    q = rng.standard_normal(n)
    np.testing.assert_allclose(fs.two_loop(q, pairs), H @ q, rtol=1e-12, atol=1e-13)


def test_restatement_leaves_a_concave_region():
    """f = sum log(1 + x_j^2) is concave for |x_j| > 1: the first pair of a far start is pushed on the convex side of the
    steepest-descent step or rejected (s^T y <= 0); a rejected pair clears the history, so no stale gamma scales the
    later steps, and the member reaches x* = 0 in a few dozen accepted steps instead of crawling to max_iter."""
    def fn(X):
        X = np.atleast_2d(X)
        return np.sum(np.log1p(X * X), axis=1), 2 * X / (1 + X * X), None
    ft = fs.NumpyFitter(np.array([[30.0, -4.0], [3.0, 50.0], [1.5, 1.5]]), -np.full(2, np.inf), np.full(2, np.inf),
                        fs.Opts(ftol=0.0))
    cleared = []
    fs.drive(ft, fn, on_step=lambda k, F: cleared.append([m.iters > 1 and not m.pairs for m in F.members]))
    x, f, g, it = ft.current()
    assert np.all(ft.status == fs.CONVERGED_G) and np.all(it < 100), (ft.status, it)
    assert np.any(cleared)                                # the rejection path ran
    assert np.abs(x).max() <= 1e-5                        # Hessian 2 I at x*: |x| <= gtol / 2
