"""Host-side checks of the ragged -LML gradient (no GPU needed): the new C entries and their argument errors, the
fold reduction and candidate replication of sweep.native_kfold_value_and_gradient on CPU tensors, what
Optimizer.Fitter.DeviceKfoldLbfgsFitter accepts, and the SciPy convergence condition of the k-fold end-to-end case
(tests/test_gpu_ragged_grad.py) on its chosen seed, with the oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _build, _native, sweep
from gaussianprocessfundamentals_amd.DataHandling.DataInput import BatchDataInput, DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import LinearMeanFunction, ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceKfoldLbfgsFitter, DeviceLbfgsFitter
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import kfold_support as ks

NONE, CHOL = mht.MatrixApproximations.NONE, mht.NumericalMatrixHandlingType.CHOLESKY_BASED
NEW = ("gpk_assemble_inverse_ragged", "gpk_potrf_aug_ragged_ex", "gpk_grad_ragged", "gpk_nlml_grad_ragged")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_library()


@pytest.fixture(autouse=True)
def _flags():
    gp.init(0)
    jitter = gp.p_cov_matrix_jitter
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False
    gp.p_cov_matrix_jitter = jitter


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_new_symbols_are_exported_and_declared(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in _native.EXPORTS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert _native.RAGGED_GRAD_ENTRIES == NEW
    assert _native.ragged_grad_supported() and _native.ragged_grad_supported(lib)
    assert lib.gpk_abi_version() == 7   # additive entries: no new ABI number

    class Old:      # a library built before the entries existed still loads; the feature test says no
        gpk_abi_version = None
    assert not _native.ragged_grad_supported(Old())


def _se_kdesc():
    kd = _native.GpkKdesc()
    kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 1, 1, 1, 0
    kd.nodes[0].op, kd.nodes[0].hyp_offset, kd.nodes[0].ard_slot, kd.nodes[0].flags = _native.OP_SE, 0, 0, 0
    return kd


def test_argument_errors_come_before_any_device_work(lib):
    """The documented -i of include/gpk.h, found on the host (no GPU here): a missing n_dev, a layout planned with
    m != n, an invalid program, a workspace that is too small."""
    kd = _se_kdesc()
    good = _native.plan(_native.GPK_F64, 3, 300, 300, 1)
    rect = _native.plan(_native.GPK_F64, 3, 300, 0, 1)      # m != n
    K, Lg, Lr = ctypes.byref(kd), ctypes.byref(good), ctypes.byref(rect)
    one = ctypes.c_void_p(8)   # (never dereferenced: every call below fails its checks first)
    need = lib.gpk_grad_workspace_bytes(K, Lg)
    assert need == 3 * 15 * 2 * 8          # batch x lower 64-tiles of n = 300 x (n_hyp + 1) doubles

    # gpk_assemble_inverse_ragged(kd, lay, hyp, hs, noise, ns, X, xbs, y, ybs, n_dev, W, stream)
    assert lib.gpk_assemble_inverse_ragged(K, Lg, one, 1, one, 1, one, 300, one, 300, None, one, None) == -11
    assert "n_dev" in _native.last_error()
    assert lib.gpk_assemble_inverse_ragged(K, Lr, one, 1, one, 1, one, 300, one, 300, one, one, None) == -2
    assert "m = n" in _native.last_error()
    bad = _se_kdesc()
    bad.n_nodes = 0
    assert lib.gpk_assemble_inverse_ragged(ctypes.byref(bad), Lg, one, 1, one, 1, one, 300, one, 300, one, one,
                                           None) == -1

    # gpk_potrf_aug_ragged_ex(lay, W, Winv, info, flags, n_dev, m_dev, stream)
    eye = _native.AUG_EXTRA_IDENTITY
    assert lib.gpk_potrf_aug_ragged_ex(Lg, one, one, one, eye, None, one, None) == -6
    assert lib.gpk_potrf_aug_ragged_ex(Lg, one, one, one, eye, one, None, None) == -7
    assert lib.gpk_potrf_aug_ragged_ex(Lg, one, one, one, 2, one, one, None) == -5
    rect_m = _native.plan(_native.GPK_F64, 3, 300, 20, 1)
    assert lib.gpk_potrf_aug_ragged_ex(ctypes.byref(rect_m), one, one, one, eye, one, one, None) == -1
    assert "m = n" in _native.last_error()

    # gpk_grad_ragged(kd, lay, hyp, hs, X, xbs, n_dev, W, info, grad, work, work_bytes, stream)
    assert lib.gpk_grad_ragged(K, Lg, one, 1, one, 300, None, one, one, one, one, need, None) == -7
    assert lib.gpk_grad_ragged(K, Lr, one, 1, one, 300, one, one, one, one, one, need, None) == -2
    assert lib.gpk_grad_ragged(ctypes.byref(bad), Lg, one, 1, one, 300, one, one, one, one, one, need, None) == -1
    assert lib.gpk_grad_ragged(K, Lg, one, 1, one, 300, one, one, one, one, one, need - 8, None) == -11
    assert "work" in _native.last_error()
    assert lib.gpk_grad_ragged(K, Lg, one, 1, one, 300, one, one, one, one, None, need, None) == -11
    assert lib.gpk_grad_ragged(K, Lg, one, 1, one, 300, one, one, one, None, one, need, None) == -10

    # gpk_nlml_grad_ragged(kd, lay, hyp, hs, noise, ns, X, xbs, y, ybs, n_dev, W, Winv, info, out, grad, work, bytes, s)
    def full(kdp, layp, n_dev=one, info=one, out=one, grad=one, work=one, nbytes=need):
        return lib.gpk_nlml_grad_ragged(kdp, layp, one, 1, one, 1, one, 300, one, 300, n_dev, one, one, info, out,
                                        grad, work, nbytes, None)
    assert full(K, Lg, n_dev=None) == -11
    assert full(K, Lr) == -2
    assert full(ctypes.byref(bad), Lg) == -1
    assert full(K, Lg, info=None) == -14
    assert full(K, Lg, out=None) == -15
    assert full(K, Lg, nbytes=need - 8) == -17
    assert full(K, Lg, work=None) == -17


def test_engine_class_needs_the_gpu():
    """No quiet fall-back: without a GPU the class raises NativeUnavailable (with one it plans m = n = max n_b)."""
    from gaussianprocessfundamentals_amd import engine
    if torch.cuda.is_available():
        f = engine.RaggedInverseFactorization([10, 7], 1)
        assert (f.layout.n, f.layout.m, f.batch) == (10, 10, 2)
    else:
        with pytest.raises(_native.NativeUnavailable):
            engine.RaggedInverseFactorization([10, 7], 1)


def test_program_runs_groups_consecutive_equal_programs():
    from gaussianprocessfundamentals_amd import engine
    a, b = _se_kdesc(), _se_kdesc()
    b.nodes[0].op = _native.OP_MAT52
    assert engine.program_runs([a, a, a]) == [(0, 3)]
    assert engine.program_runs([a, b, b, a]) == [(0, 1), (1, 3), (3, 4)]
    assert engine.program_runs([a]) == [(0, 1)]


# ------------------------------------------------------------------------------- replication and fold reduction
def test_candidate_replication_matches_numpy():
    rng = np.random.default_rng(0)
    S, F, n_hyp = 5, 3, 4
    c = rng.standard_normal((S, n_hyp + 1))
    hyp, noise = sweep.replicate_candidates(torch.tensor(c), F, _native.MAX_HYP)
    exp_h = np.zeros((S * F, _native.MAX_HYP))
    exp_n = np.zeros(S * F)
    for s in range(S):
        for f in range(F):
            exp_h[s * F + f, :n_hyp] = c[s, :n_hyp]
            exp_n[s * F + f] = c[s, n_hyp]
    assert hyp.shape == (S * F, _native.MAX_HYP) and hyp.is_contiguous() and noise.is_contiguous()
    assert np.array_equal(hyp.numpy(), exp_h) and np.array_equal(noise.numpy(), exp_n)


def test_fold_reduction_matches_numpy_and_has_a_fixed_order():
    rng = np.random.default_rng(1)
    S, F, k = 4, 3, 5
    v = rng.standard_normal(S * F) * 10.0 ** rng.integers(-8, 8, S * F)   # (the order of the additions shows)
    g = rng.standard_normal((S * F, k)) * 10.0 ** rng.integers(-8, 8, (S * F, 1))
    exp_v = np.array([((v[s * F] + v[s * F + 1]) + v[s * F + 2]) / 3.0 for s in range(S)])
    exp_g = np.stack([((g[s * F] + g[s * F + 1]) + g[s * F + 2]) / 3.0 for s in range(S)])
    assert np.array_equal(sweep.fold_mean(torch.tensor(v), F).numpy(), exp_v)
    assert np.array_equal(sweep.fold_mean(torch.tensor(g), F).numpy(), exp_g)
    # one failed fold: +inf value, NaN gradient, non-zero info for that candidate only
    v[4], g[4, 2] = np.inf, np.nan
    info = torch.zeros(S * F, dtype=torch.int32)
    info[4] = 7
    info[9] = -1
    fm, gm = sweep.fold_mean(torch.tensor(v), F).numpy(), sweep.fold_mean(torch.tensor(g), F).numpy()
    assert np.isinf(fm[1]) and np.isnan(gm[1, 2]) and np.all(np.isfinite(fm[[0, 2, 3]]))
    assert sweep.fold_info(info, F).tolist() == [0, 7, 0, 1] and sweep.fold_info(info, F).dtype == torch.int32


# --------------------------------------------------------------------------------------------- what the fitters take
def _folds(n=(20, 17, 19), mean=None):
    out = []
    for k, nk in enumerate(n):
        x = np.linspace(0.0, 1.0, nk).reshape(-1, 1) + 0.01 * k
        di = DataInput(x, np.sin(6 * x), x, np.sin(6 * x))
        di.set_mean_function(mean or ZeroMeanFunction(1))
        out.append(di)
    return out


def _make(dis, cls=DeviceKfoldLbfgsFitter, metric=MetricType.LL, approx=NONE, handling=CHOL, mean=None, **kw):
    g = GaussianProcess(bk.SquaredExponentialKernel(1), mean or ZeroMeanFunction(1))
    return cls(dis, g, metric, FitterType.GRADIENT, False, approx, handling, **kw)


def test_kfold_fitter_constructs_and_takes_range_and_n_from_fold_zero():
    dis = _folds()
    for metric in (MetricType.LL, MetricType.BIC):
        f = _make(dis, metric=metric, n_starts=4, generator=torch.Generator().manual_seed(3))
        assert isinstance(f, DeviceLbfgsFitter) and isinstance(f.metric, list) and len(f.metric) == 3
        assert (f.n_starts, f.history, f.max_iter, f.gtol, f.ftol, f.check_every) == (4, 8, 200, 1e-5, 1e-9, 8)
    single = _make(dis[0], cls=DeviceLbfgsFitter, n_starts=4, generator=torch.Generator().manual_seed(3))
    f = _make(dis, n_starts=4, generator=torch.Generator().manual_seed(3))
    assert torch.equal(f.starts(), single.starts())        # fold 0's get_x_range() and n_train (Fitter.py:64-66)
    assert f.bounds() == single.bounds()


@pytest.mark.parametrize("what", ["MSE", "BatchDataInput", "single", "BASIC_NYSTROEM", "SKI", "SOD_RANDOM",
                                  "STRICT_INVERSE", "LINEAR_CONJUGATE_GRADIENT", "LinearMeanFunction"])
def test_kfold_fitter_names_what_it_refuses(what):
    dis, kw = _folds(), {}
    if what == "MSE":
        kw["metric"] = MetricType.MSE
    elif what == "BatchDataInput":
        x = np.linspace(0, 1, 16).reshape(2, 8, 1)
        dis = [dis[0], BatchDataInput(x, np.sin(x), None, None, test_ratio=0)]
    elif what == "single":
        dis = dis[0]
    elif what in ("BASIC_NYSTROEM", "SKI"):
        kw["approx"] = mht.MatrixApproximations[what]
    elif what == "SOD_RANDOM":
        kw["approx"] = mht.SubsetOfDataApproaches.SOD_RANDOM
    elif what in ("STRICT_INVERSE", "LINEAR_CONJUGATE_GRADIENT"):
        kw["handling"] = mht.NumericalMatrixHandlingType[what]
    else:
        dis = _folds(mean=LinearMeanFunction(1))
        kw["mean"] = LinearMeanFunction(1)
    with pytest.raises(NotImplementedError, match="DeviceKfoldLbfgsFitter.*%s" % what):
        _make(dis, **kw)


def test_single_input_fitter_still_refuses_a_list():
    with pytest.raises(NotImplementedError, match="DeviceLbfgsFitter.*k-fold"):
        _make(_folds(), cls=DeviceLbfgsFitter)


def test_blockwise_gradient_names_the_strategies_it_leaves_out():
    from gaussianprocessfundamentals_amd.Metrics.LogLikelihood import BlockwiseLogLikelihood
    m = BlockwiseLogLikelihood(None, mht.MatrixApproximations.BASIC_NYSTROEM,
                               mht.NumericalMatrixHandlingType.PSEUDO_INVERSE)
    with pytest.raises(NotImplementedError, match="BASIC_NYSTROEM / PSEUDO_INVERSE"):
        m.get_metric_and_gradient([], torch.tensor(0.1, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="BASIC_NYSTROEM / PSEUDO_INVERSE"):
        m.get_gradients([], torch.tensor(0.1, dtype=torch.float64))


# ------------------------------------------------------------------------------------------ the chosen seed
@pytest.mark.parametrize("optimize_noise", [True, False])
def test_scipy_converges_from_every_start_on_the_chosen_seed(optimize_noise):
    """The k-fold end-to-end case compares the device fitter with SciPy's L-BFGS-B on the oracle's mean -LML from the
    same 8 starts; the seed of the starts (kfold_support.KF_START_SEED) is one for which SciPy converges from every
    one of them, under both noise settings, and every run reaches the same minimum to the f tolerance."""
    x, y, folds = ks.e2e_problem()
    assert [len(f[0]) for f in folds] == [66, 64, 62]
    _, _, x0, lo, hi = ks.e2e_fitter(folds, optimize_noise)
    assert x0.shape == (8, 2)
    runs = ks.scipy_runs(folds, x0, lo, hi)
    assert all(c for _, _, c in runs), runs
    best = min(f for f, _, _ in runs)
    assert max(f for f, _, _ in runs) - best <= 1e-8 * max(1.0, abs(best))
