"""Host side of the derivative matrices and the Fisher information (no GPU): the library's new entries, the
restatement against closed forms, the list shaping of get_derivative_matrices on a stub, and the refusals of the
metric, the likelihood and the fitters."""
import math
import os
import re

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _build, _native
from gaussianprocessfundamentals_amd.DataHandling.DataInput import BatchDataInput, DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Kernel as kmod
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.FisherInformation import (LaplaceEvidence, free_log_determinant,
                                                                       laplace_evidence)
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer import Fitter as fit
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import fisher_support as fs

NONE, CHOL = mht.MatrixApproximations.NONE, mht.NumericalMatrixHandlingType.CHOLESKY_BASED
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpk.h")
NAMES = ("gpk_kernel_jacobian_workspace_bytes", "gpk_kernel_jacobian", "gpk_fisher_workspace_bytes", "gpk_fisher")
SE = ("SE", {})


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_library()


@pytest.fixture(autouse=True)
def _flags():
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False


# ------------------------------------------------------------------------------------------------ the library
def test_library_has_the_entries(lib):
    assert _native.FISHER_ENTRIES == NAMES
    assert _native.fisher_supported(lib)
    _native.require_fisher(lib)
    header = open(HEADER).read()
    for name in NAMES:
        assert name in _native.EXPORTS
        assert getattr(lib, name).argtypes is not None
        assert re.search(r"\b%s\(" % name, header)
    assert lib.gpk_abi_version() == 7


def test_an_older_library_reads_as_unsupported():
    class Old:
        gpk_kernel_jacobian = gpk_fisher = None
    assert not _native.fisher_supported(Old())
    with pytest.raises(_native.NativeUnavailable, match="gpk_kernel_jacobian, gpk_fisher"):
        _native.require_fisher(Old())


# --------------------------------------------------------------------------------- the restatement, closed forms
def test_fisher_ref_at_one_point():
    for k, s2 in ((1.0, 0.05), (2.5, 0.3)):
        F = fs.fisher_ref(np.array([[k + s2]]), np.zeros((0, 1, 1)))
        assert F.shape == (1, 1)
        assert abs(F[0, 0] - 1.0 / (2.0 * (k + s2) ** 2)) <= 4 * np.finfo(float).eps * F[0, 0]


@pytest.mark.parametrize("n", [1, 7, 40])
def test_fisher_ref_of_se_at_spacing_50_l(n):
    """Points 50 l apart: exp(-1250) underflows, so K is exactly I and d_l K exactly 0."""
    l, s2 = 0.2, 0.05
    x = (50.0 * l) * np.arange(n, dtype=np.float64).reshape(-1, 1)
    K = fs.kernel_ref(SE, [l], x, x)
    assert np.array_equal(K, np.eye(n))
    J = fs.jacobian_ref(SE, [l], x, x)
    assert J.shape == (1, n, n) and not J.any()
    F = fs.fisher_ref(K + s2 * np.eye(n), J)
    fnn = n / (2.0 * (1.0 + s2) ** 2)
    assert F[0, 0] == 0.0 and F[0, 1] == 0.0 and F[1, 0] == 0.0
    assert abs(F[1, 1] - fnn) <= 4 * n * np.finfo(float).eps * fnn
    # scaled, sg = 1: d_sg K = I = d_noise K, so the sg / noise block is all F_nn
    Ks = fs.kernel_ref(SE, [l, 1.0], x, x, scaled=True)
    Fs = fs.fisher_ref(Ks + s2 * np.eye(n), fs.jacobian_ref(SE, [l, 1.0], x, x, scaled=True))
    assert not Fs[0].any() and not Fs[:, 0].any()
    assert np.all(np.abs(Fs[1:, 1:] - fnn) <= 4 * n * np.finfo(float).eps * fnn)


def test_fisher_ref_is_the_expected_hessian_of_the_oracle():
    """F against central second differences of E[-LML] is out of reach here; the identity used instead:
    F_pq = 1/2 sum_ij (K^-1 D_p K^-1)_ij (D_q)_ij, evaluated with an explicit inverse."""
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (23, 1))
    tree, hyp = ("ADD", [SE, ("PER", {})]), [0.3, 0.9, 0.5]
    K = fs.kernel_ref(tree, hyp, x, x) + 0.05 * np.eye(23)
    J = fs.jacobian_ref(tree, hyp, x, x)
    F = fs.fisher_ref(K, J)
    Ki = np.linalg.inv(K)
    D = list(J) + [np.eye(23)]
    for p in range(4):
        for q in range(4):
            ref = 0.5 * np.sum((Ki @ D[p] @ Ki) * D[q])
            assert abs(F[p, q] - ref) <= 1e-10 * max(1.0, abs(ref))
    assert np.array_equal(F, F.T) and np.linalg.eigvalsh(F).min() > 0


# ------------------------------------------------------------------------- get_derivative_matrices: list shaping
class _Stub:
    """A kernel whose planes come from the host: plane p holds the value p everywhere."""

    def __init__(self, kernel, n, m):
        self.kernel, self.n, self.m, self.calls = kernel, n, m, 0
        kernel._derivative_planes = self._planes

    def _planes(self, hyper_parameter, x, x_):
        self.calls += 1
        total = sum(max(1, torch.as_tensor(h).numel()) for h in hyper_parameter)
        return torch.arange(total, dtype=torch.float64).reshape(-1, 1, 1).expand(total, self.n, self.m).contiguous()


@pytest.mark.parametrize("case", ["scalar", "ard", "operator", "operator_ard"])
def test_derivative_matrices_list_shape(case):
    n, m, t = 5, 3, torch.tensor
    if case == "scalar":
        gp.p_scaled_base_kernel = True
        k, hyp = bk.SquaredExponentialKernel(1), [t(0.3, dtype=torch.float64), t(1.5, dtype=torch.float64)]
        shapes = [(n, m), (n, m)]
    elif case == "ard":
        gp.p_scaled_base_kernel = True
        k = bk.SquaredExponentialKernel(3, ard=True)
        hyp = [t([0.4, 0.7, 0.9], dtype=torch.float64), t(1.5, dtype=torch.float64)]
        shapes = [(3, n, m), (n, m)]
    elif case == "operator":
        k = ops.AdditionOperator(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1)])
        hyp = [t(v, dtype=torch.float64) for v in (0.3, 0.9, 0.5)]
        shapes = [(n, m)] * 3
    else:
        k = ops.MultiplicationOperator(2, [bk.SquaredExponentialKernel(2, ard=True), bk.PeriodicKernel(2)])
        hyp = [t([0.4, 0.7], dtype=torch.float64), t(0.9, dtype=torch.float64), t(0.5, dtype=torch.float64)]
        shapes = [(2, n, m), (n, m), (n, m)]
    stub = _Stub(k, n, m)
    x, x_ = np.zeros((n, k.get_dimensionality())), np.zeros((m, k.get_dimensionality()))
    out = k.get_derivative_matrices(hyp, x, x_)
    assert stub.calls == 1 and isinstance(out, list) and len(out) == len(hyp)
    assert [tuple(o.shape) for o in out] == shapes
    # entry k holds its own planes, in DFS order; the list maps back to the flat planes
    at = 0
    for o, h in zip(out, hyp):
        cnt = max(1, h.numel())
        flat = o.reshape(cnt, n, m)
        for e in range(cnt):
            assert bool((flat[e] == float(at + e)).all())
        at += cnt
    planes = kmod.stack_derivative_planes(out)
    assert tuple(planes.shape) == (at, n, m)
    back = kmod.split_derivative_planes(planes, hyp)
    assert all(torch.equal(a, b) for a, b in zip(back, out))
    # last_hyper_parameter is recorded as get_tf_tensor records it
    last = k.get_last_hyper_parameter()
    assert len(last) == len(hyp) and all(torch.equal(torch.as_tensor(a), b) for a, b in zip(last, hyp))
    with pytest.raises(ValueError, match="derivative planes"):
        kmod.split_derivative_planes(planes[:-1], hyp)
    with pytest.raises(AssertionError):
        k.get_derivative_matrices(hyp[:-1], x, x_)


# ------------------------------------------------------------------------------------------------- refusals
def _problem(n=24):
    x = np.linspace(0.0, 1.0, n).reshape(-1, 1)
    di = DataInput(x, np.sin(6 * x), x, np.sin(6 * x))
    di.set_mean_function(ZeroMeanFunction(1))
    return di, GaussianProcess(bk.SquaredExponentialKernel(1), ZeroMeanFunction(1))


def _batch_input():
    x = np.linspace(0, 1, 16).reshape(2, 8, 1)
    return BatchDataInput(x, np.sin(x), None, None, test_ratio=0)


@pytest.mark.parametrize("what", ["BatchDataInput", "BASIC_NYSTROEM", "SKI", "STRICT_INVERSE", "PSEUDO_INVERSE",
                                  "LINEAR_CONJUGATE_GRADIENT"])
def test_likelihood_refusals_are_named(what):
    di, g = _problem()
    approx, handling = NONE, CHOL
    if what == "BatchDataInput":
        di = _batch_input()
        bdi_gp = GaussianProcess(bk.SquaredExponentialKernel(1), ZeroMeanFunction(1))
        di.set_mean_function(ZeroMeanFunction(1))
        g = bdi_gp
    elif what in ("BASIC_NYSTROEM", "SKI"):
        approx = mht.MatrixApproximations[what]
    else:
        handling = mht.NumericalMatrixHandlingType[what]
    g.set_data_input(di)
    metric = get_metric_by_type(MetricType.LL, g, local_approx=approx, numerical_matrix_handling=handling)
    t = torch.tensor
    with pytest.raises(NotImplementedError, match="LogLikelihood.get_fisher_information: .*" + what):
        metric.get_fisher_information([t(0.3, dtype=torch.float64)], t(0.05, dtype=torch.float64))


@pytest.mark.parametrize("what", ["BatchDataInput", "BASIC_NYSTROEM", "STRICT_INVERSE"])
def test_metric_refusals_are_named(what):
    di, g = _problem()
    approx, handling = NONE, CHOL
    if what == "BatchDataInput":
        di = _batch_input()
    elif what == "BASIC_NYSTROEM":
        approx = mht.MatrixApproximations.BASIC_NYSTROEM
    else:
        handling = mht.NumericalMatrixHandlingType.STRICT_INVERSE
    with pytest.raises(NotImplementedError, match="LaplaceEvidence: .*" + what):
        LaplaceEvidence(di, g.covariance_matrix, approx, handling)


def test_metric_types_keep_the_reference_members():
    assert [m.name for m in MetricType] == ["LL", "MSE", "BIC", "blockwise_LL", "blockwise_MSE", "blockwise_BIC"]


def test_laplace_evidence_formula_and_free_parameters():
    F = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    nl = 12.5
    for free in ([0, 1, 2], [0, 1], [1]):
        sub = F[np.ix_(free, free)]
        ref = nl + 0.5 * np.linalg.slogdet(sub)[1] - 0.5 * len(free) * math.log(2 * math.pi)
        assert abs(laplace_evidence(nl, F, free) - ref) <= 1e-14 * abs(ref)
    # through the metric, on a stub evaluation: a pinned noise is excluded unless p_optimize_noise is on
    di, g = _problem()
    m = LaplaceEvidence(di, g.covariance_matrix)
    m._evaluate = lambda hyp, noise: (torch.tensor([nl], dtype=torch.float64), torch.as_tensor(F))
    for optimize, free in ((False, [0, 1]), (True, [0, 1, 2])):
        gp.p_optimize_noise = optimize
        out = m.get_metric([None, None], None)
        assert tuple(out.shape) == (1, 1)
        assert abs(float(out) - laplace_evidence(nl, F, free)) <= 1e-14 * abs(float(out))


def test_laplace_evidence_names_the_positions_without_information():
    """The hard INDICATOR change-point mask: d K / d cp = 0, so F has zero rows at the change points."""
    F = np.zeros((5, 5))
    F[2:, 2:] = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    with pytest.raises(ValueError, match=r"not positive definite.*position\(s\) \[0, 1\]"):
        free_log_determinant(F, [0, 1, 2, 3])
    di, g = _problem()
    m = LaplaceEvidence(di, g.covariance_matrix)
    m._evaluate = lambda hyp, noise: (torch.tensor([1.0], dtype=torch.float64), torch.as_tensor(F))
    with pytest.raises(ValueError, match=r"position\(s\) \[0, 1\]"):
        m.get_metric([None] * 4, None)
    # two parameters that carry the same information: the second one's pivot fails
    G = np.array([[2.0, 2.0, 0.0], [2.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match=r"position\(s\) \[1\]"):
        free_log_determinant(G, [0, 1, 2])
    with pytest.raises(ValueError, match="not finite"):
        free_log_determinant(np.full((2, 2), np.nan), [0, 1])
    assert abs(free_log_determinant(G, [0, 2]) - math.log(2.0)) <= 1e-15


def test_standard_errors_from_fisher():
    F = np.array([[4.0, 1.0, 0.0, 0.5], [1.0, 3.0, 0.0, 0.2], [0.0, 0.0, 0.0, 0.0], [0.5, 0.2, 0.0, 2.0]])
    se = fit.standard_errors_from_fisher(F, [True, True, True, False]).numpy()
    ref = np.sqrt(np.diag(np.linalg.inv(F[:2, :2])))
    assert np.allclose(se[:2], ref, rtol=1e-14) and np.isinf(se[2]) and np.isnan(se[3])
    se = fit.standard_errors_from_fisher(F, [True, True, False, True]).numpy()
    keep = [0, 1, 3]
    assert np.allclose(se[keep], np.sqrt(np.diag(np.linalg.inv(F[np.ix_(keep, keep)]))), rtol=1e-14)
    assert np.isnan(se[2])


def _make(cls, di, g, metric):
    return cls(di, g, metric, FitterType.GRADIENT, False, NONE, CHOL)


@pytest.mark.parametrize("name", ["DeviceMseLbfgsFitter", "DeviceLooLbfgsFitter", "DeviceKfoldLbfgsFitter",
                                  "DeviceKfoldMseLbfgsFitter"])
def test_fitters_with_another_objective_refuse(name):
    di, g = _problem()
    cls = getattr(fit, name)
    kfold = "Kfold" in name
    metric = MetricType.MSE if "Mse" in name else MetricType.LL
    f = _make(cls, [di, di] if kfold else di, g, metric)
    for accessor in ("fisher_information", "standard_errors"):
        with pytest.raises(NotImplementedError, match="%s.%s: .*not -LML" % (name, accessor)):
            getattr(f, accessor)()


def test_the_lml_fitter_asks_for_a_fit_first():
    di, g = _problem()
    f = _make(fit.DeviceLbfgsFitter, di, g, MetricType.LL)
    for accessor in ("fisher_information", "standard_errors"):
        with pytest.raises(RuntimeError, match="fit\\(\\) first"):
            getattr(f, accessor)()
