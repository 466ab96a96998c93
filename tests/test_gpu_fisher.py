"""Fisher information on the HIP path (gpk_fisher, needs the MI355X) against the restatement
(tests/fisher_support.fisher_ref fed with the oracle's K and the autodiff planes, never the device's), closed forms,
and the properties the entry promises: bit-symmetric, deterministic, batch = singles, NaN where info != 0, W only read.

Bar against the restatement: the project's tolerance 1e-7 max(1, max|F_ref|).  For these inputs
cond(K + s2 I) <= (n k_max + s2) / s2 ~ 1.4e4, so the first-order error is ~1e-11 relative: the bar is a ceiling.  The
measured maximum is printed."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.FisherInformation import LaplaceEvidence
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceLbfgsFitter
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from tests import cp_support as cs
from tests import fisher_support as fs
from tests import rq_support as rs
from tests.helpers import hyp_list, set_flags
from tests.test_gpu_fitter import (E2E_FTOL, E2E_NOISE, E2E_NOISE_FLOOR, N_E2E, _x, e2e_flags,  # noqa: F401
                                   e2e_kernel, e2e_targets)
from tests.test_grad_oracle import _inputs

pytestmark = pytest.mark.gpu

NOISE = 0.05
EPS = float(np.finfo(np.float64).eps)
# name -> (tree, hyperparameter list, d, scaled, change-point mode)
CASES = {
    "SE": (("SE", {}), [0.3], 1, False, None),
    "SE_scaled": (("SE", {}), [0.3, 1.7], 1, True, None),
    "ADD(SE,PER)": (("ADD", [("SE", {}), ("PER", {})]), [0.3, 0.9, 0.5], 1, False, None),
    "MUL(SE,PER)": (("MUL", [("SE", {}), ("PER", {})]), [0.3, 0.9, 0.5], 1, False, None),
    "SE_ARD@3": (("SE", {"ard": True}), [[0.4, 0.7, 0.9]], 3, False, None),
    "RQ": (("RQ", {}), [0.4, 1.3], 1, False, None),
    "CP(SE,SE)": (("CP", [("SE", {}), ("SE", {})]), [0.5, 0.2, 0.3], 1, False, "SIGMOID"),
}
SIZES = [1, 65, 130, 333]


@pytest.fixture(autouse=True)
def _cp_mode():
    yield
    cs.set_mode("INDICATOR")


def _kernel(tree, hyp, d):
    if tree[0] == "RQ":
        return rs.make_kernel(tree, d)
    return cs.make_kernel(tree, hyp, d)


def _data(name, n):
    tree, hyp, d, scaled, mode = CASES[name]
    if mode:
        x, y, _ = cs.cp_inputs(n, 30 + n, hyp[:1])
    else:
        x, y = _inputs(n, d, 30 + n)
    return x, y


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    tree, hyp, d, scaled, mode = CASES[name]
    x, y = _data(name, n)
    K = fs.kernel_ref(tree, hyp, x, x, scaled, False, mode or "SIGMOID") + NOISE * np.eye(n)
    F = fs.fisher_ref(K, fs.jacobian_ref(tree, hyp, x, x, scaled, False, mode or "SIGMOID"))
    F.setflags(write=False)
    return K, F


def _activate(name):
    tree, hyp, d, scaled, mode = CASES[name]
    set_flags(scaled=scaled)
    if mode:
        cs.set_mode(mode)
    return tree, hyp, d


def _factor(name, n, noise=NOISE, hyps=None, gradient=True):
    """engine.InverseFactorization run on the case (hyps: one hyperparameter list per batch member)"""
    tree, hyp, d = _activate(name)
    x, y = _data(name, n)
    k = _kernel(tree, hyp, d)
    kd = engine.kernel_descriptor(k, d)
    dev = engine.device()
    rows = [hyp] if hyps is None else hyps
    H = torch.stack([engine.pack_hyper_parameter(hyp_list(h), kd.n_hyp) for h in rows]).contiguous()
    f = engine.InverseFactorization(n, d, len(rows), torch.float64)
    nz = torch.tensor([noise], dtype=torch.float64, device=dev)
    f.run(kd, H.reshape(-1), kd.n_hyp if len(rows) > 1 else 0, nz, 0, torch.as_tensor(x, device=dev).contiguous(), 0,
          torch.as_tensor(y, device=dev).reshape(1, -1).contiguous(), 0, gradient=gradient)
    return f


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_fisher_matches_the_restatement(name, n, factor_path):
    _, F_ref = _reference(name, n)
    f = _factor(name, n)
    F = f.fisher()
    assert tuple(F.shape) == (1,) + F_ref.shape
    assert int(f.info[0]) == 0
    got = F[0].cpu().numpy()
    scale = max(1.0, float(np.max(np.abs(F_ref))))
    err = float(np.max(np.abs(got - F_ref)))
    print("FISHERERR %s n=%d %s max|F-F_ref| = %.3e  rel to max|F_ref| = %.3e"
          % (name, n, factor_path, err, err / float(np.max(np.abs(F_ref)))))
    assert err <= 1e-7 * scale
    assert np.array_equal(got, got.T)                                     # bit for bit
    assert np.linalg.eigvalsh(got).min() >= -1e-7 * np.abs(got).max()
    # results("fisher") hands back the recorded matrix and the run's info
    rec, none, info = f.results("fisher")
    assert rec is F and none is None and info is f.info


def test_closed_form_at_one_point():
    for name, k in (("SE", 1.0), ("SE_scaled", 1.7)):
        F = _factor(name, 1).fisher()[0].cpu().numpy()
        fnn = 1.0 / (2.0 * (k + NOISE) ** 2)
        assert abs(F[-1, -1] - fnn) <= 4 * EPS * fnn
        assert F[0, 0] == 0.0 and not F[0].any() and not F[:, 0].any()    # d_l k(x, x) = 0 exactly
        if name == "SE_scaled":                                           # d_sg K = 1 = d_noise K at one point
            assert np.all(np.abs(F[1:, 1:] - fnn) <= 4 * EPS * fnn)


@pytest.mark.parametrize("n", [7, 130])
@pytest.mark.parametrize("scaled", [False, True])
def test_closed_form_at_spacing_50_l(n, scaled):
    """Points 50 l apart: K is exactly I and d_l K exactly 0, so F_ll = F_l,. = 0 (==) and every other entry
    n / (2 (1 + s2)^2) to 4 n eps."""
    l = 0.2
    set_flags(scaled=scaled)
    x = (50.0 * l) * np.arange(n, dtype=np.float64).reshape(-1, 1)
    k = _kernel(("SE", {}), None, 1)
    kd = engine.kernel_descriptor(k, 1)
    dev = engine.device()
    hyp = engine.pack_hyper_parameter(hyp_list([l, 1.0] if scaled else [l]), kd.n_hyp)
    f = engine.InverseFactorization(n, 1, 1, torch.float64)
    f.run(kd, hyp, 0, torch.tensor([NOISE], dtype=torch.float64, device=dev), 0, torch.as_tensor(x, device=dev), 0,
          torch.zeros(1, n, dtype=torch.float64, device=dev), 0, gradient=False)
    F = f.fisher()[0].cpu().numpy()
    fnn = n / (2.0 * (1.0 + NOISE) ** 2)
    assert not F[0].any() and not F[:, 0].any()
    assert np.all(np.abs(F[1:, 1:] - fnn) <= 4 * n * EPS * fnn)


def test_two_calls_give_the_same_bits_and_nothing_else_changes():
    f = _factor("ADD(SE,PER)", 130)
    nl, g, W = f.nlml().clone(), f.gradient().clone(), f.W.clone()
    F1 = f.fisher().clone()
    F2 = f.fisher()
    assert torch.equal(F1, F2)
    assert torch.equal(f.nlml(), nl) and torch.equal(f.gradient(), g) and torch.equal(f.W, W)
    assert bool(torch.isfinite(F1).all())
    # a fresh factorisation object gives the same bits too
    assert torch.equal(_factor("ADD(SE,PER)", 130).fisher(), F1)


def test_batch_of_three_equals_three_runs():
    """Member b of a batch against the same candidate alone: the Fisher pass is the same arithmetic on whatever W
    holds, so equal factors give equal bits; where the batched factorisation took another schedule than the single one
    the two differ by the factorisations' rounding, cond(K) eps ~ 1.4e4 * 1.1e-16, far below 1e-9 relative."""
    hyps = [[0.3, 0.9, 0.5], [0.2, 0.7, 0.8], [0.45, 1.2, 0.35]]
    with nat.thread_tune(chain=0):
        fb = _factor("MUL(SE,PER)", 130, hyps=hyps)
        Fb = fb.fisher()
        assert tuple(Fb.shape) == (3, 4, 4)
        # the pass on member b's slice of the batch's own W, as a batch of one through the ABI: the same bits
        L, lay, dev = nat.lib(), fb.layout, engine.device()
        lay1 = nat.plan(nat.GPK_F64, 1, 130, 130, 1)
        assert (lay1.ld, lay1.p, lay1.n_pad) == (lay.ld, lay.p, lay.n_pad)
        kd, hyp, hs, X, xs = fb._loo_operands[:5]
        need = int(L.gpk_fisher_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay1)))
        assert need == int(L.gpk_fisher_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay)))   # whatever the batch
        work = torch.empty(need // 8, dtype=torch.float64, device=dev)
        for b in range(3):
            F1 = torch.empty(4, 4, dtype=torch.float64, device=dev)
            nat.check(L.gpk_fisher(ctypes.byref(kd), ctypes.byref(lay1), engine._offset_ptr(hyp, b * hs), 0,
                                   nat.ptr(X), 0, engine._offset_ptr(fb.W, b * lay.w_batch_stride),
                                   engine._offset_ptr(fb.info, b), nat.ptr(F1), nat.ptr(work), need,
                                   nat.stream_handle(dev)), "gpk_fisher")
            assert torch.equal(F1, Fb[b])
        for b, h in enumerate(hyps):
            single = _factor("MUL(SE,PER)", 130, hyps=[h])
            if torch.equal(single.W[:fb.layout.w_batch_stride], fb.W[b * fb.layout.w_batch_stride:
                                                                       (b + 1) * fb.layout.w_batch_stride]):
                assert torch.equal(single.fisher()[0], Fb[b])             # the same factor: the same bits
            F1 = single.fisher()[0].cpu().numpy()
            assert np.abs(F1 - Fb[b].cpu().numpy()).max() <= 1e-9 * np.abs(F1).max()


def test_failed_member_is_nan_and_leaves_the_others_alone():
    f = _factor("SE_scaled", 65, noise=-0.5)
    assert int(f.info[0]) != 0
    assert bool(torch.isnan(f.fisher()).all())
    # in a batch: per-member noise, one member not positive definite
    tree, hyp, d = _activate("SE_scaled")
    x, y = _data("SE_scaled", 65)
    kd = engine.kernel_descriptor(_kernel(tree, hyp, d), d)
    dev = engine.device()
    H = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp)
    fb = engine.InverseFactorization(65, d, 2, torch.float64)
    fb.run(kd, H, 0, torch.tensor([NOISE, -0.5], dtype=torch.float64, device=dev), 1,
           torch.as_tensor(x, device=dev).contiguous(), 0, torch.as_tensor(y, device=dev).reshape(1, -1).contiguous(), 0)
    Fb = fb.fisher()
    assert int(fb.info[0]) == 0 and int(fb.info[1]) != 0
    assert bool(torch.isnan(Fb[1]).all())
    _, F_ref = _reference("SE_scaled", 65)
    assert np.abs(Fb[0].cpu().numpy() - F_ref).max() <= 1e-7 * max(1.0, np.abs(F_ref).max())


def test_fp32_is_refused():
    tree, hyp, d = _activate("SE")
    kd = engine.kernel_descriptor(_kernel(tree, hyp, d), d)
    f = engine.InverseFactorization(65, d, 1, torch.float32)
    with pytest.raises(NotImplementedError, match="Fisher information is fp64 only"):
        f.fisher()
    L = nat.lib()
    assert L.gpk_fisher_workspace_bytes(ctypes.byref(kd), ctypes.byref(f.layout)) == 0
    t = torch.zeros(64, dtype=torch.float64, device=engine.device())
    rc = L.gpk_fisher(ctypes.byref(kd), ctypes.byref(f.layout), nat.ptr(t), 0, nat.ptr(t), 0, nat.ptr(t), nat.ptr(t),
                      nat.ptr(t), nat.ptr(t), 8 * 64, nat.stream_handle(engine.device()))
    assert rc == -2 and "fp64 only" in nat.last_error()
    with pytest.raises(RuntimeError, match="run"):
        engine.InverseFactorization(65, d, 1, torch.float64).fisher()


def _gp(name, n):
    tree, hyp, d = _activate(name)
    x, y = _data(name, n)
    di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(d))
    g = GaussianProcess(_kernel(tree, hyp, d), ZeroMeanFunction(d))
    g.set_data_input(di)
    return g, di, hyp


def test_likelihood_entry_equals_the_engine():
    g, di, hyp = _gp("ADD(SE,PER)", 130)
    metric = get_metric_by_type(MetricType.LL, g)
    F = metric.get_fisher_information(hyp_list(hyp), torch.tensor(NOISE, dtype=torch.float64))
    assert tuple(F.shape) == (4, 4) and F.is_cuda
    assert torch.equal(F, _factor("ADD(SE,PER)", 130).fisher()[0])


@pytest.mark.parametrize("optimize_noise", [False, True])
def test_laplace_evidence_matches_the_formula(optimize_noise, e2e_flags):  # noqa: F811
    from oracle import gp_oracle as o
    name, n = "ADD(SE,PER)", 130
    g, di, hyp = _gp(name, n)
    gp.p_optimize_noise = optimize_noise
    m = LaplaceEvidence(di, g.covariance_matrix)
    got = m.get_metric(hyp_list(hyp), torch.tensor(NOISE, dtype=torch.float64))
    assert tuple(got.shape) == (1, 1)
    x, y = _data(name, n)
    nl = o.nlml(CASES[name][0], hyp, NOISE, x, y)
    _, F_ref = _reference(name, n)
    free = list(range(3)) + ([3] if optimize_noise else [])
    ref = nl + 0.5 * np.linalg.slogdet(F_ref[np.ix_(free, free)])[1] - 0.5 * len(free) * math.log(2 * math.pi)
    print("LAPLACE %s got %.12f ref %.12f" % (optimize_noise, float(got), ref))
    assert abs(float(got) - ref) <= 1e-9 * abs(ref)
    # the hard INDICATOR mask: no information about the change point
    cs.set_mode("INDICATOR")
    gi, dii, hi = _gp("CP(SE,SE)", 130)
    cs.set_mode("INDICATOR")
    with pytest.raises(ValueError, match=r"position\(s\) \[0\]"):
        LaplaceEvidence(dii, gi.covariance_matrix).get_metric(hyp_list(hi), torch.tensor(NOISE, dtype=torch.float64))


@pytest.mark.parametrize("optimize_noise", [True, False])
def test_standard_errors_after_a_fit(optimize_noise, e2e_flags):  # noqa: F811
    """The N = 96 SE case of tests/test_gpu_fitter.py."""
    gp.p_optimize_noise = optimize_noise
    gp.p_cov_matrix_jitter = torch.tensor(E2E_NOISE_FLOOR if optimize_noise else E2E_NOISE, dtype=torch.float64)
    y = e2e_targets("SE", E2E_NOISE)
    x = _x()
    kernel = e2e_kernel("SE")
    di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    fitter = DeviceLbfgsFitter(di, g, MetricType.LL, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                               mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=8, ftol=E2E_FTOL,
                               generator=torch.Generator().manual_seed(2), bounded=True)
    fitter.fit()
    point = fitter.points[fitter.winner].numpy()
    F = fitter.fisher_information()
    assert tuple(F.shape) == (2, 2) and F.is_cuda
    se = fitter.standard_errors().numpy()
    K = fs.kernel_ref(("SE", {}), [point[0]], x, x) + point[1] * np.eye(N_E2E)
    F_ref = fs.fisher_ref(K, fs.jacobian_ref(("SE", {}), [point[0]], x, x))
    assert np.abs(F.cpu().numpy() - F_ref).max() <= 1e-7 * max(1.0, np.abs(F_ref).max())
    print("SE optimize_noise=%s point %s standard errors %s" % (optimize_noise, point, se))
    if optimize_noise:
        ref = np.sqrt(np.diag(np.linalg.inv(F_ref)))
        assert np.all(np.isfinite(se)) and np.all(se > 0)
        assert np.all(np.abs(se - ref) <= 1e-6 * ref)
    else:
        ref = math.sqrt(1.0 / F_ref[0, 0])
        assert np.isfinite(se[0]) and se[0] > 0 and abs(se[0] - ref) <= 1e-6 * ref
        assert np.isnan(se[1])                                            # the pinned noise
