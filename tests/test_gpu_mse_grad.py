"""Held-out MSE and its gradient on the HIP path (gpk_mse_grad / gpk_mse_backward) against the restatement of
tests/mse_support.py (needs the MI355X).

Value: rel < 1e-8 against oracle.gp_oracle.mse (the restatement's own value for the leaves the oracle does not know).
Gradient: |g - g_ref| <= 1e-7 max(1, |g_ref|_max) against torch autodiff, noise 0.05; every case first asserts on the
reference alone that the K term, the K_s term and the noise partial each exceed 100 x that bar.
Shapes are the smallest that cross the 64-point tile and the 128-row factorisation panel on both axes.
"""
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine, sweep
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import CrossValidation as cv
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from oracle import gp_oracle as o
from tests import cp_support, lin_support, rq_support
from tests import mse_support as ms
from tests.helpers import hyp_list, set_flags

pytestmark = pytest.mark.gpu

SE, PER = ("SE", {}), ("PER", {})
NOISE = 0.05
# name: (tree, hyperparameter list, n, m, d, scaled, change-point mode)
CASES = {
    "SE": (SE, [0.3], 64, 64, 1, False, None),
    "PER": (PER, [0.7, 0.45], 97, 33, 1, False, None),
    "MAT32": (("MAT32", {}), [0.4], 130, 70, 1, False, None),
    "MAT52": (("MAT52", {}), [0.5], 64, 1, 1, False, None),
    "LIN": (("LIN", {}), [[0.3]], 200, 130, 1, False, None),
    "RQ": (("RQ", {}), [0.3, 1.5], 97, 33, 1, False, None),
    "ADD": (("ADD", [SE, PER]), [0.3, 0.9, 0.5], 130, 70, 1, False, None),
    "MUL": (("MUL", [SE, PER]), [0.5, 0.8, 0.6], 200, 130, 1, False, None),
    "SE_scaled": (SE, [0.3, 2.0], 64, 64, 1, True, None),
    "CP": (("CP", [SE, SE]), [0.45, 0.2, 0.4], 97, 33, 1, False, "SIGMOID"),
    "SE_ard_d3": (("SE", {"ard": True}), [[0.4, 0.7, 1.1]], 130, 70, 3, False, None),
}


@pytest.fixture(autouse=True)
def _cp_mode():
    mode = gp.p_cp_operator_type
    yield
    gp.p_cp_operator_type = mode


def _kernel(tree, hyp, d):
    if ms.has_op(tree, "CP"):
        return cp_support.make_kernel(tree, hyp, d)
    if ms.has_op(tree, "LIN"):
        return lin_support.make_kernel(tree, d)
    if ms.has_op(tree, "RQ"):
        return rq_support.make_kernel(tree, d)
    from tests.helpers import make_kernel
    return make_kernel(tree, d)


def _setup(name):
    tree, hyp, n, m, d, scaled, mode = CASES[name]
    set_flags(scaled=scaled)
    if mode:
        cp_support.set_mode(mode)
    x, y, xs, ys = ms.inputs(n, m, d, 11)
    return tree, hyp, d, scaled, mode or "INDICATOR", x, y, xs, ys


def _flat(hyp):
    return np.concatenate([np.atleast_1d(np.asarray(h, dtype=np.float64)).reshape(-1) for h in hyp])


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=engine.device())


def _reference(tree, hyp, noise, x, y, xs, ys, scaled, mode):
    """(f_ref, g_ref) with the visibility of every term asserted on the reference alone."""
    f_ref, g_ref = ms.mse_autodiff(tree, hyp, noise, x, y, xs, ys, scaled, mode)
    _, _, g_k, g_ks = ms.mse_formula(tree, hyp, noise, x, y, xs, ys, scaled, mode)
    ms.assert_terms_visible(g_ref, g_k, g_ks)
    if not (ms.has_op(tree, "CP") or ms.has_op(tree, "LIN") or ms.has_op(tree, "RQ")):
        f_o = o.mse(tree, hyp, noise, x, y, xs, ys, scaled)
        assert abs(f_o - f_ref) <= 0.1 * ms.VALUE_REL * abs(f_o)   # (the two CPU references agree far inside the bar)
        f_ref = f_o
    return f_ref, g_ref


def _check(f, g, f_ref, g_ref):
    print("mse %.12e ref %.12e rel %.2e" % (f, f_ref, abs(f - f_ref) / abs(f_ref)))
    assert abs(f - f_ref) < ms.VALUE_REL * abs(f_ref)
    ms.assert_grad_close(g, g_ref)


@pytest.mark.parametrize("name", list(CASES))
def test_value_and_gradient_through_every_route(name):
    tree, hyp, d, scaled, mode, x, y, xs, ys = _setup(name)
    n, m = len(x), len(xs)
    f_ref, g_ref = _reference(tree, hyp, NOISE, x, y, xs, ys, scaled, mode)
    kernel = _kernel(tree, hyp, d)
    kd = engine.kernel_descriptor(kernel, d)
    cand = _dev(np.concatenate([_flat(hyp), [NOISE]]))
    assert cand.numel() == kd.n_hyp + 1
    X, Y, Xs, Ys = _dev(x), _dev(y).reshape(1, -1), _dev(xs), _dev(ys).reshape(1, -1)
    with nat.thread_tune(chain=0):   # (both factorisations on the launch path: the bitwise comparison is about the pass)
        # route 1: the composite
        f1 = engine.AugmentedFactorization(n, d, m, 1, torch.float64)
        f1.run_mse(kd, cand, 0, cand[kd.n_hyp:], 0, X, 0, Y, 0, Xs, 0, Ys, 0)
        v1, g1 = f1.mse().cpu().numpy(), f1.mse_grad().cpu().numpy()
        assert int(f1.info[0]) == 0
        _check(float(v1[0]), g1[0], f_ref, g_ref)
        # route 2: the pass alone on a factorisation run separately -- the composite's bits
        f2 = engine.AugmentedFactorization(n, d, m, 1, torch.float64)
        f2.run(kd, cand, 0, cand[kd.n_hyp:], 0, X, 0, Y, 0, Xs=Xs, xs_bstride=0)
        v2, g2 = f2.mse_gradient(Ys, 0)
        assert np.array_equal(v2.cpu().numpy(), v1) and np.array_equal(g2.cpu().numpy(), g1)
    # route 3: the metric (the default factorisation path of a single evaluation)
    di = DataInput(x, y.reshape(-1, 1), xs, ys.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(d))
    g = GaussianProcess(kernel, ZeroMeanFunction(d))
    g.set_data_input(di)
    metric = get_metric_by_type(MetricType.MSE, g)
    hl, nz = hyp_list(hyp), torch.tensor(NOISE, dtype=torch.float64)
    v3, grads, gn = metric.get_metric_and_gradient(hl, nz)
    assert [tuple(a.shape) for a in grads] == [tuple(h.shape) for h in hl]
    g3 = np.concatenate([a.cpu().numpy().reshape(-1) for a in grads] + [[float(gn)]])
    _check(float(v3), g3, f_ref, g_ref)
    assert abs(float(metric.get_metric(hl, nz)) - float(v3)) <= 1e-12 * abs(float(v3))
    flat = metric.get_gradients(hl, nz).cpu().numpy()
    assert flat.shape == g_ref[:-1].shape and np.max(np.abs(flat - g_ref[:-1])) <= ms.grad_bar(g_ref)


def test_batch_members_are_independent_and_deterministic():
    """Five candidates with their own hyperparameters and noise, each against its own reference; candidates 0 and 3
    are identical and give identical bits; the same call twice gives identical bits."""
    tree = ("ADD", [SE, PER])
    x, y, xs, ys = ms.inputs(130, 70, 1, 5)
    cands = np.array([[0.3, 0.9, 0.5, 0.05], [0.2, 0.7, 0.4, 0.02], [0.5, 1.2, 0.8, 0.1], [0.3, 0.9, 0.5, 0.05],
                      [0.15, 0.6, 0.3, 0.03]])
    from tests.helpers import make_kernel
    ev = sweep.native_batched_mse_value_and_gradient(make_kernel(tree, 1), _dev(x), _dev(y), _dev(xs), _dev(ys))
    assert ev.n_par == 4
    C = _dev(cands)
    f, g, info = ev(C, settle=True)
    f, g, info = f.cpu().numpy().copy(), g.cpu().numpy().copy(), info.cpu().numpy().copy()
    assert not info.any()
    for b, row in enumerate(cands):
        f_ref, g_ref = _reference(tree, list(row[:-1]), row[-1], x, y, xs, ys, False, "INDICATOR")
        _check(float(f[b]), g[b], f_ref, g_ref)
    assert f[0] == f[3] and np.array_equal(g[0], g[3])
    f2, g2, _ = ev(C)
    assert np.array_equal(f2.cpu().numpy(), f) and np.array_equal(g2.cpu().numpy(), g)
    with pytest.raises(ValueError, match="candidate rows must have 4 values"):
        ev(C[:, :3].contiguous())


RAGGED = [(97, 33), (130, 70), (64, 1)]


def _ragged_operands(fill):
    """Packed operands of the ragged batch, the unused tails of X, Xs, y and ys filled with ``fill``."""
    n, m = max(s[0] for s in RAGGED), max(s[1] for s in RAGGED)
    B = len(RAGGED)
    X, Y = np.full((B, n, 1), fill), np.full((B, n), fill)
    Xs, Ys = np.full((B, m, 1), fill), np.full((B, m), fill)
    data = []
    for b, (nb, mb) in enumerate(RAGGED):
        x, y, xs, ys = ms.inputs(nb, mb, 1, 20 + b)
        X[b, :nb], Y[b, :nb], Xs[b, :mb], Ys[b, :mb] = x, y, xs, ys
        data.append((x, y, xs, ys))
    return data, X, Y, Xs, Ys


def test_ragged_batch_and_padding_independence():
    """Members {(97, 33), (130, 70), (64, 1)} each against its own reference; the results do not depend on what lies
    in the padding (tails filled with 1e6 against zero-filled: the same bits); the pass alone on a separately run ragged
    factorisation gives the composite's bits."""
    tree = ("ADD", [SE, PER])
    hyps = np.array([[0.3, 0.9, 0.5], [0.2, 0.7, 0.4], [0.5, 1.2, 0.8]])
    noises = np.array([0.05, 0.02, 0.1])
    from tests.helpers import make_kernel
    kernel = make_kernel(tree, 1)
    kd = engine.kernel_descriptor(kernel, 1)
    H = np.zeros((3, nat.MAX_HYP))
    H[:, :3] = hyps
    res = {}
    for fill in (0.0, 1e6):
        data, X, Y, Xs, Ys = _ragged_operands(fill)
        fac = engine.RaggedFactorization([s[0] for s in RAGGED], 1, [s[1] for s in RAGGED], torch.float64)
        fac.run_mse_packed(kd, _dev(H), _dev(noises), _dev(X), _dev(Y), _dev(Xs), _dev(Ys))
        assert not fac.info.cpu().numpy().any()
        res[fill] = (fac.mse().cpu().numpy().copy(), fac.mse_grad().cpu().numpy().copy())
    assert np.array_equal(res[0.0][0], res[1e6][0]) and np.array_equal(res[0.0][1], res[1e6][1])
    f, g = res[0.0]
    for b, (x, y, xs, ys) in enumerate(data):
        f_ref, g_ref = _reference(tree, list(hyps[b]), noises[b], x, y, xs, ys, False, "INDICATOR")
        _check(float(f[b]), g[b], f_ref, g_ref)
    # the pass alone (gpk_mse_backward with n_dev / m_dev) after RaggedFactorization.run
    fac = engine.RaggedFactorization([s[0] for s in RAGGED], 1, [s[1] for s in RAGGED], torch.float64)
    fac.run([(kd, _dev(hyps[b]), _dev(d[0]), _dev(d[1]), _dev(d[2])) for b, d in enumerate(data)], _dev(noises))
    v, gg = fac.mse_gradient([_dev(d[3]) for d in data])
    assert np.array_equal(v.cpu().numpy(), f) and np.array_equal(gg.cpu().numpy(), g)


def test_failed_member_is_inf_and_nan_and_leaves_the_others_alone():
    """Member 1: noise 0, every point duplicated, length scale 5 -- K is singular in fp64 and its factorisation fails
    (info != 0): +inf and NaN for it, the other members of the same batch still meet their references."""
    x, y, xs, ys = ms.inputs(48, 33, 1, 9)
    x, y = np.concatenate([x, x]), np.concatenate([y, y])          # n = 96, every point twice
    from tests.helpers import make_kernel
    ev = sweep.native_batched_mse_value_and_gradient(make_kernel(SE, 1), _dev(x), _dev(y), _dev(xs), _dev(ys))
    good = np.array([[0.3, 0.05], [0.2, 0.1]])
    f, g, info = ev(_dev(np.array([good[0], [5.0, 0.0], good[1]])), settle=True)
    f, g, info = f.cpu().numpy().copy(), g.cpu().numpy().copy(), info.cpu().numpy().copy()
    assert info[1] != 0 and info[0] == 0 and info[2] == 0
    assert math.isinf(f[1]) and f[1] > 0 and np.all(np.isnan(g[1]))
    for b, row in zip((0, 2), good):
        f_ref, g_ref = ms.mse_autodiff(SE, [row[0]], row[1], x, y, xs, ys)
        _check(float(f[b]), g[b], f_ref, g_ref)


def test_kfold_mean_over_unequal_folds():
    """Five folds of CrossValidation.get_data_inputs at n = 103 (test sizes 21, 21, 21, 21, 19): the mean of the
    folds' MSE and gradient for two candidates against the mean of the per-fold references."""
    tree = ("ADD", [SE, PER])
    x, y, _, _ = ms.inputs(103, 1, 1, 31)
    di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    np.random.seed(7)
    folds = cv.get_data_inputs(di, 0.2)
    for fd in folds:
        fd.set_mean_function(ZeroMeanFunction(1))
    arrays = [(fd.data_x_train, fd.get_detrended_y_train(), fd.data_x_test, fd.get_detrended_y_test()) for fd in folds]
    assert len(folds) == 5 and len({int(a[2].shape[0]) for a in arrays}) > 1
    from tests.helpers import make_kernel
    ev = sweep.native_kfold_mse_value_and_gradient(make_kernel(tree, 1), arrays)
    assert ev.n_par == 4 and ev.n_folds == 5
    cands = np.array([[0.3, 0.9, 0.5, 0.05], [0.2, 0.7, 0.4, 0.02]])
    f, g, info = ev(_dev(cands))
    f, g, info = f.cpu().numpy(), g.cpu().numpy(), info.cpu().numpy()
    assert not info.any()
    host = [tuple(np.asarray(t.cpu().numpy(), dtype=np.float64) for t in a) for a in arrays]
    for s, row in enumerate(cands):
        refs = [_reference(tree, list(row[:-1]), row[-1], a[0], a[1].reshape(-1), a[2], a[3].reshape(-1), False,
                           "INDICATOR") for a in host]
        f_ref = sum(r[0] for r in refs) / 5.0
        g_ref = sum(r[1] for r in refs) / 5.0
        _check(float(f[s]), g[s], f_ref, g_ref)
