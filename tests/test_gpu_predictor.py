"""The fitted predictor on the HIP path (gpk_predict, needs the MI355X): posterior mean and latent variance at new
points from ONE kept identity-augmented factorisation, against the host restatement (tests/predict_support: K from
the oracle's kernels, scipy Cholesky and triangular solves, never the device's K, L or R), against oracle.posterior
for the plain trees, against the existing augmented path, and the properties the entry promises: the same bits for
any chunking and for repeated calls, both factorisation paths, every member of a batch, mu / var alone.

Bar: |got - ref| <= 1e-8 max(1, max|ref|) for mu and var.  On these inputs cond(K + noise I) <= 6e4, the
first-order error is ~1e-11: the bar is a ceiling; the measured maxima are printed (PREDERR lines)."""
import ctypes

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import LinearMeanFunction, ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceLbfgsFitter
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
from gaussianprocessfundamentals_amd.Statistics.Predictor import PosteriorPredictor
from oracle import gp_oracle as o
from tests import cp_support as cs
from tests import predict_support as ps
from tests import rq_support as rs
from tests.helpers import hyp_list, set_flags

pytestmark = pytest.mark.gpu

NOISE = ps.NOISE
SIZES_N = [1, 127, 128, 129, 333]
SIZES_M = [1, 63, 65, 200]


@pytest.fixture(autouse=True)
def _cp_mode():
    yield
    cs.set_mode("INDICATOR")


def _activate(name):
    tree, hyp, d, scaled, mode = ps.CASES[name]
    set_flags(scaled=scaled)
    if mode:
        cs.set_mode(mode)
    return tree, hyp, d


def _kernel(name):
    tree, hyp, d = _activate(name)
    return rs.make_kernel(tree, d) if tree[0] == "RQ" else cs.make_kernel(tree, hyp, d)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=engine.device())


def _factor(name, x, y, noise=NOISE, hyps=None, nan_fill=False):
    """engine.InverseFactorization run on the case without a gradient (hyps: one list per batch member)"""
    tree, hyp, d = _activate(name)
    kd = engine.kernel_descriptor(_kernel(name), d)
    rows = [hyp] if hyps is None else hyps
    H = torch.stack([engine.pack_hyper_parameter(hyp_list(h), kd.n_hyp) for h in rows]).contiguous()
    n = len(x)
    f = engine.InverseFactorization(n, d, len(rows), torch.float64)
    if nan_fill:   # nothing the factorisation skips or leaves unwritten may reach the prediction
        f._W.fill_(float("nan"))
        f._Winv.fill_(float("nan"))
    nz = torch.tensor([noise], dtype=torch.float64, device=engine.device())
    f.run(kd, H.reshape(-1), kd.n_hyp if len(rows) > 1 else 0, nz, 0, _dev(x), 0, _dev(y).reshape(1, -1), 0,
          gradient=False)
    return f


def _check(tag, got_mu, got_var, mu_ref, var_ref):
    gm, gv = got_mu.cpu().numpy(), got_var.cpu().numpy()
    em, ev = float(np.max(np.abs(gm - mu_ref))), float(np.max(np.abs(gv - var_ref)))
    print("PREDERR %s max|mu - ref| = %.3e (bar %.1e)  max|var - ref| = %.3e (bar %.1e)"
          % (tag, em, ps.bar(mu_ref), ev, ps.bar(var_ref)))
    assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv))
    assert em <= ps.bar(mu_ref)
    assert ev <= ps.bar(var_ref)


# ------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("n", SIZES_N)
@pytest.mark.parametrize("name", list(ps.CASES))
def test_matches_the_host_reference(name, n):
    tree, hyp, d, scaled, mode = ps.CASES[name]
    x, y = ps.case_reference(name, n, SIZES_M[0])[:2]
    f = _factor(name, x, y)     # factored once for the four point sets
    assert int(f.info[0]) == 0
    for m in SIZES_M:
        x, y, xs, mu_ref, var_ref = ps.case_reference(name, n, m)
        mu, var = f.predict(_dev(xs))
        assert tuple(mu.shape) == (m,) and tuple(var.shape) == (m,)
        _check("%s n=%d m=%d" % (name, n, m), mu, var, mu_ref, var_ref)
        if name in ps.NONSTATIONARY and m >= 63:
            # k(x*, x*) differs from point to point by O(1): one point's value for all would miss the bar
            tree_k = np.diag(ps.fs.kernel_ref(tree, hyp, xs, xs, scaled, False, mode or "SIGMOID"))
            assert float(np.ptp(tree_k)) > 0.5
            v = var.cpu().numpy()
            assert float(np.ptp(v)) > 0.1 * float(np.max(np.abs(v)))     # var differs between the test points
        if name in ps.ORACLE_CASES and m == 65:
            mu_o, cov_o = o.posterior(tree, hyp, NOISE, x, y, xs, scaled)
            _check("%s n=%d m=%d oracle" % (name, n, m), mu, var, mu_o, np.diag(cov_o))


def test_prior_variance_is_the_kernel_matrix_diagonal_bitwise():
    """What the pass leaves in its workspace (one chunk: Ks' [m, n_pad], then k(x*, x*) [m]): the values of
    gpk_kernel_matrix(Xs, X) and of diag(gpk_kernel_matrix(Xs, Xs)) bit for bit, the padding columns zeros."""
    for name in ps.CASES:
        tree, hyp, d = _activate(name)
        x, y, xs, _, _ = ps.case_reference(name, 127, 200)
        k = _kernel(name)
        f = _factor(name, x, y)
        f.predict(_dev(xs))
        lay = f.layout
        kdiag = f.work[200 * lay.n_pad:200 * lay.n_pad + 200]   # (one chunk: Ks' [200, n_pad], then kdiag)
        Kss = engine.kernel_matrix(k, hyp_list(hyp), _dev(xs), _dev(xs))
        assert torch.equal(kdiag, torch.diagonal(Kss))
        Ks = f.work[:200 * lay.n_pad].view(200, lay.n_pad)
        assert torch.equal(Ks[:, :127], engine.kernel_matrix(k, hyp_list(hyp), _dev(xs), _dev(x)))
        assert not bool(Ks[:, 127:].any())                      # padding columns are zeros


# ------------------------------------------------------------------------------- 2. against the existing path
@pytest.mark.parametrize("name", ["SE", "ADD(SE,PER)", "LIN", "CP(SE,SE)"])
def test_matches_the_augmented_path(name):
    tree, hyp, d, scaled, mode = ps.CASES[name]
    x, y, xs, mu_ref, var_ref = ps.case_reference(name, 129, 65)
    k = _kernel(name)
    di = DataInput(x, y.reshape(-1, 1), xs, np.zeros((len(xs), 1)))
    di.set_mean_function(ZeroMeanFunction(d))
    g = GaussianProcess(k, ZeroMeanFunction(d))
    g.set_data_input(di)
    mu_old = g.aux.get_posterior_mu(hyp_list(hyp), NOISE)
    var_old = g.aux.get_posterior_var_diag(hyp_list(hyp), NOISE)
    p = PosteriorPredictor(k, hyp_list(hyp), NOISE, ZeroMeanFunction(d), None, di)
    _, _, mu, var = p.predict(xs, return_var=True)
    _check("%s vs augmented path" % name, mu, var, mu_old.cpu().numpy(), var_old.cpu().numpy())
    _check("%s vs reference" % name, mu, var, mu_ref, var_ref)


# ---------------------------------------------------------------------------------- 3. chunk invariance, bitwise
@pytest.mark.parametrize("name", ["SE", "CP(SE,SE)", "SE_ARD@3"])
def test_chunking_and_repetition_do_not_change_a_bit(name):
    x, y, xs, _, _ = ps.case_reference(name, 333, 200)
    f = _factor(name, x, y)
    X = _dev(xs)
    mu1, var1 = f.predict(X)                    # one chunk
    mu2, var2 = f.predict(X, max_rows=64)       # 64 + 64 + 64 + 8
    mu3, var3 = f.predict(X, max_rows=128)      # 128 + 72
    mu4, var4 = f.predict(X)
    for mu, var in ((mu2, var2), (mu3, var3), (mu4, var4)):
        assert torch.equal(mu, mu1) and torch.equal(var, var1)
    # a point's result does not depend on its row either: the points in another order
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(5)).to(X.device)
    mu5, var5 = f.predict(X[perm].contiguous(), max_rows=64)
    assert torch.equal(mu5, mu1[perm]) and torch.equal(var5, var1[perm])


# ------------------------------------------------------------------------------ 4. both factorisation paths
@pytest.mark.parametrize("n", [129, 333])
def test_both_factorisation_paths_and_nothing_unwritten_is_read(n):
    name = "ADD(SE,PER)"
    x, y, xs, mu_ref, var_ref = ps.case_reference(name, n, 200)
    out = {}
    for path, mode in (("launch", 0), ("chain", 2)):
        with nat.thread_tune(chain=mode):
            f = _factor(name, x, y, nan_fill=True)
            assert int(f.info[0]) == 0
            mu, var = f.predict(_dev(xs), max_rows=64)
        _check("%s n=%d %s path, NaN-filled W" % (name, n, path), mu, var, mu_ref, var_ref)
        out[path] = (mu.cpu().numpy(), var.cpu().numpy())
    assert np.max(np.abs(out["launch"][0] - out["chain"][0])) <= ps.bar(mu_ref)
    assert np.max(np.abs(out["launch"][1] - out["chain"][1])) <= ps.bar(var_ref)


# --------------------------------------------------------------------------------------------- 5. member index
def test_members_of_a_batch_equal_single_factorisations():
    name = "MAT52_scaled"
    x, y, xs, _, _ = ps.case_reference(name, 129, 65)
    hyps = [[1.1, 1.6], [0.7, 0.9], [1.3, 2.2]]
    fb = _factor(name, x, y, hyps=hyps)
    assert not bool(fb.info.any())
    X = _dev(xs)
    tree, _, d, scaled, mode = ps.CASES[name]
    for b, h in enumerate(hyps):
        mu_b, var_b = fb.predict(X, member=b)
        mu_s, var_s = _factor(name, x, y, hyps=[h]).predict(X)
        mu_ref, var_ref = ps.posterior_ref(tree, h, NOISE, x, y, xs, scaled, mode)
        _check("member %d" % b, mu_b, var_b, mu_ref, var_ref)
        _check("member %d vs B = 1" % b, mu_b, var_b, mu_s.cpu().numpy(), var_s.cpu().numpy())
    with pytest.raises(ValueError, match="member 3 of a batch of 3"):
        fb.predict(X, member=3)


# ---------------------------------------------------------------------------------------- 6. mu only / var only
def test_mu_alone_and_var_alone_are_the_same_bits():
    x, y, xs, _, _ = ps.case_reference("RQ", 333, 200)
    f = _factor("RQ", x, y)
    X = _dev(xs)
    mu, var = f.predict(X, max_rows=64)
    mu_only, none = f.predict(X, want_var=False, max_rows=64)
    none2, var_only = f.predict(X, want_mu=False, max_rows=64)
    assert none is None and none2 is None
    assert torch.equal(mu_only, mu) and torch.equal(var_only, var)


def test_the_run_is_not_disturbed():
    x, y, xs, _, _ = ps.case_reference("SE", 129, 65)
    tree, hyp, d = _activate("SE")
    kd = engine.kernel_descriptor(_kernel("SE"), d)
    f = engine.InverseFactorization(len(x), d, 1, torch.float64)
    nz = torch.tensor([NOISE], dtype=torch.float64, device=engine.device())
    f.run(kd, engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp), 0, nz, 0, _dev(x), 0, _dev(y).reshape(1, -1), 0)
    val, grad, _ = f.results("nlml")
    val0, grad0, W0 = val.clone(), grad.clone(), f.W.clone()
    F0 = f.fisher().clone()
    f.predict(_dev(xs), max_rows=64)
    val1, grad1, _ = f.results("nlml")
    assert torch.equal(val1, val0) and torch.equal(grad1, grad0)
    # W is only read (compared as bits: the tiles the factorisation skips hold whatever was there, NaNs included)
    assert torch.equal(f.W.view(torch.int64), W0.view(torch.int64))
    assert torch.equal(f.results("fisher")[0], F0) and torch.equal(f.fisher(), F0)


# ------------------------------------------------------------------------------------------------------ 7. API
def _gp_case(name, n, m, mean_function=None):
    tree, hyp, d, scaled, mode = ps.CASES[name]
    x, y, xs, mu_ref, var_ref = ps.case_reference(name, n, m)
    k = _kernel(name)
    mf = mean_function or ZeroMeanFunction(d)
    di = DataInput(x, y.reshape(-1, 1), xs[:1], np.zeros((1, 1)))
    di.set_mean_function(mf)
    g = GaussianProcess(k, mf)
    g.set_data_input(di)
    return g, hyp, x, y, xs, mu_ref, var_ref


def test_get_predictor_with_a_linear_mean_function():
    name = "SE"
    tree, hyp, d, scaled, mode = ps.CASES[name]
    slope = 0.35
    g, hyp, x, y, xs, _, _ = _gp_case(name, 129, 65, LinearMeanFunction(d))
    mean_hyp = [torch.tensor([slope], dtype=torch.float64)]
    p = g.get_predictor(hyp_list(hyp), mean_hyp, NOISE)
    total, mean, mu, var = p.predict(xs, return_var=True)
    mean_ref = slope * xs[:, 0]
    mu_ref, var_ref = ps.posterior_ref(tree, hyp, NOISE, x, y - slope * x[:, 0], xs, scaled, mode)
    assert np.max(np.abs(mean.cpu().numpy() - mean_ref)) <= 1e-13 * max(1.0, np.max(np.abs(mean_ref)))
    _check("linear mean", mu, var, mu_ref, var_ref)
    assert torch.equal(total, mean + mu)
    assert np.max(np.abs(total.cpu().numpy() - (mean_ref + mu_ref))) <= ps.bar(mean_ref + mu_ref)
    # the triple without a variance; include_noise adds exactly the noise
    triple = p.predict(xs)
    assert len(triple) == 3 and torch.equal(triple[0], total) and torch.equal(triple[2], mu)
    noisy = p.predict(xs, return_var=True, include_noise=True)[3]
    assert torch.equal(noisy, var + torch.tensor(NOISE, dtype=torch.float64, device=var.device))
    # log predictive density against numpy from the reference's mu / var
    y_new = np.sin(0.9 * xs[:, 0]) + 0.2
    lpd = float(p.log_predictive_density(xs, y_new))
    ref = ps.log_density_ref(y_new, mean_ref + mu_ref, var_ref + NOISE)
    assert abs(lpd - ref) <= 1e-9 * abs(ref)
    with pytest.raises(ValueError, match="x_new must be"):
        p.predict(np.zeros((3, d + 1)))


def test_get_predictor_defaults_are_those_of_predict():
    g, hyp, x, y, xs, _, _ = _gp_case("SE", 129, 65)
    g.kernel.set_last_hyper_parameter(hyp_list(hyp))
    p = g.get_predictor()
    assert float(p.noise[0]) == float(torch.as_tensor(gp.p_cov_matrix_jitter))
    total, mean, mu = p.predict(xs)
    assert not bool(mean.any()) and torch.equal(total, mu)
    # (jitter-sized noise: K is ill-conditioned, so the defaults are pinned against the explicit arguments, bitwise)
    q = PosteriorPredictor(g.kernel, hyp_list(hyp), gp.p_cov_matrix_jitter, g.mean_function,
                           g.mean_function.get_default_hyper_parameter(), g.data_input)
    assert torch.equal(q.predict(xs)[2], mu)


def test_a_kernel_that_is_not_positive_definite_raises_at_construction():
    """PER's L1 form is not PD above d = 1."""
    set_flags()
    rng = np.random.default_rng(11)
    x = rng.uniform(0.0, 10.0, (129, 3))
    y = np.sin(x.sum(1))
    di = DataInput(x, y.reshape(-1, 1), x[:1], y[:1].reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(3))
    k = bk.PeriodicKernel(3)
    with pytest.raises(engine.CholeskyError):
        PosteriorPredictor(k, hyp_list([0.3, 2.0]), 1e-8, ZeroMeanFunction(3), None, di)


def test_fitter_predictor_is_the_predictor_at_the_winning_point():
    set_flags()
    x, y, xs, _, _ = ps.case_reference("SE", 129, 65)
    di = DataInput(x, y.reshape(-1, 1), xs[:1], np.zeros((1, 1)))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(bk.SquaredExponentialKernel(1), ZeroMeanFunction(1))
    old = gp.p_optimize_noise
    gp.p_optimize_noise = True
    try:
        fitter = DeviceLbfgsFitter(di, g, MetricType.LL, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                                   mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=2, max_iter=6,
                                   generator=torch.Generator().manual_seed(3), bounded=True)
        fitter.fit()
        p = fitter.predictor()
    finally:
        gp.p_optimize_noise = old
    point = fitter.points[fitter.winner]
    assert float(p.noise[0]) == float(point[-1])
    total, mean, mu, var = p.predict(xs, return_var=True)
    by_hand = PosteriorPredictor(g.kernel, [point[:1].clone()], point[-1].clone(), ZeroMeanFunction(1), None, di)
    t2, _, mu2, var2 = by_hand.predict(xs, return_var=True)
    assert torch.equal(mu, mu2) and torch.equal(var, var2) and torch.equal(total, t2)
    assert bool(torch.isfinite(mu).all()) and bool(torch.isfinite(var).all())


# --------------------------------------------------------------------------------------------- 8. repeated use
def test_one_predictor_many_point_sets():
    name = "MUL(SE,PER)"
    tree, hyp, d, scaled, mode = ps.CASES[name]
    x, y, _, _, _ = ps.case_reference(name, 333, 200)
    k = _kernel(name)
    di = DataInput(x, y.reshape(-1, 1), x[:1], y[:1].reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(d))
    p = PosteriorPredictor(k, hyp_list(hyp), NOISE, ZeroMeanFunction(d), None, di)
    for m in (200, 1, 65):
        xs = ps.case_reference(name, 333, m)[2] if m != 1 else ps.case_reference(name, 333, 200)[2][7:8]
        got = p.predict(xs, return_var=True)
        fresh = PosteriorPredictor(k, hyp_list(hyp), NOISE, ZeroMeanFunction(d), None, di).predict(xs, return_var=True)
        assert torch.equal(got[2], fresh[2]) and torch.equal(got[3], fresh[3])
        mu_ref, var_ref = ps.posterior_ref(tree, hyp, NOISE, x, y, xs, scaled, mode)
        _check("repeated m=%d" % m, got[2], got[3], mu_ref, var_ref)


# ------------------------------------------------------------------------------------------- the C ABI directly
def test_c_abi_refuses_a_short_workspace_and_runs_with_exactly_one_tile():
    x, y, xs, mu_ref, var_ref = ps.case_reference("SE", 129, 200)
    f = _factor("SE", x, y)
    L, lay, kd = f.L, f.layout, f.kd
    hyp = f._loo_operands[1]
    X, Xs = _dev(x), _dev(xs)
    dev = engine.device()
    mu = torch.empty(200, dtype=torch.float64, device=dev)
    var = torch.empty(200, dtype=torch.float64, device=dev)
    need = int(L.gpk_predict_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay), 64))
    work = torch.empty(need // 8, dtype=torch.float64, device=dev)
    s = nat.stream_handle(dev)
    args = (ctypes.byref(kd), ctypes.byref(lay), nat.ptr(hyp), nat.ptr(X), nat.ptr(f.W), 0, nat.ptr(Xs), 200)
    assert L.gpk_predict(*args, nat.ptr(mu), nat.ptr(var), nat.ptr(work), need - 8, s) == -11
    nat.check(L.gpk_predict(*args, nat.ptr(mu), nat.ptr(var), nat.ptr(work), need, s), "gpk_predict")
    _check("one tile of workspace", mu, var, mu_ref, var_ref)
    mu1, var1 = f.predict(Xs)
    assert torch.equal(mu, mu1) and torch.equal(var, var1)
