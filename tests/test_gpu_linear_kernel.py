"""The LIN leaf (LinearKernel, GPK_OP_LIN) on the HIP path vs the restatement of tests/lin_support.py (needs the MI355X).

Sizes sit around the 64-point assemble tile and the 128-column factor panel.  Tolerances:
  kernel matrices   a LIN leaf |dev - ref| <= 1e-12 sum_k |x_k - c_k||y_k - c_k| + 1e-13 (<= 16 fused terms of eps
                    each: ~4e-15 of that sum -- the project's rel 1e-12 / abs 1e-13 headroom; LIN cancels across
                    dimensions, so a flat rtol on |K| would not hold), propagated through ADD (sum of bounds) and MUL
                    (|a| db + |b| da) with the restatement's own node values (lin_support.kernel_and_bound)
  -LML              rel <= 1e-9; posterior mu / diag Sigma abs <= 1e-8 (the project's C2 bars)
  gradients         |g - g_ref| <= 1e-7 max(1, |g_ref|_max) (tests/test_gpu_grad.py's bar)
  fp32              -LML rel <= 1e-3 against the fp64 oracle
The oracle modules learn the leaf through the ``lin_oracle`` fixture for the duration of a test."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests.helpers import GOLDEN, hyp_list, set_flags
from tests.lin_support import (LIN, kernel_and_bound, lin_inputs, lin_nlml_closed_form, lin_oracle,  # noqa: F401
                               make_kernel, with_sg)

from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import BlockwiseDataInput, DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import BlockwiseGaussianProcess, GaussianProcess

pytestmark = pytest.mark.gpu

F64 = torch.float64
SE = ("SE", {})
PER = ("PER", {})
MAT52 = ("MAT52", {})


def T(v):
    return torch.tensor(v, dtype=F64)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def offsets(d, seed=0):
    """d offsets in [-0.5, 0.5], both signs."""
    return list(np.random.default_rng(900 + seed).uniform(-0.5, 0.5, d))


def build_gp(tree, x, y, xs=None):
    d = x.shape[-1]
    if xs is None:
        di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    else:
        di = DataInput(x, y.reshape(-1, 1), xs, np.zeros(len(xs)).reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(d))
    g = GaussianProcess(make_kernel(tree, d), ZeroMeanFunction(d))
    g.set_data_input(di)
    return g


def check_grad(got, exp, tol=1e-7):
    scale = max(1.0, max(float(np.max(np.abs(e))) for e in exp))
    for g, e in zip(got, exp):
        np.testing.assert_allclose(np.asarray(g), np.asarray(e).reshape(np.shape(g)), rtol=0, atol=tol * scale)


# ------------------------------------------------------------------------------ 1. kernel matrix
def _tree_cases(d):
    c1, c2 = offsets(d, 1), offsets(d, 2)
    return [
        ("LIN", LIN, [c1]),
        ("SE+LIN", ("ADD", [SE, LIN]), [0.6, c1]),
        ("LIN+SE", ("ADD", [LIN, SE]), [c1, 0.6]),          # the pair dispatch must pick the LIN leaf in either slot
        ("LINxLIN", ("MUL", [LIN, LIN]), [c1, c2]),
        ("LINxPER", ("MUL", [LIN, PER]), [c1, 0.9, 0.7]),
        ("PERxLIN", ("MUL", [PER, LIN]), [0.9, 0.7, c1]),
        ("SExLIN+MAT52", ("ADD", [("MUL", [SE, LIN]), MAT52]), [0.6, c1, 0.8]),
    ]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("case", range(7))
@pytest.mark.parametrize("d", [1, 3, 16])
def test_kernel_matrix_matches_restatement(d, case, scaled):
    """get_tf_tensor at n = 130, m = 70 (whole, edge and partial tiles, non-square) against the restatement, inside
    the bound propagated from the leaves."""
    name, tree, hyp = _tree_cases(d)[case]
    set_flags(scaled=scaled)
    if scaled:
        hyp = with_sg(tree, hyp, [0.7, 1.3, 0.9])
    rng = np.random.default_rng(3)
    x, xs = rng.uniform(-1, 1, (130, d)), rng.uniform(-1, 1, (70, d))
    k = make_kernel(tree, d)
    got = k.get_tf_tensor(hyp_list(hyp), x, xs).cpu().numpy()
    exp, bound = kernel_and_bound(tree, hyp, x, xs, scaled)
    assert got.shape == (130, 70)
    err = np.abs(got - exp)
    print("%s d=%d scaled=%s: max err %.3e, max err / bound %.3e" % (name, d, scaled, err.max(), (err / bound).max()))
    assert np.all(err <= bound), (name, float((err / bound).max()))
    assert k.get_last_hyper_parameter() is not None


def test_kernel_matrix_symmetric_and_fp32_output():
    rng = np.random.default_rng(4)
    x = rng.uniform(-1, 1, (100, 3))
    c = offsets(3)
    k = make_kernel(LIN, 3)
    K = k.get_tf_tensor(hyp_list([c]), x, x)
    assert torch.equal(K, K.T)                       # the fused products commute: K(a, b) == K(b, a) bit for bit
    K32 = engine.kernel_matrix(k, hyp_list([c]), x, x, out_dtype=torch.float32)
    assert K32.dtype == torch.float32 and torch.equal(K32, K.to(torch.float32))


# ------------------------------------------------------------------------------ 2. same bits on every build path
@pytest.mark.parametrize("tree,hyp,d", [
    (LIN, [[0.2, -0.4, 0.1]], 3),
    (("ADD", [SE, LIN]), [0.6, [0.2, -0.4, 0.1]], 3),
    (LIN, [offsets(8)], 8),                                         # the widest interior instantiation
    (("MUL", [PER, LIN]), [0.9, 0.7, [0.3]], 1),                    # the periodic leaf's sin / cos form beside LIN
    (("ADD", [LIN, SE]), [[0.2, -0.4, 0.1], 0.6], 3),               # LIN in slot 0 of the two-leaf dispatch
    (("MUL", [LIN, PER]), [[0.2, -0.4, 0.1], 0.9, 0.7], 3),
    (("MUL", [LIN, LIN]), [[0.3, -0.6], [0.45, 0.1]], 2),
    (("ADD", [("MUL", [SE, LIN]), MAT52]), [0.6, [0.2, -0.4, 0.1], 0.8], 3),   # the general tree loop
])
def test_augmented_build_is_bitwise_the_plain_build(tree, hyp, d):
    """The n x n training block of the augmented build (interior, edge and generic tiles, noise on the diagonal)
    equals gpk_kernel_matrix's plain build (lower triangle, diag_add = noise) bit for bit, and matches the
    restatement."""
    n, noise = 200, 0.1
    x, y, _ = lin_inputs(n, d, 21)
    dev = engine.device()
    k = make_kernel(tree, d)
    kd = engine.kernel_descriptor(k, d)
    H = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp).reshape(1, -1).contiguous()
    X = torch.as_tensor(x, device=dev).contiguous()
    Y = torch.as_tensor(y, device=dev).reshape(1, -1).contiguous()
    NZ = torch.tensor([noise], dtype=F64, device=dev)
    f = engine.AugmentedFactorization(n, d, 0, 1, F64)
    f.W.zero_()
    nat.check(nat.lib().gpk_assemble(ctypes.byref(kd), ctypes.byref(f.layout), nat.ptr(H), kd.n_hyp, nat.ptr(NZ), 0,
                                     nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W),
                                     nat.stream_handle(f.W.device)), "gpk_assemble")
    torch.cuda.synchronize()
    aug = torch.tril(f.w(0)[:n, :n]).cpu().numpy()
    plain = torch.tril(engine.kernel_matrix(k, hyp_list(hyp), x, x, diag_add=noise, lower=True)).cpu().numpy()
    diff = int(np.count_nonzero(aug.view(np.uint64) != plain.view(np.uint64)))
    assert diff == 0, "%d of %d lower-triangle words differ" % (diff, aug.size)
    exp, bound = kernel_and_bound(tree, hyp, x, x)
    assert np.all(np.abs(aug - np.tril(exp + noise * np.eye(n))) <= np.tril(bound) + 1e-15)
    lay = f.layout                                                  # padding rows: identity, never a LIN value
    w = f.w(0).cpu().numpy()
    assert np.array_equal(np.tril(w[:lay.n_pad, :lay.n_pad])[n:], np.eye(lay.n_pad)[n:])
    assert np.array_equal(w[lay.y_row, :n], y) and np.all(w[lay.y_row, n:lay.n_pad] == 0.0)


# ------------------------------------------------------------------------------ 3. -LML and posterior, both paths
MODELS = {
    # name: tree, hyp, d, noise
    "LIN": (LIN, [[0.25]], 1, 0.1),
    "SE+LIN": (("ADD", [SE, LIN]), [0.6, [0.2, -0.4, 0.1]], 3, 0.1),
}


def _evaluate(tree, hyp, x, y, xs, noise, chain):
    before = nat.chain_stats()["launches"]
    with nat.thread_tune(chain=2 if chain else 0):     # (as tests/test_gpu_chain.py selects the path)
        g = build_gp(tree, x, y, xs)
        m = get_metric_by_type(MetricType.LL, g)
        nl = m.get_metric_checked(hyp_list(hyp), T(noise)).reshape(-1)[0].item()
        mu = g.predict(hyp_list(hyp), noise=T(noise))[2].reshape(-1).cpu().numpy()
        var = g.aux.get_posterior_var_diag(hyp_list(hyp), T(noise)).reshape(-1).cpu().numpy()
    launched = nat.chain_stats()["launches"] - before
    assert (launched > 0) if chain else (launched == 0)
    return nl, mu, var


@pytest.mark.parametrize("name", sorted(MODELS))
def test_nlml_and_posterior_match_oracle_on_both_paths(name, lin_oracle):
    """LogLikelihood.get_metric and GaussianProcess.predict (mu, diag Sigma) at n = 200, m = 70 against the patched
    oracle, through the persistent single-launch factorisation and the launch-per-panel path: bitwise equal.
    cond(K + noise I) of these inputs, computed on the CPU (numpy.linalg.cond): LIN D = 1 7.7e2, SE + LIN D = 3
    1.3e3 -- both far below 1e6, so n eps cond is inside the 1e-9 / 1e-8 bars."""
    tree, hyp, d, noise = MODELS[name]
    x, y, xs = lin_inputs(200, d, 31, m=70)
    assert np.linalg.cond(lin_oracle.k_noised(tree, hyp, noise, x)) <= 1e6
    nl_ref = lin_oracle.nlml(tree, hyp, noise, x, y)
    mu_ref, var_ref = lin_oracle.posterior(tree, hyp, noise, x, y, xs)
    chain = _evaluate(tree, hyp, x, y, xs, noise, True)
    launch = _evaluate(tree, hyp, x, y, xs, noise, False)
    for nl, mu, var in (chain, launch):
        print("%s: -LML rel %.3e, mu abs %.3e, var abs %.3e" % (name, rel(nl, nl_ref), np.abs(mu - mu_ref).max(),
                                                                np.abs(var - np.diag(var_ref)).max()))
        assert rel(nl, nl_ref) <= 1e-9
        np.testing.assert_allclose(mu, mu_ref, rtol=0, atol=1e-8)
        np.testing.assert_allclose(var, np.diag(var_ref), rtol=0, atol=1e-8)
    assert chain[0] == launch[0]
    assert np.array_equal(chain[1].view(np.uint64), launch[1].view(np.uint64))
    assert np.array_equal(chain[2].view(np.uint64), launch[2].view(np.uint64))


def test_golden_lin_small():
    """The recorded fixture (tests/golden/make_golden_lin.py): K, -LML, mu, diag Sigma of ADD(SE, LIN) at n = 200,
    m = 70, D = 3 -- independent of the helper module at test time."""
    g = np.load(GOLDEN + "/lin_small.npz")
    x, y, xs, noise = g["x"], g["y"], g["xs"], float(g["noise"])
    c = g["c"]
    hyp = [float(g["l"]), list(c)]
    kernel = ops.AdditionOperator(3, [bk.SquaredExponentialKernel(3), bk.LinearKernel(3)])
    K = kernel.get_tf_tensor(hyp_list(hyp), x, x).cpu().numpy()
    # SE part at the project's bar, LIN part at 1e-12 sum_k |x_k - c_k||y_k - c_k| + 1e-13
    k_se = o.kernel_matrix(SE, [hyp[0]], x, x)
    bound = (1e-12 * np.abs(k_se) + 1e-13) + (1e-12 * (np.abs(x - c) @ np.abs(x - c).T) + 1e-13)
    assert np.all(np.abs(K - g["K"]) <= bound)
    gp_ = build_gp(("ADD", [SE, LIN]), x, y, xs)
    nl = float(get_metric_by_type(MetricType.LL, gp_).get_metric_checked(hyp_list(hyp), T(noise)))
    assert rel(nl, float(g["nlml"])) <= 1e-9
    mu = gp_.predict(hyp_list(hyp), noise=T(noise))[2].reshape(-1).cpu().numpy()
    var = gp_.aux.get_posterior_var_diag(hyp_list(hyp), T(noise)).reshape(-1).cpu().numpy()
    np.testing.assert_allclose(mu, g["mu"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(var, g["var_diag"], rtol=0, atol=1e-8)


# ------------------------------------------------------------------------------ 4. closed form
def test_nlml_closed_form_d1():
    """D = 1, sg LIN + s2 I with sg = 1, s2 = 0.1, n = 300, x uniform on [-1, 1]: the device -LML against the
    determinant lemma / Sherman-Morrison formula (lin_support.lin_nlml_closed_form) -- no kernel-matrix code on the
    reference side.  cond ~ 1e3, so n eps cond is far inside rel 1e-9."""
    set_flags(scaled=True)
    rng = np.random.default_rng(41)
    x = rng.uniform(-1, 1, (300, 1))
    y = 0.7 * x[:, 0] + 0.3 * rng.standard_normal(300)
    c, sg, s2 = 0.25, 1.0, 0.1
    g = build_gp(LIN, x, y)
    got = float(get_metric_by_type(MetricType.LL, g).get_metric_checked(hyp_list([[c], sg]), T(s2)))
    exp = lin_nlml_closed_form(x, y, c, sg, s2)
    print("closed form: device %.12f exact %.12f rel %.3e" % (got, exp, rel(got, exp)))
    assert rel(got, exp) <= 1e-9


# ------------------------------------------------------------------------------ 5. fp32
def test_fp32_engine_against_fp64_oracle(lin_oracle):
    tree, hyp, d, noise = MODELS["SE+LIN"]
    x, y, _ = lin_inputs(200, d, 31)
    exp = lin_oracle.nlml(tree, hyp, noise, x, y)
    set_flags(dtype=torch.float32)
    g = build_gp(tree, x, y)
    m = get_metric_by_type(MetricType.LL, g)
    got = float(m.get_metric_checked(hyp_list(hyp), T(noise)))          # raises unless info == 0
    assert int(g.covariance_matrix.factorization(hyp_list(hyp), T(noise)).info.abs().max()) == 0
    print("fp32 SE + LIN: device %.6f oracle %.6f rel %.3e" % (got, exp, rel(got, exp)))
    assert rel(got, exp) <= 1e-3


# ------------------------------------------------------------------------------ 6. LML gradient
GRAD_TREES = [
    # tree, hyp, d, scaled
    (LIN, [[0.2, -0.4, 0.1], 0.7], 3, True),
    (("ADD", [SE, LIN]), [0.6, [0.2, -0.4, 0.1]], 3, False),
    (("MUL", [LIN, PER]), [[0.3], 0.9, 0.7], 1, False),
    (("MUL", [LIN, LIN]), [[0.3, -0.6], 0.5, [0.45, 0.1], 0.9], 2, True),
]


@pytest.mark.parametrize("case", range(len(GRAD_TREES)))
def test_lml_gradient_matches_autodiff_oracle(case, lin_oracle):
    """get_metric_and_gradient and autograd through get_metric at n = 150: every entry of c, sg and the noise."""
    tree, hyp, d, scaled = GRAD_TREES[case]
    set_flags(scaled=scaled)
    x, y, _ = lin_inputs(150, d, 60 + case)
    noise = 0.1
    nl_ref, g_ref, gn_ref = ad.nlml_and_grad(tree, hyp, noise, x, y, scaled)
    m = get_metric_by_type(MetricType.LL, build_gp(tree, x, y))
    nl, grads, gn = m.get_metric_and_gradient(hyp_list(hyp), T(noise))
    assert rel(float(nl), nl_ref) <= 1e-9
    assert [tuple(g.shape) for g in grads] == [np.shape(h) for h in hyp]
    check_grad([g.cpu().numpy() for g in grads] + [float(gn)], list(g_ref) + [gn_ref])
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(noise, dtype=F64, requires_grad=True)
    out = m.get_metric(h, nz)
    assert out.requires_grad and rel(float(out.detach()), nl_ref) <= 1e-9
    (2.0 * out.sum()).backward()
    check_grad([t.grad.numpy() for t in h] + [float(nz.grad)], [2.0 * g for g in g_ref] + [2.0 * gn_ref])


# ------------------------------------------------------------------------------ 7. kernel_vjp, Nystroem
@pytest.mark.parametrize("tree,hyp,scaled", [
    (("ADD", [SE, LIN]), [0.6, [0.2, -0.4, 0.1]], False),
    (("MUL", [LIN, SE]), [[0.2, -0.4, 0.1], 1.3, 0.6, 0.8], True),
])
def test_kernel_vjp_matches_autograd(tree, hyp, scaled, lin_oracle):
    set_flags(scaled=scaled)
    rng = np.random.default_rng(70)
    x, z = rng.uniform(-1, 1, (70, 3)), rng.uniform(-1, 1, (65, 3))
    G = rng.standard_normal((70, 65))
    params = [torch.tensor(np.asarray(h, dtype=np.float64), requires_grad=True) for h in hyp]
    Zt = torch.tensor(z, requires_grad=True)
    K = ad.kernel_matrix_t(tree, params, torch.tensor(x), Zt, scaled)
    gref = torch.autograd.grad(torch.sum(torch.tensor(G) * K), params + [Zt])
    gh, gz = engine.kernel_vjp(make_kernel(tree, 3), hyp_list(hyp), x, z, G=torch.tensor(G, device=engine.device()),
                               want_z=True)
    exp_h = np.concatenate([g.numpy().reshape(-1) for g in gref[:-1]])
    check_grad([gh.cpu().numpy()], [exp_h])
    check_grad([gz.cpu().numpy()], [gref[-1].numpy()])


def test_nystroem_metric_and_gradient(lin_oracle):
    """BASIC_NYSTROEM (CHOLESKY_BASED) -LML and its gradient w.r.t. hyperparameters, noise and the 20 inducing
    inputs for SE + LIN at n = 150 (tests/test_gpu_approx_grad.py's tolerances: value rel 1e-9, gradients 1e-7 of
    max |g_ref|)."""
    tree, hyp, noise, m = ("ADD", [SE, LIN]), [0.05, [0.4]], 0.05, 20
    x, y = o.make_inputs("C1", n=150, seed=3)
    z = (np.linspace(0.03, 0.97, m) + 0.004 * np.sin(np.arange(m))).reshape(m, 1)
    di = DataInput(x, y.reshape(-1, 1), x[:5], y[:5].reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(make_kernel(tree, 1), ZeroMeanFunction(1))
    g.set_data_input(di)
    met = get_metric_by_type(MetricType.LL, g, mht.MatrixApproximations.BASIC_NYSTROEM,
                             mht.NumericalMatrixHandlingType.CHOLESKY_BASED, subset_size=m)
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(noise, dtype=F64, requires_grad=True)
    zt = torch.tensor(z, dtype=F64, requires_grad=True)
    out = met.get_metric(h, nz, zt)
    out.sum().backward()
    nl, gh, gn, gz = ad.nystroem_nlml_and_grad(tree, hyp, noise, x, y, z, "CHOLESKY_BASED")
    assert rel(float(out.detach()), nl) <= 1e-9
    got = np.concatenate([t.grad.numpy().reshape(-1) for t in h] + [[float(nz.grad)]])
    exp = np.concatenate([np.asarray(v).reshape(-1) for v in gh] + [[gn]])
    assert np.max(np.abs(got - exp)) <= 1e-7 * np.max(np.abs(exp)), (got, exp)
    assert np.max(np.abs(zt.grad.numpy() - gz)) <= 1e-7 * np.max(np.abs(gz))


def _approx_gp(tree, x, y):
    di = DataInput(x, y.reshape(-1, 1), x[:5], y[:5].reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(make_kernel(tree, 1), ZeroMeanFunction(1))
    g.set_data_input(di)
    return g


@pytest.mark.parametrize("tree,hyp,d,scaled", [
    (("ADD", [SE, LIN]), [0.6, 1.2, [0.2, -0.4, 0.1], 0.8], 3, True),
    (("MUL", [LIN, PER]), [[0.3], 0.9, 0.7], 1, False),
])
def test_trace_adjoint_of_a_non_stationary_tree(tree, hyp, d, scaled, lin_oracle, monkeypatch):
    """The adjoint of trace(K) behind the SKC lower bound (NystroemAdjoint.diag_adjoint): with a LIN leaf k(x, x)
    depends on x, so it is the sum over all training points -- here over three chunks (64, 64, 22) -- against torch
    autograd of sum_i k(x_i, x_i) on the restatement, at the gradient bar 1e-7 max(1, |g_ref|_max)."""
    from gaussianprocessfundamentals_amd.Metrics._approx_grad import NystroemAdjoint
    set_flags(scaled=scaled)
    x, _, _ = lin_inputs(150, d, 75)
    params = [torch.tensor(np.asarray(h, dtype=np.float64), requires_grad=True) for h in hyp]
    K = ad.kernel_matrix_t(tree, params, torch.tensor(x), torch.tensor(x), scaled)
    gref = torch.autograd.grad(torch.trace(K), params)
    monkeypatch.setattr(NystroemAdjoint, "DIAG_CHUNK", 64)
    adj = NystroemAdjoint(make_kernel(tree, d), hyp_list(hyp), torch.as_tensor(x, device=engine.device()), None, 0.1)
    assert not adj.stationary
    check_grad([adj.diag_adjoint().cpu().numpy()], [np.concatenate([g.numpy().reshape(-1) for g in gref])])
    set_flags(scaled=False)
    assert NystroemAdjoint(make_kernel(SE, d), hyp_list([0.5]), torch.as_tensor(x, device=engine.device()), None,
                           0.1).stationary


@pytest.mark.parametrize("scaled", [False, True])
def test_skc_lower_bound_metric_and_gradient(scaled, lin_oracle):
    """SKC_LOWER_BOUND (CHOLESKY_BASED) for SE + LIN at n = 150, 20 inducing inputs: its trace correction
    trace(K_hat + noise I - K) / (2 jitter) differentiates k(x_i, x_i) at every training point.  Tolerances of
    tests/test_gpu_approx_grad.py's lower-bound cases: value rel 1e-9, gradients 1e-5 of max |g_ref| (the 1 / (2 jitter)
    = 5e7 factor amplifies the rounding of the trace terms)."""
    import gaussianprocessfundamentals_amd.global_parameters as gpar
    set_flags(scaled=scaled)
    tree, noise, m = ("ADD", [SE, LIN]), 0.05, 20
    hyp = [0.05, 1.2, [0.4], 0.8] if scaled else [0.05, [0.4]]
    x, y = o.make_inputs("C1", n=150, seed=3)
    z = (np.linspace(0.03, 0.97, m) + 0.004 * np.sin(np.arange(m))).reshape(m, 1)
    met = get_metric_by_type(MetricType.LL, _approx_gp(tree, x, y), mht.MatrixApproximations.SKC_LOWER_BOUND,
                             mht.NumericalMatrixHandlingType.CHOLESKY_BASED, subset_size=m)
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(noise, dtype=F64, requires_grad=True)
    zt = torch.tensor(z, dtype=F64, requires_grad=True)
    out = met.get_metric(h, nz, zt)
    out.sum().backward()
    nl, gh, gn, gz = ad.nystroem_nlml_and_grad(tree, hyp, noise, x, y, z, "CHOLESKY_BASED", True,
                                               float(gpar.p_cov_matrix_jitter), scaled)
    assert rel(float(out.detach()), nl) <= 1e-9
    got = np.concatenate([t.grad.numpy().reshape(-1) for t in h] + [[float(nz.grad)]])
    exp = np.concatenate([np.asarray(v).reshape(-1) for v in gh] + [[gn]])
    print("SKC lower bound scaled=%s: |g - g_ref| / max|g_ref| %s" % (scaled, np.abs(got - exp) / np.max(np.abs(exp))))
    assert np.max(np.abs(got - exp)) <= 1e-5 * np.max(np.abs(exp)), (got, exp)
    assert np.max(np.abs(zt.grad.numpy() - gz)) <= 1e-5 * np.max(np.abs(gz))


def test_ski_metric_and_gradient(lin_oracle):
    """SKI (STRICT_INVERSE), SE + LIN, n = 150, 40 inducing points (tests/test_gpu_approx_grad.py's SKI tolerances)."""
    tree, hyp, noise, m = ("ADD", [SE, LIN]), [0.05, [0.4]], 0.05, 40
    x, y = o.make_inputs("C1", n=150, seed=3)
    met = get_metric_by_type(MetricType.LL, _approx_gp(tree, x, y), mht.MatrixApproximations.SKI,
                             mht.NumericalMatrixHandlingType.STRICT_INVERSE, subset_size=m)
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(noise, dtype=F64, requires_grad=True)
    out = met.get_metric(h, nz)
    out.sum().backward()
    nl, gh, gn = ad.ski_nlml_and_grad(tree, hyp, noise, x, y, m, "STRICT_INVERSE")
    assert rel(float(out.detach()), nl) <= 1e-9
    got = np.concatenate([t.grad.numpy().reshape(-1) for t in h] + [[float(nz.grad)]])
    exp = np.concatenate([np.asarray(v).reshape(-1) for v in gh] + [[gn]])
    assert np.max(np.abs(got - exp)) <= 1e-7 * np.max(np.abs(exp)), (got, exp)


# ------------------------------------------------------------------------------ 8. segmented models
def test_change_point_model_with_lin_child(lin_oracle):
    n, cp, noise = 200, 0.5, 1e-2
    rng = np.random.default_rng(80)
    x = np.sort(rng.uniform(0, 1, n)).reshape(-1, 1)
    y = np.where(x[:, 0] < cp, 1.5 * x[:, 0], np.cos(6 * x[:, 0])) + 0.05 * rng.standard_normal(n)
    xt = np.sort(rng.uniform(0, 1, 40)).reshape(-1, 1)
    kernel = ops.ChangePointOperator(1, [bk.LinearKernel(1), bk.SquaredExponentialKernel(1)], [T(cp)])
    di = BlockwiseDataInput(x, y.reshape(-1, 1), xt, np.zeros((40, 1)), [T(cp)])
    di.set_mean_function(ZeroMeanFunction(1))
    g = BlockwiseGaussianProcess(kernel, ZeroMeanFunction(1))
    g.set_data_input(di)
    hyp = [[0.3], 0.1]                                 # children only (the reference slices from offset 0)
    got = float(get_metric_by_type(MetricType.blockwise_LL, g).get_metric(hyp_list(hyp), T(noise)))
    a = x[:, 0] < cp
    exp = lin_oracle.blockwise_nlml([(LIN, [[0.3]], x[a], y[a]), (SE, [0.1], x[~a], y[~a])], noise)
    assert rel(got, exp) <= 1e-9, (got, exp)


def test_ragged_batch_with_lin_members(lin_oracle):
    sizes, noise, d = [70, 130], 1e-2, 3
    specs = [(LIN, [[0.2, -0.4, 0.1]]), (("ADD", [SE, LIN]), [0.6, [0.1, 0.3, -0.2]])]
    dev = engine.device()
    members, segs = [], []
    for b, (n, (tree, hyp)) in enumerate(zip(sizes, specs)):
        x, y, _ = lin_inputs(n, d, 85 + b)
        kd = engine.kernel_descriptor(make_kernel(tree, d), d)
        members.append((kd, engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp), torch.tensor(x, device=dev),
                        torch.tensor(y, device=dev), None))
        segs.append((tree, hyp, x, y))
    f = engine.RaggedFactorization(sizes, d)
    f.run(members, T(noise))
    f.check_info()
    nl = f.nlml().cpu().numpy()
    for b, (tree, hyp, x, y) in enumerate(segs):
        assert rel(float(nl[b]), lin_oracle.nlml(tree, hyp, noise, x, y)) <= 1e-9
    assert rel(float(nl.sum()), lin_oracle.blockwise_nlml(segs, noise)) <= 1e-9


# ------------------------------------------------------------------------------ 9. rejection
def _lin_kdesc(d, n_hyp, flags=0, slot=-1, n_ard=0):
    kd = nat.GpkKdesc()
    kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 1, n_hyp, d, n_ard
    kd.nodes[0].op, kd.nodes[0].hyp_offset, kd.nodes[0].ard_slot, kd.nodes[0].flags = nat.OP_LIN, 0, slot, flags
    return kd


def test_invalid_lin_descriptors_are_rejected():
    """A LIN node with GPK_NODE_ARD (or the expanded / standard flags), or with n_hyp one short, is refused by
    gpk_kernel_matrix with the negative bad-argument code before anything is launched; K stays untouched."""
    d, n = 3, 10
    dev = engine.device()
    X = torch.zeros((n, d), dtype=F64, device=dev)
    hyp = torch.full((d + 1,), 0.1, dtype=F64, device=dev)
    K = torch.full((n, n), 7.0, dtype=F64, device=dev)
    L = nat.lib()

    def call(kd):
        return L.gpk_kernel_matrix(ctypes.byref(kd), nat.ptr(hyp), nat.GPK_F64, 0, nat.ptr(X), n, nat.ptr(X), n, d, 0.0,
                                   nat.ptr(K), n, nat.stream_handle(dev))

    bad = [_lin_kdesc(d, d, nat.NODE_ARD, 0, 1), _lin_kdesc(d, d, nat.NODE_SE_EXPANDED), _lin_kdesc(d, d, nat.NODE_STANDARD),
           _lin_kdesc(d, d - 1), _lin_kdesc(d, d, nat.NODE_SCALED), _lin_kdesc(d, d, 0, 0)]
    for kd in bad:
        assert call(kd) == -1
    torch.cuda.synchronize()
    assert bool(torch.all(K == 7.0))
    assert call(_lin_kdesc(d, d)) == 0 and call(_lin_kdesc(d, d + 1, nat.NODE_SCALED)) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(K.cpu().numpy(), 0.1 * (3 * 0.01), rtol=1e-14, atol=0)   # x = 0: sg sum_k c_k^2
