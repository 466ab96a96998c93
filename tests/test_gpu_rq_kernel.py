"""The RQ leaf (RationalQuadraticKernel, GPK_OP_RQ) on the HIP path vs the restatement of tests/rq_support.py (needs the
MI355X).

k = sg (1 + u)^(-a), u = s / (2 a l^2), s the squared Euclidean distance.  Shapes: N = 200 training and M = 37 test
points (more than one 64-point tile per side, no side a multiple of the tile edge), D in {1, 3, 16} (16 takes the
generic tile loop, 1 and 3 the interior loops).  Inputs on [-1, 1]^D, l in [0.2, 1], a in {0.3, 2, 50}, noise 1e-2.
Tolerances:
  kernel matrices   the project's bar rel 1e-12 |k| + abs 1e-13 per leaf, propagated through ADD (sum of bounds) and
                    MUL (|a| db + |b| da) with the restatement's own node values (rq_support.kernel_and_bound).  The
                    exponent a log1p(u) stays below 1000 for these inputs (asserted), so its rounding,
                    <= a log1p(u) eps <= 2.3e-13 relative in k, is inside the bar.
  -LML              rel <= 1e-9; posterior mu / diag Sigma abs <= 1e-8 (the project's C2 bars); alpha within
                    2 n eps cond(K + noise I) ||alpha||_2 (two Cholesky solves, the oracle's and the device's)
  gradients         |g - g_ref| <= 1e-7 max(1, |g_ref|_max) (tests/test_gpu_grad.py's bar)
  fp32              -LML rel <= 1e-3 against the fp64 oracle
  d k / d a         rel 1e-12 against mpmath where u / (1 + u) - log1p(u) cancels
The oracle modules learn the leaf through the ``rq_oracle`` fixture for the duration of a test."""
import ctypes

import mpmath
import numpy as np
import pytest
import torch

from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests import cp_support as cs
from tests.helpers import hyp_list, set_flags
from tests.rq_support import (RQ, g_exact, kernel_and_bound, make_kernel, rq_inputs, rq_numpy, rq_oracle,  # noqa: F401
                              rq_u_numpy, with_sg)

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess

pytestmark = pytest.mark.gpu

F64 = torch.float64
SE = ("SE", {})
PER = ("PER", {})
MAT52 = ("MAT52", {})
N, M, NOISE = 200, 37, 1e-2
EPS = float(np.finfo(np.float64).eps)


def T(v):
    return torch.tensor(v, dtype=F64)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


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


def augmented_training_block(tree, hyp, x, y, noise, dtype=F64):
    """(lower triangle of the n x n training block of gpk_assemble's augmented matrix, the whole matrix, its layout)"""
    n, d = x.shape
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(tree, d), d)
    H = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp).reshape(1, -1).contiguous()
    X = torch.as_tensor(x, device=dev).contiguous()
    Y = torch.as_tensor(y, device=dev).reshape(1, -1).contiguous()
    NZ = torch.tensor([noise], dtype=F64, device=dev)
    f = engine.AugmentedFactorization(n, d, 0, 1, dtype)
    f.W.zero_()
    nat.check(nat.lib().gpk_assemble(ctypes.byref(kd), ctypes.byref(f.layout), nat.ptr(H), kd.n_hyp, nat.ptr(NZ), 0,
                                     nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W),
                                     nat.stream_handle(f.W.device)), "gpk_assemble")
    torch.cuda.synchronize()
    w = f.w(0).cpu().numpy()
    return np.tril(w[:n, :n]), w, f.layout


# ------------------------------------------------------------------------------ 1. kernel matrix
A_VALUES = (0.3, 2.0, 50.0)
L_VALUES = (0.2, 0.6, 1.0)


def _tree_cases(ia):
    l, a = L_VALUES[ia], A_VALUES[ia]
    return [("RQ", RQ, [l, a]),
            ("SE+RQ", ("ADD", [SE, RQ]), [0.6, l, a]),
            ("RQxPER", ("MUL", [RQ, PER]), [l, a, 0.9, 0.7])]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("ia", range(3))
@pytest.mark.parametrize("d", [1, 3, 16])
def test_kernel_matrix_matches_restatement(d, ia, case, scaled):
    """get_tf_tensor at 200 x 37 (whole, edge and partial tiles, non-square) and the training block of the augmented
    build at 200 x 200 against the restatement, inside the bound propagated from the leaves."""
    name, tree, hyp = _tree_cases(ia)[case]
    set_flags(scaled=scaled)
    if scaled:
        hyp = with_sg(tree, hyp, [0.7, 1.3])
    x, y, xs = rq_inputs(N, d, 3, m=M)
    # the exponent a log1p(u) of every element: below 1000, so its rounding (<= that times eps) is inside rel 1e-12
    u = rq_u_numpy([L_VALUES[ia], A_VALUES[ia]], x, x)
    expo = float((A_VALUES[ia] * np.log1p(u)).max())
    assert expo < 1000.0
    k = make_kernel(tree, d)
    got = k.get_tf_tensor(hyp_list(hyp), x, xs).cpu().numpy()
    exp, bound = kernel_and_bound(tree, hyp, x, xs, scaled)
    assert got.shape == (N, M)
    err = np.abs(got - exp)
    print("%s d=%d a=%g scaled=%s: max exponent %.1f, max err %.3e, max err / bound %.3e"
          % (name, d, A_VALUES[ia], scaled, expo, err.max(), (err / bound).max()))
    assert np.all(err <= bound), (name, float((err / bound).max()))
    assert k.get_last_hyper_parameter() is not None
    aug, _, _ = augmented_training_block(tree, hyp, x, y, NOISE)
    exp, bound = kernel_and_bound(tree, hyp, x, x, scaled)
    err = np.abs(aug - np.tril(exp + NOISE * np.eye(N)))
    print("   augmented build: max err / bound %.3e" % (err / (bound + 1e-15)).max())
    assert np.all(err <= np.tril(bound) + 1e-15)


# ------------------------------------------------------------------------------ 2. symmetry, fp32 output
@pytest.mark.parametrize("d", [1, 3, 16])
def test_kernel_matrix_symmetric_and_fp32_output(d):
    x, _, _ = rq_inputs(N, d, 4)
    k = make_kernel(RQ, d)
    hyp = [0.6, 2.0]
    K = k.get_tf_tensor(hyp_list(hyp), x, x)
    assert torch.equal(K, K.T)                       # (a_k - b_k)^2 == (b_k - a_k)^2: K(a, b) == K(b, a) bit for bit
    assert bool(torch.all(torch.diagonal(K) == 1.0))  # u = 0 exactly: log1p(0) = 0, exp(-0) = 1
    K32 = engine.kernel_matrix(k, hyp_list(hyp), x, x, out_dtype=torch.float32)
    assert K32.dtype == torch.float32 and torch.equal(K32, K.to(torch.float32))


# ------------------------------------------------------------------------------ 3. same bits on every build path
@pytest.mark.parametrize("tree,hyp,d", [
    (RQ, [0.5, 2.0], 3),
    (RQ, [0.2, 50.0], 1),
    (RQ, [0.8, 0.3], 8),                                            # the widest interior instantiation
    (RQ, [1.0, 0.3], 16),                                           # no interior loop: the generic tile loop
    (("ADD", [SE, RQ]), [0.6, 0.4, 0.3], 3),
    (("ADD", [RQ, SE]), [0.4, 0.3, 0.6], 3),
    (("MUL", [RQ, PER]), [0.5, 2.0, 0.9, 0.7], 1),                  # the periodic leaf's sin / cos form beside RQ
    (("ADD", [("MUL", [SE, RQ]), MAT52]), [0.6, 0.5, 2.0, 0.8], 3),  # the general tree loop
])
def test_augmented_build_is_bitwise_the_plain_build(tree, hyp, d):
    """The n x n training block of the augmented build (interior, edge and generic tiles, noise on the diagonal)
    equals gpk_kernel_matrix's plain build (lower triangle, diag_add = noise) bit for bit, and matches the
    restatement."""
    x, y, _ = rq_inputs(N, d, 21)
    aug, w, lay = augmented_training_block(tree, hyp, x, y, NOISE)
    k = make_kernel(tree, d)
    plain = torch.tril(engine.kernel_matrix(k, hyp_list(hyp), x, x, diag_add=NOISE, lower=True)).cpu().numpy()
    diff = int(np.count_nonzero(aug.view(np.uint64) != plain.view(np.uint64)))
    assert diff == 0, "%d of %d lower-triangle words differ" % (diff, aug.size)
    exp, bound = kernel_and_bound(tree, hyp, x, x)
    assert np.all(np.abs(aug - np.tril(exp + NOISE * np.eye(N))) <= np.tril(bound) + 1e-15)
    assert np.array_equal(np.tril(w[:lay.n_pad, :lay.n_pad])[N:], np.eye(lay.n_pad)[N:])   # padding rows: identity
    assert np.array_equal(w[lay.y_row, :N], y) and np.all(w[lay.y_row, N:lay.n_pad] == 0.0)


# ------------------------------------------------------------------------------ 4. the SE limit
@pytest.mark.parametrize("a", [1e6, 1e10, 1e14])
def test_se_limit_inequality(a):
    """u - u^2 / 2 <= log1p(u) <= u gives, elementwise, k_SE <= k_RQ <= k_SE exp(s^2 / (8 a l^4)); each side widened by
    the project's bar rel 1e-12 + abs 1e-13 (the device's exponent a log1p(u) = s / (2 l^2) (1 + O(eps)) is at most
    ~24 here, so its rounding is <= 1e-14 relative)."""
    l, d = 0.5, 3
    x, _, xs = rq_inputs(N, d, 5, m=M)
    got = make_kernel(RQ, d).get_tf_tensor(hyp_list([l, a]), x, xs).cpu().numpy()
    s = o.squared_l2_direct(x, xs)
    kse = o.kernel_matrix(SE, [l], x, xs)
    lo, hi = kse, kse * np.exp(s * s / (8.0 * a * l ** 4))
    print("a = %g: min (k - lo) %.3e, min (hi - k) %.3e, max hi / lo - 1 %.3e"
          % (a, (got - lo).min(), (hi - got).min(), (hi / lo).max() - 1.0))
    assert np.all(got >= lo - (1e-12 * lo + 1e-13))
    assert np.all(got <= hi + (1e-12 * hi + 1e-13))


# ------------------------------------------------------------------------------ 5. -LML, alpha, posterior: both paths
MODELS = {
    # name: tree, hyp, d
    "RQ": (RQ, [0.5, 2.0], 3),
    "RQ-a50-d1": (RQ, [0.2, 50.0], 1),
    "RQ-a0.3-d16": (RQ, [1.0, 0.3], 16),
    "SE+RQ": (("ADD", [SE, RQ]), [0.6, 0.4, 0.3], 3),
    "RQxPER": (("MUL", [RQ, PER]), [0.5, 2.0, 0.9, 0.7], 1),
}


def _evaluate(tree, hyp, x, y, xs, noise, chain):
    before = nat.chain_stats()["launches"]
    with nat.thread_tune(chain=2 if chain else 0):     # (as tests/test_gpu_chain.py selects the path)
        g = build_gp(tree, x, y, xs)
        m = get_metric_by_type(MetricType.LL, g)
        nl = m.get_metric_checked(hyp_list(hyp), T(noise)).reshape(-1)[0].item()
        alpha = m.get_alpha_cholesky(hyp_list(hyp), T(noise)).reshape(-1).cpu().numpy()
        mu = g.predict(hyp_list(hyp), noise=T(noise))[2].reshape(-1).cpu().numpy()
        var = g.aux.get_posterior_var_diag(hyp_list(hyp), T(noise)).reshape(-1).cpu().numpy()
        cov = g.aux.get_posterior_var(hyp_list(hyp), T(noise)).cpu().numpy()
    launched = nat.chain_stats()["launches"] - before
    assert (launched > 0) if chain else (launched == 0)
    return nl, alpha, mu, var, cov


@pytest.mark.parametrize("name", sorted(MODELS))
def test_nlml_alpha_and_posterior_match_oracle_on_both_paths(name, rq_oracle):
    """LogLikelihood.get_metric, alpha and GaussianProcess.predict (mu, Sigma) at n = 200, m = 37 against the patched
    oracle, through the persistent single-launch factorisation and the launch-per-panel path: bitwise equal.  The
    oracle's own factorisation must succeed and K + noise I be well conditioned (lambda_min, cond printed; cond <= 1e6,
    so n eps cond is inside the 1e-9 / 1e-8 bars) before anything is compared."""
    tree, hyp, d = MODELS[name]
    x, y, xs = rq_inputs(N, d, 31, m=M)
    Kn = rq_oracle.k_noised(tree, hyp, NOISE, x)
    lam = np.linalg.eigvalsh(Kn)
    np.linalg.cholesky(Kn)                                   # (raises LinAlgError if the oracle cannot factorise)
    cond = float(lam[-1] / lam[0])
    print("%s: lambda_min %.4f, cond %.3e" % (name, lam[0], cond))
    assert lam[0] > 0.0 and cond <= 1e6
    nl_ref = rq_oracle.nlml(tree, hyp, NOISE, x, y)
    alpha_ref = np.linalg.solve(Kn, y)
    mu_ref, var_ref = rq_oracle.posterior(tree, hyp, NOISE, x, y, xs)
    chain = _evaluate(tree, hyp, x, y, xs, NOISE, True)
    launch = _evaluate(tree, hyp, x, y, xs, NOISE, False)
    alpha_bar = 2.0 * N * EPS * cond * float(np.linalg.norm(alpha_ref))
    for nl, alpha, mu, var, cov in (chain, launch):
        print("%s: -LML rel %.3e, alpha abs %.3e (bar %.3e), mu abs %.3e, var abs %.3e, cov abs %.3e"
              % (name, rel(nl, nl_ref), np.abs(alpha - alpha_ref).max(), alpha_bar, np.abs(mu - mu_ref).max(),
                 np.abs(var - np.diag(var_ref)).max(), np.abs(cov - var_ref).max()))
        assert rel(nl, nl_ref) <= 1e-9
        assert np.abs(alpha - alpha_ref).max() <= alpha_bar
        np.testing.assert_allclose(mu, mu_ref, rtol=0, atol=1e-8)
        np.testing.assert_allclose(var, np.diag(var_ref), rtol=0, atol=1e-8)
        np.testing.assert_allclose(cov.reshape(var_ref.shape), var_ref, rtol=0, atol=1e-8)
    assert chain[0] == launch[0]
    for a, b in zip(chain[1:], launch[1:]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("name", ["RQ", "SE+RQ"])
def test_fp32_engine_against_fp64_oracle(name, rq_oracle):
    tree, hyp, d = MODELS[name]
    x, y, _ = rq_inputs(N, d, 31)
    exp = rq_oracle.nlml(tree, hyp, NOISE, x, y)
    set_flags(dtype=torch.float32)
    g = build_gp(tree, x, y)
    m = get_metric_by_type(MetricType.LL, g)
    got = float(m.get_metric_checked(hyp_list(hyp), T(NOISE)))          # raises unless info == 0
    assert int(g.covariance_matrix.factorization(hyp_list(hyp), T(NOISE)).info.abs().max()) == 0
    print("fp32 %s: device %.6f oracle %.6f rel %.3e" % (name, got, exp, rel(got, exp)))
    assert rel(got, exp) <= 1e-3


# ------------------------------------------------------------------------------ 6. LML gradient
GRAD_TREES = [
    # tree, hyp, d, scaled
    (RQ, [0.5, 2.0, 0.7], 3, True),
    (RQ, [0.2, 50.0], 1, False),
    (RQ, [1.0, 0.3, 1.3], 16, True),
    (("ADD", [SE, RQ]), [0.6, 0.4, 0.3], 3, False),
    (("ADD", [SE, RQ]), [0.6, 1.2, 0.4, 2.0, 0.8], 3, True),
    (("MUL", [RQ, PER]), [0.5, 2.0, 0.9, 0.7], 1, False),
    (("MUL", [RQ, PER]), [0.3, 50.0, 0.7, 0.9, 0.7, 1.1], 1, True),
]


@pytest.mark.parametrize("case", range(len(GRAD_TREES)))
def test_lml_gradient_matches_autodiff_oracle(case, rq_oracle):
    """get_metric_and_gradient and autograd through get_metric at n = 200: l, a, sg of every leaf and the noise."""
    tree, hyp, d, scaled = GRAD_TREES[case]
    set_flags(scaled=scaled)
    x, y, _ = rq_inputs(N, d, 60 + case)
    nl_ref, g_ref, gn_ref = ad.nlml_and_grad(tree, hyp, NOISE, x, y, scaled)
    m = get_metric_by_type(MetricType.LL, build_gp(tree, x, y))
    nl, grads, gn = m.get_metric_and_gradient(hyp_list(hyp), T(NOISE))
    assert rel(float(nl), nl_ref) <= 1e-9
    assert [tuple(g.shape) for g in grads] == [np.shape(h) for h in hyp]
    print("case %d: g %s g_ref %s" % (case, [float(g) for g in grads] + [float(gn)], [float(g) for g in g_ref] + [gn_ref]))
    check_grad([g.cpu().numpy() for g in grads] + [float(gn)], list(g_ref) + [gn_ref])
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(NOISE, dtype=F64, requires_grad=True)
    out = m.get_metric(h, nz)
    assert out.requires_grad and rel(float(out.detach()), nl_ref) <= 1e-9
    (2.0 * out.sum()).backward()
    check_grad([t.grad.numpy() for t in h] + [float(nz.grad)], [2.0 * g for g in g_ref] + [2.0 * gn_ref])


def test_lml_gradient_of_a_change_point_model_with_an_rq_child(rq_oracle):
    """ChangePointOperator([RQ, SE]) under SIGMOID at n = 200, inputs inside the transition zone: the window adjoint
    multiplies an RQ child.  tests/test_gpu_change_point.py's bar, 1e-7 of max |g_ref|, with and without the change point."""
    old = gp.p_cp_operator_type
    try:
        cs.set_mode("SIGMOID")
        tree, hyp = ("CP", [RQ, SE]), [0.5, 0.2, 2.0, 0.15]
        x, y, _ = cs.cp_inputs(N, 51, [0.5])
        nl_ref, g_ref, gn_ref = cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, "SIGMOID")
        kernel = ops.ChangePointOperator(1, [bk.RationalQuadraticKernel(1), bk.SquaredExponentialKernel(1)], [T(0.5)])
        di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
        di.set_mean_function(ZeroMeanFunction(1))
        g = GaussianProcess(kernel, ZeroMeanFunction(1))
        g.set_data_input(di)
        m = get_metric_by_type(MetricType.LL, g)
        nl, grads, gn = m.get_metric_and_gradient(hyp_list(hyp), T(NOISE))
        assert rel(float(nl), nl_ref) <= 1e-9
        got = np.concatenate([t.cpu().numpy().reshape(-1) for t in grads] + [[float(gn)]])
        exp = np.concatenate([g_ref, [gn_ref]])
        err = np.abs(got - exp)
        print("CP([RQ, SE]) SIGMOID: |g - g_ref| %s  g_ref %s" % (err, exp))
        assert np.max(err) <= 1e-7 * np.max(np.abs(exp))
        assert np.max(err[1:]) <= 1e-7 * np.max(np.abs(exp[1:]))
        assert abs(exp[2]) > 0.0                                       # the RQ child's a really enters
    finally:
        gp.p_cp_operator_type = old


# ------------------------------------------------------------------------------ 7. kernel_vjp
@pytest.mark.parametrize("tree,hyp,scaled,d", [
    (RQ, [0.5, 2.0], False, 3),
    (RQ, [0.5, 2.0, 0.7], True, 3),
    (RQ, [1.0, 0.3, 1.3], True, 16),
    (("ADD", [SE, RQ]), [0.6, 0.4, 0.3], False, 3),
    (("MUL", [RQ, SE]), [0.3, 50.0, 1.3, 0.6, 0.8], True, 3),
])
def test_kernel_vjp_matches_autograd(tree, hyp, scaled, d, rq_oracle):
    """Hyperparameter adjoints and the adjoints of the second argument's points at 70 x 65, five of the second
    argument's points coincident with first-argument points (the analytic 0 contribution there, never NaN)."""
    set_flags(scaled=scaled)
    rng = np.random.default_rng(70)
    x, z = rng.uniform(-1, 1, (70, d)), rng.uniform(-1, 1, (65, d))
    z[:5] = x[10:15]
    G = rng.standard_normal((70, 65))
    params = [torch.tensor(np.asarray(h, dtype=np.float64), requires_grad=True) for h in hyp]
    Zt = torch.tensor(z, requires_grad=True)
    K = ad.kernel_matrix_t(tree, params, torch.tensor(x), Zt, scaled)
    gref = torch.autograd.grad(torch.sum(torch.tensor(G) * K), params + [Zt])
    gh, gz = engine.kernel_vjp(make_kernel(tree, d), hyp_list(hyp), x, z, G=torch.tensor(G, device=engine.device()),
                               want_z=True)
    assert bool(torch.all(torch.isfinite(gh))) and bool(torch.all(torch.isfinite(gz)))
    exp_h = np.concatenate([g.numpy().reshape(-1) for g in gref[:-1]])
    check_grad([gh.cpu().numpy()], [exp_h])
    check_grad([gz.cpu().numpy()], [gref[-1].numpy()])


@pytest.mark.parametrize("scaled", [False, True])
def test_kernel_vjp_at_a_coincident_point_is_the_analytic_zero(scaled):
    set_flags(scaled=scaled)
    x = np.array([[0.3, -0.2, 0.9]])
    hyp = [0.5, 2.0, 0.7] if scaled else [0.5, 2.0]
    gh, gz = engine.kernel_vjp(make_kernel(RQ, 3), hyp_list(hyp), x, x.copy(), G=torch.ones((1, 1), dtype=F64,
                               device=engine.device()), want_z=True)
    gh, gz = gh.cpu().numpy(), gz.cpu().numpy()
    assert np.all(gz == 0.0) and gh[0] == 0.0 and gh[1] == 0.0          # s = 0: d k / d z = d k / d l = d k / d a = 0
    if scaled:
        assert gh[2] == 1.0                                             # d k / d sg = the unscaled value k(x, x) = 1


# ------------------------------------------------------------------------------ 8. d k / d a where g(u) cancels
@pytest.mark.parametrize("u_target", [1e-12, 1e-8, 1e-4])
def test_a_partial_at_small_u(u_target):
    """kernel_vjp with n = m = 1, G = [[1]], D = 1, l = 1, a = 1 and |x - z| = sqrt(2 u): d k / d a against
    k g_exact(u) in mpmath (of the u the doubles x, z really give), within rel 1e-12.  The direct form
    u / (1 + u) - log1p(u) misses this by 4.8e-5 at u = 1e-12 and 2.9e-9 at 1e-8."""
    set_flags(scaled=False)
    z = float(np.sqrt(2.0 * u_target))
    gh, _ = engine.kernel_vjp(make_kernel(RQ, 1), hyp_list([1.0, 1.0]), np.array([[0.0]]), np.array([[z]]),
                              G=torch.ones((1, 1), dtype=F64, device=engine.device()), want_z=True)
    got = float(gh[1])
    with mpmath.workdps(60):
        u = mpmath.mpf(z) ** 2 / 2
        exact = g_exact(u) / (1 + u)                                    # k = (1 + u)^-1 at a = 1
        err = float(abs((mpmath.mpf(got) - exact) / exact))
    print("u = %.3e: d k / d a %.17e exact %s rel %.3e" % (u_target, got, mpmath.nstr(exact, 20), err))
    assert err <= 1e-12


# ------------------------------------------------------------------------------ 9. approximations, ragged batches
def _approx_gp(tree, x, y):
    di = DataInput(x, y.reshape(-1, 1), x[:5], y[:5].reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(make_kernel(tree, 1), ZeroMeanFunction(1))
    g.set_data_input(di)
    return g


def _inducing(m):
    return (np.linspace(0.03, 0.97, m) + 0.004 * np.sin(np.arange(m))).reshape(m, 1)


def test_nystroem_metric_and_gradient(rq_oracle):
    """BASIC_NYSTROEM (CHOLESKY_BASED) -LML and its gradient w.r.t. hyperparameters, noise and the 20 inducing inputs
    for SE + RQ at n = 150 (tests/test_gpu_approx_grad.py's tolerances: value rel 1e-9, gradients 1e-7 of max |g_ref|).
    NystroemAdjoint treats the tree as stationary: k(x, x) = sg for an RQ leaf."""
    from gaussianprocessfundamentals_amd.Metrics._approx_grad import NystroemAdjoint
    tree, hyp, noise, m = ("ADD", [SE, RQ]), [0.05, 0.4, 2.0], 0.05, 20
    x, y = o.make_inputs("C1", n=150, seed=3)
    z = _inducing(m)
    assert NystroemAdjoint(make_kernel(tree, 1), hyp_list(hyp), torch.as_tensor(x, device=engine.device()), None,
                           noise).stationary
    met = get_metric_by_type(MetricType.LL, _approx_gp(tree, x, y), mht.MatrixApproximations.BASIC_NYSTROEM,
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
    print("Nystroem: |g - g_ref| / max|g_ref| %s" % (np.abs(got - exp) / np.max(np.abs(exp))))
    assert np.max(np.abs(got - exp)) <= 1e-7 * np.max(np.abs(exp)), (got, exp)
    assert np.max(np.abs(zt.grad.numpy() - gz)) <= 1e-7 * np.max(np.abs(gz))


@pytest.mark.parametrize("scaled", [False, True])
def test_skc_lower_bound_metric_and_gradient(scaled, rq_oracle):
    """SKC_LOWER_BOUND (CHOLESKY_BASED) for SE + RQ at n = 150, 20 inducing inputs: its trace correction uses
    n d k(x, x) / d theta, right only if k(x, x) is the same for every x -- sg for an RQ leaf.  Tolerances of
    tests/test_gpu_approx_grad.py's lower-bound cases: value rel 1e-9, gradients 1e-5 of max |g_ref| (the
    1 / (2 jitter) = 5e7 factor amplifies the rounding of the trace terms)."""
    set_flags(scaled=scaled)
    tree, noise, m = ("ADD", [SE, RQ]), 0.05, 20
    hyp = [0.05, 1.2, 0.4, 2.0, 0.8] if scaled else [0.05, 0.4, 2.0]
    x, y = o.make_inputs("C1", n=150, seed=3)
    z = _inducing(m)
    met = get_metric_by_type(MetricType.LL, _approx_gp(tree, x, y), mht.MatrixApproximations.SKC_LOWER_BOUND,
                             mht.NumericalMatrixHandlingType.CHOLESKY_BASED, subset_size=m)
    h = [torch.tensor(v, dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(noise, dtype=F64, requires_grad=True)
    zt = torch.tensor(z, dtype=F64, requires_grad=True)
    out = met.get_metric(h, nz, zt)
    out.sum().backward()
    nl, gh, gn, gz = ad.nystroem_nlml_and_grad(tree, hyp, noise, x, y, z, "CHOLESKY_BASED", True,
                                               float(gp.p_cov_matrix_jitter), scaled)
    assert rel(float(out.detach()), nl) <= 1e-9
    got = np.concatenate([t.grad.numpy().reshape(-1) for t in h] + [[float(nz.grad)]])
    exp = np.concatenate([np.asarray(v).reshape(-1) for v in gh] + [[gn]])
    print("SKC lower bound scaled=%s: |g - g_ref| / max|g_ref| %s" % (scaled, np.abs(got - exp) / np.max(np.abs(exp))))
    assert np.max(np.abs(got - exp)) <= 1e-5 * np.max(np.abs(exp)), (got, exp)
    assert np.max(np.abs(zt.grad.numpy() - gz)) <= 1e-5 * np.max(np.abs(gz))


def test_ski_metric_and_gradient(rq_oracle):
    """SKI (STRICT_INVERSE), SE + RQ, n = 150, 40 inducing points (tests/test_gpu_approx_grad.py's SKI tolerances)."""
    tree, hyp, noise, m = ("ADD", [SE, RQ]), [0.05, 0.4, 2.0], 0.05, 40
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


def test_ragged_batch_mixes_rq_and_se_members(rq_oracle):
    sizes, d = [70, 130, 200], 3
    specs = [(RQ, [0.5, 2.0]), (SE, [0.6]), (("ADD", [SE, RQ]), [0.6, 0.4, 0.3])]
    dev = engine.device()
    members, segs = [], []
    for b, (n, (tree, hyp)) in enumerate(zip(sizes, specs)):
        x, y, _ = rq_inputs(n, d, 85 + b)
        kd = engine.kernel_descriptor(make_kernel(tree, d), d)
        members.append((kd, engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp), torch.tensor(x, device=dev),
                        torch.tensor(y, device=dev), None))
        segs.append((tree, hyp, x, y))
    f = engine.RaggedFactorization(sizes, d)
    f.run(members, T(NOISE))
    f.check_info()
    nl = f.nlml().cpu().numpy()
    for b, (tree, hyp, x, y) in enumerate(segs):
        assert rel(float(nl[b]), rq_oracle.nlml(tree, hyp, NOISE, x, y)) <= 1e-9
    assert rel(float(nl.sum()), rq_oracle.blockwise_nlml(segs, NOISE)) <= 1e-9


# ------------------------------------------------------------------------------ 10. rejection
def _rq_kdesc(d, n_hyp, flags=0, slot=-1, n_ard=0):
    kd = nat.GpkKdesc()
    kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 1, n_hyp, d, n_ard
    kd.nodes[0].op, kd.nodes[0].hyp_offset, kd.nodes[0].ard_slot, kd.nodes[0].flags = nat.OP_RQ, 0, slot, flags
    return kd


def test_invalid_rq_descriptors_are_rejected():
    """An RQ node with GPK_NODE_ARD (or the expanded / standard flags), with ard_slot 0, or with n_hyp one short is
    refused by gpk_kernel_matrix with the negative bad-argument code before anything is launched (K stays untouched),
    and gpk_grad_workspace_bytes sizes no workspace for it."""
    d, n = 3, 10
    dev = engine.device()
    X = torch.zeros((n, d), dtype=F64, device=dev)
    hyp = torch.tensor([0.5, 2.0, 0.7, 0.0], dtype=F64, device=dev)
    K = torch.full((n, n), 7.0, dtype=F64, device=dev)
    L = nat.lib()
    lay = nat.plan(nat.GPK_F64, 1, n, 0, d)

    def call(kd):
        return L.gpk_kernel_matrix(ctypes.byref(kd), nat.ptr(hyp), nat.GPK_F64, 0, nat.ptr(X), n, nat.ptr(X), n, d, 0.0,
                                   nat.ptr(K), n, nat.stream_handle(dev))

    bad = [_rq_kdesc(d, d + 1, nat.NODE_ARD, 0, 1), _rq_kdesc(d, 2, nat.NODE_SE_EXPANDED), _rq_kdesc(d, 2, nat.NODE_STANDARD),
           _rq_kdesc(d, 1), _rq_kdesc(d, 2, nat.NODE_SCALED), _rq_kdesc(d, 2, 0, 0)]
    for kd in bad:
        assert call(kd) == -1
        assert L.gpk_grad_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay)) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(K == 7.0))
    assert L.gpk_grad_workspace_bytes(ctypes.byref(_rq_kdesc(d, 2)), ctypes.byref(lay)) > 0
    assert call(_rq_kdesc(d, 2)) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(K == 1.0))                                    # x = 0 everywhere: u = 0, k = 1
    assert call(_rq_kdesc(d, 3, nat.NODE_SCALED)) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(K == 0.7))                                    # sg * 1
