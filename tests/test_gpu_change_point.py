"""ChangePointOperator as ONE device program (window leaves, GPK_OP_CPW) vs the references of tests/cp_support.py
(needs the MI355X).

Two references: ``cp_numpy`` (oracle.gp_oracle.change_point_matrix) and the operator's own ``get_tf_tensor`` (one
launch per child, masks by torch) for K; ``cp_torch`` + torch.linalg.cholesky + autograd on the CPU for -LML, its
gradient and the posterior.  Inputs come from ``cp_inputs``: points inside every SIGMOID transition zone, without
which the change-point gradient would be ~0 and its tests vacuous (tests/test_change_point_host.py checks that).

Tolerances (the project's own):
  kernel matrices   |dev - ref| <= 1e-13 + 1e-12 |ref| (tests/test_gpu_segmented.py's bar for this operator).  The
                    window is computed once per point with the reference's formula (~2 ulp of tanh / exp), so an
                    element's error is a few eps of w(x) w(y) |K_i|: ~1e-15 relative.  A LIN child cancels inside its
                    own dot product, so its term of the bound scales with w(x) w(y) |x - c||y - c| instead of |K_i|
                    (DESIGN 14); for positive children the two coincide.
  -LML              rel <= 1e-9 (cond(K + 1e-2 I) ~ 6e3 on these inputs: n eps cond ~ 3e-10 at worst)
  gradients         max |g - g_ref| <= 1e-7 max |g_ref| (tests/test_gpu_approx_grad.py's rule), over the whole vector
                    and again over the vector WITHOUT the change points, whose entries dominate the maximum
  posterior         mu / diag Sigma abs <= 1e-8 (the parity tests' bar)"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gp_oracle as o
from tests import cp_support as cs
from tests.helpers import hyp_list
from tests.lin_support import LIN, lin_abs_numpy, lin_oracle  # noqa: F401

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess

pytestmark = pytest.mark.gpu

F64 = torch.float64
SE, PER, MAT52, MAT32 = ("SE", {}), ("PER", {}), ("MAT52", {}), ("MAT32", {})
NOISE = 1e-2
TREES = {
    # name: tree, hyperparameter list [change points, children...], the change points' flat positions
    "CP3": (("CP", [SE, PER, MAT52]), [0.31, 0.62, 0.2, 0.9, 0.35, 0.3], [0, 1]),
    "CP2-LIN": (("CP", [LIN, SE]), [0.5, [0.3], 0.15], [0]),
    "SE+CP2": (("ADD", [SE, ("CP", [SE, MAT32])]), [0.6, 0.4, 0.1, 0.25], [1]),
}


@pytest.fixture(autouse=True)
def _restore_mode():
    old = gp.p_cp_operator_type
    yield
    gp.p_cp_operator_type = old


def T(v):
    return torch.tensor(v, dtype=F64)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def cps_of(name):
    _, hyp, at = TREES[name]
    return [float(np.asarray(hyp[i])) for i in at]


def k_bound(name, hyp, ref, x, x_, mode):
    """1e-13 + 1e-12 |ref|; for the tree with a LIN child, the LIN term of |ref| replaced by the magnitude its rounding
    scales with (w(x) w(y) sum_k |x_k - c_k||y_k - c_k|; |K_SE| for the other child)."""
    if name != "CP2-LIN":
        return 1e-13 + 1e-12 * np.abs(ref)
    a, a_ = o.cp_indicator(x, hyp[0], mode), o.cp_indicator(x_, hyp[0], mode)
    mag = np.outer(a, a_) * lin_abs_numpy([hyp[1]], x, x_) + \
        np.outer(1 - a, 1 - a_) * o.kernel_matrix(SE, [hyp[2]], x, x_)
    return 1e-13 + 1e-12 * mag


def build_gp(kernel, x, y, xs=None):
    if xs is None:
        di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    else:
        di = DataInput(x, y.reshape(-1, 1), xs, np.zeros(len(xs)).reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    g.set_data_input(di)
    return g


# ------------------------------------------------------------------------------ 1. K through the device program
def _check_k(name, hyp, x, xs, mode, tag):
    tree = TREES[name][0]
    cs.set_mode(mode)
    kernel = cs.make_kernel(tree, hyp)
    got = engine.kernel_matrix(kernel, hyp_list(hyp), x, xs).cpu().numpy()
    ref = cs.cp_numpy(tree, hyp, x, xs, mode)
    own = kernel.get_tf_tensor(hyp_list(hyp), x, xs).cpu().numpy()
    bound = k_bound(name, hyp, ref, x, xs, mode)
    e1, e2 = np.abs(got - ref), np.abs(got - own)
    print("%s %s %s: vs oracle max err / bound %.3e, vs get_tf_tensor %.3e" % (name, mode, tag, (e1 / bound).max(),
                                                                               (e2 / bound).max()))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.all(e1 <= bound), (name, mode, tag, float((e1 / bound).max()))
    assert np.all(e2 <= bound), (name, mode, tag, float((e2 / bound).max()))
    return got


@pytest.mark.parametrize("mode", cs.MODES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_kernel_matrix_matches_both_references(name, mode, lin_oracle):
    """engine.kernel_matrix at n = 200, m = 77 (unsorted; whole, edge and partial tiles) and at n = m = 130 (a ragged
    last tile), against change_point_matrix and against the operator's own get_tf_tensor."""
    hyp = TREES[name][1]
    x, _, xs = cs.cp_inputs(200, 3, cps_of(name), m=77)
    got = _check_k(name, hyp, x, xs, mode, "200x77")
    assert got.shape == (200, 77)
    x2, _, _ = cs.cp_inputs(130, 4, cps_of(name))
    got = _check_k(name, hyp, x2, x2, mode, "130x130")
    assert np.array_equal(got, got.T)                    # w(x) w(y) and the children commute: K bitwise symmetric


@pytest.mark.parametrize("mode", cs.MODES)
def test_kernel_matrix_degenerate_change_points(mode):
    """A change point outside the data (child 0 empty under the hard mask) and cp_1 < cp_0 (the middle child empty)."""
    x, _, xs = cs.cp_inputs(130, 5, [0.31, 0.62], m=77)
    _check_k("CP3", [-0.4, 0.62, 0.2, 0.9, 0.35, 0.3], x, xs, mode, "cp_0 below the data")
    _check_k("CP3", [0.62, 0.31, 0.2, 0.9, 0.35, 0.3], x, xs, mode, "cp_1 < cp_0")


def test_kernel_matrix_fp32_output():
    tree, hyp, _ = TREES["CP3"]
    cs.set_mode("SIGMOID")
    x, _, xs = cs.cp_inputs(130, 6, cps_of("CP3"), m=77)
    kernel = cs.make_kernel(tree, hyp)
    K = engine.kernel_matrix(kernel, hyp_list(hyp), x, xs)
    K32 = engine.kernel_matrix(kernel, hyp_list(hyp), x, xs, out_dtype=torch.float32)
    assert K32.dtype == torch.float32 and torch.equal(K32, K.to(torch.float32))


# ------------------------------------------------------------------------------ 2. same bits on every build path
def _augmented(kernel, hyp, x, y, noise):
    """(factorisation object holding the assembled, unfactored W; its n x n training block's lower triangle)"""
    n = x.shape[0]
    dev = engine.device()
    kd = engine.kernel_descriptor(kernel, 1)
    H = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp).reshape(1, -1).contiguous()
    X = torch.as_tensor(x, device=dev).contiguous()
    Y = torch.as_tensor(y, device=dev).reshape(1, -1).contiguous()
    NZ = torch.tensor([noise], dtype=F64, device=dev)
    f = engine.AugmentedFactorization(n, 1, 0, 1, F64)
    f.W.zero_()
    nat.check(nat.lib().gpk_assemble(ctypes.byref(kd), ctypes.byref(f.layout), nat.ptr(H), kd.n_hyp, nat.ptr(NZ), 0,
                                     nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W),
                                     nat.stream_handle(f.W.device)), "gpk_assemble")
    torch.cuda.synchronize()
    return f, torch.tril(f.w(0)[:n, :n])


@pytest.mark.parametrize("mode", cs.MODES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_augmented_build_is_bitwise_the_plain_build(name, mode, lin_oracle):
    """The n x n training block of the augmented build (interior tree loop on whole tiles, generic loop on the edge
    tiles, noise on the diagonal) equals gpk_kernel_matrix's plain build (lower triangle, diag_add = noise) bit for
    bit; padding rows are identity rows, the y row holds y -- never a window value."""
    tree, hyp, _ = TREES[name]
    cs.set_mode(mode)
    n, noise = 200, 0.1
    x, y, _ = cs.cp_inputs(n, 21, cps_of(name))
    kernel = cs.make_kernel(tree, hyp)
    f, aug = _augmented(kernel, hyp, x, y, noise)
    aug = aug.cpu().numpy()
    plain = torch.tril(engine.kernel_matrix(kernel, hyp_list(hyp), x, x, diag_add=noise, lower=True)).cpu().numpy()
    diff = int(np.count_nonzero(aug.view(np.uint64) != plain.view(np.uint64)))
    assert diff == 0, "%d of %d lower-triangle words differ" % (diff, aug.size)
    ref = cs.cp_numpy(tree, hyp, x, x, mode)
    bound = k_bound(name, hyp, ref, x, x, mode)
    assert np.all(np.abs(aug - np.tril(ref + noise * np.eye(n))) <= np.tril(bound) + 1e-15)
    lay = f.layout
    w = f.w(0).cpu().numpy()
    assert np.array_equal(np.tril(w[:lay.n_pad, :lay.n_pad])[n:], np.eye(lay.n_pad)[n:])
    assert np.array_equal(w[lay.y_row, :n], y) and np.all(w[lay.y_row, n:lay.n_pad] == 0.0)


# ------------------------------------------------------------------------------ 3. the tile-level child skip
@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("mode", ["INDICATOR", "SIGMOID"])
def test_child_skip_changes_no_value(mode, order):
    """gpk_tune cp_skip 1 against 0 at n = 300 (sorted x: most tiles lie inside one segment and skip the other two
    children; unsorted: hardly any does), plain and augmented builds: equal under == (a skipped term is +0.0 where
    the unskipped one is +-0.0)."""
    tree, hyp, _ = TREES["CP3"]
    cs.set_mode(mode)
    x, y, _ = cs.cp_inputs(300, 31, cps_of("CP3"))
    if order == "sorted":
        x = np.sort(x, axis=0)
    kernel = cs.make_kernel(tree, hyp)
    out = {}
    old = nat.tune("cp_skip", 1)
    try:
        for skip in (1, 0):
            nat.tune("cp_skip", skip)
            K = engine.kernel_matrix(kernel, hyp_list(hyp), x, x)
            _, aug = _augmented(kernel, hyp, x, y, 0.1)
            out[skip] = (K, aug.clone())
    finally:
        nat.tune("cp_skip", old)
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])
    ref = cs.cp_numpy(tree, hyp, x, x, mode)
    assert np.all(np.abs(out[1][0].cpu().numpy() - ref) <= 1e-13 + 1e-12 * np.abs(ref))
    if order == "sorted" and mode == "INDICATOR":       # (the premise: whole tiles of exact zeros exist to be skipped)
        assert np.all(ref[:64, 236:] == 0.0)


# ------------------------------------------------------------------------------ 4. -LML
def _nlml(kernel, hyp, x, y, chain=None):
    g = build_gp(kernel, x, y)
    m = get_metric_by_type(MetricType.LL, g)
    if chain is None:
        return float(m.get_metric_checked(hyp_list(hyp), T(NOISE))), m
    before = nat.chain_stats()["launches"]
    with nat.thread_tune(chain=2 if chain else 0):      # (as tests/test_gpu_chain.py selects the path)
        v = float(m.get_metric_checked(hyp_list(hyp), T(NOISE)))
    launched = nat.chain_stats()["launches"] - before
    assert (launched > 0) if chain else (launched == 0)
    return v, m


@pytest.mark.parametrize("mode", cs.MODES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_nlml_matches_restatement(name, mode, lin_oracle):
    """GaussianProcess + LogLikelihood.get_metric at n = 200 against cp_torch + torch.linalg.cholesky."""
    tree, hyp, _ = TREES[name]
    cs.set_mode(mode)
    x, y, _ = cs.cp_inputs(200, 41, cps_of(name))
    exp, _, _ = cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, mode)
    got, _ = _nlml(cs.make_kernel(tree, hyp), hyp, x, y)
    print("%s %s: device %.10f restatement %.10f rel %.3e" % (name, mode, got, exp, rel(got, exp)))
    assert rel(got, exp) <= 1e-9


def test_nlml_both_factorisation_paths_and_mode_switch():
    """The persistent launch and the launch-per-panel path give the same bits; switching p_cp_operator_type between
    two calls on the same objects changes the value accordingly (the mask form is read at emission, nothing caches
    a descriptor)."""
    tree, hyp, _ = TREES["CP3"]
    x, y, _ = cs.cp_inputs(200, 41, cps_of("CP3"))
    cs.set_mode("SIGMOID")
    kernel = cs.make_kernel(tree, hyp)
    chain, _ = _nlml(kernel, hyp, x, y, chain=True)
    launch, m = _nlml(kernel, hyp, x, y, chain=False)
    assert chain == launch
    exp = {mode: cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, mode)[0] for mode in cs.MODES}
    assert rel(launch, exp["SIGMOID"]) <= 1e-9
    assert rel(exp["SIGMOID"], exp["INDICATOR"]) > 1e-6          # (the modes are distinguishable on these inputs)
    for mode in ("INDICATOR", "APPROX_INDICATOR", "SIGMOID"):
        cs.set_mode(mode)
        got = float(m.get_metric_checked(hyp_list(hyp), T(NOISE)))
        assert rel(got, exp[mode]) <= 1e-9, mode


# ------------------------------------------------------------------------------ 5. gradient
def _check_gradient(got, exp, cp_at, what):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    err = np.abs(got - exp)
    print("%s: |g - g_ref| %s  g_ref %s" % (what, err, exp))
    assert np.max(err) <= 1e-7 * np.max(np.abs(exp)), (what, got, exp)
    rest = [i for i in range(len(exp)) if i not in cp_at]
    assert np.max(err[rest]) <= 1e-7 * np.max(np.abs(exp[rest])), (what + " (without the change points)", got, exp)


@pytest.mark.parametrize("mode", ["SIGMOID", "APPROX_INDICATOR"])
@pytest.mark.parametrize("name", ["CP3", "CP2-LIN"])
def test_lml_gradient_matches_autograd(name, mode, lin_oracle):
    """get_gradients, get_metric_and_gradient and get_metric(...).backward() at n = 200 against autograd of cp_torch.
    cp_0 of the three-window tree is the bound of two window leaves: its two partial sums must ADD."""
    tree, hyp, cp_at = TREES[name]
    cs.set_mode(mode)
    x, y, _ = cs.cp_inputs(200, 51, cps_of(name))
    nl_ref, g_ref, gn_ref = cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, mode)
    m = get_metric_by_type(MetricType.LL, build_gp(cs.make_kernel(tree, hyp), x, y))
    g1 = m.get_gradients(hyp_list(hyp), T(NOISE)).cpu().numpy()
    nl, grads, gn = m.get_metric_and_gradient(hyp_list(hyp), T(NOISE))
    assert rel(float(nl), nl_ref) <= 1e-9
    g2 = np.concatenate([g.cpu().numpy().reshape(-1) for g in grads])
    if name == "CP3" and mode == "SIGMOID":
        # the inner change point cp_0: upper bound of window 0 AND lower bound of window 1 (two writers of one slot)
        assert abs(g1[0] - g_ref[0]) <= 1e-7 * np.max(np.abs(g_ref)), \
            "d(-LML)/d cp_0 (two window leaves write it): %r vs %r" % (g1[0], g_ref[0])
    _check_gradient(g1, g_ref, cp_at, "%s %s get_gradients" % (name, mode))
    _check_gradient(list(g2) + [float(gn)], list(g_ref) + [gn_ref], cp_at, "%s %s get_metric_and_gradient" % (name, mode))
    h = [torch.tensor(np.asarray(v, dtype=np.float64), dtype=F64, requires_grad=True) for v in hyp]
    nz = torch.tensor(NOISE, dtype=F64, requires_grad=True)
    out = m.get_metric(h, nz)
    assert out.requires_grad
    out.sum().backward()
    g3 = np.concatenate([t.grad.numpy().reshape(-1) for t in h] + [[float(nz.grad)]])
    _check_gradient(g3, list(g_ref) + [gn_ref], cp_at, "%s %s backward" % (name, mode))
    if not (name == "CP3" and mode == "APPROX_INDICATOR"):      # (there the rising mask all but removes the inner child)
        assert np.min(np.abs(g_ref[cp_at])) > 1e-3 * np.max(np.abs(g_ref))


def test_lml_gradient_hard_mask_passes_none():
    """INDICATOR: tf.less passes no gradient, so the change points' components are exactly 0.0; the children's match."""
    tree, hyp, cp_at = TREES["CP3"]
    cs.set_mode("INDICATOR")
    x, y, _ = cs.cp_inputs(200, 51, cps_of("CP3"))
    _, g_ref, _ = cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, "INDICATOR")
    m = get_metric_by_type(MetricType.LL, build_gp(cs.make_kernel(tree, hyp), x, y))
    g = m.get_gradients(hyp_list(hyp), T(NOISE)).cpu().numpy()
    assert g[0] == 0.0 and g[1] == 0.0
    _check_gradient(g, g_ref, cp_at, "CP3 INDICATOR")


# ------------------------------------------------------------------------------ 6. posterior
def test_posterior_matches_restatement():
    tree, hyp, _ = TREES["CP3"]
    cs.set_mode("SIGMOID")
    x, y, xs = cs.cp_inputs(200, 61, cps_of("CP3"), m=40)
    mu_ref, var_ref = cs.cp_posterior(tree, hyp, NOISE, x, y, xs, "SIGMOID")
    g = build_gp(cs.make_kernel(tree, hyp), x, y, xs)
    mu = g.predict(hyp_list(hyp), noise=T(NOISE))[2].reshape(-1).cpu().numpy()
    var = g.aux.get_posterior_var_diag(hyp_list(hyp), T(NOISE)).reshape(-1).cpu().numpy()
    print("posterior: mu abs %.3e, var abs %.3e" % (np.abs(mu - mu_ref).max(), np.abs(var - var_ref).max()))
    np.testing.assert_allclose(mu, mu_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(var, var_ref, rtol=0, atol=1e-8)


# ------------------------------------------------------------------------------ 7. ragged batch
def test_ragged_batch_with_a_change_point_member():
    cs.set_mode("SIGMOID")
    sizes = [70, 130]
    specs = [(TREES["CP3"][0], TREES["CP3"][1]), (SE, [0.2])]
    dev = engine.device()
    members, exp = [], []
    for b, (n, (tree, hyp)) in enumerate(zip(sizes, specs)):
        x, y, _ = cs.cp_inputs(n, 70 + b, cps_of("CP3"))
        kd = engine.kernel_descriptor(cs.make_kernel(tree, hyp), 1)
        members.append((kd, engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp), torch.tensor(x, device=dev),
                        torch.tensor(y, device=dev), None))
        exp.append(cs.cp_nlml_and_grad(tree, hyp, NOISE, x, y, "SIGMOID")[0])
    f = engine.RaggedFactorization(sizes, 1)
    f.run(members, T(NOISE))
    f.check_info()
    nl = f.nlml().cpu().numpy()
    for b in range(2):
        assert rel(float(nl[b]), exp[b]) <= 1e-9, (b, nl[b], exp[b])


# ------------------------------------------------------------------------------ 8. reverse mode
def test_kernel_vjp_matches_autograd():
    """engine.kernel_vjp on K(X, Z), n = 150, m = 40, random weights: hyperparameter adjoints (the shared slot cp_0
    included) and the adjoint of Z, whose window term is what the Nystroem inducing-input gradient needs."""
    tree, hyp, cp_at = TREES["CP3"]
    cs.set_mode("SIGMOID")
    x, _, z = cs.cp_inputs(150, 81, cps_of("CP3"), m=40)
    G = np.random.default_rng(82).standard_normal((150, 40))
    params = cs.as_params(hyp)
    Zt = torch.tensor(z, requires_grad=True)
    K = cs.cp_torch(tree, params, torch.tensor(x), Zt, "SIGMOID")
    gref = torch.autograd.grad(torch.sum(torch.tensor(G) * K), params + [Zt])
    gh, gz = engine.kernel_vjp(cs.make_kernel(tree, hyp), hyp_list(hyp), x, z, G=torch.tensor(G, device=engine.device()),
                               want_z=True)
    exp_h = np.array([float(g) for g in gref[:-1]])
    _check_gradient(gh.cpu().numpy(), exp_h, cp_at, "kernel_vjp hyperparameters")
    exp_z = gref[-1].numpy()
    assert np.max(np.abs(exp_z)) > 1.0                             # (points inside a transition: the window term is live)
    assert np.max(np.abs(gz.cpu().numpy() - exp_z)) <= 1e-7 * np.max(np.abs(exp_z))


def test_trace_adjoint_of_a_change_point_tree(monkeypatch):
    """NystroemAdjoint.diag_adjoint: k(x, x) = sum_i w_i(x)^2 k_i(x, x) depends on x, so the tree is not stationary and
    the adjoint of trace(K) sums over all training points (three chunks) -- against autograd of trace(K)."""
    from gaussianprocessfundamentals_amd.Metrics._approx_grad import NystroemAdjoint
    tree, hyp, cp_at = TREES["CP3"]
    cs.set_mode("SIGMOID")
    x, _, _ = cs.cp_inputs(150, 91, cps_of("CP3"))
    params = cs.as_params(hyp)
    K = cs.cp_torch(tree, params, torch.tensor(x), torch.tensor(x), "SIGMOID")
    gref = torch.autograd.grad(torch.trace(K), params, allow_unused=True)
    exp = np.array([0.0 if g is None else float(g) for g in gref])
    monkeypatch.setattr(NystroemAdjoint, "DIAG_CHUNK", 64)
    adj = NystroemAdjoint(cs.make_kernel(tree, hyp), hyp_list(hyp), torch.as_tensor(x, device=engine.device()), None, 0.1)
    assert not adj.stationary
    got = adj.diag_adjoint().cpu().numpy()
    print("trace adjoint: got %s exp %s" % (got, exp))
    assert np.max(np.abs(exp[cp_at])) > 1.0
    assert np.max(np.abs(got - exp)) <= 1e-7 * np.max(np.abs(exp))
