"""The predictor's joint posterior covariance and draws on the HIP path (gpk_predict_vt, gpk_predict_cov; needs the
MI355X): V' = k(Xs, X) L^-T and Sigma = K_ss - V' V'^T at new points from ONE kept identity-augmented factorisation,
against the host restatement (tests/predict_cov_support: K from the oracle's kernels, scipy Cholesky and triangular
solves, never the device's K, L or R), known answers, and the properties the entries promise: bit symmetry, the same
bits for any chunk, block or order of the points, both factorisation paths, every member of a batch.

Bar: |got - ref| <= 1e-8 max(1, max|ref|).  The measured maxima are printed (COVERR lines)."""
import ctypes

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Statistics.Predictor import PosteriorPredictor
from tests import cp_support as cs
from tests import predict_cov_support as pcs
from tests import predict_support as ps
from tests import rq_support as rs
from tests.helpers import hyp_list, set_flags

pytestmark = pytest.mark.gpu

NOISE = ps.NOISE
SIZES_N = [1, 127, 128, 129, 333]
SIZES_M = [1, 63, 64, 65, 200]
EPS = pcs.EPS
# Trees whose plain K build gives an element other bits when its point sits in another 64-block of points.  Measured:
# for ADD(SE,PER) gpk_kernel_matrix(cat(Xb, Xa), X)[mb:] and gpk_kernel_matrix(Xa, X) differ in 62 of 65 x 129 elements by
# <= 1.3e-15 (the two-leaf SE + periodic build chooses its sin / cos form per 64-point block); the other seven trees
# give the same bits.  test_blocks_of_points_do_not_change_a_bit holds such a tree to the bar and checks that it is
# the K build that moves.
POSITION_DEPENDENT_K = ("ADD(SE,PER)",)


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


def _factor(name, x, y, noise=NOISE, hyps=None, nan_fill=False, gradient=False):
    """engine.InverseFactorization run on the case (hyps: one list per batch member)"""
    tree, hyp, d = _activate(name)
    kd = engine.kernel_descriptor(_kernel(name), d)
    rows = [hyp] if hyps is None else hyps
    H = torch.stack([engine.pack_hyper_parameter(hyp_list(h), kd.n_hyp) for h in rows]).contiguous()
    n = len(x)
    f = engine.InverseFactorization(n, d, len(rows), torch.float64)
    if nan_fill:   # nothing the factorisation skips or leaves unwritten may reach the covariance
        f._W.fill_(float("nan"))
        f._Winv.fill_(float("nan"))
    nz = torch.tensor([noise], dtype=torch.float64, device=engine.device())
    f.run(kd, H.reshape(-1), kd.n_hyp if len(rows) > 1 else 0, nz, 0, _dev(x), 0, _dev(y).reshape(1, -1), 0,
          gradient=gradient)
    return f


def _predictor(name, n):
    tree, hyp, d = _activate(name)
    x, y, _ = pcs.train_factor(name, n)
    di = DataInput(x, y.reshape(-1, 1), x[:1], np.zeros((1, 1)))
    di.set_mean_function(ZeroMeanFunction(d))
    return PosteriorPredictor(_kernel(name), hyp_list(hyp), NOISE, ZeroMeanFunction(d), None, di)


def _close(tag, got, ref):
    g = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert g.shape == np.shape(ref), (tag, g.shape, np.shape(ref))
    err = float(np.max(np.abs(g - ref)))
    print("COVERR %s max|got - ref| = %.3e (bar %.1e)" % (tag, err, ps.bar(ref)))
    assert np.all(np.isfinite(g))
    assert err <= ps.bar(ref)


# ------------------------------------------------------------------------- 1 - 4. against the host reference
@pytest.mark.parametrize("n", SIZES_N)
@pytest.mark.parametrize("name", list(ps.CASES))
def test_vt_and_covariance_match_the_host_reference(name, n):
    x, y, _ = pcs.train_factor(name, n)
    f = _factor(name, x, y)     # factored once for the five point sets
    assert int(f.info[0]) == 0
    for m in SIZES_M:
        _, _, xs, V_ref, S_ref, mu_ref, var_ref = pcs.case_reference(name, n, m)
        X = _dev(xs)
        V = f.predict_vt(X)
        assert tuple(V.shape) == (m, n) and V.stride(0) == f.layout.n_pad
        _close("%s n=%d m=%d V'" % (name, n, m), V, V_ref)
        S = f.predict_cov(X)
        assert tuple(S.shape) == (m, m)
        _close("%s n=%d m=%d Sigma" % (name, n, m), S, S_ref)
        assert torch.equal(S, S.T)                                   # symmetric bit for bit
        # the diagonal and the streamed variance: each inside the bar of the same reference
        _close("%s n=%d m=%d diag Sigma" % (name, n, m), torch.diagonal(S), var_ref)
        _close("%s n=%d m=%d predict var" % (name, n, m), f.predict(X)[1], var_ref)


@pytest.mark.parametrize("name", ["SE", "LIN", "CP(SE,SE)", "SE_ARD@3"])
def test_covariance_between_two_sets_of_points(name):
    n = 129
    x, y, _ = pcs.train_factor(name, n)
    xa, xb = ps.case_reference(name, n, 65)[2], ps.case_reference(name, n, 200)[2]
    f = _factor(name, x, y)
    C = f.predict_cov(_dev(xa), _dev(xb))
    assert tuple(C.shape) == (65, 200)
    _close("%s cross 65 x 200" % name, C, pcs.cov_ref(name, n, xa, xb))
    _close("%s cross 200 x 65" % name, f.predict_cov(_dev(xb), _dev(xa)), pcs.cov_ref(name, n, xb, xa))


# --------------------------------------------------------------------------------------- 5. known answers
@pytest.mark.parametrize("name", ["SE", "MAT52_scaled", "LIN", "CP(SE,SE)"])
@pytest.mark.parametrize("n", [129, 333])
def test_at_the_training_points_sigma_is_noise_times_i_minus_noise_k_inv(name, n):
    """Sigma(X, X) = K - K (K + s I)^-1 K = s (I - s (K + s I)^-1), with k_inv() of the same factorisation."""
    x, y, _ = pcs.train_factor(name, n)
    f = _factor(name, x, y)
    S = f.predict_cov(_dev(x))
    eye = torch.eye(n, dtype=torch.float64, device=S.device)
    want = (NOISE * (eye - NOISE * f.k_inv(0))).cpu().numpy()
    _close("%s n=%d Sigma at the training points" % (name, n), S, want)
    _close("%s n=%d the same against the host" % (name, n), S, pcs.cov_ref(name, n, x))


def test_far_from_the_data_sigma_is_the_prior_bitwise():
    """SE, the new points 1e3 away: every k(x*, x) underflows to 0, V' is 0 and k - 0 = k exactly -- the lower
    triangle is the K build's, bit for bit (the upper one is its mirror)."""
    name, n, m = "SE", 129, 200
    tree, hyp, d = _activate(name)
    x, y, xs = pcs.case_reference(name, n, m)[:3]
    f = _factor(name, x, y)
    X = _dev(xs + 1e3)
    assert not bool(f.predict_vt(X).any())
    S = f.predict_cov(X)
    Kss = engine.kernel_matrix(_kernel(name), hyp_list(hyp), X, X)
    assert torch.equal(torch.tril(S), torch.tril(Kss))
    assert torch.equal(S, S.T)


# ------------------------------------------------------------------------- 6. blocks and chunks, bit for bit
@pytest.mark.parametrize("name", ["SE", "CP(SE,SE)", "SE_ARD@3"])
def test_chunks_and_order_do_not_change_a_bit_of_vt(name):
    n, m = 333, 200
    x, y, xs = pcs.case_reference(name, n, m)[:3]
    f = _factor(name, x, y)
    X = _dev(xs)
    V1 = f.predict_vt(X).clone()                      # one chunk
    assert torch.equal(f.predict_vt(X, max_rows=64), V1)     # 64 + 64 + 64 + 8
    assert torch.equal(f.predict_vt(X, max_rows=128), V1)    # 128 + 72
    assert torch.equal(f.predict_vt(X), V1)
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(5)).to(X.device)
    assert torch.equal(f.predict_vt(X[perm].contiguous(), max_rows=64), V1[perm])


@pytest.mark.parametrize("name", list(ps.CASES))
def test_blocks_of_points_do_not_change_a_bit(name):
    """ma = 65, mb = 130: the rectangular block of the symmetric run is the two-set run, its leading principal block
    the symmetric run of the first set alone.  A tree in POSITION_DEPENDENT_K is held to the bar instead -- and must
    show that it is the K build that moves."""
    n, ma, mb = 129, 65, 130
    tree, hyp, d = _activate(name)
    x, y, _ = pcs.train_factor(name, n)
    xa = ps.case_reference(name, n, ma)[2]
    xb = ps.case_reference(name, n, 200)[2][:mb]
    f = _factor(name, x, y)
    Xa, Xb = _dev(xa), _dev(xb)
    Xc = torch.cat([Xb, Xa]).contiguous()
    full, cross, lead = f.predict_cov(Xc), f.predict_cov(Xa, Xb), f.predict_cov(Xb)
    if name in POSITION_DEPENDENT_K:
        k, X = _kernel(name), _dev(x)
        assert not torch.equal(engine.kernel_matrix(k, hyp_list(hyp), Xc, X)[mb:],
                               engine.kernel_matrix(k, hyp_list(hyp), Xa, X))
        _close("%s block vs two sets" % name, full[mb:, :mb], cross.cpu().numpy())
        _close("%s leading block" % name, full[:mb, :mb], lead.cpu().numpy())
    else:
        assert torch.equal(full[mb:, :mb], cross)
        assert torch.equal(full[:mb, :mb], lead)
    _close("%s 195 points" % name, full, pcs.cov_ref(name, n, np.concatenate([xb, xa])))


# --------------------------------------------------------------------------- 7. both factorisation paths
@pytest.mark.parametrize("n", [129, 333])
def test_both_factorisation_paths_and_nothing_unwritten_is_read(n):
    name, m = "ADD(SE,PER)", 200
    x, y, xs, V_ref, S_ref, _, _ = pcs.case_reference(name, n, m)
    out = {}
    for path, mode in (("launch", 0), ("chain", 2)):
        with nat.thread_tune(chain=mode):
            f = _factor(name, x, y, nan_fill=True)
            assert int(f.info[0]) == 0
            V = f.predict_vt(_dev(xs), max_rows=64).clone()
            S = f.predict_cov(_dev(xs))
        _close("%s n=%d %s path, NaN-filled W: V'" % (name, n, path), V, V_ref)
        _close("%s n=%d %s path, NaN-filled W: Sigma" % (name, n, path), S, S_ref)
        out[path] = (V, S)
    assert torch.equal(out["launch"][0], out["chain"][0])
    assert torch.equal(out["launch"][1], out["chain"][1])


# ------------------------------------------------------------------------------------------ 8. member index
def test_members_of_a_batch_equal_single_factorisations_bitwise():
    name, n, m = "MAT52_scaled", 129, 65
    x, y, xs = pcs.case_reference(name, n, m)[:3]
    hyps = [[1.1, 1.6], [0.7, 0.9], [1.3, 2.2]]
    fb = _factor(name, x, y, hyps=hyps)
    assert not bool(fb.info.any())
    X = _dev(xs)
    seen = []
    for b, h in enumerate(hyps):
        fs_ = _factor(name, x, y, hyps=[h])
        assert torch.equal(fb.predict_vt(X, member=b), fs_.predict_vt(X))
        S = fb.predict_cov(X, member=b)
        assert torch.equal(S, fs_.predict_cov(X))
        seen.append(S)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0], seen[2])   # (the members do differ)
    _close("member 0", seen[0], pcs.case_reference(name, n, m)[4])                   # (member 0 has the case's hyp)
    with pytest.raises(ValueError, match="member 3 of a batch of 3"):
        fb.predict_cov(X, member=3)


# --------------------------------------------------------------------------------------- 9. nothing disturbed
def test_the_run_is_not_disturbed():
    name, n, m = "SE", 129, 65
    x, y, xs = pcs.case_reference(name, n, m)[:3]
    f = _factor(name, x, y, gradient=True)
    X = _dev(xs)
    val, grad, _ = f.results("nlml")
    val0, grad0, W0 = val.clone(), grad.clone(), f.W.clone()
    mu0, var0 = (t.clone() for t in f.predict(X))
    f.predict_vt(X, max_rows=64)
    f.predict_cov(X)
    f.predict_cov(X, _dev(x))
    val1, grad1, _ = f.results("nlml")
    assert torch.equal(val1, val0) and torch.equal(grad1, grad0)
    assert torch.equal(f.W.view(torch.int64), W0.view(torch.int64))     # W is only read (compared as bits)
    mu1, var1 = f.predict(X)
    assert torch.equal(mu1, mu0) and torch.equal(var1, var0)


# ------------------------------------------------------------------------------------------------ 10. draws
def test_covariance_api_and_noise():
    name, n, m = "SE", 129, 65
    _, _, xs, _, S_ref, _, _ = pcs.case_reference(name, n, m)
    p = _predictor(name, n)
    S = p.covariance(xs)
    _close("covariance()", S, S_ref)
    noisy = p.covariance(xs, include_noise=True)
    assert torch.equal(torch.tril(noisy, -1), torch.tril(S, -1)) and torch.equal(torch.triu(noisy, 1), torch.triu(S, 1))
    assert torch.equal(torch.diagonal(noisy), torch.diagonal(S) + NOISE)
    xo = ps.case_reference(name, n, 63)[2]
    _close("covariance(x, x_other)", p.covariance(xs, xo), pcs.cov_ref(name, n, xs, xo))
    with pytest.raises(ValueError, match="x_new must be"):
        p.covariance(np.zeros((3, 2)))


@pytest.mark.parametrize("name", list(ps.CASES))
def test_a_draw_is_its_parts(name):
    """Latent draws: Sigma + 1e-8 I has eigenvalues at the jitter for most trees, so a host Cholesky is no reference
    (1e-13 in Sigma moves a draw by up to 9e-6).  The draw is held as a composition: the factor reproduces the device's
    own Sigma + jitter I inside DESIGN 2's factor bar 8 m eps max|A|, and with z given the result is total + L z
    inside the dot-product bound 2 m eps (|L| |z|) plus the rounding of the two final sums (eps |ref| each side: a
    result of size |total| cannot be closer to anything than that)."""
    n, m, cols = 129, 65, 8
    xs = pcs.case_reference(name, n, m)[2]
    p = _predictor(name, n)
    jitter = float(torch.as_tensor(gp.p_cov_matrix_jitter))
    total, L = p.draw_factor(xs)
    assert torch.equal(total, p.predict(xs)[0])
    assert tuple(L.shape) == (m, m) and not bool(torch.triu(L, 1).any())
    A = p.covariance(xs).cpu().numpy() + jitter * np.eye(m)
    Ll = L.cpu().numpy().astype(np.longdouble)
    err = float(np.max(np.abs((Ll @ Ll.T).astype(np.float64) - A)))
    print("COVERR %s |L L^T - A| = %.3e (bar %.3e)" % (name, err, 8 * m * EPS * np.max(np.abs(A))))
    assert err <= 8 * m * EPS * float(np.max(np.abs(A)))
    z = np.random.default_rng(17).standard_normal((m, cols))
    got = p.sample(xs, cols, z=z)
    assert tuple(got.shape) == (m, cols)
    Lc, tc = L.cpu(), total.cpu()
    ref = tc.reshape(-1, 1) + Lc @ torch.as_tensor(z)
    bound = 2 * m * EPS * (Lc.abs() @ torch.as_tensor(z).abs()) + 2 * EPS * ref.abs()
    excess = float(((got.cpu() - ref).abs() - bound).max())
    print("COVERR %s draw vs total + L z: max excess over the bound %.3e" % (name, excess))
    assert excess <= 0.0


@pytest.mark.parametrize("n,m", [(127, 63), (129, 65), (333, 200)])
@pytest.mark.parametrize("name", list(ps.CASES))
def test_noisy_draws_match_the_host_draws(name, n, m):
    """With the noise on the diagonal the matrix has condition <= 172 on these inputs: a host Cholesky is a reference."""
    xs = pcs.case_reference(name, n, m)[2]
    z = np.random.default_rng(23 + n).standard_normal((m, 8))
    jitter = float(torch.as_tensor(gp.p_cov_matrix_jitter))
    got = _predictor(name, n).sample(xs, 8, include_noise=True, z=z)
    _close("%s n=%d m=%d noisy draws" % (name, n, m), got, pcs.draws_ref(name, n, m, z, NOISE + jitter))


@pytest.mark.parametrize("n,m", [(127, 63), (129, 65), (333, 200)])
def test_latent_draws_of_a_well_conditioned_posterior_match_the_host_draws(n, m):
    """SE-ARD at d = 3: the smallest eigenvalue of Sigma is 5e-3, so the latent draws have a host reference too."""
    name = "SE_ARD@3"
    xs = pcs.case_reference(name, n, m)[2]
    z = np.random.default_rng(29 + n).standard_normal((m, 8))
    jitter = float(torch.as_tensor(gp.p_cov_matrix_jitter))
    got = _predictor(name, n).sample(xs, 8, z=z)
    _close("%s n=%d m=%d latent draws" % (name, n, m), got, pcs.draws_ref(name, n, m, z, jitter))


def test_the_same_seed_gives_the_same_draw():
    name, n, m = "RQ", 129, 65
    xs = pcs.case_reference(name, n, m)[2]
    p = _predictor(name, n)
    gen = torch.Generator(device=engine.device())
    a = p.sample(xs, 4, generator=gen.manual_seed(7))
    b = p.sample(xs, 4, generator=gen.manual_seed(7))
    c = p.sample(xs, 4, generator=gen.manual_seed(8))
    assert tuple(a.shape) == (m, 4) and torch.equal(a, b) and not torch.equal(a, c)
    assert bool(torch.isfinite(a).all())


# ------------------------------------------------------------------------------------- 11. the C ABI directly
def test_c_abi_refuses_a_short_workspace_and_runs_with_exactly_one_tile():
    name, n, m = "SE", 129, 200
    x, y, xs, V_ref, S_ref, _, _ = pcs.case_reference(name, n, m)
    f = _factor(name, x, y)
    L, lay, kd = f.L, f.layout, f.kd
    hyp = f._loo_operands[1]
    X, Xs = _dev(x), _dev(xs)
    dev = engine.device()
    Vt = torch.full((m, n + 3), -7.0, dtype=torch.float64, device=dev)      # ldv = n + 3: the tail stays untouched
    need = int(L.gpk_predict_vt_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay), 64))
    work = torch.empty(need // 8, dtype=torch.float64, device=dev)
    s = nat.stream_handle(dev)
    args = (ctypes.byref(kd), ctypes.byref(lay), nat.ptr(hyp), nat.ptr(X), nat.ptr(f.W), 0, nat.ptr(Xs), m)
    assert L.gpk_predict_vt(*args, nat.ptr(Vt), n + 3, nat.ptr(work), need - 8, s) == -11
    nat.check(L.gpk_predict_vt(*args, nat.ptr(Vt), n + 3, nat.ptr(work), need, s), "gpk_predict_vt")
    assert bool((Vt[:, n:] == -7.0).all())
    _close("one tile of workspace", Vt[:, :n], V_ref)
    assert torch.equal(Vt[:, :n], f.predict_vt(Xs))
    # gpk_predict_cov on these rows, C with a wider row stride too
    C = torch.full((m, m + 5), -7.0, dtype=torch.float64, device=dev)
    nat.check(L.gpk_predict_cov(ctypes.byref(kd), 1, nat.ptr(hyp), nat.ptr(Xs), m, nat.ptr(Vt), n + 3, nat.ptr(Xs), m,
                                nat.ptr(Vt), n + 3, n, nat.ptr(C), m + 5, 1, s), "gpk_predict_cov")
    assert bool((C[:, m:] == -7.0).all())
    assert torch.equal(C[:, :m], f.predict_cov(Xs))
    _close("C ABI Sigma", C[:, :m], S_ref)
