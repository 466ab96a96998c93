"""The ragged -LML gradient on the HIP path (needs the MI355X): engine.RaggedInverseFactorization (gpk_assemble_inverse_ragged,
gpk_potrf_aug_ragged_ex, gpk_grad_ragged), BlockwiseLogLikelihood's gradient, sweep.native_kfold_value_and_gradient and
Optimizer.Fitter.DeviceKfoldLbfgsFitter.

Oracle: oracle/gp_autodiff.nlml_and_grad on each member alone; a segmented model's gradient is the per-segment results
put together.  Bars, imported or restated from the tests that own them: -LML rel < 1e-9
(tests/test_gpu_segmented.test_ragged_nlml_factor_alpha_match_oracle); gradient tests/test_gpu_grad._check_grad at its
own tol, 1e-7 max(1, |g_ref|_max); K^-1 normwise relative < 1e-8 and alpha rtol = 1e-7, atol = 1e-7 |alpha|_max
(tests/test_gpu_grad.test_gradient_at_multi_group_sizes_and_inverse)."""
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import engine, sweep
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import PartitioningModel as pm
from gaussianprocessfundamentals_amd.KernelBasics.PartitionOperator import PartitionOperator
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import PartitionedGaussianProcess
from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests import cp_support as cps
from tests import fit_support as fs
from tests import kfold_support as ks
from tests.helpers import hyp_list, make_kernel, set_flags
from tests.test_gpu_fitter import E2E_FTOL, E2E_MEASURED_GAP, E2E_NOISE, E2E_NOISE_FLOOR, projected_gradient_norm
from tests.test_gpu_grad import _check_grad
from tests.test_gpu_segmented import CHILD_HYPS, CHILD_TREES, NOISE, T, blockwise_setup, rel
from tests.test_grad_oracle import GRAD_CASES, _inputs
from tests.test_segmented_host import Interval

pytestmark = pytest.mark.gpu

NZ = 0.05
SE, MAT52, PER = ("SE", {}), ("MAT52", {}), ("PER", {})
SE_PER = ("ADD", [SE, PER])


@pytest.fixture(autouse=True)
def _default_flags():
    yield
    set_flags()
    cps.set_mode("INDICATOR")


def member(tree, hyp, n, d, seed, x=None, y=None):
    """(engine member, (tree, hyp, x, y)) with the data of tests/test_grad_oracle._inputs."""
    if x is None:
        x, y = _inputs(n, d, seed)
    kd = engine.kernel_descriptor(make_kernel(tree, d), d)
    h = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp)
    dev = engine.device()
    return (kd, h, torch.tensor(x, device=dev), torch.tensor(y, device=dev)), (tree, hyp, x, y)


def run(members, sizes, d, noise=NZ, gradient=True):
    f = engine.RaggedInverseFactorization(sizes, d)
    f.run(members, noise if isinstance(noise, torch.Tensor) else T(noise), gradient=gradient)
    return f


def check_member(f, b, data, noise=NZ, scaled=False, expanded=False, inverse=True):
    tree, hyp, x, y = data
    nl_ref, g_ref, gn_ref = ad.nlml_and_grad(tree, hyp, noise, x, y, scaled, expanded)
    nl = float(f.nlml()[b])
    assert rel(nl, nl_ref) < 1e-9, (b, nl, nl_ref)
    g = f.gradient(b).cpu().numpy()
    flat_ref = np.concatenate([np.asarray(e, dtype=np.float64).reshape(-1) for e in g_ref])
    assert g.shape == (flat_ref.size + 1,)
    _check_grad([g[:-1], g[-1]], [flat_ref, gn_ref])
    if inverse:
        Kn = o.k_noised(tree, hyp, noise, x, scaled, expanded)
        Ki = np.linalg.inv(Kn)
        got = f.k_inv(b).cpu().numpy()
        assert got.shape == Ki.shape
        assert np.linalg.norm(got - Ki) / np.linalg.norm(Ki) < 1e-8
        Li = np.linalg.inv(np.linalg.cholesky(Kn))
        assert np.linalg.norm(f.l_inv(b).cpu().numpy() - Li) / np.linalg.norm(Li) < 1e-8
        a = np.linalg.solve(Kn, y)
        got_a = f.alpha(b).cpu().numpy()
        assert got_a.shape == a.shape
        np.testing.assert_allclose(got_a, a, rtol=1e-7, atol=1e-7 * np.abs(a).max())


# ------------------------------------------------------------------------------------------ 1. per-member parity
# 300: the largest member; 37: smaller than one 64-tile; 128: ends on a panel boundary below the maximum (whole panels
# of padding); 257: just past a tile edge.  d = 3: 200 / 64 (one tile exactly) / 129.
SIZES_1D, SIZES_3D = [300, 37, 128, 257], [200, 64, 129]
PARITY = [(0, SIZES_1D), (1, SIZES_1D), (3, SIZES_1D), (8, SIZES_1D), (11, SIZES_1D), (12, SIZES_1D), (13, SIZES_1D),
          (7, SIZES_3D)]   # GRAD_CASES: single leaves (SE, scaled SE, PER), ARD (d = 1, d = 3), ADD, MUL, MUL of ADD


@pytest.mark.parametrize("case,sizes", PARITY)
def test_every_member_matches_its_own_oracle(case, sizes):
    tree, hyp, d, scaled, expanded = GRAD_CASES[case]
    assert d == (3 if sizes is SIZES_3D else 1)
    set_flags(scaled=scaled, expanded=expanded)
    built = [member(tree, hyp, n, d, 300 + 10 * case + b) for b, n in enumerate(sizes)]
    f = run([m for m, _ in built], sizes, d)
    f.check_info()
    assert np.array_equal(f.out.view(-1, 4)[:, 3].cpu().numpy(), np.array(sizes, dtype=np.float64))
    for b, (_, data) in enumerate(built):
        check_member(f, b, data, scaled=scaled, expanded=expanded)


# ------------------------------------------------------------------------------------- 2. heterogeneous programs
HETERO = [(SE, [0.3]), (MAT52, [0.4]), (SE_PER, [0.3, 0.9, 0.5]), (SE, [0.2])]


def test_members_with_different_programs():
    """SE, MAT52, SE + PER and SE again: four runs of one member (no two neighbours share a program), then
    [SE, SE, MAT52, MAT52]: two runs of two members (a batch-2 layout with offset pointers)."""
    sizes = [257, 37, 300, 128]
    built = [member(t, h, n, 1, 500 + b) for b, ((t, h), n) in enumerate(zip(HETERO, sizes))]
    f = run([m for m, _ in built], sizes, 1)
    f.check_info()
    assert len(engine.program_runs(f.kd)) == 4
    for b, (_, data) in enumerate(built):
        check_member(f, b, data)
    order = [(SE, [0.3]), (SE, [0.2]), (MAT52, [0.4]), (MAT52, [0.25])]
    built = [member(t, h, n, 1, 520 + b) for b, ((t, h), n) in enumerate(zip(order, sizes))]
    f = run([m for m, _ in built], sizes, 1)
    assert engine.program_runs(f.kd) == [(0, 2), (2, 4)]
    for b, (_, data) in enumerate(built):
        check_member(f, b, data, inverse=False)


# ---------------------------------------------------------------------------------------------- 3. independence
def test_a_member_does_not_depend_on_its_batch():
    """Member 1 of [300, 37, 128] and the same member in [37, 257]: bitwise equal -LML and gradient (the tile index
    of a partial sum does not depend on the layout's n, and zeros are added to the reduction).  Against
    InverseFactorization on the member alone: the -LML and gradient bars, and -- measured bitwise equal on the MI355X
    at this size, one panel on either path -- the bitwise comparison too."""
    tree, hyp = SE_PER, [0.3, 0.9, 0.5]
    a = [member(tree, hyp, n, 1, 600 + b) for b, n in enumerate([300, 37, 128])]
    m37, d37 = a[1]
    other, _ = member(tree, hyp, 257, 1, 650)
    fa = run([m for m, _ in a], [300, 37, 128], 1)
    fb = run([m37, other], [37, 257], 1)
    assert torch.equal(fa.nlml()[1], fb.nlml()[0])
    assert torch.equal(fa.gradient(1), fb.gradient(0))
    assert torch.equal(fa.k_inv(1), fb.k_inv(0))
    kd, h, X, Y = m37
    single = engine.InverseFactorization(37, 1, 1)
    dev = engine.device()
    single.run(kd, h, kd.n_hyp, T(NZ).reshape(1).to(dev), 0, X.contiguous(), 0, Y.reshape(1, -1).contiguous(), 0)
    gs = single.gradient()[0].cpu().numpy()
    g = fa.gradient(1).cpu().numpy()
    print("ragged vs single: max |dg| = %.3e, d(-LML) = %.3e"
          % (np.abs(g - gs).max(), abs(float(fa.nlml()[1]) - float(single.nlml()[0]))))
    assert rel(float(fa.nlml()[1]), float(single.nlml()[0])) < 1e-9
    _check_grad([g], [gs])
    # measured on the MI355X: both differences are exactly 0 (n = 37 is one panel on either path), so the bitwise
    # form is asserted as well
    assert torch.equal(fa.nlml()[1], single.nlml()[0]) and torch.equal(fa.gradient(1), single.gradient()[0])


def test_f32_layout_runs_the_same_template():
    """The uniform gradient path accepts an f32 layout, so the ragged one does (grad_kernel<float, ., true>).  Checked
    here: it runs, every member factors (info 0) with finite results, and a member is bitwise the same in two different
    batches.  (No accuracy bar: the f32 gradient has none elsewhere in the suite to take over.)"""
    tree, hyp = SE_PER, [0.3, 0.9, 0.5]
    a = [member(tree, hyp, n, 1, 600 + b) for b, n in enumerate([300, 37, 128])]
    other, _ = member(tree, hyp, 257, 1, 650)
    fa = engine.RaggedInverseFactorization([300, 37, 128], 1, torch.float32).run([m for m, _ in a], T(NZ))
    fb = engine.RaggedInverseFactorization([37, 257], 1, torch.float32).run([a[1][0], other], T(NZ))
    fa.check_info()
    fb.check_info()
    assert fa.W.dtype == torch.float32
    for b in range(3):
        assert bool(torch.isfinite(fa.gradient(b)).all()) and math.isfinite(float(fa.nlml()[b]))
    assert torch.equal(fa.nlml()[1], fb.nlml()[0]) and torch.equal(fa.gradient(1), fb.gradient(0))


# --------------------------------------------------------------------------------------------------- 4. failure
def test_a_singular_member_fails_alone():
    sizes = [128, 70, 257]
    built = [member(SE, [0.3], n, 1, 700 + b) for b, n in enumerate(sizes)]
    good = run([m for m, _ in built], sizes, 1, noise=torch.tensor([NZ, NZ, NZ], dtype=torch.float64))
    good.check_info()
    bad_members = [m for m, _ in built]
    kd, h, X, Y = bad_members[1]
    bad_members[1] = (kd, h, torch.zeros_like(X), Y)     # duplicated points, noise 0: singular
    bad = run(bad_members, sizes, 1, noise=torch.tensor([NZ, 0.0, NZ], dtype=torch.float64))
    info = bad.info.cpu().numpy()
    assert info[0] == 0 and info[1] != 0 and info[2] == 0
    assert math.isinf(float(bad.nlml()[1])) and float(bad.nlml()[1]) > 0
    assert bool(torch.isnan(bad.gradient(1)).all())
    with pytest.raises(engine.CholeskyError):
        bad.check_info()
    for b in (0, 2):
        assert torch.equal(bad.nlml()[b], good.nlml()[b])
        assert torch.equal(bad.gradient(b), good.gradient(b))
        assert torch.equal(bad.k_inv(b), good.k_inv(b))


# ---------------------------------------------------------------------------------------- 5. workspace sentinel
def _nan_workspace(f, n_hyp_max):
    nt = (f.n + 63) // 64
    f.work = torch.full((f.batch * (nt * (nt + 1) // 2) * (n_hyp_max + 1),), math.nan, dtype=torch.float64,
                        device=engine.device())
    return f.work.data_ptr()


def test_empty_tiles_write_their_partial_sums():
    """The gradient workspace holds NaN before the run: a tile at or beyond n_b that left a partial sum unwritten
    would make that member's gradient NaN."""
    sizes = [300, 37, 128, 257]
    built = [member(t, h, n, 1, 800 + b) for b, ((t, h), n) in enumerate(zip(HETERO, sizes))]
    f = engine.RaggedInverseFactorization(sizes, 1)
    at = _nan_workspace(f, 3)
    f.run([m for m, _ in built], T(NZ))
    assert f.work.data_ptr() == at          # (the run used the poisoned buffer)
    for b, (_, data) in enumerate(built):
        assert bool(torch.isfinite(f.gradient(b)).all()), b
        check_member(f, b, data, inverse=False)


def test_empty_tiles_of_a_change_point_program_leave_zeros_in_shared_slots():
    """ChangePointOperator over two SE children: its two window leaves share the bound's slot (the later leaf adds to
    what the earlier one wrote); n = 200 and 70, so member 1's tiles of rows >= 128 are empty.  SIGMOID windows: the
    bound's derivative is not zero."""
    cps.set_mode("SIGMOID")
    tree, hyp = ("CP", [SE, SE]), [0.5, 0.08, 0.25]
    sizes, built = [200, 70], []
    dev = engine.device()
    for b, n in enumerate(sizes):
        x, y, _ = cps.cp_inputs(n, 900 + b, [0.5])
        kd = engine.kernel_descriptor(cps.make_kernel(tree, hyp, 1), 1)
        h = engine.pack_hyper_parameter(hyp_list(hyp), kd.n_hyp)
        built.append(((kd, h, torch.tensor(x, device=dev), torch.tensor(y, device=dev)), (x, y)))
    f = engine.RaggedInverseFactorization(sizes, 1)
    at = _nan_workspace(f, 3)
    f.run([m for m, _ in built], T(NZ))
    assert f.work.data_ptr() == at
    f.check_info()
    for b, (_, (x, y)) in enumerate(built):
        g = f.gradient(b).cpu().numpy()
        assert np.all(np.isfinite(g)), (b, g)
        nl_ref, g_ref, gn_ref = cps.cp_nlml_and_grad(tree, hyp, NZ, x, y, "SIGMOID")
        assert rel(float(f.nlml()[b]), nl_ref) < 1e-9
        assert abs(g_ref[0]) > 0
        _check_grad([g[:-1], g[-1]], [g_ref, gn_ref])


# ------------------------------------------------------------------------------------ 6. BlockwiseLogLikelihood
def _segment_oracle(trees, hyps, segs, noise):
    vals, grads, gn = 0.0, [], 0.0
    for t, h, s in zip(trees, hyps, segs):
        if len(s[0]) == 0:
            grads.append(np.zeros(len(h)))
            continue
        v, g, n_ = ad.nlml_and_grad(t, h, noise, s[0], s[1])
        vals += v
        grads.append(np.array([float(a) for a in g]))
        gn += n_
    return vals, np.concatenate(grads), gn


def test_blockwise_log_likelihood_gradient():
    g, segs = blockwise_setup(n=700, n_test=90)
    m = get_metric_by_type(MetricType.blockwise_LL, g)
    flat = [0.08, 0.3, 0.9, 0.45]
    exp_v, exp_g, exp_gn = _segment_oracle(CHILD_TREES, CHILD_HYPS, segs, NOISE)
    val, grads, gn = m.get_metric_and_gradient(hyp_list(flat), T(NOISE))
    assert tuple(val.shape) == (1, 1) and rel(float(val), exp_v) < 1e-9
    assert [tuple(a.shape) for a in grads] == [()] * 4
    got = np.array([float(a) for a in grads])
    _check_grad([got, float(gn)], [exp_g, exp_gn])
    # the value is the one get_metric gives without gradients (the plain ragged batch)
    assert rel(float(val), float(m.get_metric(hyp_list(flat), T(NOISE)))) < 1e-9
    # get_gradients: the flat vector
    gg = m.get_gradients(hyp_list(flat), T(NOISE)).cpu().numpy()
    assert gg.shape == (4,)
    _check_grad([gg], [exp_g])
    # autograd: get_metric(...).backward() as the reference's tape
    h = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in flat]
    nz = torch.tensor(NOISE, dtype=torch.float64, requires_grad=True)
    out = m.get_metric(h, nz)
    assert out.shape == (1, 1) and out.requires_grad and rel(float(out), exp_v) < 1e-9
    (2.0 * out.sum()).backward()
    _check_grad([np.array([float(t.grad) for t in h]), float(nz.grad)], [2.0 * exp_g, 2.0 * exp_gn])
    with torch.no_grad():
        assert not m.get_metric(h, nz).requires_grad
    # the offset quirk: a full list [cp1, cp2, children...] is sliced from 0; the entries no segment reads get zeros
    full = [0.25, 0.6] + flat
    q_trees, q_hyps = CHILD_TREES, [[0.25], [0.6], [0.08, 0.3]]
    q_v, q_g, q_gn = _segment_oracle(q_trees, q_hyps, segs, NOISE)
    val, grads, gn = m.get_metric_and_gradient(hyp_list(full), T(NOISE))
    assert rel(float(val), q_v) < 1e-9 and len(grads) == 6
    got = np.array([float(a) for a in grads])
    assert np.array_equal(got[4:], np.zeros(2))
    _check_grad([got[:4], float(gn)], [q_g, q_gn])


def test_blockwise_gradient_with_an_empty_segment_and_a_failing_one():
    model = pm.PartitioningModel(pm.PartitioningClass.SELF_SUFFICIENT, [])
    for lo, hi in [(0.0, 0.5), (0.5, 0.8), (0.8, 1.1)]:
        model.add_partitioning_criterion(Interval(lo, hi))
    rng = np.random.default_rng(9)
    x = rng.uniform(0, 0.8, (300, 1))                # nothing in the last partition's training set
    y = np.sin(5 * x[:, 0]) + 0.05 * rng.standard_normal(300)
    xt = rng.uniform(0, 1, (40, 1))
    pdi = model.partition_data_input(DataInput(x, y.reshape(-1, 1), xt, np.sin(5 * xt)))
    pdi.set_mean_function(ZeroMeanFunction(1))
    kernel = PartitionOperator(1, [bk.SquaredExponentialKernel(1), bk.SquaredExponentialKernel(1),
                                   bk.SquaredExponentialKernel(1)], model)
    g = PartitionedGaussianProcess(kernel, ZeroMeanFunction(1))
    g.set_data_input(pdi)
    tr = model.get_data_record_indices_per_partition(x)
    assert len(tr[2]) == 0
    segs = [(x[i], y[i]) for i in tr]
    hyps = [[0.1], [0.2], [0.3]]
    exp_v, exp_g, exp_gn = _segment_oracle([SE] * 3, hyps, segs, NOISE)
    m = get_metric_by_type(MetricType.blockwise_LL, g)
    val, grads, gn = m.get_metric_and_gradient(hyp_list([0.1, 0.2, 0.3]), T(NOISE))
    assert rel(float(val), exp_v) < 1e-9
    got = np.array([float(a) for a in grads])
    assert got[2] == 0.0                             # the empty segment contributes nothing
    _check_grad([got, float(gn)], [exp_g, exp_gn])
    # a segment that is not positive definite: +inf and NaN gradients
    val, grads, gn = m.get_metric_and_gradient(hyp_list([0.1, 0.2, 0.3]), T(-1.0))
    assert math.isinf(float(val)) and float(val) > 0
    assert all(math.isnan(float(a)) for a in grads) and math.isnan(float(gn))


# ------------------------------------------------------------------------------------------------------ 7. k-fold
def test_kfold_evaluator_matches_the_mean_of_the_fold_oracles():
    """n = 101 in 3 folds (67, 67 and 68 training points): f and g are the mean over the folds of the per-fold oracle,
    at the bars of the batched evaluator (tests/test_gpu_fitter.test_batched_value_and_gradient: -LML rel 1e-9, gradient
    1e-7 max(1, |g|_max)); a candidate whose folds fail reports info != 0, +inf and NaN, and only that one."""
    x, y = _inputs(101, 1, 41)
    folds = ks.fold_arrays(x, y, (34, 34, 33), 6)
    assert [len(f[0]) for f in folds] == [67, 67, 68]
    kernel = make_kernel(SE_PER, 1)
    ev = sweep.native_kfold_value_and_gradient(kernel, [(f[0], f[1]) for f in folds])
    assert ev.n_par == 4 and ev.n_folds == 3
    rng = np.random.default_rng(2)
    cands = np.column_stack([rng.uniform(0.1, 0.4, 5), rng.uniform(0.5, 1.5, 5), rng.uniform(0.3, 2.0, 5),
                             rng.uniform(0.01, 0.1, 5)])
    cands[3, 3] = -1.0                                                  # not positive definite
    C = torch.as_tensor(cands, device=engine.device())
    f, g, info = ev(C)
    assert f.shape == (5,) and g.shape == (5, 4) and info.shape == (5,) and info.dtype == torch.int32
    fn = ks.oracle_mean(SE_PER, folds)
    info_h = info.cpu().numpy()
    for b in range(5):
        if b == 3:
            assert info_h[b] != 0 and math.isinf(float(f[b])) and bool(torch.isnan(g[b]).all())
            continue
        f_ref, g_ref = fn(cands[b])
        assert info_h[b] == 0 and rel(float(f[b]), f_ref) < 1e-9
        _check_grad([g[b].cpu().numpy()], [g_ref])
    f2, g2, _ = ev(C)       # a second call reuses the factorisation and returns the same bits
    keep = [0, 1, 2, 4]
    assert torch.equal(f2[keep], f[keep]) and torch.equal(g2[keep], g[keep])


@pytest.fixture
def e2e_flags():
    gp.init(0)
    jitter = gp.p_cov_matrix_jitter
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False
    gp.p_cov_matrix_jitter = jitter


@pytest.mark.parametrize("optimize_noise", [True, False])
def test_kfold_fit_end_to_end(optimize_noise, e2e_flags):
    """N = 96, three folds of 66 / 64 / 62 training points, SE, 8 starts, bounded: the construction, the gradient check
    and the value bar of tests/test_gpu_fitter.test_fit_end_to_end, with the mean over the folds of the oracle's -LML as
    the objective SciPy's L-BFGS-B minimises from the same starts (it converges from every one of them on this seed:
    tests/test_ragged_grad_host.py).

    Gradient check: as there, the oracle's projected-gradient inf-norm at every start's returned point is <= gtol +
    1e-7 max(1, |g_ref|_max), and starts that ended on CONVERGED_F are exempt, at most 2 of 8.  One difference, made
    after the first run on the MI355X: there the winner must not have ended on CONVERGED_F; here the winner is held to
    the gradient bar itself, whatever its status.  All 8 starts of this problem reach the same minimum to 1e-13, so
    which of them is the argmin is decided by rounding, and with the noise pinned it is start 0, which ended on the f
    test (projected gradient 1.173e-05 against a bar of 1.693e-05: it passes).  What the original rule protects -- the
    returned point is stationary to the gradient bar -- is asserted directly.

    Value check: device_best - scipy_best <= max(2 x the largest gap of the e2e cases, ftol max(1, |f|)).  Measured on
    the MI355X: -5.862e-14 with the noise optimised, -1.243e-14 with it pinned."""
    x, y, folds = ks.e2e_problem()
    fitter, kernel, x0, lo, hi = ks.e2e_fitter(folds, optimize_noise)
    pre, post, hyp, noise, indices = fitter.fit()
    assert indices is None and pre.shape == (1, 1) and post.shape == (1, 1)
    print("kfold", optimize_noise, "report", fitter.report, "steps", fitter.steps, "reads", fitter.status_reads)
    assert fitter.status_reads == fitter.steps // fitter.check_every      # the only planned host synchronisation
    assert [float(a) for a in kernel.get_last_hyper_parameter()] == [float(a) for a in hyp]
    assert float(kernel.get_noise()) == float(noise)
    fn = ks.oracle_mean(ks.SE, folds)
    # pre- and post-fit metrics: the mean of the folds' get_metric (opt_kfold)
    assert rel(float(pre), fn(x0[0])[0]) < 1e-9 and float(post) <= float(pre)
    if not optimize_noise:
        assert float(noise) == E2E_NOISE
    else:
        assert np.all(x0[:, -1] == E2E_NOISE_FLOOR) and lo[-1] == E2E_NOISE_FLOOR
        assert E2E_NOISE_FLOOR < 0.5 * E2E_NOISE < float(noise) < 2 * E2E_NOISE
    status = [r[1] for r in fitter.report]
    fdev = np.array([r[0] for r in fitter.report])
    pts = fitter.points.numpy()
    w = fitter.winner
    assert fdev[w] == np.min(fdev[np.isfinite(fdev)])
    assert np.array_equal(np.abs(pts[w]), np.abs(np.array([float(a) for a in hyp] + [float(noise)])))
    assert np.all(pts >= lo) and np.all(pts <= hi)
    exempt = [b for b in range(8) if status[b] == "CONVERGED_F"]
    figures = []
    for b in range(8):
        fb, gb = fn(pts[b])
        gbar = 1e-5 + 1e-7 * max(1.0, float(np.max(np.abs(gb))))
        pg = projected_gradient_norm(pts[b], gb, lo, hi)
        print("  start %d%s %s f %.17g oracle f %.17g projected gradient %.3e (bar %.3e)"
              % (b, " (winner)" if b == w else "", status[b], fdev[b], fb, pg, gbar))
        figures.append((fb, pg, gbar))
    assert len(exempt) <= 2, (status, w)
    for b, (fb, pg, gbar) in enumerate(figures):
        assert abs(fb - fdev[b]) <= 1e-9 * abs(fb)
        if b == w or b not in exempt:      # the winner is held to the gradient bar whatever its status
            assert pg <= gbar, (b, status[b], pg, gbar)
    device_best, gw = fn(pts[w])
    assert rel(float(post), device_best) < 1e-9
    if optimize_noise:
        assert pts[w, -1] == float(noise) and fs.free_set(pts[w], gw, lo, hi)[-1]
        assert abs(gw[-1]) <= 1e-5 + 1e-7 * max(1.0, float(np.max(np.abs(gw))))
    ref = ks.scipy_runs(folds, x0, lo, hi)
    assert all(c for _, _, c in ref)
    scipy_best = min(f for f, _, _ in ref)
    gap = device_best - scipy_best
    floor = E2E_FTOL * max(1.0, abs(scipy_best))
    print("kfold", optimize_noise, "device_best - scipy_best = %.3e (floor %.3e)" % (gap, floor))
    assert gap <= max(2 * E2E_MEASURED_GAP, floor)
