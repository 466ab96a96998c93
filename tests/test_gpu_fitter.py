"""The device-resident multi-start L-BFGS fitter on the MI355X: gpk_fit_init / gpk_fit_step (engine.LbfgsState) against
the numpy restatement of tests/fit_support.py and analytic objectives, sweep.native_batched_value_and_gradient, and
Optimizer.Fitter.DeviceLbfgsFitter end to end against SciPy's L-BFGS-B on the autodiff oracle.

f and g of the analytic cases are computed by torch in fp64 from x_trial, on the device, between the steps."""
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine, sweep
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer.Fitter import DeviceLbfgsFitter, pack_bounds
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests import cp_support as cps
from tests import fit_support as fs
from tests.helpers import make_kernel
from tests.test_gpu_parity import build_gp

pytestmark = pytest.mark.gpu

U = fs.U
INF = float("inf")


def dev():
    return engine.device()


def T(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev())


# ------------------------------------------------------------------------------------- objectives on the device
def row_sum(t):
    """Row sums by one elementwise add per column: the same additions in the same order whatever the batch."""
    s = t[:, 0].clone()
    for j in range(1, t.shape[1]):
        s = s + t[:, j]
    return s


def diag_quadratic_t(h, xstar, exact_rows=False):
    h, xstar = T(h), T(xstar)

    def fn(X):
        E = X - xstar
        G = h * E
        return 0.5 * (row_sum(G * E) if exact_rows else torch.sum(G * E, dim=1)), G, None
    return fn


def quadratic_t(A, xstar):
    A, xstar = T(A), T(xstar)

    def fn(X):
        E = X - xstar
        G = E @ A
        return 0.5 * torch.sum(G * E, dim=1), G, None
    return fn


def rosenbrock_t(X):
    x, y = X[:, 0], X[:, 1]
    r = y - x * x
    f = (1 - x) ** 2 + 100 * r * r
    return f, torch.stack([-2 * (1 - x) - 400 * x * r, 200 * r], dim=1), None


def pseudo_huber_t(xstar):
    """fit_support.pseudo_huber on the device."""
    xstar = T(xstar)

    def fn(X):
        E = X - xstar
        r = torch.sqrt(1.0 + E * E)
        return torch.sum(r - 1.0, dim=1), E / r, None
    return fn


def walled_t(inner, wall):
    """``inner`` left of x_0 = wall; beyond it +inf, NaN gradients and info = 1."""
    def fn(X):
        f, g, _ = inner(X)
        bad = X[:, 0] > wall
        return (torch.where(bad, torch.full_like(f, INF), f),
                torch.where(bad[:, None], torch.full_like(g, float("nan")), g), bad.to(torch.int32))
    return fn


def run(state, objective, max_steps=4000, check_every=16, each=None):
    """Drive an engine.LbfgsState to completion (the status words read every check_every steps)."""
    for k in range(max_steps):
        f, g, info = objective(state.x_trial)
        state.step(f, g, info)
        if each is not None:
            each(k, state)
        if (k + 1) % check_every == 0 and not bool((state.status == nat.FIT_RUNNING).any()):
            return k + 1
    assert not bool((state.status == nat.FIT_RUNNING).any()), "not finished after %d steps" % max_steps
    return max_steps


def accepted_steps(state, objective, k):
    """Step until every member has accepted exactly k steps more than INIT (members that got there wait: their
    evaluation is repeated at the same x_trial only through the others' progress, so stop at the first step after
    which all have iterations >= k and equal)."""
    for _ in range(60 * (k + 1)):
        f, g, info = objective(state.x_trial)
        state.step(f, g, info)
        it = state.header()[:, 2].cpu().numpy()
        if np.all(it >= k):
            return it
    raise AssertionError("no %d accepted steps" % k)


# ---------------------------------------------------------------------------------------------------- first step
@pytest.mark.parametrize("batch", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("n_par", [1, 2, 63, 64, 65])
def test_first_step(n_par, batch):
    """After init and one step on a quadratic: x_trial = clamp(x0 - min(1, 1 / |g|_2) g) (unbounded and boxed).

    Bound.  t = min(1, 1 / sqrt(sum g_j^2)): the sum of P products has relative error <= gamma_{P+1} (P roundings of
    the products and fused adds along any tree path, Higham (3.5)); the square root halves it and adds one rounding,
    the reciprocal one more: |dt| / t <= ((P + 1) / 2 + 2) u.  x_trial = fl(fma(t, d, x)) adds one rounding of the result:
    |x_trial - exact| <= ((P + 1) / 2 + 2) u |t d| + u |exact|, times 1.01 for the second-order terms; the clamp is
    1-Lipschitz, and a clamped coordinate must be the bound itself.  The reference is evaluated in extended
    precision (its own error is 2^-11 of the bound)."""
    rng = np.random.default_rng(1000 * n_par + batch)
    h = rng.uniform(0.5, 3.0, n_par)
    xstar = rng.standard_normal(n_par)
    x0 = rng.standard_normal((batch, n_par))
    x0[0] = xstar + 1e-3 * rng.standard_normal(n_par) / h        # |g| < 1: t = 1
    for boxed in (False, True):
        lo = np.where(np.arange(n_par) % 3 == 0, -0.5, -INF) if boxed else np.full(n_par, -INF)
        hi = np.where(np.arange(n_par) % 2 == 0, 0.7, INF) if boxed else np.full(n_par, INF)
        st = engine.LbfgsState(T(x0), T(lo), T(hi))
        xc = np.minimum(np.maximum(x0, lo), hi)
        assert np.array_equal(st.x_trial.cpu().numpy(), xc)                     # init: the clamp, exactly
        obj = diag_quadratic_t(h, xstar)
        f, g, _ = obj(st.x_trial)
        gn = g.cpu().numpy()
        st.step(f, g)
        got = st.x_trial.cpu().numpy()
        assert np.all(got >= lo) and np.all(got <= hi)
        free = fs.free_set(xc, gn, lo, hi) if boxed else np.ones_like(xc, dtype=bool)
        d = np.where(free, -gn, 0.0).astype(np.longdouble)
        nrm = np.sqrt(np.sum(d * d, axis=1, keepdims=True))
        with np.errstate(divide="ignore"):
            t = np.minimum(np.longdouble(1.0), 1.0 / nrm)
        exact = xc.astype(np.longdouble) + t * d
        bar = 1.01 * (((n_par + 1) / 2 + 2) * U * np.abs(t * d) + U * np.abs(exact))
        ref = np.minimum(np.maximum(exact, lo), hi)
        assert np.all(np.abs(got - ref) <= bar), float(np.max(np.abs(got - ref) / np.maximum(bar, 1e-300)))
        assert float(t[0, 0]) == 1.0
        x, fx, gx, it = st.current()
        assert np.array_equal(x.cpu().numpy(), xc) and np.array_equal(gx.cpu().numpy(), gn)
        assert np.array_equal(fx.cpu().numpy(), f.cpu().numpy()) and not it.any()


# ------------------------------------------------------------------------------- direction vs the restatement
DIRECTION_WORST = {}


@pytest.mark.parametrize("n_par", [5, 64, 65])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_direction_matches_restatement(k, n_par):
    """k accepted steps with history m = 4 (k = 1, m, m + 3: the ring wraps), then S, Y and g are read back and the
    next x_trial - x (t = 1) is compared with the numpy two-loop recursion on those same pairs.  The bar is the
    propagated rounding bound of the recursion's 4 m + 2 inner products of length n_par
    (fit_support.two_loop_rounding_bound: gamma_{n + 3} (4 m + 2) times the recursion run on magnitudes), plus the
    rounding of forming x + d and subtracting x again, 2 u (|x| + |d|).  Derived, not tuned."""
    m, batch = 4, 3
    rng = np.random.default_rng(77 + n_par)
    Q, _ = np.linalg.qr(rng.standard_normal((n_par, n_par)))
    A = Q @ np.diag(fs.log_spaced(30.0, n_par)) @ Q.T
    A = 0.5 * (A + A.T)
    xstar = rng.standard_normal(n_par)
    st = engine.LbfgsState(T(xstar + rng.standard_normal((batch, n_par))), history=m, gtol=0.0, ftol=0.0)
    it = accepted_steps(st, quadratic_t(A, xstar), k)
    hdr = st.header().cpu().numpy()
    S, Y, rho, cnt, head = (a.cpu().numpy() for a in st.ring())
    x, _, g, _ = (a.cpu().numpy() for a in st.current())
    xt = st.x_trial.cpu().numpy()
    worst = 0.0
    for b in range(batch):
        assert hdr[b, 1] == nat.FIT_RUNNING and hdr[b, 3] == 0 and it[b] >= k
        assert hdr[b, 9] == 0     # a convex quadratic: every accepted step pushed its pair, no steepest-descent restart
        c, hd = int(cnt[b]), int(head[b])
        assert c == min(int(it[b]), m) and hdr[b, 7] == 1.0
        order = [(hd - c + i) % m for i in range(c)]               # oldest first
        pairs = [(S[b, i], Y[b, i]) for i in order]
        for i in order:
            assert abs(rho[b, i] * np.dot(S[b, i], Y[b, i]) - 1.0) <= (n_par + 2) * U * (
                np.dot(np.abs(S[b, i]), np.abs(Y[b, i])) / abs(np.dot(S[b, i], Y[b, i])))
        d = -fs.two_loop(g[b], pairs)
        bar = fs.two_loop_rounding_bound(n_par, m, pairs, g[b]) + 2 * U * (np.abs(x[b]) + np.abs(d))
        ratio = float(np.max(np.abs((xt[b] - x[b]) - d) / bar))
        worst = max(worst, ratio)
    DIRECTION_WORST[(k, n_par)] = worst
    print("direction worst ratio to the bar k=%d n_par=%d: %.3g" % (k, n_par, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------- properties
def _box_problem():
    n_par = 6
    h = np.array([1.0, 4.0, 2.0, 9.0, 0.5, 1.0])
    xstar = np.array([2.0, -3.0, 0.25, 0.1, -0.4, 0.7])
    lo = np.array([-1.0, -1.0, -1.0, -INF, -2.0, 0.4])
    hi = np.array([1.0, 1.0, 1.0, INF, INF, 0.4])               # the last coordinate is pinned
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-1.5, 1.5, (9, n_par))
    return n_par, h, xstar, lo, hi, x0


def _trajectory(x0, lo, hi, obj, steps, **kw):
    st = engine.LbfgsState(T(x0), T(lo), T(hi), **kw)
    xs, fa, sts = [st.x_trial.clone()], [], []

    def each(k, s):
        xs.append(s.x_trial.clone())
        fa.append(s.header()[:, 6].clone())
        sts.append(s.status.clone())
    for k in range(steps):
        f, g, info = obj(st.x_trial)
        st.step(f, g, info)
        each(k, st)
    return st, torch.stack(xs).cpu().numpy(), torch.stack(fa).cpu().numpy(), torch.stack(sts).cpu().numpy()


def test_properties_exact():
    n_par, h, xstar, lo, hi, x0 = _box_problem()
    obj = diag_quadratic_t(h, xstar, exact_rows=True)
    steps = 64
    # (ftol = 0: only the gradient test ends a member, so the distances below follow from gtol and the Hessian)
    st, xs, fa, sts = _trajectory(x0, lo, hi, obj, steps, ftol=0.0)
    assert not np.any(sts[-1] == nat.FIT_RUNNING)
    # every trial point inside the box, compared on the values themselves
    assert np.all(xs >= lo) and np.all(xs <= hi)
    assert np.all(xs[:, :, 5] == 0.4)                                   # the pinned coordinate never moves
    assert np.all(np.diff(fa, axis=0) <= 0.0)                           # accepted f never increases
    x = st.current()[0].cpu().numpy()
    assert np.all(x[:, 0] == 1.0) and np.all(x[:, 1] == -1.0)           # the active face
    assert np.abs(x[:, 2] - 0.25).max() <= 1e-5 / 2.0 and np.abs(x[:, 3] - 0.1).max() <= 1e-5 / 9.0
    assert np.abs(x[:, 4] + 0.4).max() <= 1e-5 / 0.5
    assert np.all(sts[-1] == nat.FIT_CONVERGED_G)
    # two runs: the same bits, states included
    st2, xs2, fa2, sts2 = _trajectory(x0, lo, hi, obj, steps, ftol=0.0)
    assert np.array_equal(xs, xs2) and np.array_equal(fa, fa2) and np.array_equal(sts, sts2)
    assert torch.equal(st.state, st2.state)
    # member b of the batch of 9 follows, bit for bit, the trajectory it follows alone
    for b in (0, 3, 4, 8):
        st1, xs1, fa1, sts1 = _trajectory(x0[b:b + 1], lo, hi, obj, steps, ftol=0.0)
        assert np.array_equal(xs1[:, 0], xs[:, b]) and np.array_equal(fa1[:, 0], fa[:, b])
        assert np.array_equal(sts1[:, 0], sts[:, b])
        assert torch.equal(st1.state[0, :11], st.state[b, :11]) and torch.equal(st1.state[0, 12:], st.state[b, 12:])
    # frozen members: 5 further steps (with garbage evaluations) change neither their state nor x_trial
    before, xt_before = st.state.clone(), st.x_trial.clone()
    for _ in range(5):
        st.step(torch.full((9,), -1e9, dtype=torch.float64, device=dev()),
                torch.ones((9, n_par), dtype=torch.float64, device=dev()))
    assert torch.equal(st.state, before) and torch.equal(st.x_trial, xt_before)
    assert np.array_equal(st.status.cpu().numpy(), sts[-1])


def test_strided_inputs_and_status_of_foreign_state():
    """f and g read through strides (a [B, 4] read-out buffer, a wider gradient buffer) give the bits of the contiguous
    call; a state initialised for another n_par is refused with status -1 and left alone."""
    n_par, h, xstar, lo, hi, x0 = _box_problem()
    obj = diag_quadratic_t(h, xstar, exact_rows=True)
    a = engine.LbfgsState(T(x0), T(lo), T(hi))
    b = engine.LbfgsState(T(x0), T(lo), T(hi))
    for _ in range(6):
        f, g, _i = obj(a.x_trial)
        a.step(f, g)
        out = torch.zeros((9, 4), dtype=torch.float64, device=dev())
        wide = torch.full((9, n_par + 3), float("nan"), dtype=torch.float64, device=dev())
        f2, g2, _i = obj(b.x_trial)
        out[:, 0] = f2
        wide[:, :n_par] = g2
        b.step(out[:, 0], wide[:, :n_par], torch.zeros(9, dtype=torch.int32, device=dev()))
    assert torch.equal(a.state, b.state) and torch.equal(a.x_trial, b.x_trial)
    with pytest.raises(ValueError):
        a.step(f, g[:, :n_par - 1])
    before = a.state.clone()
    rc = a.L.gpk_fit_step(n_par - 1, 9, None, nat.ptr(f), 1, nat.ptr(g), n_par, None, nat.ptr(a.state),
                          nat.ptr(a.x_trial), n_par, nat.ptr(a.status), nat.stream_handle(dev()))
    assert rc == 0 and np.all(a.status.cpu().numpy() == -1) and torch.equal(a.state, before)
    # gpk_fit_current on it: every output says so (NaN, iterations -1) instead of staying unwritten
    xo = torch.zeros((9, n_par - 1), dtype=torch.float64, device=dev())
    go, fo = torch.zeros_like(xo), torch.zeros(9, dtype=torch.float64, device=dev())
    io = torch.zeros(9, dtype=torch.int32, device=dev())
    rc = a.L.gpk_fit_current(n_par - 1, 9, nat.ptr(a.state), nat.ptr(xo), n_par - 1, nat.ptr(fo), nat.ptr(go),
                             n_par - 1, nat.ptr(io), nat.stream_handle(dev()))
    assert rc == 0 and bool(torch.isnan(xo).all() and torch.isnan(go).all() and torch.isnan(fo).all())
    assert bool((io == -1).all())


# ---------------------------------------------------------------------------------------------- failed trials
def test_failed_trials_backtrack_and_bad_start_is_contained():
    """Beyond the wall x_0 > 0.5 the objective is +inf with NaN gradients and info = 1.  Members 0 .. 2 start far out
    on the feasible side of a pseudo-Huber bowl (x* = (0.45, 0), next to the wall), where the curvature is tiny: their
    first quasi-Newton steps overshoot x* across the wall, they backtrack and converge on the feasible side.  Member
    3 -- same workgroup -- starts beyond the wall: BAD_START, its neighbours unaffected; member 4 is alone in the second
    workgroup.  The Hessian at x* is the identity, so |x - x*|_inf <= gtol to first order (asserted with a factor 2)."""
    inner = pseudo_huber_t([0.45, 0.0])
    x0 = np.array([[-30.0, 2.0], [-8.0, -1.0], [-50.0, 5.0], [0.9, 0.0], [-20.0, 0.1]])
    st = engine.LbfgsState(T(x0))
    seen_bad = []
    run(st, walled_t(inner, 0.5), each=lambda k, s: seen_bad.append((s.x_trial[:, 0] > 0.5).cpu().numpy()))
    status = st.status.cpu().numpy()
    x, f, g, it = (a.cpu().numpy() for a in st.current())
    assert status[3] == nat.FIT_BAD_START and np.array_equal(x[3], x0[3]) and it[3] == 0
    ok = [0, 1, 2, 4]
    assert np.all(np.isin(status[ok], (nat.FIT_CONVERGED_G, nat.FIT_CONVERGED_F)))
    assert np.abs(x[ok] - [0.45, 0.0]).max() <= 2e-5 and np.all(np.isfinite(f[ok]))
    assert np.all(np.any(np.array(seen_bad)[:, ok], axis=0))   # every one of them had trials beyond the wall
    # the same members without the bad neighbour: the same bits
    st2 = engine.LbfgsState(T(x0[ok]))
    run(st2, walled_t(inner, 0.5))
    assert np.array_equal(st2.current()[0].cpu().numpy(), x[ok])


def test_only_nan_gradient_or_only_info_fail_the_trial():
    inner = diag_quadratic_t([1.0, 1.0], [0.45, 0.0])

    def nan_g(X):
        f, g, _ = inner(X)
        bad = X[:, 0] > 0.5
        g = g.clone()
        g[:, 1] = torch.where(bad, torch.full_like(f, float("nan")), g[:, 1])
        return f, g, None

    def info_only(X):
        f, g, _ = inner(X)
        return f, g, (X[:, 0] > 0.5).to(torch.int32)
    for obj in (nan_g, info_only):
        st = engine.LbfgsState(T([[-3.0, 2.0]]))
        xs = []
        run(st, obj, each=lambda k, s: xs.append(s.current()[0].cpu().numpy()))
        assert np.all(np.array(xs)[:, 0, 0] <= 0.5)                      # no accepted point beyond the wall
        assert np.abs(st.current()[0].cpu().numpy() - [0.45, 0.0]).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ convergence
def test_ill_conditioned_quadratic_65d():
    """H = diag(h), 65 log-spaced values from 1 to 1e6 (ftol = 0: only the gradient test may end it).  At the end
    |g|_inf <= gtol and g_j = h_j (x_j - x*_j), so |x_j - x*_j| <= gtol / h_j <= gtol / min h = gtol."""
    h = fs.log_spaced(1e6, 65)
    xstar = np.linspace(-1.0, 1.0, 65)
    x0 = np.stack([np.zeros(65), xstar + 0.5, -xstar])
    st = engine.LbfgsState(T(x0), max_iter=20000, ftol=0.0)
    run(st, diag_quadratic_t(h, xstar), max_steps=40000, check_every=256)
    x, f, g, it = (a.cpu().numpy() for a in st.current())
    assert np.all(st.status.cpu().numpy() == nat.FIT_CONVERGED_G), (st.status, it)
    assert np.abs(g).max() <= 1e-5
    assert np.all(np.abs(x - xstar) <= 1e-5 / h * (1 + 1e-12) + 4 * U * np.abs(xstar))


def test_rosenbrock():
    """Ends on CONVERGED_G, or CONVERGED_F with |g|_inf below gtol.  Near x* = (1, 1) the Hessian is
    [[802, -400], [-400, 200]] with smallest eigenvalue 0.39936; g = H (x - x*) + O(|x - x*|^2), so
    |x - x*|_inf <= |x - x*|_2 <= |g|_2 / 0.39936 <= sqrt(2) gtol / 0.39936 to first order -- asserted with a factor 2
    for the second-order term (|x - x*| ~ 4e-5 changes H by 1e-2 relative)."""
    st = engine.LbfgsState(T([[-1.2, 1.0], [0.0, 0.0], [2.0, -1.0]]), max_iter=2000)
    run(st, rosenbrock_t)
    x, f, g, it = (a.cpu().numpy() for a in st.current())
    status = st.status.cpu().numpy()
    assert np.all(np.isin(status, (nat.FIT_CONVERGED_G, nat.FIT_CONVERGED_F))), (status, it)
    assert np.abs(g).max() <= 1e-5
    assert np.abs(x - 1.0).max() <= 2 * math.sqrt(2) * 1e-5 / 0.39936


# ------------------------------------------------------------------- sweep.native_batched_value_and_gradient
N_E2E = 96


def _x():
    return np.linspace(0.0, 1.0, N_E2E).reshape(-1, 1)


def test_batched_value_and_gradient():
    """Row b is, bit for bit, what engine.InverseFactorization(batch = 5) driven directly gives, and matches
    get_metric_and_gradient of candidate b at the bars tests/test_gpu_grad.py uses between batched and single
    evaluations (-LML rel 1e-9, gradient 1e-7 max(1, |g|_max))."""
    tree = ("ADD", [("SE", {}), ("PER", {})])
    x = _x()
    y = np.sin(9 * x[:, 0]) + 0.3 * np.cos(31 * x[:, 0])
    kernel = make_kernel(tree, 1)
    ev = sweep.native_batched_value_and_gradient(kernel, x, y)
    rng = np.random.default_rng(2)
    cands = np.column_stack([rng.uniform(0.1, 0.4, 5), rng.uniform(0.5, 1.5, 5), rng.uniform(0.3, 2.0, 5),
                             rng.uniform(0.01, 0.1, 5)])
    cands[4, 3] = -1.0                                                  # not positive definite
    C = T(cands)
    f, g, info = ev(C)
    f, g, info = f.clone(), g.clone(), info.clone()
    assert f.shape == (5,) and g.shape == (5, 4) and info.dtype == torch.int32
    kd = engine.kernel_descriptor(kernel, 1)
    direct = engine.InverseFactorization(N_E2E, 1, 5, torch.float64)
    flat = C.reshape(-1)
    direct.run(kd, flat, 4, flat[3:], 4, T(x), 0, T(y).reshape(1, -1), 0)
    assert torch.equal(direct.nlml(), f) or (torch.equal(direct.nlml()[:4], f[:4]) and math.isinf(float(f[4])))
    assert torch.equal(direct.gradient()[:4], g[:4]) and torch.equal(direct.info, info)
    assert int(info[4]) != 0 and math.isinf(float(f[4])) and bool(torch.isnan(g[4]).all())
    metric = build_gp(tree, x, y)
    from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
    m = get_metric_by_type(MetricType.LL, metric)
    for b in range(4):
        nl, grads, gn = m.get_metric_and_gradient([torch.tensor(v, dtype=torch.float64) for v in cands[b, :3]],
                                                  torch.tensor(cands[b, 3], dtype=torch.float64))
        single = np.array([float(v) for v in grads] + [float(gn)])
        assert abs(float(f[b]) - float(nl)) <= 1e-9 * abs(float(nl))
        assert np.abs(g[b].cpu().numpy() - single).max() <= 1e-7 * max(1.0, np.abs(single).max())
    # a second call reuses the factorisation and returns the same bits
    f2, g2, _ = ev(C)
    assert torch.equal(f2[:4], f[:4]) and torch.equal(g2[:4], g[:4])


# --------------------------------------------------------------------------------------------------- end to end
# name -> (tree, hyperparameters the targets are drawn with, seed of the targets, seed of the starts)
E2E = {
    "SE": (("SE", {}), [0.12], 11, 2),
    "ADD": (("ADD", [("SE", {}), ("PER", {})]), [0.25, 0.8, -1.9], 11, 2),
    "CP": (("CP", [("SE", {}), ("SE", {})]), [0.5, 0.08, 0.25], 11, 2),
}
E2E_NOISE = 0.05        # the noise the targets are drawn with; with p_optimize_noise off, also p_cov_matrix_jitter
E2E_NOISE_FLOOR = 1e-3  # p_cov_matrix_jitter with p_optimize_noise on: the noise's start and lower bound, far below it


def e2e_jitter(optimize_noise):
    return E2E_NOISE_FLOOR if optimize_noise else E2E_NOISE
E2E_FTOL = 1e-13        # both optimisers: the f test only ends a run at the rounding level of f (|f| ~ 1e2)
# the largest device_best - scipy_best measured on the MI355X over the six cases (ADD, noise optimised; DESIGN.md
# section 19 lists all six); the bar is twice it, and never below the floor ftol max(1, |f|)
E2E_MEASURED_GAP = 4.832e-13


def e2e_kernel(name):
    tree, hyp = E2E[name][0], E2E[name][1]
    return cps.make_kernel(tree, hyp, 1) if name == "CP" else make_kernel(tree, 1)


def e2e_targets(name, noise):
    tree, hyp, yseed = E2E[name][0], E2E[name][1], E2E[name][2]
    x = _x()
    K = (cps.cp_numpy(tree, hyp, x, x, gp.p_cp_operator_type.name) if name == "CP"
         else o.kernel_matrix(tree, hyp, x, x)) + noise * np.eye(N_E2E)
    return np.linalg.cholesky(K) @ np.random.default_rng(yseed).standard_normal(N_E2E)


def e2e_oracle(name, y):
    """v [n_hyp + 1] -> (-LML, gradient) from the autodiff oracle (the change-point tree: its torch restatement in
    tests/cp_support.py, the oracle module has no CP node); (inf, NaN) where K + noise I is not positive definite."""
    tree, x = E2E[name][0], _x()

    def fn(v):
        try:
            if name == "CP":
                f, gh, gn = cps.cp_nlml_and_grad(tree, list(v[:-1]), v[-1], x, y, gp.p_cp_operator_type.name)
            else:
                f, gh, gn = ad.nlml_and_grad(tree, list(v[:-1]), v[-1], x, y)
                gh = [float(a) for a in gh]
            if not np.isfinite(f):
                raise ValueError
            return f, np.array(list(gh) + [gn], dtype=np.float64)
        except Exception:
            return INF, np.full(len(v), np.nan)
    return fn


def e2e_scipy(fn, x0, lo, hi):
    """SciPy's L-BFGS-B from every start with the same bounds and tolerances: [(f, x, converged)]."""
    from scipy.optimize import minimize
    bounds = [(a if np.isfinite(a) else None, b if np.isfinite(b) else None) for a, b in zip(lo, hi)]
    out = []
    for row in x0:
        r = minimize(fn, np.minimum(np.maximum(row, lo), hi), jac=True, method="L-BFGS-B", bounds=bounds,
                     options=dict(gtol=1e-5, ftol=E2E_FTOL, maxiter=200, maxcor=8))
        out.append((float(r.fun), r.x, bool(r.success)))
    return out


def projected_gradient_norm(x, g, lo, hi):
    return float(np.max(np.abs(g) * fs.free_set(x, g, lo, hi)))


@pytest.fixture
def e2e_flags():
    gp.init(0)
    jitter = gp.p_cov_matrix_jitter
    yield
    gp.p_optimize_noise = False
    gp.p_check_hyper_parameters = False
    gp.p_cov_matrix_jitter = jitter


@pytest.mark.parametrize("optimize_noise", [True, False])
@pytest.mark.parametrize("name", list(E2E))
def test_fit_end_to_end(name, optimize_noise, e2e_flags):
    """N = 96, D = 1, fp64, 8 starts, bounded.  With p_optimize_noise off the noise is pinned at
    p_cov_matrix_jitter, set to the noise the targets were drawn with, 0.05 (at the default 1e-8 the matrix is singular
    to working precision and neither optimiser can resolve a gradient of 1e-5).  With p_optimize_noise on,
    p_cov_matrix_jitter -- the noise of every start and its lower bound -- is 1e-3, far below the drawn noise: the
    optimum is interior in the noise, the fitter has to move it there, and the returned noise is checked as a free
    coordinate.

    Gradient check (derived): at every start's returned point the oracle's projected-gradient inf-norm is <= gtol +
    the device-against-oracle gradient bar of tests/test_gpu_grad.py, 1e-7 max(1, |g_ref|_max); starts that ended on
    CONVERGED_F are exempt, at most 2 of 8 and never the winner.
    Value check (measured): device_best - scipy_best <= max(2 x the largest gap measured on the MI355X,
    ftol max(1, |f|))."""
    gp.p_optimize_noise = optimize_noise
    gp.p_cov_matrix_jitter = torch.tensor(e2e_jitter(optimize_noise), dtype=torch.float64)
    y = e2e_targets(name, E2E_NOISE)
    x = _x()
    kernel = e2e_kernel(name)
    from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput
    from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
    from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess
    di = DataInput(x, y.reshape(-1, 1), x, y.reshape(-1, 1))
    di.set_mean_function(ZeroMeanFunction(1))
    g = GaussianProcess(kernel, ZeroMeanFunction(1))
    fitter = DeviceLbfgsFitter(di, g, MetricType.LL, FitterType.GRADIENT, False, mht.MatrixApproximations.NONE,
                               mht.NumericalMatrixHandlingType.CHOLESKY_BASED, n_starts=8, ftol=E2E_FTOL,
                               generator=torch.Generator().manual_seed(E2E[name][3]), bounded=True)
    x0 = fitter.starts().numpy()
    fitter.generator = torch.Generator().manual_seed(E2E[name][3])
    lo, hi = (np.array(v) for v in pack_bounds(kernel, di.get_x_range(), N_E2E, True, optimize_noise))
    pre, post, hyp, noise, indices = fitter.fit()
    assert indices is None and pre.shape == (1, 1) and post.shape == (1, 1)
    print(name, optimize_noise, "report", fitter.report, "steps", fitter.steps, "reads", fitter.status_reads)
    assert fitter.status_reads == fitter.steps // fitter.check_every      # the only planned host synchronisation

    # the returned point is the kernel's, and the post-fit metric is get_metric there, bit for bit
    assert [float(a) for a in kernel.get_last_hyper_parameter()] == [float(a) for a in hyp]
    assert float(kernel.get_noise()) == float(noise)
    again = fitter.metric.get_metric(kernel.get_last_hyper_parameter(), kernel.get_noise())
    assert torch.equal(again, post) and float(post) <= float(pre)
    if not optimize_noise:
        assert float(noise) == E2E_NOISE
    else:
        # the noise moved: every start begins on its lower bound E2E_NOISE_FLOOR, the optimum is interior
        assert np.all(x0[:, -1] == E2E_NOISE_FLOOR) and lo[-1] == E2E_NOISE_FLOOR
        assert E2E_NOISE_FLOOR < 0.5 * E2E_NOISE < float(noise) < 2 * E2E_NOISE

    # the device's accepted points, start by start (fitter.points: as the optimiser left them, signs included)
    fn = e2e_oracle(name, y)
    status = [r[1] for r in fitter.report]
    fdev = np.array([r[0] for r in fitter.report])
    pts = fitter.points.numpy()
    w = fitter.winner
    assert fdev[w] == np.min(fdev[np.isfinite(fdev)])
    assert np.array_equal(np.abs(pts[w]), np.abs(np.array([float(a) for a in hyp] + [float(noise)])))
    assert np.all(pts >= lo) and np.all(pts <= hi)
    exempt = [b for b in range(8) if status[b] == "CONVERGED_F"]
    assert len(exempt) <= 2 and w not in exempt, (status, w)
    for b in range(8):
        fb, gb = fn(pts[b])
        assert abs(fb - fdev[b]) <= 1e-9 * abs(fb)
        if b in exempt:
            continue
        gbar = 1e-5 + 1e-7 * max(1.0, float(np.max(np.abs(gb))))
        pg = projected_gradient_norm(pts[b], gb, lo, hi)
        print("  start %d %s oracle projected gradient %.3e (bar %.3e)" % (b, status[b], pg, gbar))
        assert pg <= gbar, (b, status[b], pg, gbar)
    device_best, gw = fn(pts[w])
    if optimize_noise:
        # the winner's noise is a free coordinate, and the oracle's d(-LML)/d(noise) there passes the gradient bar
        assert pts[w, -1] == float(noise) and fs.free_set(pts[w], gw, lo, hi)[-1]
        assert abs(gw[-1]) <= 1e-5 + 1e-7 * max(1.0, float(np.max(np.abs(gw))))

    # SciPy's L-BFGS-B on the oracle from the same 8 starts
    ref = e2e_scipy(fn, x0, lo, hi)
    assert sum(c for _, _, c in ref) >= 6
    scipy_best = min(f for f, _, _ in ref)
    # (both values from the oracle: the evaluation parity of device and oracle, 1e-9 relative, is asserted above and
    # is not what this gap is about)
    gap = device_best - scipy_best
    floor = E2E_FTOL * max(1.0, abs(scipy_best))
    print(name, optimize_noise, "device_best - scipy_best = %.3e (floor %.3e)" % (gap, floor))
    assert gap <= max(2 * E2E_MEASURED_GAP, floor)
