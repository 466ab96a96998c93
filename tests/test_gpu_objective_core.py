"""The contract the five native_*_value_and_gradient evaluators of sweep share through one core
(sweep._value_and_gradient over engine.AugmentedFactorization.results), held on all of them at once (needs the MI355X).

Shapes: d = 1, 70 training points (they cross a 64-row gradient tile and pad to n_pad = 128) and 5 test points; the
k-fold evaluators take two folds of 70 / 69 training and 5 / 4 test points, a ragged batch.  Kernels: SE, and ADD(SE,
PER) with several leaves sharing part[].  B = 1 lets a uniform batch take the persistent launch, so ``settle`` has
something to settle: those cases run under gpk_tune chain = 2 (70 points are below the automatic threshold) and assert
that the persistent launch was taken; B = 3 runs on the launch path.  Every comparison here is bit for bit: the
numbers themselves are checked against their references in test_gpu_fitter / test_gpu_ragged_grad /
test_gpu_mse_grad / test_gpu_loo.
"""
import contextlib

import numpy as np
import pytest
import torch

from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine, sweep
from tests.helpers import make_kernel, set_flags

pytestmark = pytest.mark.gpu

SE, PER = ("SE", {}), ("PER", {})
KERNELS = {"SE": SE, "ADD": ("ADD", [SE, PER])}
FACTORIES = ("nlml", "kfold_nlml", "mse", "kfold_mse", "loo_lpd", "loo_mse")
N, M = 70, 5
FOLDS = ((70, 5), (69, 4))


@pytest.fixture(autouse=True)
def _flags():
    set_flags()


def _points(n, seed):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 1.0, size=(n, 1)), axis=0)
    return x, np.sin(6.0 * x[:, 0]) + 0.1 * rng.standard_normal(n)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=engine.device())


_EVALUATORS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_evaluators():
    yield
    _EVALUATORS.clear()   # (their factorisations' device buffers go with them)


def _evaluator(factory, kname):
    """(evaluator, n_hyp): built once per factory and kernel, shared by this module's tests (its per-B state is part
    of what they exercise)."""
    if (factory, kname) not in _EVALUATORS:
        _EVALUATORS[factory, kname] = _build(factory, kname)
    return _EVALUATORS[factory, kname]


def _build(factory, kname):
    kernel = make_kernel(KERNELS[kname], 1)
    n_hyp = engine.kernel_descriptor(kernel, 1).n_hyp
    x, y = (_dev(a) for a in _points(N, 1))
    xs, ys = (_dev(a) for a in _points(M, 2))
    folds = [tuple(_dev(a) for a in _points(n, 10 + k) + _points(m, 20 + k)) for k, (n, m) in enumerate(FOLDS)]
    if factory == "nlml":
        ev = sweep.native_batched_value_and_gradient(kernel, x, y)
    elif factory == "kfold_nlml":
        ev = sweep.native_kfold_value_and_gradient(kernel, [f[:2] for f in folds])
    elif factory == "mse":
        ev = sweep.native_batched_mse_value_and_gradient(kernel, x, y, xs, ys)
    elif factory == "kfold_mse":
        ev = sweep.native_kfold_mse_value_and_gradient(kernel, folds)
    else:
        ev = sweep.native_batched_loo_value_and_gradient(kernel, x, y,
                                                         nat.LOO_LPD if factory == "loo_lpd" else nat.LOO_MSE)
    return ev, n_hyp


def _candidates(n_hyp, B, shift=0.0):
    """B rows of positive hyperparameters and a noise, every row different."""
    rows = [[0.3 + 0.11 * k + 0.07 * b + shift for k in range(n_hyp)] + [0.05 + 0.01 * b + shift] for b in range(B)]
    return _dev(rows)


def _bits(t):
    return t.cpu().numpy().tobytes()


def _same_bits(a, b):
    return all(_bits(u) == _bits(v) for u, v in zip(a, b))


CASES = [(f, k, B) for f in FACTORIES for k in KERNELS for B in (1, 3)]


@pytest.mark.parametrize("factory,kname,B", CASES)
def test_shapes_settle_repeat_and_earlier_views(factory, kname, B):
    ev, n_hyp = _evaluator(factory, kname)
    dev = engine.device()
    assert ev.n_par == n_hyp + 1
    if factory.startswith("kfold"):
        assert ev.n_folds == len(FOLDS)
    cands = _candidates(n_hyp, B)
    persistent = B == 1 and not factory.startswith("kfold")   # (a uniform batch of one: the persistent launch)
    with nat.thread_tune(chain=2) if persistent else contextlib.nullcontext():
        _check_contract(ev, n_hyp, B, cands, dev, persistent)


def _check_contract(ev, n_hyp, B, cands, dev, persistent):
    first = ev(cands)
    if persistent:   # (the plain call left a persistent run for settle=True to verify)
        assert nat.last_factorisation_was_chain()
    f, g, info = first
    # 1. shapes, types, device
    assert tuple(f.shape) == (B,) and f.dtype == torch.float64 and f.device == dev
    assert tuple(g.shape) == (B, n_hyp + 1) and g.dtype == torch.float64 and g.device == dev
    assert tuple(info.shape) == (B,) and info.dtype == torch.int32 and info.device == dev
    held = [_bits(t) for t in first]
    assert not info.cpu().numpy().any()
    assert np.isfinite(f.cpu().numpy()).all() and np.isfinite(g.cpu().numpy()).all()
    # 2. settled and unsettled results: equal bits
    assert _same_bits(ev(cands, settle=True), first)
    # 3. the same candidates again: equal bits
    assert _same_bits(ev(cands), first)
    # 4. other candidates: the tensors of the first call still hold its values (nobody cloned them)
    other = ev(_candidates(n_hyp, B, shift=0.02))
    assert _bits(other[0]) != held[0] and _bits(other[1]) != held[1]
    assert [_bits(t) for t in first] == held


@pytest.mark.parametrize("factory,kname", [(f, k) for f in FACTORIES for k in KERNELS])
def test_a_failed_candidate_leaves_the_others_alone(factory, kname):
    """Noise -1.0: K is a smooth kernel on 70 points in [0, 1], so K - I is indefinite.  That row reports info != 0,
    f = +inf and a NaN gradient; the other rows are finite and carry the bits they have without the bad candidate
    (the same rows of a batch whose third candidate is a good one)."""
    ev, n_hyp = _evaluator(factory, kname)
    good = _candidates(n_hyp, 3)
    bad = good.clone()
    bad[2, n_hyp] = -1.0
    f0, g0, i0 = (t.cpu().numpy().copy() for t in ev(good))
    f, g, info = (t.cpu().numpy() for t in ev(bad))
    assert info[2] != 0 and f[2] == np.inf and np.isnan(g[2]).all()
    assert not info[:2].any() and np.isfinite(f[:2]).all() and np.isfinite(g[:2]).all()
    assert not i0.any()
    assert f[:2].tobytes() == f0[:2].tobytes() and g[:2].tobytes() == g0[:2].tobytes()


@pytest.mark.parametrize("kname", list(KERNELS))
def test_candidate_refusals_are_the_same_everywhere(kname):
    """Wrong width, wrong dtype, non-contiguous, on the CPU: ValueError, the same text from every evaluator."""
    texts = {}
    for factory in FACTORIES:
        ev, n_hyp = _evaluator(factory, kname)
        w = n_hyp + 1
        good = _candidates(n_hyp, 2)
        wrong = {
            "width": torch.cat([good, good[:, :1]], dim=1).contiguous(),
            "dtype": good.to(torch.float32),
            "strided": torch.cat([good, good], dim=1)[:, :w],
            "cpu": good.cpu(),
        }
        assert not wrong["strided"].is_contiguous()
        for what, cands in wrong.items():
            with pytest.raises(ValueError) as err:
                ev(cands)
            texts.setdefault(what, set()).add(str(err.value))
    assert all(len(t) == 1 for t in texts.values()), texts
    assert len(texts["dtype"] | texts["strided"] | texts["cpu"]) == 1   # (one sentence for the three)


def test_loo_pass_after_a_timed_out_run_loo_returns_what_it_was_asked_for():
    """gpk_tune("chain_force_timeout", 1): the persistent launch of run_loo(LPD, gradient=True) reports a timeout.
    loo(MSE, gradient=False) right after it settles that run first (the re-run records its own LPD results), then
    writes and returns its own buffers: no gradient, and the bits of the same pass on a launch-path factorisation."""
    kd = engine.kernel_descriptor(make_kernel(SE, 1), 1)
    x, y = (_dev(a) for a in _points(N, 1))
    flat = _candidates(kd.n_hyp, 1).reshape(-1)
    operands = (kd, flat, kd.n_hyp + 1, flat[kd.n_hyp:], kd.n_hyp + 1, x, 0, y.reshape(1, -1), 0)
    ref = engine.InverseFactorization(N, 1, 1, torch.float64)
    with nat.thread_tune(chain=0):
        ref.run(*operands, gradient=False)
        want = ref.loo(nat.LOO_MSE, gradient=False)
    f = engine.InverseFactorization(N, 1, 1, torch.float64)
    before = engine.CHAIN_FALLBACKS
    with nat.thread_tune(chain=2):
        nat.tune("chain_force_timeout", 1)
        try:
            f.run_loo(nat.LOO_LPD, *operands, gradient=True)
        finally:
            nat.tune("chain_force_timeout", 0)
        assert f._pending is not None
        got = f.loo(nat.LOO_MSE, gradient=False)
    assert engine.CHAIN_FALLBACKS == before + 1 and f._pending is None
    assert got[1] is None and f.loo_results()[1] is None
    assert not f.info.cpu().numpy().any()
    for a, b in zip((got[0], got[2], got[3]), (want[0], want[2], want[3])):
        assert _bits(a) == _bits(b)
    kept = f.loo_results()   # (the record is the pass's own, too)
    assert all(_bits(got[i]) == _bits(kept[i]) for i in (0, 2, 3))
