"""Sharded hyperparameter sweeps: the multi-GPU form of the LML hot path.

The reference evaluates independent likelihoods in Python loops (k-fold lists,
gpbasics/Optimizer/Fitter.py:27-33 / :97-98; blockwise sub-GPs,
gpbasics/Metrics/LogLikelihood.py:85-104; any user sweep).  Here one process per GPU takes a
contiguous slice of the candidate list, evaluates the slice as ONE batched factorisation
(every launch of gpk_potrf_aug factors all of its members), and a single all-gather of
(nlml, info) pairs -- 16 bytes per candidate over RCCL/xGMI -- gives every rank the full result.
X and y are replicated (each rank holds its own copy); there is no other collective.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.distributed as dist

from . import engine
from . import global_parameters as gp


def shard_range(n_items: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous balanced slice [start, stop) of n_items for rank (the first n % world ranks
    take one extra item)."""
    if world <= 0 or rank < 0 or rank >= world:
        raise ValueError("bad rank/world")
    base, extra = divmod(n_items, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def native_batched_evaluator(kernel, X: torch.Tensor, y: torch.Tensor, noise, dtype=None,
                             max_batch: Optional[int] = None,
                             pipeline: int = 1, mean_function=None) -> Callable[[torch.Tensor], torch.Tensor]:
    """Evaluator running gpk_assemble/gpk_potrf_aug/gpk_finalize over candidate batches.

    Candidates are factored in chunks of ``max_batch`` (all at once when None).  With
    ``pipeline`` = P > 1 the chunks rotate over P factorisation buffers on P HIP streams, so one
    chunk's exposed panel chain overlaps the next chunk's trailing updates (the panel look-ahead
    is then left to the pipelining: each chunk runs its kernels on its own stream).  The result is
    ordered on the caller's stream.

    With a ``mean_function`` the candidate rows are [kernel hyperparameters | mean hyperparameters] (both flat, DFS
    order): each chunk's targets are detrended per candidate by one gpk_mean_eval into a [b, n] buffer
    (allocated on the chunk's stream), which the factorisation reads with a batch stride of n.

    Returns f(cands [c, n_hyp] fp64) -> [c, 2] fp64 device tensor of (nlml, info)."""
    X = engine.as_device_f64(X)
    yv = engine.as_device_f64(y).reshape(1, -1).contiguous()
    n, d = int(X.shape[0]), int(X.shape[1])
    kd = engine.kernel_descriptor(kernel, d)
    n_mean = engine.mean_descriptor(mean_function, d).n_hyp if mean_function is not None else 0
    from .Statistics.CovarianceMatrix import noise_vector
    nv = noise_vector(noise)
    dt = dtype or gp.p_dtype
    cache = {}
    P = max(1, int(pipeline))
    streams = [torch.cuda.Stream(X.device) for _ in range(P - 1)] if P > 1 else []

    def evaluate(cands: torch.Tensor) -> torch.Tensor:
        cands = cands.to(device=X.device, dtype=torch.float64).contiguous()
        c = int(cands.shape[0])
        out = torch.empty((c, 2), dtype=torch.float64, device=X.device)
        if c == 0:
            return out
        if cands.shape[1] != kd.n_hyp + n_mean:
            raise ValueError("candidate rows must have %d hyperparameter values" % (kd.n_hyp + n_mean))
        if n_mean:
            khyp, mhyp = cands[:, :kd.n_hyp].contiguous(), cands[:, kd.n_hyp:].contiguous()
        else:
            khyp = cands
        step = c if max_batch is None else max(1, int(max_batch))
        caller = torch.cuda.current_stream(X.device)
        slots = [caller] + streams
        for st in streams:
            st.wait_stream(caller)
        # the chunks' factorisations overlap on P streams: no look-ahead side streams, no panel solve fused
        # into the diagonal-block launch (its redundant workgroups would take CUs from the other chunks'
        # updates: C5 38.2 -> 36.4 evals/s at 3 in flight) and no persistent launch (it would claim every
        # CU) -- pinned for this thread's calls only (gpk_tune_thread), not for other threads
        from . import _native as nat
        knobs = nat.thread_tune(lookahead=0, fuse_trsm=0, chain=0) if P > 1 else nat.thread_tune()
        with knobs:
            for i, s0 in enumerate(range(0, c, step)):
                s1 = min(c, s0 + step)
                b = s1 - s0
                slot = i % P
                f = cache.get((b, slot))
                if f is None:
                    f = engine.AugmentedFactorization(n, d, 0, b, dt)
                    cache[(b, slot)] = f
                with torch.cuda.stream(slots[slot]):
                    if n_mean:
                        # (a fresh [b, n] buffer per chunk: the stream-ordered caching allocator keeps it until the
                        # slot's stream has passed the factorisation that reads it)
                        yd = engine.mean_vector(mean_function, mhyp[s0:s1], X, yv[0])
                        f.run(kd, khyp[s0:s1], kd.n_hyp, nv, 0, X, 0, yd, n)
                    else:
                        f.run(kd, khyp[s0:s1], kd.n_hyp, nv, 0, X, 0, yv, 0)
                    out[s0:s1, 0] = f.nlml()
                    out[s0:s1, 1] = f.info.to(torch.float64)
        for st in streams:
            caller.wait_stream(st)
        return out

    return evaluate


def _check_candidates(cands: torch.Tensor, width: int, dev) -> None:
    if cands.dim() != 2 or int(cands.shape[1]) != width:
        raise ValueError("candidate rows must have %d values (hyperparameters, then the noise)" % width)
    if cands.dtype != torch.float64 or cands.device != dev or not cands.is_contiguous():
        raise ValueError("candidates must be a contiguous float64 tensor on %s" % (dev,))


def _value_and_gradient(dev, width: int, make, run, kind: str = "nlml", n_folds: Optional[int] = None):
    """The core of every native_*_value_and_gradient factory: f(cands [B, width] fp64 on ``dev``, the noise last,
    settle=False) -> (f [B], g [B, width], info [B] int32) with ``.n_par`` (and ``.n_folds``).

    ``make(B)`` builds what a batch of B candidates needs -- a factorisation of engine, or a tuple starting with one;
    it is kept per B and reused.  ``run(state, hyp, hyp_stride, noise, noise_stride)`` enqueues one evaluation on it
    and returns the factorisation, whose ``results(kind, settle)`` are the return value: unsettled views by default
    (enqueue only, no host synchronisation), settled ones with ``settle=True`` (one 4-byte read-back, and only after
    a persistent run; engine.AugmentedFactorization.results).  Candidate rows are read in place: the noise operand
    is the same buffer from element width - 1 on (the last member's noise is its last element).  With ``n_folds``
    = F the batch is S * F ragged members: the rows are replicated on the device (:func:`replicate_candidates`) and
    the folds reduced in a fixed order (:func:`fold_mean`, :func:`fold_info`)."""
    from . import _native as nat
    cache = {}

    def evaluate(cands: torch.Tensor, settle: bool = False):
        _check_candidates(cands, width, dev)
        B = int(cands.shape[0])
        state = cache.get(B)
        if state is None:
            state = cache[B] = make(B)
        if n_folds is None:
            flat = cands.reshape(-1)
            fac = run(state, flat, width, flat[width - 1:], width)
            return fac.results(kind, settle)
        hyp, noise = replicate_candidates(cands, n_folds, nat.MAX_HYP)
        f, g, info = run(state, hyp, nat.MAX_HYP, noise, 1).results(kind, settle)
        return fold_mean(f, n_folds), fold_mean(g, n_folds), fold_info(info, n_folds)

    evaluate.n_par = width
    if n_folds is not None:
        evaluate.n_folds = n_folds
    return evaluate


def native_batched_value_and_gradient(kernel, X: torch.Tensor, y: torch.Tensor, dtype=None):
    """-LML and its gradient for a batch of (hyperparameters, noise) candidates by ONE identity-augmented batched
    factorisation per call (gpk_nlml_grad) -- the evaluation a multi-start fitter repeats (Optimizer.Fitter).

    Returns f(cands [B, n_hyp + 1] fp64 on the device, the noise last) -> (f [B], g [B, n_hyp + 1], info [B] int32):
    device tensors, views of the factorisation's read-out and gradient buffers (a new pair per call: earlier views
    stay valid).  One engine.InverseFactorization per batch size is kept and reused; candidate rows are read in place
    (hyp_stride = noise_stride = n_hyp + 1).

    The call only enqueues: no host synchronisation.  A run that took the persistent launch is NOT settled by a plain
    call (engine.CHAIN_VERIFY defers that to the first settled read, which these views bypass): a wait that timed out
    shows as info = -1 for its members, which a fitter treats as a failed trial.  ``f(cands, settle=True)`` reads the
    settled results instead: a persistent run is then verified (one 4-byte read-back, which waits for it) and, had it
    timed out, run again on the launch path before the views are returned; a run on the launch path has nothing to
    verify and does not synchronise.  A fitter settles the evaluations it is about to synchronise on anyway, and the
    first one."""
    X = engine.as_device_f64(X)
    yv = engine.as_device_f64(y).reshape(1, -1).contiguous()
    n, d = int(X.shape[0]), int(X.shape[1])
    if int(yv.shape[1]) != n:
        raise ValueError("y has %d values, X has %d points" % (int(yv.shape[1]), n))
    kd = engine.kernel_descriptor(kernel, d)
    dt = dtype or gp.p_dtype
    return _value_and_gradient(X.device, kd.n_hyp + 1, lambda B: engine.InverseFactorization(n, d, B, dt),
                               lambda f, h, hs, nz, ns: f.run(kd, h, hs, nz, ns, X, 0, yv, 0, gradient=True))


def replicate_candidates(cands: torch.Tensor, n_folds: int, width: int):
    """Candidate rows [S, n_hyp + 1] (the noise last) -> (hyp [S * F, width] zero-filled past n_hyp, noise [S * F]):
    member s * F + f is candidate s on fold f.  Tensor ops on the candidates' device only (no host round trip)."""
    S, n_hyp = int(cands.shape[0]), int(cands.shape[1]) - 1
    hyp = torch.zeros((S * n_folds, width), dtype=cands.dtype, device=cands.device)
    hyp[:, :n_hyp] = cands[:, :n_hyp].repeat_interleave(n_folds, dim=0)
    noise = cands[:, n_hyp].repeat_interleave(n_folds).contiguous()
    return hyp, noise


def fold_mean(values: torch.Tensor, n_folds: int) -> torch.Tensor:
    """Mean over the folds of per-member values [S * F] or [S * F, k] (member s * F + f): the folds are added in fold
    order, one after the other, then divided by F -- a fixed order, the same bits on every call."""
    v = values.reshape((-1, n_folds) + tuple(values.shape[1:]))
    acc = v[:, 0]
    for f in range(1, n_folds):
        acc = acc + v[:, f]
    return acc / float(n_folds)


def fold_info(info: torch.Tensor, n_folds: int) -> torch.Tensor:
    """[S] int32: non-zero where any fold's info is (the largest magnitude among the candidate's folds)."""
    return info.reshape(-1, n_folds).abs().amax(dim=1).to(torch.int32)


def _pack_folds(folds, with_test: bool):
    """Folds of device tensors (X_f [n_f, d], y_f [n_f][, Xs_f [m_f, d], ys_f [m_f]]) -> [Xf [F, n, d], yf [F, n]
    (, Xsf [F, m, d], ysf [F, m])] with n / m the largest fold's counts, zero-filled past each fold's own."""
    def pad(parts):
        out = torch.zeros((len(parts), max(int(t.shape[0]) for t in parts)) + tuple(parts[0].shape[1:]),
                          dtype=torch.float64, device=parts[0].device)
        for k, t in enumerate(parts):
            out[k, :int(t.shape[0])] = t
        return out
    columns = list(zip(*folds))   # (every fold's X, every fold's y[, every fold's Xs, every fold's ys])
    return [pad(parts) for parts in columns[:4 if with_test else 2]]


def _replicate(packed, S: int):
    """The packed fold operands [F, ...] tiled to the S * F members of S candidates (member s * F + f: fold f)."""
    return [t.repeat((S,) + (1,) * (t.dim() - 1)).contiguous() for t in packed]


def native_kfold_value_and_gradient(kernel, folds, dtype=None):
    """Mean over k folds of -LML and of its gradient for a batch of (hyperparameters, noise) candidates: the reference's
    opt_kfold / opt_optimize_noise_kfold objective (gpbasics/Optimizer/Fitter.py:97-102) under its tape, as ONE ragged
    identity-augmented batch of S * F members per call (engine.RaggedInverseFactorization -> gpk_grad_ragged).  The
    folds of Metrics/CrossValidation.get_data_inputs differ in n_train whenever n is not divisible by k, which a uniform
    batch cannot take.

    ``folds``: a list of (X_f [n_f, d], y_f [n_f]).  Returns f(cands [S, n_hyp + 1] fp64 on the device, the noise last)
    -> (f [S], g [S, n_hyp + 1], info [S] int32): device tensors; f is +inf and g NaN where any fold's factorisation
    failed (info non-zero).  Candidate rows are replicated to the members on the device (:func:`replicate_candidates`)
    and the folds reduced in a fixed order (:func:`fold_mean`).  The call only enqueues: no host synchronisation
    (``settle`` is accepted for the signature of native_batched_value_and_gradient: ragged batches never take the
    persistent launch, so there is nothing to verify)."""
    folds = [(engine.as_device_f64(X), engine.as_device_f64(y).reshape(-1)) for X, y in folds]
    if not folds:
        raise ValueError("at least one fold is needed")
    F = len(folds)
    d = int(folds[0][0].shape[1])
    sizes = []
    for X, y in folds:
        if X.dim() != 2 or int(X.shape[1]) != d or int(y.numel()) != int(X.shape[0]) or int(X.shape[0]) < 1:
            raise ValueError("every fold needs X [n_f >= 1, %d] and y with n_f values" % d)
        sizes.append(int(X.shape[0]))
    kd = engine.kernel_descriptor(kernel, d)
    dt = dtype or gp.p_dtype
    packed = _pack_folds(folds, False)

    def make(S):
        Xp, yp = _replicate(packed, S)
        return engine.RaggedInverseFactorization(sizes * S, d, dt), [kd] * (S * F), Xp, yp

    def run(state, hyp, hyp_stride, noise, noise_stride):   # (packed operands: the strides are the layout's own)
        fac, kds, Xp, yp = state
        return fac.run_packed(kds, hyp, noise, Xp, yp, gradient=True)

    return _value_and_gradient(folds[0][0].device, kd.n_hyp + 1, make, run, n_folds=F)


def _check_mse_shapes(X, y, Xs, ys, d=None):
    """Host-only shape check of one (X, y, X_test, y_test) quadruple; returns (n, m, d)."""
    if X.dim() != 2 or Xs.dim() != 2 or int(X.shape[0]) < 1:
        raise ValueError("X must be [n >= 1, d] and X_test [m, d]")
    n, dd, m = int(X.shape[0]), int(X.shape[1]), int(Xs.shape[0])
    if int(Xs.shape[1]) != dd or (d is not None and dd != d):
        raise ValueError("X and X_test must share the dimension %d" % (dd if d is None else d))
    if m < 1:
        raise ValueError("the MSE needs at least one test point")
    if int(y.numel()) != n:
        raise ValueError("y has %d values, X has %d points" % (int(y.numel()), n))
    if int(ys.numel()) != m:
        raise ValueError("y_test has %d values, X_test has %d points" % (int(ys.numel()), m))
    return n, m, dd


def _as_tensor(t) -> torch.Tensor:
    return t if isinstance(t, torch.Tensor) else torch.as_tensor(t)


def native_batched_mse_value_and_gradient(kernel, X: torch.Tensor, y: torch.Tensor, Xs: torch.Tensor,
                                          ys: torch.Tensor):
    """Held-out MSE mean((K_s^T (K + noise I)^-1 y - y_test)^2) and its gradient for a batch of (hyperparameters,
    noise) candidates by ONE batched factorisation with the test points as extra rows per call (gpk_mse_grad) -- the
    n^3/3 factorisation, not the identity-augmented n^3 one of the -LML gradient.

    Returns f(cands [B, n_hyp + 1] fp64 on the device, the noise last, settle=False) -> (f [B], g [B, n_hyp + 1],
    info [B] int32): the contract of :func:`native_batched_value_and_gradient` -- ``.n_par``, candidate rows read in
    place, enqueue only, ``settle=True`` reads the settled results (a persistent run is then verified and, had it
    timed out, run again on the launch path).  fp64 only."""
    n, m, d = _check_mse_shapes(_as_tensor(X), _as_tensor(y), _as_tensor(Xs), _as_tensor(ys))
    X, Xs = engine.as_device_f64(X).contiguous(), engine.as_device_f64(Xs).contiguous()
    yv = engine.as_device_f64(y).reshape(1, -1).contiguous()
    ysv = engine.as_device_f64(ys).reshape(1, -1).contiguous()
    kd = engine.kernel_descriptor(kernel, d)
    return _value_and_gradient(X.device, kd.n_hyp + 1,
                               lambda B: engine.AugmentedFactorization(n, d, m, B, torch.float64),
                               lambda f, h, hs, nz, ns: f.run_mse(kd, h, hs, nz, ns, X, 0, yv, 0, Xs, 0, ysv, 0),
                               kind="mse")


def native_batched_loo_value_and_gradient(kernel, X: torch.Tensor, y: torch.Tensor, loss, dtype=None):
    """Leave-one-out objective (``loss``: _native.LOO_LPD, minus the LOO log predictive density, or _native.LOO_MSE)
    and its gradient for a batch of (hyperparameters, noise) candidates by ONE batched identity-augmented factorisation
    plus the LOO pass per call (gpk_loo_grad) -- the factorisation of the -LML gradient, then one n^3 product for the
    cotangent.

    Returns f(cands [B, n_hyp + 1] fp64 on the device, the noise last, settle=False) -> (f [B], g [B, n_hyp + 1],
    info [B] int32): the contract of :func:`native_batched_value_and_gradient` -- ``.n_par``, candidate rows read in
    place, enqueue only, ``settle=True`` reads the settled results (a persistent run is then verified and, had it
    timed out, run again on the launch path).  fp64 only (``dtype``: None or torch.float64)."""
    from . import _native as nat
    if dtype not in (None, torch.float64):
        raise NotImplementedError("leave-one-out is fp64 only")
    code = nat.loo_loss_code(loss)
    if _as_tensor(X).dim() != 2 or int(_as_tensor(X).shape[0]) < 1:
        raise ValueError("X must be [n >= 1, d]")
    n, d = int(_as_tensor(X).shape[0]), int(_as_tensor(X).shape[1])
    if int(_as_tensor(y).numel()) != n:
        raise ValueError("y has %d values, X has %d points" % (int(_as_tensor(y).numel()), n))
    X = engine.as_device_f64(X).contiguous()
    yv = engine.as_device_f64(y).reshape(1, -1).contiguous()
    kd = engine.kernel_descriptor(kernel, d)
    return _value_and_gradient(X.device, kd.n_hyp + 1,
                               lambda B: engine.InverseFactorization(n, d, B, torch.float64),
                               lambda f, h, hs, nz, ns: f.run_loo(code, kd, h, hs, nz, ns, X, 0, yv, 0, gradient=True),
                               kind="loo")


def native_kfold_mse_value_and_gradient(kernel, folds):
    """Mean over k folds of the held-out MSE and of its gradient for a batch of (hyperparameters, noise) candidates:
    the gradient of what CrossValidation(metric_type=MSE) evaluates, as ONE ragged batch of S * F members per call
    (engine.RaggedFactorization.run_mse_packed -> gpk_mse_grad with n_dev / m_dev).  The folds of
    Metrics/CrossValidation.get_data_inputs differ in n_train and n_test whenever n is not divisible.

    ``folds``: a list of (X_f [n_f, d], y_f [n_f], Xs_f [m_f >= 1, d], ys_f [m_f]).  Returns f(cands [S, n_hyp + 1],
    settle=False) -> (f [S], g [S, n_hyp + 1], info [S] int32) as :func:`native_kfold_value_and_gradient`: every fold
    contributes its own MSE, the folds are reduced in a fixed order (:func:`fold_mean`, :func:`fold_info`); f is +inf
    and g NaN where any fold's factorisation failed.  Enqueue only (ragged batches never take the persistent launch:
    ``settle`` has nothing to verify)."""
    if not folds:
        raise ValueError("at least one fold is needed")
    d, sizes, tsizes = None, [], []
    for fold in folds:
        if len(fold) != 4:
            raise ValueError("every fold is (X, y, X_test, y_test)")
        nf, mf, d = _check_mse_shapes(*[_as_tensor(t) for t in fold], d=d)
        sizes.append(nf)
        tsizes.append(mf)
    folds = [(engine.as_device_f64(X), engine.as_device_f64(y).reshape(-1), engine.as_device_f64(Xs),
              engine.as_device_f64(ys).reshape(-1)) for X, y, Xs, ys in folds]
    kd = engine.kernel_descriptor(kernel, d)
    packed = _pack_folds(folds, True)

    def make(S):
        Xp, yp, Xsp, ysp = _replicate(packed, S)
        return engine.RaggedFactorization(sizes * S, d, tsizes * S, torch.float64), Xp, yp, Xsp, ysp

    def run(state, hyp, hyp_stride, noise, noise_stride):   # (packed operands: the strides are the layout's own)
        fac, Xp, yp, Xsp, ysp = state
        return fac.run_mse_packed(kd, hyp, noise, Xp, yp, Xsp, ysp)

    return _value_and_gradient(folds[0][0].device, kd.n_hyp + 1, make, run, kind="mse", n_folds=len(folds))


class HyperparameterSweep:
    """Evaluate -LML for every row of a candidate matrix across the ranks of ``group``.

    ``evaluator(cands [c, n_hyp]) -> [c, 2]`` (nlml, info); by default the native batched
    device evaluator.  Works with world size 1 and without an initialised process group."""

    def __init__(self, evaluator: Callable[[torch.Tensor], torch.Tensor], group=None,
                 comm_device: Optional[torch.device] = None):
        self.evaluator = evaluator
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.world = dist.get_world_size(group) if self.distributed else 1
        if comm_device is None:
            backend = dist.get_backend(group) if self.distributed else "none"
            comm_device = engine.device() if backend == "nccl" else torch.device("cpu")
        self.comm_device = comm_device

    def local_slice(self, n_candidates: int) -> Tuple[int, int]:
        return shard_range(n_candidates, self.rank, self.world)

    def run(self, candidates: torch.Tensor):
        """Returns (nlml [C], info [C] int32, argmin index) on every rank."""
        C = int(candidates.shape[0])
        s0, s1 = self.local_slice(C)
        local = self.evaluator(candidates[s0:s1])
        if not self.distributed or self.world == 1:
            allv = local.to(self.comm_device)
        else:
            chunk = -(-C // self.world)
            buf = torch.full((chunk, 2), float("nan"), dtype=torch.float64, device=self.comm_device)
            buf[:s1 - s0] = local.to(self.comm_device)
            gathered = torch.empty((self.world * chunk, 2), dtype=torch.float64, device=self.comm_device)
            dist.all_gather_into_tensor(gathered, buf, group=self.group)
            parts = []
            for r in range(self.world):
                a, b = shard_range(C, r, self.world)
                parts.append(gathered[r * chunk:r * chunk + (b - a)])
            allv = torch.cat(parts, dim=0)
        nlml = allv[:, 0]
        info = allv[:, 1].to(torch.int32)
        masked = torch.where(info == 0, nlml, torch.full_like(nlml, float("inf")))
        best = int(torch.argmin(masked).item()) if C else -1
        return nlml, info, best
