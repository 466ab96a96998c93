"""Device engine: the glue between the gpbasics-style Python objects and libgpk.

* :func:`kernel_descriptor` flattens a kernel tree (KernelBasics) into the postfix program the
  HIP kernels evaluate (include/gpk.h, ``gpk_kdesc``).
* :func:`pack_hyper_parameter` concatenates a hyperparameter list in DFS order, the layout of
  ``Component.serialize_hyper_parameter`` (gpbasics/Auxiliary/BasicGPComponent.py:16-23).
* :class:`AugmentedFactorization` owns the device buffers of one factorisation of the augmented
  matrix (training block + optional extra rows + the y row) and reads results out of it.

All arithmetic runs in libgpk on the GPU; torch only allocates and views device memory.
"""
from __future__ import annotations

import ctypes
import functools
import logging
import os
from typing import List, Optional, Sequence

import torch

from . import _native as nat
from . import global_parameters as gp

# A single f64 factorisation may run as ONE persistent launch (gpk_tune "chain", include/gpk.h).  Its
# inter-workgroup waits are bounded; a wait that times out (the device shared with another process past
# chain_timeout_ms, a preempted workgroup) leaves info = -1 and the factorisation incomplete.  With
# CHAIN_VERIFY (default) a run that took the persistent launch is verified lazily: run() itself never
# synchronises (calls enqueue ahead of the device), and the FIRST read of its results -- info, out, W and every
# read-out accessor -- reads info back (one 4-byte device-to-host copy, which waits for that run) and, on -1,
# assembles and factors again on the launch path, on the run's own stream, before returning; CHAIN_FALLBACKS
# counts those re-runs.  (The re-run reads the operands passed to run(): they must not be overwritten in
# between.)  The reference's tf.linalg.cholesky never fails spuriously
# (gpbasics/Statistics/CovarianceMatrix.py:250), so neither may this.
CHAIN_VERIFY = True
CHAIN_FALLBACKS = 0


class CholeskyError(RuntimeError):
    """Cholesky of K + noise*I failed (not positive definite).  The reference propagates
    TensorFlow's InvalidArgumentError from tf.linalg.cholesky
    (gpbasics/Statistics/CovarianceMatrix.py:250)."""

    def __init__(self, info):
        super().__init__("Cholesky decomposition was not successful: leading minor of order %s is "
                         "not positive definite" % (info,))
        self.info = info


def device() -> torch.device:
    d = torch.device(gp.p_device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def as_device_f64(x) -> torch.Tensor:
    """fp64 device copy/view of array-like x (the reference casts every input to p_dtype=fp64,
    gpbasics/DataHandling/DataInput.py:198-206)."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        t = torch.as_tensor(x)
    return t.to(device=device(), dtype=torch.float64).contiguous()


# ----------------------------------------------------------------------------- kernel programs
def kernel_descriptor(kernel, dim: Optional[int] = None) -> nat.GpkKdesc:
    """Flatten ``kernel`` (a Kernel tree) to the postfix program of include/gpk.h."""
    dim = int(dim if dim is not None else kernel.get_dimensionality())
    nodes: List[tuple] = []
    slots: List[int] = []
    n_hyp = kernel._emit(nodes, 0, slots, dim)
    if len(nodes) > nat.MAX_NODES:
        raise ValueError("kernel tree too large for the device program (%d > %d nodes)"
                         % (len(nodes), nat.MAX_NODES))
    if len(slots) > nat.MAX_ARD:
        raise ValueError("at most %d ARD base kernels per tree" % nat.MAX_ARD)
    if n_hyp > nat.MAX_HYP:
        raise ValueError("too many hyperparameters (%d > %d)" % (n_hyp, nat.MAX_HYP))
    if dim < 1 or dim > nat.MAX_DIM:
        raise ValueError("input dimensionality must be in [1, %d]" % nat.MAX_DIM)
    kd = nat.GpkKdesc()
    kd.n_nodes = len(nodes)
    kd.n_hyp = n_hyp
    kd.dim = dim
    kd.n_ard = len(slots)
    for i, (op, off, slot, flags) in enumerate(nodes):
        kd.nodes[i].op = op
        kd.nodes[i].hyp_offset = off
        kd.nodes[i].ard_slot = slot
        kd.nodes[i].flags = flags
    return kd


# small host values (hyperparameters, noise) reach the device through one asynchronous copy from pinned memory
# (torch's caching host allocator keeps the block until the copy is done) instead of a synchronous pageable copy
# per tensor; GPK_PINNED_H2D=0 restores the plain copy (A/B)
PINNED_H2D = os.environ.get("GPK_PINNED_H2D", "1") != "0"


def host_f64_to_device(values) -> torch.Tensor:
    """fp64 device vector of a short list of host floats (asynchronous, stream-ordered on the current stream)."""
    t = torch.tensor(values, dtype=torch.float64)
    dev = device()
    if PINNED_H2D and dev.type == "cuda":
        return t.pin_memory().to(dev, non_blocking=True)
    return t.to(dev)


def _host_values(hyper_parameter: Sequence) -> Optional[List[float]]:
    """The flat host floats of a hyperparameter list, or None if an entry lives on the device."""
    for h in hyper_parameter:
        if isinstance(h, torch.Tensor) and h.device.type != "cpu":
            return None
    vals: List[float] = []
    for h in hyper_parameter:
        if isinstance(h, torch.Tensor):
            vals.extend(float(v) for v in h.detach().reshape(-1).tolist())
        else:
            try:
                vals.extend(float(v) for v in h)
            except TypeError:
                vals.append(float(h))
    return vals


def pack_hyper_parameter_and_noise(hyper_parameter: Sequence, noise, n_expected: int):
    """(hyperparameter vector, 1-element noise vector) on the device; when both are host values, through ONE
    asynchronous copy (one buffer, two views) instead of one per operand.  noise None: the caller's own."""
    host_noise = not isinstance(noise, torch.Tensor) or (noise.device.type == "cpu" and not noise.requires_grad)
    vals = _host_values(hyper_parameter) if host_noise and not (
        isinstance(hyper_parameter, torch.Tensor) and hyper_parameter.dim() == 1) else None
    if vals is None:
        return pack_hyper_parameter(hyper_parameter, n_expected), None
    if len(vals) != n_expected:
        raise ValueError("hyperparameter vector has %d values, kernel expects %d" % (len(vals), n_expected))
    t = host_f64_to_device(vals + [float(noise)])
    return t[:n_expected], t[n_expected:]


def pack_hyper_parameter(hyper_parameter: Sequence, n_expected: Optional[int] = None) -> torch.Tensor:
    """Flat fp64 device vector of a hyperparameter list (each entry reshaped to [-1], concatenated;
    BasicGPComponent.serialize_hyper_parameter, gpbasics/Auxiliary/BasicGPComponent.py:16-23)."""
    dev = device()
    if isinstance(hyper_parameter, torch.Tensor) and hyper_parameter.dim() == 1:
        flat = hyper_parameter.to(device=dev, dtype=torch.float64)
    else:
        parts = []
        host_vals = _host_values(hyper_parameter)
        if host_vals is not None:
            flat = host_f64_to_device(host_vals)
        else:
            for h in hyper_parameter:
                parts.append(torch.as_tensor(h).to(device=dev, dtype=torch.float64).reshape(-1))
            flat = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64, device=dev)
    if n_expected is not None and flat.numel() != n_expected:
        raise ValueError("hyperparameter vector has %d values, kernel expects %d"
                         % (flat.numel(), n_expected))
    return flat.contiguous()


def kernel_matrix(kernel, hyper_parameter, x, x_, diag_add: float = 0.0, lower: bool = False,
                  out_dtype=None) -> torch.Tensor:
    """k(x, x_) as an [n, m] device tensor via gpk_kernel_matrix (K/Kernel.py:51-52)."""
    L = nat.lib()
    x = as_device_f64(x)
    x_ = as_device_f64(x_)
    if x.dim() != 2 or x_.dim() != 2 or x.shape[1] != x_.shape[1]:
        raise ValueError("kernel inputs must be [n, D] and [m, D]")
    kd = kernel_descriptor(kernel, x.shape[1])
    hyp = pack_hyper_parameter(hyper_parameter, kd.n_hyp)
    dt = out_dtype or torch.float64
    n, m = x.shape[0], x_.shape[0]
    K = torch.empty((n, m), dtype=dt, device=x.device)
    if n == 0 or m == 0:
        return K
    nat.check(L.gpk_kernel_matrix(ctypes.byref(kd), nat.ptr(hyp), nat.dtype_code(dt), 1 if lower else 0,
                                  nat.ptr(x), n, nat.ptr(x_), m, x.shape[1], float(diag_add),
                                  nat.ptr(K), m, nat.stream_handle(x.device)), "gpk_kernel_matrix")
    return K


# ----------------------------------------------------------------------------- mean programs
def mean_descriptor(mean_function, dim: Optional[int] = None) -> nat.GpkMdesc:
    """Flatten ``mean_function`` (a MeanFunction tree) to the postfix mean program of include/gpk.h."""
    dim = int(dim if dim is not None else mean_function.input_dimensionality)
    if not nat.mean_op_supported(nat.MOP_LIN):
        raise nat.NativeUnavailable("this libgpk.so has no mean-function programs (stale build): rebuild it with "
                                    "__graft_entry__.build()")
    if dim < 1 or dim > nat.MAX_DIM:
        raise ValueError("input dimensionality must be in [1, %d]" % nat.MAX_DIM)
    nodes: List[tuple] = []
    n_hyp = mean_function._emit(nodes, 0, dim)
    if len(nodes) > nat.MAX_NODES:
        raise ValueError("mean-function tree too large for the device program (%d > %d nodes)"
                         % (len(nodes), nat.MAX_NODES))
    if n_hyp > nat.MAX_HYP:
        raise ValueError("too many mean hyperparameters (%d > %d)" % (n_hyp, nat.MAX_HYP))
    md = nat.GpkMdesc()
    md.n_nodes = len(nodes)
    md.n_hyp = n_hyp
    md.dim = dim
    md.reserved = 0
    for i, (op, off, slot, flags) in enumerate(nodes):
        md.nodes[i].op = op
        md.nodes[i].hyp_offset = off
        md.nodes[i].ard_slot = slot
        md.nodes[i].flags = flags
    return md


def _mean_operands(mean_function, hyper_parameter, x):
    """(md, hyp, hyp_stride, X, x_bstride, n, batch or None): ``x`` [n, d] or [B, n, d]; ``hyper_parameter`` a
    hyperparameter list / flat vector (shared by the members) or a [B, n_hyp] matrix (one row per member)."""
    x = as_device_f64(x)
    if x.dim() not in (2, 3):
        raise ValueError("mean-function inputs must be [n, D] or [B, n, D]")
    n, d = int(x.shape[-2]), int(x.shape[-1])
    md = mean_descriptor(mean_function, d)
    if isinstance(hyper_parameter, torch.Tensor) and hyper_parameter.dim() == 2:
        hyp = hyper_parameter.detach().to(device=x.device, dtype=torch.float64).contiguous()
        if hyp.shape[1] != md.n_hyp:
            raise ValueError("hyperparameter rows have %d values, the mean function expects %d"
                             % (hyp.shape[1], md.n_hyp))
        hb = int(hyp.shape[0])
    else:
        hyp, hb = pack_hyper_parameter(hyper_parameter, md.n_hyp), None
    xb = int(x.shape[0]) if x.dim() == 3 else None
    if hb is not None and xb is not None and hb != xb:
        raise ValueError("%d hyperparameter rows for %d input members" % (hb, xb))
    batch = hb if hb is not None else xb
    return md, hyp, (md.n_hyp if hb is not None else 0), x, (n * d if xb is not None else 0), n, batch


def mean_vector(mean_function, hyper_parameter, x, y=None) -> torch.Tensor:
    """m(x) -- or, with targets ``y``, the detrended targets y - m(x) -- by gpk_mean_eval: [n], or [B, n] when the
    inputs ([B, n, d]), the hyperparameters ([B, n_hyp]) or the targets ([B, n] / [B, n, 1]) carry a batch.
    The reference's MeanFunction.get_tf_tensor and DataInput.get_detrended_y_* (DataHandling/DataInput.py:244-264)."""
    L = nat.lib()
    md, hyp, hyp_stride, X, x_bstride, n, batch = _mean_operands(mean_function, hyper_parameter, x)
    yv, y_bstride = None, 0
    if y is not None:
        yv = as_device_f64(y)
        if yv.dim() >= 2 and yv.shape[-1] == 1 and yv.shape[-2] == n:
            yv = yv.reshape(yv.shape[:-1])
        if yv.dim() == 2:
            if batch is not None and int(yv.shape[0]) != batch:
                raise ValueError("%d target members for a batch of %d" % (yv.shape[0], batch))
            batch, y_bstride = int(yv.shape[0]), n
        if yv.dim() not in (1, 2) or int(yv.shape[-1]) != n:
            raise ValueError("targets must hold %d values per member" % n)
        yv = yv.contiguous()
    B = batch or 1
    out = torch.empty((B, n), dtype=torch.float64, device=X.device)
    if n > 0:
        nat.check(L.gpk_mean_eval(ctypes.byref(md), nat.ptr(hyp), hyp_stride, nat.ptr(X), n, x_bstride, B,
                                  nat.ptr(yv), y_bstride, nat.ptr(out), n, nat.stream_handle(X.device)),
                  "gpk_mean_eval")
    return out if batch is not None else out[0]


def mean_vjp(mean_function, hyper_parameter, x, g: torch.Tensor) -> torch.Tensor:
    """sum_i g_i dm(x_i) / d(hyperparameters) by gpk_mean_vjp: the flat adjoint [n_hyp] (DFS order), or [B, n_hyp]
    for batched operands (see :func:`mean_vector`; ``g`` [n] or [B, n]).  A float64 ``g`` whose rows are contiguous
    is read where it lies, whatever its batch stride -- e.g. the -alpha rows of an identity-augmented factorisation
    (:meth:`InverseFactorization.neg_alpha_rows`)."""
    L = nat.lib()
    md, hyp, hyp_stride, X, x_bstride, n, batch = _mean_operands(mean_function, hyper_parameter, x)
    g = g.detach()
    if g.dim() >= 2 and g.shape[-1] == 1 and g.shape[-2] == n:
        g = g.reshape(g.shape[:-1])
    if g.dim() not in (1, 2) or int(g.shape[-1]) != n:
        raise ValueError("g must hold %d weights per member" % n)
    if g.dim() == 2:
        if batch is not None and int(g.shape[0]) != batch:
            raise ValueError("%d weight members for a batch of %d" % (g.shape[0], batch))
        batch = int(g.shape[0])
    if g.dtype != torch.float64 or g.device != X.device or g.stride(-1) != 1 or (g.dim() == 2 and g.stride(0) < 0):
        g = g.to(device=X.device, dtype=torch.float64).contiguous()
    g_bstride = int(g.stride(0)) if g.dim() == 2 else 0
    B = batch or 1
    grad = torch.zeros((B, md.n_hyp), dtype=torch.float64, device=X.device)
    if n > 0:
        wb = int(L.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), n, B))
        work = torch.empty(max(1, (wb + 7) // 8), dtype=torch.float64, device=X.device)
        nat.check(L.gpk_mean_vjp(ctypes.byref(md), nat.ptr(hyp), hyp_stride, nat.ptr(X), n, x_bstride, B, nat.ptr(g),
                                 g_bstride, nat.ptr(grad), nat.ptr(work), wb, nat.stream_handle(X.device)),
                  "gpk_mean_vjp")
    return grad if batch is not None else grad[0]


class _MeanValue(torch.autograd.Function):
    """m(x) with the device reverse mode: autograd through a mean function's get_tf_tensor, as the reference's
    tape differentiates it (Optimizer/Fitter.py:104-158)."""

    @staticmethod
    def forward(ctx, mean_function, x, *hyper_parameter):
        ctx.mean_function, ctx.x = mean_function, x
        ctx.like = [(h.shape, h.device, h.dtype) for h in hyper_parameter]
        ctx.flat = pack_hyper_parameter([h.detach() for h in hyper_parameter])
        return mean_vector(mean_function, ctx.flat, x)

    @staticmethod
    def backward(ctx, gout):
        flat = mean_vjp(ctx.mean_function, ctx.flat, ctx.x, gout.contiguous())
        grads, i = [], 0
        for shape, dev, dt in ctx.like:
            k = 1
            for s in shape:
                k *= int(s)
            grads.append(flat[i:i + k].reshape(shape).to(device=dev, dtype=dt))
            i += k
        return (None, None) + tuple(grads)


def mean_tensor(mean_function, hyper_parameter: Sequence, x) -> torch.Tensor:
    """get_tf_tensor of the device mean functions: [n] fp64, differentiable in the hyperparameters when one of
    them requires a gradient (the backward pass is gpk_mean_vjp)."""
    hs = list(hyper_parameter)
    if torch.is_grad_enabled() and any(isinstance(h, torch.Tensor) and h.requires_grad for h in hs):
        return _MeanValue.apply(mean_function, x, *[h if isinstance(h, torch.Tensor)
                                                    else torch.as_tensor(h, dtype=torch.float64) for h in hs])
    return mean_vector(mean_function, hs, x)


# ----------------------------------------------------------------------------- factorisation
def _check_operand(name: str, t: torch.Tensor, bstride: int, per_member: int, batch: int,
                   dev: torch.device) -> None:
    if t is None:
        raise ValueError("%s is required" % name)
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev:
        raise ValueError("%s must be a contiguous float64 tensor on %s (got %s, %s, contiguous=%s)"
                         % (name, dev, t.dtype, t.device, t.is_contiguous()))
    need = (batch - 1) * int(bstride) + int(per_member) if batch > 0 else 0
    if int(bstride) < 0 or t.numel() < need:
        raise ValueError("%s holds %d elements, the layout reads %d (batch %d, stride %d, %d per member)"
                         % (name, t.numel(), need, batch, bstride, per_member))


class AugmentedFactorization:
    """One factorisation of the augmented matrix W (include/gpk.h) for ``batch`` problems.

    After :meth:`run`, W's first n_pad columns hold L, the y row holds z = L^-1 y, the extra rows
    hold V^T = Ks^T L^-T and the corner holds the Schur complement (posterior covariance,
    -posterior mean, -z^T z).
    """

    def __init__(self, n: int, d: int, m: int = 0, batch: int = 1, dtype=None):
        self.L = nat.lib()
        self.dtype = dtype or gp.p_dtype
        self.code = nat.dtype_code(self.dtype)
        self.n, self.d, self.m, self.batch = int(n), int(d), int(m), int(batch)
        self.layout = nat.plan(self.code, self.batch, self.n, self.m, self.d)
        lay = self.layout
        dev = device()
        es = 8 if self.code == nat.GPK_F64 else 4
        self._pending = None   # (rerun, stream) of a persistent run not yet verified (see CHAIN_VERIFY)
        self._W = torch.empty(lay.w_bytes // es, dtype=self.dtype, device=dev)
        self._dev = self._W.device   # (cached: every launch and result buffer asks for it)
        # _new(*shape): a new fp64 result buffer per evaluation (the caching allocator's, no device work), so views of an
        # earlier evaluation's results stay valid without a copy (LogLikelihood.get_metric returns one)
        self._new = functools.partial(torch.empty, dtype=torch.float64, device=self._dev)
        self._Winv = torch.empty(max(1, lay.inv_bytes // es), dtype=self.dtype, device=dev)
        self._info = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self._out = torch.empty(self.batch * 4, dtype=torch.float64, device=dev)
        self._mu = torch.empty(max(1, self.batch * self.m), dtype=torch.float64, device=dev)
        self._var = torch.empty(max(1, self.batch * self.m), dtype=torch.float64, device=dev)
        self.kd = None
        self.done = False
        self.shape_key = None
        self.work = None            # the passes' workspace: grow-only, kept between calls (_workspace)
        self._keep = (None, None)   # operand lifetimes: (the last run's, a later pass's) until the stream is past them
        self._alphas = None
        self._mse_operands = self._loo_operands = None
        self._loo_out = None
        self._results = {}          # run kind -> (read-out buffer, gradient or None, extras ...), see _record
        self._record("nlml", self._out)

    # -- result buffers: every read settles a pending persistent run first ---------------------
    @property
    def W(self) -> torch.Tensor:
        self._settle()
        return self._W

    @property
    def Winv(self) -> torch.Tensor:
        self._settle()
        return self._Winv

    @property
    def info(self) -> torch.Tensor:
        self._settle()
        return self._info

    @property
    def out(self) -> torch.Tensor:
        self._settle()
        return self._out

    @property
    def mu(self) -> torch.Tensor:
        self._settle()
        return self._mu

    @property
    def var(self) -> torch.Tensor:
        self._settle()
        return self._var

    # -- launches ---------------------------------------------------------------------------
    def _defer_verify(self, rerun) -> None:
        """After a run: if libgpk took the persistent launch for it, remember how to re-run it; the first read
        of a result verifies it (:meth:`_settle`).  No synchronisation here."""
        self._pending = None
        if CHAIN_VERIFY and nat.last_factorisation_was_chain():
            self._pending = (rerun, torch.cuda.current_stream(self._dev))

    def _settle(self) -> None:
        """Verify a pending persistent run: if a wait timed out (info = -1), run it again on the launch path on
        the run's own stream and count the fallback.  Synchronises with that run."""
        global CHAIN_FALLBACKS
        pend = self._pending
        if pend is None:
            return
        self._pending = None
        rerun, stream = pend
        with torch.cuda.stream(stream):
            if not bool((self._info == -1).any()):   # (waits for the run)
                return
            CHAIN_FALLBACKS += 1
            logging.warning("persistent factorisation timed out (gpk_tune chain_timeout_ms): re-running it on the "
                            "launch path (%d fallbacks so far)", CHAIN_FALLBACKS)
            with nat.thread_tune(chain=0):
                rerun()

    def _enqueue(self, once, *args):
        """Every run kind's launch: ``once(*args)`` now, and again from :meth:`_settle` should the persistent launch
        it took time out.  Invariant: a ``once`` body reads the raw buffers ``_W`` / ``_Winv`` / ``_info`` (and
        ``_out``, ``_mu``, ``_var``), never the settling properties -- a re-run must not settle itself."""
        self._pending = None   # (the previous run's results are overwritten unread)
        once(*args)
        self._defer_verify(lambda: once(*args))
        return self

    def _check_operands(self, n_hyp, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                        X_test=None, y_test=None) -> None:
        """The device reads these extents blindly: check them here (an undersized operand would be read out of
        bounds, not reported).  ``X_test`` / ``y_test``: (tensor, batch stride) where the run reads them."""
        B, dev = self.batch, self._dev
        _check_operand("hyper_parameter", hyp, hyp_stride, n_hyp, B, dev)
        _check_operand("noise", noise, noise_stride, 1, B, dev)
        _check_operand("X", X, x_bstride, self.n * self.d, B, dev)
        _check_operand("y", y, y_bstride, self.n, B, dev)
        if X_test is not None:
            _check_operand("X_test", X_test[0], X_test[1], self.m * self.d, B, dev)
        if y_test is not None:
            _check_operand("y_test", y_test[0], y_test[1], self.m, B, dev)

    def _workspace(self, need: int) -> torch.Tensor:
        """At least ``need`` bytes of fp64 device workspace, kept between calls (it only grows).  One buffer serves
        every pass of this factorisation: they follow each other on the stream."""
        if self.work is None or self.work.numel() * 8 < need:
            self.work = torch.empty(max(1, need // 8), dtype=torch.float64, device=self._dev)
        return self.work

    def _record(self, kind: str, out: torch.Tensor, grad=None, *extras) -> None:
        """The one place a run kind ("nlml", "mse", "loo") keeps its results: the [B * 4] read-out buffer (column 0:
        the value), the gradient [B, n_hyp + 1] or None, then extras (the LOO mu / var)."""
        self._results[kind] = (out, grad) + extras

    def _views(self, kind: str):
        """(value [B], gradient or None, extras ...) of the last run of ``kind``, as recorded."""
        r = self._results[kind]
        return (r[0].view(self.batch, 4)[:, 0],) + r[1:]

    def results(self, kind: str = "nlml", settle: bool = True):
        """(f [B], g [B, n_hyp + 1] or None, info [B] int32) device views of the last run of ``kind``.  Settled: a
        pending persistent run is verified first (:meth:`_settle`).  Unsettled: no host synchronisation, for callers
        that pipeline runs and only forward the values on the device -- a wait that timed out shows as info = -1
        there, and the run is not re-done."""
        if settle:
            self._settle()
        r = self._results.get(kind)
        if r is None:
            raise RuntimeError({"mse": "run_mse(...) or mse_gradient(...) first",
                                "loo": "run_loo(...) or loo(...) first", "fisher": "fisher() first"}[kind])
        if kind == "fisher":   # (a matrix per member, not a read-out row: (F [B, n_hyp + 1, n_hyp + 1], None, info))
            return r[0], None, self._info
        return r[0].view(self.batch, 4)[:, 0], r[1], self._info

    def run(self, kd: nat.GpkKdesc, hyp: torch.Tensor, hyp_stride: int, noise: torch.Tensor,
            noise_stride: int, X: torch.Tensor, x_bstride: int, y: torch.Tensor, y_bstride: int,
            Xs: Optional[torch.Tensor] = None, xs_bstride: int = 0,
            E: Optional[torch.Tensor] = None, e_bstride: int = 0):
        """Enqueue the factorisation (asynchronous: a persistent run is verified at the first read, see
        CHAIN_VERIFY)."""
        return self._enqueue(self._run_once, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                             Xs, xs_bstride, E, e_bstride)

    def _fresh_out(self) -> None:
        """A new -LML read-out buffer for this evaluation (see ``_new``), no gradient recorded yet."""
        self._out = self._new(self.batch * 4)
        self._record("nlml", self._out)

    def _run_once(self, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride, Xs, xs_bstride,
                  E, e_bstride):
        lay = self.layout
        B, n, m = self.batch, self.n, self.m
        self._alphas = None
        self._fresh_out()
        self._check_operands(kd.n_hyp, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                             X_test=(Xs, xs_bstride) if m and E is None and Xs is not None else None)
        if m:
            if E is not None:
                _check_operand("E", E, e_bstride, m * n, B, self._dev)
            elif Xs is None:
                raise ValueError("m = %d extra rows need X_test or E" % m)
        s = nat.stream_handle(self._dev)
        L = self.L
        if m == 0:
            # gpk_nlml: K build (fused into the first trailing update for single-node kernels) +
            # factorisation + read-out; zeroes info itself
            nat.check(L.gpk_nlml(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(hyp), hyp_stride, nat.ptr(noise),
                                 noise_stride, nat.ptr(X), x_bstride, nat.ptr(y), y_bstride, nat.ptr(self._W),
                                 nat.ptr(self._Winv), nat.ptr(self._info), nat.ptr(self._out), s), "gpk_nlml")
            self.kd = kd
            self.done = True
            return self
        self._info.zero_()
        # (what mse_gradient needs of this run: kernel rows only -- explicit extra rows have no test points)
        self._mse_operands = (kd, hyp, hyp_stride, X, x_bstride, Xs, xs_bstride) if E is None else None
        nat.check(L.gpk_assemble(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(hyp), hyp_stride,
                                 nat.ptr(noise), noise_stride, nat.ptr(X), x_bstride,
                                 nat.ptr(Xs), xs_bstride, nat.ptr(E), e_bstride,
                                 nat.ptr(y), y_bstride, nat.ptr(self._W), s), "gpk_assemble")
        nat.check(L.gpk_potrf_aug(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._Winv),
                                  nat.ptr(self._info), s), "gpk_potrf_aug")
        nat.check(L.gpk_finalize(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._info),
                                 nat.ptr(self._out), nat.ptr(self._mu), nat.ptr(self._var), s), "gpk_finalize")
        self.kd = kd
        self.done = True
        return self

    # -- read-out (device views, no host synchronisation) -----------------------------------
    def w(self, b: int = 0) -> torch.Tensor:
        lay = self.layout
        return self.W[b * lay.w_batch_stride:(b + 1) * lay.w_batch_stride].view(lay.p, lay.ld)

    def nlml(self) -> torch.Tensor:
        return self.results("nlml")[0]

    def unsettled_results(self):
        """(-LML, info) device views WITHOUT settling a pending persistent run (:meth:`results`, settle=False).
        Everyone who does not pipeline runs reads nlml() / info."""
        f, _, info = self.results("nlml", settle=False)
        return f, info

    def fit(self) -> torch.Tensor:
        return self.out.view(self.batch, 4)[:, 1]

    def logdet(self) -> torch.Tensor:
        return self.out.view(self.batch, 4)[:, 2]

    def _counts(self, b: int):
        """(training points, extra rows) of member b: what the size-aware read-outs slice by (ragged batches: the
        member's own counts)."""
        return self.n, self.m

    def cholesky(self, b: int = 0) -> torch.Tensor:
        """L (lower, [n_b, n_b], p_dtype)."""
        nb, _ = self._counts(b)
        return torch.tril(self.w(b)[:nb, :nb])

    def z(self, b: int = 0) -> torch.Tensor:
        return self.w(b)[self.layout.y_row, :self._counts(b)[0]]

    def extra_rows(self, b: int = 0) -> torch.Tensor:
        """Rows n_pad .. n_pad+m_b-1 restricted to the first n_b columns: V^T = Ks^T L^-T (or E L^-T)."""
        lay, (nb, mb) = self.layout, self._counts(b)
        return self.w(b)[lay.n_pad:lay.n_pad + mb, :nb]

    def corner(self, b: int = 0) -> torch.Tensor:
        """Symmetrised m_b x m_b Schur complement: Kss - V^T V (or -E K^-1 E^T)."""
        lay, (_, mb) = self.layout, self._counts(b)
        c = self.w(b)[lay.n_pad:lay.n_pad + mb, lay.n_pad:lay.n_pad + mb]
        return torch.tril(c) + torch.tril(c, -1).transpose(0, 1)

    def posterior_mu(self, b: int = 0) -> torch.Tensor:
        return self.mu[b * self.m:b * self.m + self._counts(b)[1]]

    def posterior_var_diag(self, b: int = 0) -> torch.Tensor:
        return self.var[b * self.m:b * self.m + self._counts(b)[1]]

    def alphas(self) -> torch.Tensor:
        """[batch, n]: alpha_b = L_b^-T z_b = (K_b + noise I)^-1 y_b for every member from ONE batched
        backward solve (gpk_trsv; a ragged member's padding rows carry z = 0), computed once per run and kept until
        the next one."""
        if self._alphas is None:
            lay = self.layout
            x = torch.zeros((self.batch, lay.n_pad), dtype=torch.float64, device=self.W.device)
            x[:, :self.n] = self.W.view(self.batch, lay.p, lay.ld)[:, lay.y_row, :self.n]
            nat.check(self.L.gpk_trsv(ctypes.byref(lay), 1, nat.ptr(self.W), nat.ptr(self.Winv),
                                      nat.ptr(x), nat.stream_handle(self.W.device)), "gpk_trsv")
            self._alphas = x[:, :self.n]
        return self._alphas

    def alpha(self, b: int = 0) -> torch.Tensor:
        """alpha = L^-T z = (K + noise I)^-1 y of member b (see :meth:`alphas`)."""
        return self.alphas()[b]

    # -- held-out MSE and its gradient (gpk_mse_backward / gpk_mse_grad) ------------------------
    def _mse_buffers(self, kd):
        """(out [B * 4], grad [B, n_hyp + 1], work) of the MSE pass, recorded as the "mse" results."""
        nat.require_mse_grad(self.L)
        if self.m < 1:
            raise ValueError("the MSE needs test points: this factorisation was planned with m = 0")
        if self.code != nat.GPK_F64:
            raise NotImplementedError("the MSE gradient is fp64 only")
        need = int(self.L.gpk_mse_grad_workspace_bytes(ctypes.byref(kd), ctypes.byref(self.layout)))
        if need == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % self.d)
        work = self._workspace(need)
        out, grad = self._new(self.batch * 4), self._new(self.batch, kd.n_hyp + 1)
        self._record("mse", out, grad)
        return out, grad, work

    def _ragged_counts(self):
        """(n_dev, m_dev) pointers of a ragged batch; (None, None) here."""
        return None, None

    def mse_gradient(self, ys: torch.Tensor, ys_bstride: int = 0):
        """The MSE pass alone on the last :meth:`run` (test points as extra rows): (mse [B], grad [B, n_hyp + 1])
        device views, the gradient laid out as InverseFactorization.gradient() (noise last); +inf / NaN where
        info != 0.  ``ys``: test targets, member b's at ys[b * ys_bstride:].  Enqueues only (a pending persistent run is
        settled first, like every read of W)."""
        ops = self._mse_operands if self.done else None
        if ops is None:
            raise RuntimeError("run(..., Xs=...) with test points first")
        kd, hyp, hyp_stride, X, x_bstride, Xs, xs_bstride = ops
        out, grad, work = self._mse_buffers(kd)
        dev = self._dev
        _check_operand("y_test", ys, ys_bstride, self.m, self.batch, dev)
        n_ptr, m_ptr = self._ragged_counts()
        nat.check(self.L.gpk_mse_backward(
            ctypes.byref(kd), ctypes.byref(self.layout), nat.ptr(hyp), hyp_stride, nat.ptr(X), x_bstride,
            nat.ptr(Xs), xs_bstride, nat.ptr(ys), ys_bstride, n_ptr, m_ptr, nat.ptr(self.W), nat.ptr(self.Winv),
            nat.ptr(self.info), nat.ptr(out), nat.ptr(grad), nat.ptr(work), work.numel() * 8,
            nat.stream_handle(dev)), "gpk_mse_backward")
        self._keep = (self._keep[0], ys)
        return out.view(self.batch, 4)[:, 0], grad

    def run_mse(self, kd: nat.GpkKdesc, hyp: torch.Tensor, hyp_stride: int, noise: torch.Tensor, noise_stride: int,
                X: torch.Tensor, x_bstride: int, y: torch.Tensor, y_bstride: int, Xs: torch.Tensor, xs_bstride: int,
                ys: torch.Tensor, ys_bstride: int):
        """K build + factorisation + MSE value and gradient as one call (gpk_mse_grad); asynchronous, a persistent
        run is verified at the first read (:meth:`mse`, :meth:`mse_grad`, info).  ``unsettled_mse()`` gives the views
        without that."""
        return self._enqueue(self._run_mse_once, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                             Xs, xs_bstride, ys, ys_bstride)

    def _run_mse_once(self, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride, Xs, xs_bstride,
                      ys, ys_bstride):
        dev = self._dev
        self._alphas = None
        out, grad, work = self._mse_buffers(kd)
        self._check_operands(kd.n_hyp, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                             X_test=(Xs, xs_bstride), y_test=(ys, ys_bstride))
        n_ptr, m_ptr = self._ragged_counts()
        nat.check(self.L.gpk_mse_grad(
            ctypes.byref(kd), ctypes.byref(self.layout), nat.ptr(hyp), hyp_stride, nat.ptr(noise), noise_stride,
            nat.ptr(X), x_bstride, nat.ptr(Xs), xs_bstride, nat.ptr(y), y_bstride, nat.ptr(ys), ys_bstride,
            n_ptr, m_ptr, nat.ptr(self._W), nat.ptr(self._Winv), nat.ptr(self._info), nat.ptr(out), nat.ptr(grad),
            nat.ptr(work), work.numel() * 8, nat.stream_handle(dev)), "gpk_mse_grad")
        self._mse_operands = (kd, hyp, hyp_stride, X, x_bstride, Xs, xs_bstride)
        self._keep = ((noise, y, ys), None)
        self.kd = kd
        self.done = True
        return self

    def mse(self) -> torch.Tensor:
        """[batch] mean squared errors of the last run_mse / mse_gradient (+inf where info != 0)."""
        return self.results("mse")[0]

    def mse_grad(self) -> torch.Tensor:
        """[batch, n_hyp + 1] fp64: d mse / d hyp (DFS order), then d mse / d noise."""
        return self.results("mse")[1]

    def unsettled_mse(self):
        """(mse, gradient, info) device views WITHOUT settling a pending persistent run (see unsettled_results)."""
        return self.results("mse", settle=False)

    def check_info(self):
        """Raise CholeskyError if any batch member failed (synchronises)."""
        info = self.info.cpu()
        bad = torch.nonzero(info).flatten()
        if bad.numel():
            if int(info[bad[0]]) < 0:
                # (run() re-runs a timed-out persistent launch on the launch path, so this is reached only
                # with CHAIN_VERIFY off: an infrastructure failure, never "not positive definite")
                raise RuntimeError("device factorisation aborted: a wait of the persistent factorisation timed "
                                   "out (gpk_tune chain_timeout_ms)")
            raise CholeskyError(int(info[bad[0]]))


class _IdentityReadout:
    """Read-outs of an identity-augmented factorisation (extra rows e_t): the extra rows hold L^-T, the corner -K^-1
    and the corner's y row -alpha^T (include/gpk.h), each sliced to the member's own size."""

    def k_inv(self, b: int = 0) -> torch.Tensor:
        """(K_b + noise I)^-1 [n_b, n_b], symmetrised from the corner's lower triangle."""
        return -self.corner(b)

    def l_inv(self, b: int = 0) -> torch.Tensor:
        """L_b^-1 (lower): the transpose of the extra rows, which hold L_b^-T."""
        return torch.triu(self.extra_rows(b)).transpose(0, 1)

    def alpha(self, b: int = 0) -> torch.Tensor:
        """alpha_b [n_b], read from the corner's y row."""
        lay = self.layout
        return -self.w(b)[lay.y_row, lay.n_pad:lay.n_pad + self._counts(b)[0]].to(torch.float64)


class InverseFactorization(_IdentityReadout, AugmentedFactorization):
    """Factorisation of the augmented matrix with identity extra rows (m = n), optionally followed
    by the -LML gradient (``gpk_nlml_grad``).

    After :meth:`run` the extra rows hold L^-T, the corner -K^-1 and the corner's y row -alpha^T
    (include/gpk.h); tiles of structurally zero identity rows are skipped, so the factorisation
    costs n^3 flops -- the work of potrf + trtri + lauum, i.e. of the reference's explicit
    tf.linalg.inv(L) / inv(K) (gpbasics/Statistics/CovarianceMatrix.py:267-275).
    ``gradient()[b]`` = d(-LML)/d(hyperparameters in DFS order) followed by d(-LML)/d(noise).
    """

    def __init__(self, n: int, d: int, batch: int = 1, dtype=None):
        super().__init__(n, d, n, batch, dtype)

    def run(self, kd: nat.GpkKdesc, hyp: torch.Tensor, hyp_stride: int, noise: torch.Tensor,
            noise_stride: int, X: torch.Tensor, x_bstride: int, y: torch.Tensor, y_bstride: int,
            gradient: bool = True, **unused):
        """Enqueue the identity-augmented factorisation (+ gradient); single evaluations take the persistent
        launch like the value path and are verified at the first read (CHAIN_VERIFY)."""
        return self._enqueue(self._run_inverse, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride,
                             gradient)

    def _run_inverse(self, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride, gradient):
        lay, L = self.layout, self.L
        self._alphas = None
        self._out = self._new(self.batch * 4)
        grad = self._new(self.batch, kd.n_hyp + 1) if gradient else None
        self._record("nlml", self._out, grad)
        self._results.pop("fisher", None)   # (of an earlier run)
        self._check_operands(kd.n_hyp, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride)
        work, work_bytes = None, 0
        if gradient:
            work_bytes = int(L.gpk_grad_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay)))
            work = self._workspace(work_bytes)
        nat.check(L.gpk_nlml_grad(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(hyp), hyp_stride,
                                  nat.ptr(noise), noise_stride, nat.ptr(X), x_bstride, nat.ptr(y), y_bstride,
                                  nat.ptr(self._W), nat.ptr(self._Winv), nat.ptr(self._info), nat.ptr(self._out),
                                  nat.ptr(grad), nat.ptr(work), work_bytes, nat.stream_handle(self._dev)),
                  "gpk_nlml_grad")
        self._loo_operands = (kd, hyp, hyp_stride, X, x_bstride, y, y_bstride)   # (what loo() needs of this run)
        self.kd = kd
        self.done = True
        return self

    # -- leave-one-out cross-validation (gpk_loo_backward / gpk_loo_grad) ------------------------
    def _loo_buffers(self, kd, gradient: bool):
        """(out [B * 4], mu [B, n], var [B, n], grad [B, n_hyp + 1] or None, work) of the LOO pass, recorded as the
        "loo" results."""
        nat.require_loo(self.L)
        if self.code != nat.GPK_F64:
            raise NotImplementedError("leave-one-out is fp64 only")
        need = int(self.L.gpk_loo_workspace_bytes(ctypes.byref(kd), ctypes.byref(self.layout)))
        if need == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % self.d)
        work = self._workspace(need)
        B, n = self.batch, self.n
        self._loo_out = out = self._new(B * 4)
        mu, var = self._new(B, n), self._new(B, n)
        grad = self._new(B, kd.n_hyp + 1) if gradient else None
        self._record("loo", out, grad, mu, var)
        return out, mu, var, grad, work

    def loo(self, loss, gradient: bool = True):
        """The leave-one-out pass alone on the last :meth:`run` (gpk_loo_backward; W is only read):
        (f [B], grad [B, n_hyp + 1] or None, mu [B, n], var [B, n]) device views, enqueued without a host
        synchronisation (a pending persistent run is settled first, like every read of W).  ``loss``:
        nat.LOO_LPD (minus the LOO log predictive density) or nat.LOO_MSE; f is +inf, the rest NaN where info != 0.
        mu is in the units of the y that was factored."""
        ops = self._loo_operands if self.done else None
        if ops is None:
            raise RuntimeError("run(...) first")
        loss = nat.loo_loss_code(loss)
        kd, hyp, hyp_stride, X, x_bstride, y, y_bstride = ops
        self._settle()   # (before the buffers: a re-run of a timed-out run_loo records its own)
        out, mu, var, grad, work = self._loo_buffers(kd, gradient)
        nat.check(self.L.gpk_loo_backward(
            loss, ctypes.byref(kd), ctypes.byref(self.layout), nat.ptr(hyp), hyp_stride, nat.ptr(X), x_bstride,
            nat.ptr(y), y_bstride, None, nat.ptr(self.W), nat.ptr(self.info), nat.ptr(out), nat.ptr(mu), nat.ptr(var),
            nat.ptr(grad), nat.ptr(work), work.numel() * 8, nat.stream_handle(self._dev)), "gpk_loo_backward")
        return self._views("loo")

    def run_loo(self, loss, kd: nat.GpkKdesc, hyp: torch.Tensor, hyp_stride: int, noise: torch.Tensor,
                noise_stride: int, X: torch.Tensor, x_bstride: int, y: torch.Tensor, y_bstride: int,
                gradient: bool = True):
        """K build + identity-augmented factorisation + the leave-one-out pass as one call (gpk_loo_grad);
        asynchronous, a persistent run is verified at the first read (:meth:`loo_results`, info).
        ``unsettled_loo()`` gives the views without that."""
        return self._enqueue(self._run_loo_once, nat.loo_loss_code(loss), kd, hyp, hyp_stride, noise, noise_stride,
                             X, x_bstride, y, y_bstride, gradient)

    def _run_loo_once(self, loss, kd, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride, gradient):
        self._alphas = None
        self._record("nlml", self._out)   # (no -LML gradient of this run)
        self._results.pop("fisher", None)
        out, mu, var, grad, work = self._loo_buffers(kd, gradient)
        self._check_operands(kd.n_hyp, hyp, hyp_stride, noise, noise_stride, X, x_bstride, y, y_bstride)
        nat.check(self.L.gpk_loo_grad(
            loss, ctypes.byref(kd), ctypes.byref(self.layout), nat.ptr(hyp), hyp_stride, nat.ptr(noise), noise_stride,
            nat.ptr(X), x_bstride, nat.ptr(y), y_bstride, None, nat.ptr(self._W), nat.ptr(self._Winv),
            nat.ptr(self._info), nat.ptr(out), nat.ptr(mu), nat.ptr(var), nat.ptr(grad), nat.ptr(work),
            work.numel() * 8, nat.stream_handle(self._dev)), "gpk_loo_grad")
        self._loo_operands = (kd, hyp, hyp_stride, X, x_bstride, y, y_bstride)
        self._keep = (noise, None)
        self.kd = kd
        self.done = True
        return self

    def loo_results(self):
        """(f [B], grad [B, n_hyp + 1] or None, mu [B, n], var [B, n]) of the last run_loo / loo (settles a pending
        persistent run)."""
        self.results("loo")
        return self._views("loo")

    def unsettled_loo(self):
        """(f, gradient, info) device views WITHOUT settling a pending persistent run (see unsettled_results)."""
        return self.results("loo", settle=False)

    # -- Fisher information (gpk_fisher) ------------------------------------------------------------
    def fisher(self) -> torch.Tensor:
        """The Fisher information of the last :meth:`run` (gpk_fisher; W is only read): a device view
        [B, n_hyp + 1, n_hyp + 1], F_pq = 1/2 tr(K^-1 d_pK K^-1 d_qK) with the hyperparameters in DFS order and the noise
        last, enqueued without a host synchronisation (a pending persistent run is settled first, like every read of
        W).  NaN for a member whose info != 0.  Recorded as the "fisher" results."""
        if self.code != nat.GPK_F64:
            raise NotImplementedError("Fisher information is fp64 only")
        nat.require_fisher(self.L)
        ops = self._loo_operands if self.done else None
        if ops is None:
            raise RuntimeError("run(...) first")
        kd, hyp, hyp_stride, X, x_bstride = ops[:5]
        self._settle()
        need = int(self.L.gpk_fisher_workspace_bytes(ctypes.byref(kd), ctypes.byref(self.layout)))
        if need == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % self.d)
        work = self._workspace(need)
        np1 = kd.n_hyp + 1
        F = self._new(self.batch, np1, np1)
        self._results["fisher"] = (F, None)
        nat.check(self.L.gpk_fisher(ctypes.byref(kd), ctypes.byref(self.layout), nat.ptr(hyp), hyp_stride, nat.ptr(X),
                                    x_bstride, nat.ptr(self._W), nat.ptr(self._info), nat.ptr(F), nat.ptr(work),
                                    work.numel() * 8, nat.stream_handle(self._dev)), "gpk_fisher")
        return F

    # -- prediction at new points from the kept factor (gpk_predict) ------------------------------------
    PREDICT_WORK_BYTES = 256 << 20   # default bound of the prediction workspace (see predict)

    def predict(self, Xs: torch.Tensor, want_var: bool = True, max_rows: Optional[int] = None, member: int = 0,
                want_mu: bool = True):
        """(mu [m], var [m] or None) device tensors at the new points ``Xs`` [m, d] from member ``member`` of the last
        :meth:`run` (gpk_predict): mu = k(Xs, X) alpha in the units of the y that was factored, var the latent
        posterior variance (no noise added).  Nothing is factored again and W is only read, so ``results("nlml")`` and
        ``fisher()`` of the run stay what they were; enqueued without a host synchronisation (a pending persistent run
        is settled first, like every read of W).  The caller checks ``info`` (:meth:`check_info`): the outputs of a
        failed factorisation are meaningless.
        The test points pass through the workspace ``max_rows`` at a time, 8 (n_pad + 1 + ceil(n / 64)) bytes each.
        Default: as many as PREDICT_WORK_BYTES (256 MiB) hold, rounded down to a multiple of 64 and at least 64 -- 4032
        rows at n = 8192 -- so the workspace stays bounded for any m; the result does not depend on it, bit for bit.
        ``want_mu=False`` skips the mean (var only)."""
        if self.code != nat.GPK_F64:
            raise NotImplementedError("prediction is fp64 only")
        nat.require_predict(self.L)
        ops = self._loo_operands if self.done else None
        if ops is None:
            raise RuntimeError("run(...) first")
        if not (want_mu or want_var):
            raise ValueError("nothing to predict: want_mu and want_var are both off")
        if not 0 <= int(member) < self.batch:
            raise ValueError("member %d of a batch of %d" % (member, self.batch))
        kd, hyp, hyp_stride, X, x_bstride = ops[:5]
        Xs = as_device_f64(Xs)
        if Xs.dim() != 2 or int(Xs.shape[1]) != self.d or int(Xs.shape[0]) < 1:
            raise ValueError("Xs must be [m >= 1, %d], got %s" % (self.d, tuple(Xs.shape)))
        Xs = Xs.contiguous()
        m = int(Xs.shape[0])
        self._settle()
        lay = self.layout
        per_row = int(self.L.gpk_predict_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay), 1))
        if per_row == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % self.d)
        if max_rows is None:
            max_rows = max(64, self.PREDICT_WORK_BYTES // per_row // 64 * 64)
        elif int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        rows = min(m, max(min(m, 64), int(max_rows)))   # (the entry needs one tile of rows, or all of them)
        work = self._workspace(rows * per_row)
        mu = self._new(m) if want_mu else None
        var = self._new(m) if want_var else None
        nat.check(self.L.gpk_predict(ctypes.byref(kd), ctypes.byref(lay), _offset_ptr(hyp, member * hyp_stride),
                                     _offset_ptr(X, member * x_bstride), nat.ptr(self._W), int(member), nat.ptr(Xs), m,
                                     nat.ptr(mu), nat.ptr(var), nat.ptr(work), rows * per_row,
                                     nat.stream_handle(self._dev)), "gpk_predict")
        self._keep = (self._keep[0], Xs)
        return mu, var

    # -- the joint posterior covariance at new points (gpk_predict_vt, gpk_predict_cov) -----------------
    def _predict_operands(self, member: int):
        """(kd, the member's hyp pointer, the member's X pointer) of the last run, after the checks every pass over
        new points shares."""
        if self.code != nat.GPK_F64:
            raise NotImplementedError("prediction is fp64 only")
        nat.require_predict_cov(self.L)
        ops = self._loo_operands if self.done else None
        if ops is None:
            raise RuntimeError("run(...) first")
        if not 0 <= int(member) < self.batch:
            raise ValueError("member %d of a batch of %d" % (member, self.batch))
        kd, hyp, hyp_stride, X, x_bstride = ops[:5]
        return kd, _offset_ptr(hyp, member * hyp_stride), _offset_ptr(X, member * x_bstride)

    def _new_points(self, Xs, name: str) -> torch.Tensor:
        Xs = as_device_f64(Xs)
        if Xs.dim() != 2 or int(Xs.shape[1]) != self.d or int(Xs.shape[0]) < 1:
            raise ValueError("%s must be [m >= 1, %d], got %s" % (name, self.d, tuple(Xs.shape)))
        return Xs.contiguous()

    def predict_vt(self, Xs: torch.Tensor, max_rows: Optional[int] = None, member: int = 0) -> torch.Tensor:
        """V' = k(Xs, X) L^-T = (L^-1 K_s)^T at the new points ``Xs`` [m, d] from member ``member`` of the last
        :meth:`run` (gpk_predict_vt): an [m, n] view of a new [m, n_pad] buffer, so that Sigma = K_ss - V' V'^T.
        Settling, operand lifetimes and the workspace bound are those of :meth:`predict`: the points pass through
        the workspace ``max_rows`` at a time, 8 n_pad bytes each, by default as many as PREDICT_WORK_BYTES hold; the
        result does not depend on it, bit for bit.  W is only read."""
        kd, hyp_p, X_p = self._predict_operands(member)
        Xs = self._new_points(Xs, "Xs")
        m = int(Xs.shape[0])
        self._settle()
        lay = self.layout
        per_row = int(self.L.gpk_predict_vt_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay), 1))
        if per_row == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % self.d)
        if max_rows is None:
            max_rows = max(64, self.PREDICT_WORK_BYTES // per_row // 64 * 64)
        elif int(max_rows) < 1:
            raise ValueError("max_rows must be >= 1")
        rows = min(m, max(min(m, 64), int(max_rows)))   # (the entry needs one tile of rows, or all of them)
        work = self._workspace(rows * per_row)
        Vt = self._new(m, lay.n_pad)
        nat.check(self.L.gpk_predict_vt(ctypes.byref(kd), ctypes.byref(lay), hyp_p, X_p, nat.ptr(self._W), int(member),
                                        nat.ptr(Xs), m, nat.ptr(Vt), lay.n_pad, nat.ptr(work), rows * per_row,
                                        nat.stream_handle(self._dev)), "gpk_predict_vt")
        self._keep = (self._keep[0], Xs)
        return Vt[:, :self.n]

    def predict_cov(self, Xa: torch.Tensor, Xb: Optional[torch.Tensor] = None, member: int = 0) -> torch.Tensor:
        """The latent posterior covariance [ma, mb] between the new points ``Xa`` [ma, d] and ``Xb`` [mb, d] from
        member ``member`` of the last :meth:`run`: k(Xa, Xb) - Va Vb^T with the rows of :meth:`predict_vt`
        (gpk_predict_cov).  ``Xb=None`` is the symmetric mode, Sigma of ``Xa`` with itself: half the product's work,
        symmetric bit for bit.  Nothing is factored again; enqueued without a host synchronisation."""
        kd, hyp_p, _ = self._predict_operands(member)
        Xa = self._new_points(Xa, "Xa")
        Va = self.predict_vt(Xa, member=member)
        symmetric = Xb is None
        if symmetric:
            Xb, Vb = Xa, Va
        else:
            Xb = self._new_points(Xb, "Xb")
            Vb = self.predict_vt(Xb, member=member)
        ma, mb, ld = int(Xa.shape[0]), int(Xb.shape[0]), int(self.layout.n_pad)
        C = self._new(ma, mb)
        nat.check(self.L.gpk_predict_cov(ctypes.byref(kd), self.d, hyp_p, nat.ptr(Xa), ma, nat.ptr(Va), ld,
                                         nat.ptr(Xb), mb, nat.ptr(Vb), ld, self.n, nat.ptr(C), mb, int(symmetric),
                                         nat.stream_handle(self._dev)), "gpk_predict_cov")
        self._keep = (self._keep[0], (Xa, Xb, Va, Vb))
        return C

    def gradient(self) -> torch.Tensor:
        """[batch, n_hyp + 1] fp64: d(-LML)/d hyp (DFS order), then d(-LML)/d noise."""
        g = self.results("nlml")[1]
        if g is None:
            raise RuntimeError("run(..., gradient=True) first")
        return g

    def neg_alpha_rows(self) -> torch.Tensor:
        """[batch, n] view of the -alpha rows inside W (element y_row * ld + n_pad of every member, batch stride
        w_batch_stride): what gpk_mean_vjp reads in place for d(-LML)/d(mean hyperparameters)."""
        lay = self.layout
        return self.W.view(self.batch, lay.p, lay.ld)[:, lay.y_row, lay.n_pad:lay.n_pad + self.n]


def _offset_ptr(t: torch.Tensor, elements: int):
    """ctypes pointer to element ``elements`` of t (for per-member launches)."""
    return ctypes.c_void_p(t.data_ptr() + int(elements) * t.element_size())


class RaggedFactorization(AugmentedFactorization):
    """One factorisation of independent problems of DIFFERENT sizes (gpk_*_ragged).

    Member b has ``sizes[b]`` training points and ``test_sizes[b]`` test points; the layout is
    planned for the largest member and every smaller member's block is completed with identity
    rows (training) or zero rows (test), which the device skips tile by tile.  This replaces the
    reference's one-segment-at-a-time loops over constituent GPs (SegmentedCovarianceMatrix
    get_*_blocks, gpbasics/Statistics/CovarianceMatrix.py:289-565; BlockwiseLogLikelihood,
    gpbasics/Metrics/LogLikelihood.py:68-104) by one set of batched launches: the panel chain is
    paid once for all segments instead of once per segment.

    Members may carry different kernel trees (the children of a change-point or partition
    operator): members sharing one device program are assembled by one launch, the others by a
    launch each; the factorisation and read-out are always one set of launches.
    """

    def __init__(self, sizes: Sequence[int], d: int, test_sizes: Optional[Sequence[int]] = None, dtype=None):
        sizes = [int(s) for s in sizes]
        if not sizes or min(sizes) < 1:
            raise ValueError("every member of a ragged batch needs at least one training point")
        tsz = [int(s) for s in test_sizes] if test_sizes is not None else [0] * len(sizes)
        if len(tsz) != len(sizes) or min(tsz) < 0:
            raise ValueError("test_sizes must hold one count >= 0 per member")
        super().__init__(max(sizes), d, max(tsz), len(sizes), dtype)
        self.sizes, self.test_sizes = sizes, tsz
        dev = self.W.device
        self.n_dev = torch.tensor(sizes, dtype=torch.int64, device=dev)
        self.m_dev = torch.tensor(tsz, dtype=torch.int64, device=dev)

    def _counts(self, b: int):
        return self.sizes[b], self.test_sizes[b]

    def run(self, members: Sequence, noise) -> "RaggedFactorization":
        """members[b] = (kdesc, hyp [n_hyp] fp64, X_b [n_b, d], y_b [n_b], Xs_b [m_b, d] or None);
        noise: rank-0 or one value per member."""
        self._pending = None
        B, n, m, d = self.batch, self.n, self.m, self.d
        self._alphas = None
        kds, hyp, nz, X, y, Xs = _pack_members(self, members, noise, self.test_sizes)
        dev = self._dev
        L, s = self.L, nat.stream_handle(dev)
        lay = self.layout
        self._info.zero_()
        mptr = nat.ptr(self.m_dev) if m else None
        xs_ptr = nat.ptr(Xs) if m else None
        same = all(bytes(k) == bytes(kds[0]) for k in kds)
        if same:
            nat.check(L.gpk_assemble_ragged(ctypes.byref(kds[0]), ctypes.byref(lay), nat.ptr(hyp), nat.MAX_HYP,
                                            nat.ptr(nz), 1, nat.ptr(X), n * d, xs_ptr, max(m, 1) * d,
                                            nat.ptr(y), n, nat.ptr(self.n_dev), mptr, nat.ptr(self._W), s),
                      "gpk_assemble_ragged")
        else:
            one = nat.plan(self.code, 1, n, m, d)   # same p / ld as the batched layout
            for b, kd in enumerate(kds):
                nat.check(L.gpk_assemble_ragged(
                    ctypes.byref(kd), ctypes.byref(one), _offset_ptr(hyp, b * nat.MAX_HYP), 0,
                    _offset_ptr(nz, b), 0, _offset_ptr(X, b * n * d), 0,
                    _offset_ptr(Xs, b * max(m, 1) * d) if m else None, 0, _offset_ptr(y, b * n), 0,
                    _offset_ptr(self.n_dev, b), _offset_ptr(self.m_dev, b) if m else None,
                    _offset_ptr(self._W, b * lay.w_batch_stride), s), "gpk_assemble_ragged")
        nat.check(L.gpk_potrf_aug_ragged(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._Winv),
                                         nat.ptr(self._info), nat.ptr(self.n_dev), mptr, s), "gpk_potrf_aug_ragged")
        nat.check(L.gpk_finalize_ragged(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._info),
                                        nat.ptr(self.n_dev), nat.ptr(self._out),
                                        nat.ptr(self._mu) if m else None, nat.ptr(self._var) if m else None, s),
                  "gpk_finalize_ragged")
        self._keep = ((X, y, Xs, hyp, nz), None)
        # (what mse_gradient needs of this run: one program for every member)
        self._mse_operands = (kds[0], hyp, nat.MAX_HYP, X, n * d, Xs, max(m, 1) * d) if same and m else None
        self.kd = kds
        self.done = True
        return self

    # -- held-out MSE of a ragged batch ---------------------------------------------------------
    def _ragged_counts(self):
        if min(self.test_sizes) < 1:
            raise ValueError("the MSE needs at least one test point per member (test_sizes %s)" % (self.test_sizes,))
        return nat.ptr(self.n_dev), nat.ptr(self.m_dev)

    def mse_gradient(self, ys, ys_bstride: Optional[int] = None):
        """As AugmentedFactorization.mse_gradient for members sharing one kernel program.  ``ys``: one tensor of
        m_b test targets per member, or a packed [B, m] device tensor (what lies past m_b is not read)."""
        if isinstance(ys, (list, tuple)):
            if len(ys) != self.batch:
                raise ValueError("expected %d test-target vectors, got %d" % (self.batch, len(ys)))
            packed = torch.zeros((self.batch, self.m), dtype=torch.float64, device=self._dev)
            for b, v in enumerate(ys):
                if v.numel() != self.test_sizes[b]:
                    raise ValueError("member %d: y_test must hold %d values" % (b, self.test_sizes[b]))
                packed[b, :self.test_sizes[b]] = v.detach().reshape(-1)
            ys, ys_bstride = packed, self.m
        if self.done and self._mse_operands is None and self.m:
            raise ValueError("mse_gradient needs members that share one kernel program")
        return super().mse_gradient(ys, self.m if ys_bstride is None else ys_bstride)

    def run_mse_packed(self, kd: nat.GpkKdesc, hyp: torch.Tensor, noise: torch.Tensor, X: torch.Tensor,
                       y: torch.Tensor, Xs: torch.Tensor, ys: torch.Tensor) -> "RaggedFactorization":
        """K build + factorisation + MSE value and gradient of a ragged batch whose members share one program, on
        operands already packed on the device (gpk_mse_grad with n_dev / m_dev): hyp [B, MAX_HYP], noise [B],
        X [B, n, d], y [B, n], Xs [B, m, d], ys [B, m]; what lies past a member's own counts is not read.  No host
        round trip; read mse() / mse_grad() / info (ragged batches never take the persistent launch)."""
        n, m, d = self.n, self.m, self.d
        self.run_mse(kd, hyp, nat.MAX_HYP, noise, 1, X, n * d, y, n, Xs, m * d, ys, m)
        self.kd = [kd] * self.batch
        return self

    def alphas(self) -> List[torch.Tensor]:
        """alpha_b [n_b] for every member (one batched backward solve, see AugmentedFactorization.alphas)."""
        rows = super().alphas()
        return [rows[b, :self.sizes[b]] for b in range(self.batch)]


def _pack_members(f, members: Sequence, noise, test_sizes=None):
    """(kds, hyp [B, MAX_HYP], noise [B], X [B, n, d], y [B, n], Xs [B, max(m, 1), d] or None) of a ragged batch on
    the device, zero-filled past each member's counts.  members[b] = (kdesc, hyp, X_b, y_b[, Xs_b]); ``noise``
    rank-0 or one value per member; ``test_sizes``: the members' test counts where they carry test points."""
    B, n, d = f.batch, f.n, f.d
    if len(members) != B:
        raise ValueError("expected %d members, got %d" % (B, len(members)))
    dev = f._dev
    X = torch.zeros((B, n, d), dtype=torch.float64, device=dev)
    y = torch.zeros((B, n), dtype=torch.float64, device=dev)
    Xs = torch.zeros((B, max(f.m, 1), d), dtype=torch.float64, device=dev) if test_sizes is not None else None
    hyp = torch.zeros((B, nat.MAX_HYP), dtype=torch.float64, device=dev)
    kds = []
    for b, (kd, h, xb, yb, *xsb) in enumerate(members):
        nb = f.sizes[b]
        if tuple(xb.shape) != (nb, d) or yb.numel() != nb:
            raise ValueError("member %d: X must be [%d, %d] and y hold %d values" % (b, nb, d, nb))
        if h.numel() != kd.n_hyp:
            raise ValueError("member %d: %d hyperparameters, kernel expects %d" % (b, h.numel(), kd.n_hyp))
        X[b, :nb] = xb.detach()
        y[b, :nb] = yb.detach().reshape(-1)
        if test_sizes is not None and test_sizes[b]:
            mb = test_sizes[b]
            if not xsb or xsb[0] is None or tuple(xsb[0].shape) != (mb, d):
                raise ValueError("member %d: X_test must be [%d, %d]" % (b, mb, d))
            Xs[b, :mb] = xsb[0].detach()
        hyp[b, :kd.n_hyp] = h.detach().reshape(-1)
        kds.append(kd)
    nz = noise if isinstance(noise, torch.Tensor) else torch.as_tensor(noise, dtype=torch.float64)
    nz = nz.detach().to(device=dev, dtype=torch.float64).reshape(-1)
    nz = (nz.expand(B) if nz.numel() == 1 else nz).contiguous()
    if nz.numel() != B:
        raise ValueError("noise must be rank-0 or hold one value per member")
    return kds, hyp, nz, X, y, Xs


def program_runs(kds: Sequence) -> List[tuple]:
    """Maximal runs (start, stop) of consecutive members whose device programs are byte-identical: each run is one
    launch of the per-program passes (K build, gradient) of a ragged batch."""
    runs, b0 = [], 0
    for b in range(1, len(kds) + 1):
        if b == len(kds) or bytes(kds[b]) != bytes(kds[b0]):
            runs.append((b0, b))
            b0 = b
    return runs


class RaggedInverseFactorization(_IdentityReadout, AugmentedFactorization):
    """Identity-augmented factorisation (+ -LML gradient) of independent problems of DIFFERENT sizes: the sibling of
    :class:`RaggedFactorization` for what :class:`InverseFactorization` computes (gpk_assemble_inverse_ragged,
    gpk_potrf_aug_ragged_ex, gpk_finalize_ragged, gpk_grad_ragged).

    The layout is planned with m = n = max(sizes).  Member b's training rows past ``sizes[b]`` are identity padding,
    its extra rows t < sizes[b] are e_t and the rest zero rows; after :meth:`run` its corner holds -K_b^-1, the
    corner's y row -alpha_b^T and its extra rows L_b^-T.  This serves the gradient of the reference's blockwise_LL
    (gpbasics/Metrics/LogLikelihood.py:68-104 under the tape of gpbasics/Optimizer/Fitter.py:124-158), the k-fold
    objective (Fitter.py:97-102) and the per-segment inverses of SegmentedCovarianceMatrix
    (gpbasics/Statistics/CovarianceMatrix.py:520-556) with ONE panel chain for all members.

    Consecutive members sharing a device program are assembled and differentiated by one launch (a batch layout with
    offset pointers), the others by a launch each; the factorisation and the read-out are always one set of launches.
    """

    def __init__(self, sizes: Sequence[int], d: int, dtype=None):
        sizes = [int(s) for s in sizes]
        if not sizes or min(sizes) < 1:
            raise ValueError("every member of a ragged batch needs at least one training point")
        if not nat.ragged_grad_supported():
            raise nat.NativeUnavailable("this libgpk.so was built before the ragged identity-augmented entries "
                                        "(gpk_grad_ragged and its kin) existed: rebuild it")
        super().__init__(max(sizes), d, max(sizes), len(sizes), dtype)
        self.sizes = sizes
        self.n_dev = torch.tensor(sizes, dtype=torch.int64, device=self.W.device)
        self._grads = self._runs = self._packed = None

    def _counts(self, b: int):
        return self.sizes[b], self.sizes[b]

    def run(self, members: Sequence, noise, gradient: bool = True) -> "RaggedInverseFactorization":
        """members[b] = (kdesc, hyp [n_hyp] fp64, X_b [n_b, d], y_b [n_b]); noise: rank-0 or one value per member.
        Asynchronous; ``gradient()`` / ``nlml()`` are device tensors."""
        kds, hyp, nz, X, y, _ = _pack_members(self, members, noise)
        return self.run_packed(kds, hyp, nz, X, y, gradient)

    def _program_runs(self, kds: Sequence) -> List[tuple]:
        """(b0, b1, program, sub-layout) per run of :func:`program_runs`: the batch layout of the run's b1 - b0
        members (same p / ld / strides as the whole batch's), to be used with pointers offset to member b0."""
        lays = {self.batch: self.layout}
        runs = []
        for b0, b1 in program_runs(kds):
            if b1 - b0 not in lays:
                lays[b1 - b0] = nat.plan(self.code, b1 - b0, self.n, self.n, self.d)
            runs.append((b0, b1, kds[b0], lays[b1 - b0]))
        return runs

    def run_packed(self, kds: Sequence, hyp: torch.Tensor, noise: torch.Tensor, X: torch.Tensor, y: torch.Tensor,
                   gradient: bool = True) -> "RaggedInverseFactorization":
        """:meth:`run` on operands already packed on the device: hyp [B, MAX_HYP], noise [B], X [B, n, d] and
        y [B, n] (zero-filled past each member's size), kds one program per member.  No host round trip."""
        self._pending = None
        self._alphas = None
        B, n, d = self.batch, self.n, self.d
        dev = self._dev
        if len(kds) != B:
            raise ValueError("expected %d programs, got %d" % (B, len(kds)))
        self._check_operands(nat.MAX_HYP, hyp, nat.MAX_HYP, noise, 1, X, n * d, y, n)
        self._fresh_out()
        L, s, lay = self.L, nat.stream_handle(dev), self.layout
        runs = self._program_runs(kds)
        self._info.zero_()
        for b0, b1, kd, sl in runs:
            nat.check(L.gpk_assemble_inverse_ragged(
                ctypes.byref(kd), ctypes.byref(sl), _offset_ptr(hyp, b0 * nat.MAX_HYP),
                nat.MAX_HYP, _offset_ptr(noise, b0), 1, _offset_ptr(X, b0 * n * d), n * d, _offset_ptr(y, b0 * n), n,
                _offset_ptr(self.n_dev, b0), _offset_ptr(self._W, b0 * lay.w_batch_stride), s),
                "gpk_assemble_inverse_ragged")
        nat.check(L.gpk_potrf_aug_ragged_ex(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._Winv),
                                            nat.ptr(self._info), nat.AUG_EXTRA_IDENTITY, nat.ptr(self.n_dev),
                                            nat.ptr(self.n_dev), s), "gpk_potrf_aug_ragged_ex")
        nat.check(L.gpk_finalize_ragged(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._info),
                                        nat.ptr(self.n_dev), nat.ptr(self._out), None, None, s),
                  "gpk_finalize_ragged")
        self._grads = None
        if gradient:
            # one workspace for every run (sized for the run that needs most; the runs follow each other on the stream)
            work = self._workspace(max(int(L.gpk_grad_workspace_bytes(ctypes.byref(kd), ctypes.byref(sl)))
                                       for _, _, kd, sl in runs))
            self._grads = []
            for b0, b1, kd, sl in runs:
                g = self._new(b1 - b0, kd.n_hyp + 1)
                nat.check(L.gpk_grad_ragged(
                    ctypes.byref(kd), ctypes.byref(sl), _offset_ptr(hyp, b0 * nat.MAX_HYP), nat.MAX_HYP,
                    _offset_ptr(X, b0 * n * d), n * d, _offset_ptr(self.n_dev, b0),
                    _offset_ptr(self._W, b0 * lay.w_batch_stride), _offset_ptr(self._info, b0), nat.ptr(g),
                    nat.ptr(work), work.numel() * 8, s), "gpk_grad_ragged")
                self._grads.append(g)
            if len(runs) == 1:   # (one program: the gradient of the whole batch is one tensor)
                self._record("nlml", self._out, self._grads[0])
        self._runs = runs
        self._packed = (hyp, X, y)   # (what loo() needs of this run)
        self._keep = ((X, y, hyp, noise), None)
        self.kd = list(kds)
        self.done = True
        return self

    # -- leave-one-out cross-validation (gpk_loo_backward with n_dev) ----------------------------
    def loo(self, loss, gradient: bool = True):
        """The leave-one-out pass alone on the last :meth:`run` for every member (gpk_loo_backward with the members'
        sizes; W is only read): (f [B], grads, mu [B, n], var [B, n]) device views, enqueued without a host
        synchronisation.  ``grads``: None without ``gradient``, else a list with member b's [n_hyp_b + 1] gradient
        (noise last).  mu / var are zero past a member's size; f is +inf, the rest NaN where info[b] != 0.  The
        workspace is kept between calls; the result buffers are the caching allocator's per evaluation."""
        if not self.done:
            raise RuntimeError("run(...) first")
        nat.require_loo(self.L)
        if self.code != nat.GPK_F64:
            raise NotImplementedError("leave-one-out is fp64 only")
        loss = nat.loo_loss_code(loss)
        hyp, X, y = self._packed
        B, n, d = self.batch, self.n, self.d
        L, lay = self.L, self.layout
        s = nat.stream_handle(self._dev)
        need = max(int(L.gpk_loo_workspace_bytes(ctypes.byref(kd), ctypes.byref(sl))) for _, _, kd, sl in self._runs)
        if need == 0:
            raise ValueError("the kernel program is not valid for dimension %d" % d)
        work = self._workspace(need)
        out, mu, var = self._new(B * 4), self._new(B, n), self._new(B, n)
        grads = [] if gradient else None
        for b0, b1, kd, sl in self._runs:
            g = self._new(b1 - b0, kd.n_hyp + 1) if gradient else None
            nat.check(L.gpk_loo_backward(
                loss, ctypes.byref(kd), ctypes.byref(sl), _offset_ptr(hyp, b0 * nat.MAX_HYP), nat.MAX_HYP,
                _offset_ptr(X, b0 * n * d), n * d, _offset_ptr(y, b0 * n), n, _offset_ptr(self.n_dev, b0),
                _offset_ptr(self._W, b0 * lay.w_batch_stride), _offset_ptr(self._info, b0), _offset_ptr(out, b0 * 4),
                _offset_ptr(mu, b0 * n), _offset_ptr(var, b0 * n), nat.ptr(g), nat.ptr(work), work.numel() * 8, s),
                "gpk_loo_backward")
            if gradient:
                grads.extend(g[k] for k in range(b1 - b0))
        return out.view(B, 4)[:, 0], grads, mu, var

    # -- per-member read-out (device views, no host synchronisation) ---------------------------
    def gradients(self) -> torch.Tensor:
        """[B, n_hyp + 1] of a batch whose members share one program (the k-fold case)."""
        g = self._results["nlml"][1]
        if g is None:
            raise RuntimeError("run(..., gradient=True) on members sharing one program first")
        return g

    def gradient(self, b: int) -> torch.Tensor:
        """[n_hyp_b + 1] fp64: d(-LML_b)/d hyp (DFS order), then d(-LML_b)/d noise; NaN where info[b] != 0."""
        if self._grads is None:
            raise RuntimeError("run(..., gradient=True) first")
        for (b0, b1, _, _), g in zip(self._runs, self._grads):
            if b0 <= b < b1:
                return g[b - b0]
        raise IndexError(b)

    def alphas(self):
        return [self.alpha(b) for b in range(self.batch)]


def gemv(A: torch.Tensor, x: torch.Tensor, y: Optional[torch.Tensor] = None, alpha: float = 1.0,
         beta: float = 0.0) -> torch.Tensor:
    """y <- alpha A x + beta y on the device (gpk_gemv; A row-major fp64 [n, m], x [m] or [m, 1]).
    Returns y with x's trailing shape ([n] or [n, 1])."""
    if A.dim() != 2 or A.dtype != torch.float64 or A.stride(1) != 1:
        raise ValueError("A must be a row-major float64 matrix")
    n, m = int(A.shape[0]), int(A.shape[1])
    xv = x.reshape(-1)
    if xv.numel() != m or xv.dtype != torch.float64:
        raise ValueError("x must hold %d float64 values" % m)
    xv = xv.contiguous()
    out_shape = (n, 1) if x.dim() == 2 else (n,)
    if y is None:
        y = torch.empty(out_shape, dtype=torch.float64, device=A.device)
        beta = 0.0
    elif y.numel() != n or not y.is_contiguous():
        raise ValueError("y must be a contiguous tensor of %d values" % n)
    nat.check(nat.lib().gpk_gemv(nat.ptr(A), n, m, int(A.stride(0)), nat.ptr(xv), nat.ptr(y), float(alpha),
                                 float(beta), nat.stream_handle(A.device)), "gpk_gemv")
    return y


# ----------------------------------------------------------------------------- approximation paths
# Dense device building blocks of the Nystroem / SKC / SKI matrices (include/gpk.h
# "approximation paths").  Matrices are row-major fp64 device tensors, [n, m] or batched [B, n, m].
def _mat_args(t: torch.Tensor, name: str):
    if t.dtype != torch.float64 or t.device != device():
        raise ValueError("%s must be a float64 tensor on %s" % (name, device()))
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError("%s must be a row-major [n, m] or [B, n, m] matrix" % name)
    return t, int(t.stride(1)), int(t.stride(0)) if t.shape[0] > 1 else 0


def dgemm(A: torch.Tensor, B: torch.Tensor, trans_a: bool = False, trans_b: bool = False, alpha: float = 1.0,
          beta: float = 0.0, C: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C <- alpha op(A) op(B) + beta C on f64 MFMA (gpk_dgemm); the tf.matmul / tf.tensordot products
    of gpbasics/Statistics/Nystroem_K.py and Metrics/StructuredKernelInterpolation.py."""
    squeeze = A.dim() == 2 and B.dim() == 2 and (C is None or C.dim() == 2)
    A3, lda, abs_ = _mat_args(A, "A")
    B3, ldb, bbs = _mat_args(B, "B")
    batch = max(A3.shape[0], B3.shape[0])
    if A3.shape[0] not in (1, batch) or B3.shape[0] not in (1, batch):
        raise ValueError("batch sizes of A and B differ")
    M = A3.shape[2] if trans_a else A3.shape[1]
    K = A3.shape[1] if trans_a else A3.shape[2]
    Kb = B3.shape[2] if trans_b else B3.shape[1]
    N = B3.shape[1] if trans_b else B3.shape[2]
    if K != Kb:
        raise ValueError("inner dimensions differ: %d vs %d" % (K, Kb))
    if C is None:
        C3 = torch.empty((batch, M, N), dtype=torch.float64, device=A.device)
        beta = 0.0
    else:
        C3 = C.unsqueeze(0) if C.dim() == 2 else C
        if tuple(C3.shape) != (batch, M, N) or not C3.is_contiguous():
            raise ValueError("C must be a contiguous [%d, %d, %d] tensor" % (batch, M, N))
    nat.check(nat.lib().gpk_dgemm(int(trans_a), int(trans_b), M, N, K, float(alpha), nat.ptr(A3), lda, abs_,
                                  nat.ptr(B3), ldb, bbs, float(beta), nat.ptr(C3), N, M * N, batch,
                                  nat.stream_handle(A.device)), "gpk_dgemm")
    return C3[0] if squeeze else C3


def syevj(A: torch.Tensor, max_sweeps: int = 60):
    """Eigendecomposition of a symmetric [m, m] (or [B, m, m]) device matrix by two-sided Jacobi
    (gpk_syevj): returns (lam [.., m], V [.., m, m] with the eigenvectors in its columns, sweeps)."""
    A3, lda, abs_ = _mat_args(A, "A")
    batch, m = A3.shape[0], A3.shape[1]
    if A3.shape[2] != m:
        raise ValueError("A must be square")
    L = nat.lib()
    V = torch.empty((batch, m, m), dtype=torch.float64, device=A.device)
    lam = torch.empty((batch, m), dtype=torch.float64, device=A.device)
    wb = int(L.gpk_syevj_workspace_bytes(m, batch))
    work = torch.empty(max(1, (wb + 7) // 8), dtype=torch.float64, device=A.device)
    sweeps = ctypes.c_int32(0)
    nat.check(L.gpk_syevj(m, batch, nat.ptr(A3), lda, abs_, nat.ptr(V), nat.ptr(lam), nat.ptr(work), wb,
                          int(max_sweeps), ctypes.byref(sweeps), nat.stream_handle(A.device)), "gpk_syevj")
    if A.dim() == 2:
        return lam[0], V[0], int(sweeps.value)
    return lam, V, int(sweeps.value)


def syevd(A: torch.Tensor):
    """Eigendecomposition of a symmetric [m, m] (or [B, m, m]) device matrix by the tridiagonal route
    (gpk_syevd: blocked Householder tridiagonalisation, divide and conquer on the tridiagonal matrix,
    compact-WY back-transformation): returns (lam, V with the eigenvectors in its columns), eigenvalues in no
    particular order (any m up to gpk_syevd's cap, 46340)."""
    A3, lda, abs_ = _mat_args(A, "A")
    batch, m = A3.shape[0], A3.shape[1]
    if A3.shape[2] != m:
        raise ValueError("A must be square")
    L = nat.lib()
    V = torch.empty((batch, m, m), dtype=torch.float64, device=A.device)
    lam = torch.empty((batch, m), dtype=torch.float64, device=A.device)
    wb = int(L.gpk_syevd_workspace_bytes(m))
    work = torch.empty(max(1, (wb + 7) // 8), dtype=torch.float64, device=A.device)
    nat.check(L.gpk_syevd(m, batch, nat.ptr(A3), lda, abs_, nat.ptr(V), nat.ptr(lam), nat.ptr(work), wb,
                          nat.stream_handle(A.device)), "gpk_syevd")
    if A.dim() == 2:
        return lam[0], V[0]
    return lam, V


def eigh(A: torch.Tensor):
    """The product's symmetric eigensolver: syevd (tridiagonal route); returns (lam, V, 0) like syevj."""
    lam, V = syevd(A)
    return lam, V, 0


def pinv_factor(lam: torch.Tensor, V: torch.Tensor, mode: int, rcond: float = -1.0, return_mu: bool = False):
    """U = V diag(mu) with tf.linalg.pinv's cutoff (gpk_pinv_factor): mode 0 mu = 1/lam (pinv = U V^T),
    mode 1 mu = lam^-1/2 (pinv = U U^T), mode 2 mu = |lam|^-1/2 (pinv = U diag(sign lam) U^T).  Returns (U, rank
    [B] int32 device tensor) (+ mu)."""
    squeeze = V.dim() == 2
    V3 = V.unsqueeze(0) if squeeze else V
    lam2 = lam.unsqueeze(0) if lam.dim() == 1 else lam
    batch, m = V3.shape[0], V3.shape[1]
    U = torch.empty_like(V3)
    mu = torch.empty((batch, m), dtype=torch.float64, device=V.device)
    rank = torch.empty(batch, dtype=torch.int32, device=V.device)
    nat.check(nat.lib().gpk_pinv_factor(m, batch, nat.ptr(V3.contiguous()), nat.ptr(lam2.contiguous()),
                                        float(rcond), int(mode), nat.ptr(mu), nat.ptr(U), nat.ptr(rank),
                                        nat.stream_handle(V.device)), "gpk_pinv_factor")
    if return_mu:
        return (U[0] if squeeze else U), rank, (mu[0] if squeeze else mu)
    return (U[0] if squeeze else U), rank


def pinv_sym(A: torch.Tensor, rcond: float = -1.0) -> torch.Tensor:
    """tf.linalg.pinv of a symmetric matrix (gpbasics/Statistics/Nystroem_K.py:53): the eigendecomposition
    (:func:`eigh`, gpk_syevd), the reference's cutoff 10 m eps max|lam|, then V diag(1/lam) V^T on MFMA."""
    lam, V, _ = eigh(A)
    U, _ = pinv_factor(lam, V, 0, rcond)
    return dgemm(U, V, trans_b=True)


def pinv_backward(lam: torch.Tensor, V: torch.Tensor, mu: torch.Tensor, Pbar: Optional[torch.Tensor] = None,
                  T: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of a symmetric A from the adjoint Pbar of pinv(A) (tf.linalg.pinv's reverse mode,
    gpbasics/Statistics/Nystroem_K.py:53): V (F o sym(V^T Pbar V)) V^T with the Daleckii-Krein quotients of
    f = 1/lam over the kept eigenvalues (gpk_pinv_backward_scale); lam, V from :func:`eigh`, mu the mode-0
    factors of :func:`pinv_factor`.  T: the adjoint already in the eigenbasis (V^T Pbar V) instead."""
    m = int(V.shape[-1])
    if T is None:
        T = dgemm(dgemm(V, Pbar.contiguous(), trans_a=True), V)
    T = T.contiguous().clone()
    nat.check(nat.lib().gpk_pinv_backward_scale(m, 1, nat.ptr(lam.contiguous()), nat.ptr(mu.contiguous()),
                                                nat.ptr(T), nat.stream_handle(V.device)), "gpk_pinv_backward_scale")
    return dgemm(dgemm(V, T), V, trans_b=True)


def kernel_vjp(kernel, hyper_parameter, X, Z, G: Optional[torch.Tensor] = None, gu: Optional[torch.Tensor] = None,
               gv: Optional[torch.Tensor] = None, want_z: bool = False):
    """Reverse mode of K = kernel(X, Z) (gpk_kernel_vjp) for the adjoint G [n, m] of K, or the rank-1
    adjoint gu gv^T: returns (flat hyperparameter adjoint [n_hyp], adjoint of Z [m, d] or None)."""
    L = nat.lib()
    X = as_device_f64(X)
    Z = as_device_f64(Z)
    n, d = int(X.shape[0]), int(X.shape[1])
    m = int(Z.shape[0])
    kd = kernel_descriptor(kernel, d)
    hyp = pack_hyper_parameter(hyper_parameter, kd.n_hyp)
    gh = torch.zeros(max(1, kd.n_hyp), dtype=torch.float64, device=X.device)
    gz = torch.zeros((m, d), dtype=torch.float64, device=X.device) if want_z else None
    if n == 0 or m == 0:
        return gh[:kd.n_hyp], gz
    if G is not None:
        G = G.to(dtype=torch.float64)
        if G.dim() != 2 or tuple(G.shape) != (n, m) or G.stride(1) != 1:
            raise ValueError("G must be a row-major [%d, %d] matrix" % (n, m))
        ldg = int(G.stride(0))
    else:
        gu = gu.reshape(-1).to(dtype=torch.float64).contiguous()
        gv = gv.reshape(-1).to(dtype=torch.float64).contiguous()
        if gu.numel() != n or gv.numel() != m:
            raise ValueError("rank-1 weights must hold %d and %d values" % (n, m))
        ldg = m
    wb = int(L.gpk_kernel_vjp_workspace_bytes(ctypes.byref(kd), n, m, d, int(want_z)))
    work = torch.empty(max(1, (wb + 7) // 8), dtype=torch.float64, device=X.device)
    nat.check(L.gpk_kernel_vjp(ctypes.byref(kd), nat.ptr(hyp), nat.ptr(X), n, nat.ptr(Z), m, d,
                               nat.ptr(G) if G is not None else None, ldg,
                               nat.ptr(gu) if G is None else None, nat.ptr(gv) if G is None else None,
                               nat.ptr(gh), nat.ptr(gz) if want_z else None, nat.ptr(work), wb,
                               nat.stream_handle(X.device)), "gpk_kernel_vjp")
    return gh[:kd.n_hyp], gz


def kernel_jacobian(kernel, hyper_parameter, x, x_) -> torch.Tensor:
    """The derivative matrices of K = kernel(x, x_) (gpk_kernel_jacobian): a device tensor [n_hyp, n, m] whose plane p
    is d K / d (flat hyperparameter p, DFS order) -- the analytic derivatives kernel_vjp sums, every element written."""
    L = nat.lib()
    nat.require_fisher(L)
    X = as_device_f64(x).contiguous()
    Z = as_device_f64(x_).contiguous()
    n, d = int(X.shape[0]), int(X.shape[1])
    m = int(Z.shape[0])
    kd = kernel_descriptor(kernel, d)
    hyp = pack_hyper_parameter(hyper_parameter, kd.n_hyp)
    J = torch.empty((kd.n_hyp, n, m), dtype=torch.float64, device=X.device)
    if n == 0 or m == 0 or kd.n_hyp == 0:
        return J
    nat.check(L.gpk_kernel_jacobian(ctypes.byref(kd), nat.ptr(hyp), 0, 1, nat.ptr(X), n, 0, nat.ptr(Z), m, 0, d,
                                    nat.ptr(J), m, n * m, kd.n_hyp * n * m, None, 0, nat.stream_handle(X.device)),
              "gpk_kernel_jacobian")
    return J


def ski_weights(X: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """SKI interpolation weights [n, m] (gpk_ski_weights; StructuredKernelInterpolation.py:31-49)."""
    X = as_device_f64(X)
    Z = as_device_f64(Z)
    n, d = X.shape
    m = Z.shape[0]
    Wm = torch.empty((n, m), dtype=torch.float64, device=X.device)
    work = torch.empty(2 * n + 1, dtype=torch.float64, device=X.device)
    nat.check(nat.lib().gpk_ski_weights(nat.ptr(X), n, nat.ptr(Z), m, d, nat.ptr(Wm), nat.ptr(work),
                                        nat.stream_handle(X.device)), "gpk_ski_weights")
    return Wm


def add_diagonal(A: torch.Tensor, value: float) -> torch.Tensor:
    """A += value * I in place (gpk_add_diagonal)."""
    A3, lda, abs_ = _mat_args(A, "A")
    n = min(A3.shape[1], A3.shape[2])
    nat.check(nat.lib().gpk_add_diagonal(nat.ptr(A3), n, lda, abs_, A3.shape[0], float(value),
                                         nat.stream_handle(A.device)), "gpk_add_diagonal")
    return A


class DenseFactorization(AugmentedFactorization):
    """Augmented factorisation of a caller-supplied dense SPD matrix A + noise I (gpk_assemble_dense):
    the approximate covariance matrices of the metrics (Nystroem, SKI) go through the same blocked
    Cholesky as K.  ``inverse=True`` carries identity extra rows, so the corner holds -(A + noise I)^-1
    (read out by :meth:`k_inv`); ``m`` > 0 with explicit rows E gives -E A^-1 E^T in the corner."""

    def __init__(self, n: int, m: int = 0, batch: int = 1, inverse: bool = False):
        self.inverse = bool(inverse)
        super().__init__(n, 1, n if inverse else m, batch, torch.float64)

    def run(self, A: torch.Tensor, noise, y: Optional[torch.Tensor] = None, E: Optional[torch.Tensor] = None):
        return self._enqueue(self._run_once, A, noise, y, E)

    def _run_once(self, A, noise, y, E):
        A3, lda, abs_ = _mat_args(A, "A")
        B, n = self.batch, self.n
        if A3.shape[1] < n or A3.shape[2] < n or A3.shape[0] not in (1, B):
            raise ValueError("A must hold [%d, %d] per member" % (n, n))
        dev = self._dev
        noise_t = torch.as_tensor(noise, dtype=torch.float64).to(dev).reshape(-1).contiguous()
        if noise_t.numel() not in (1, B):
            raise ValueError("noise must be a scalar or one value per member")
        ns = 1 if noise_t.numel() == B and B > 1 else 0
        if y is None:
            y = torch.zeros(n, dtype=torch.float64, device=dev)
        y = y.to(device=dev, dtype=torch.float64).contiguous()
        ybs = n if y.numel() == B * n and B > 1 else 0
        _check_operand("y", y, ybs, n, B, dev)
        ebs = 0
        if self.m and not self.inverse:
            if E is None:
                raise ValueError("m = %d extra rows need E" % self.m)
            E = E.to(device=dev, dtype=torch.float64).contiguous()
            ebs = self.m * n if E.numel() == B * self.m * n and B > 1 else 0
            _check_operand("E", E, ebs, self.m * n, B, dev)
        s = nat.stream_handle(dev)
        L = self.L
        lay = self.layout
        self._info.zero_()
        self._alphas = None
        nat.check(L.gpk_assemble_dense(ctypes.byref(lay), nat.ptr(A3), lda, abs_, nat.ptr(noise_t), ns,
                                       nat.ptr(E) if E is not None else None, ebs, int(self.inverse),
                                       nat.ptr(y), ybs, nat.ptr(self._W), s), "gpk_assemble_dense")
        nat.check(L.gpk_potrf_aug_ex(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._Winv), nat.ptr(self._info),
                                     nat.AUG_EXTRA_IDENTITY if self.inverse else 0, s), "gpk_potrf_aug_ex")
        nat.check(L.gpk_finalize(ctypes.byref(lay), nat.ptr(self._W), nat.ptr(self._info), nat.ptr(self._out),
                                 nat.ptr(self._mu) if self.m else None, nat.ptr(self._var) if self.m else None, s),
                  "gpk_finalize")
        self.done = True
        return self

    def k_inv(self, b: int = 0) -> torch.Tensor:
        if not self.inverse:
            raise RuntimeError("DenseFactorization(..., inverse=True) carries the inverse")
        return -self.corner(b)


# ------------------------------------------------------------------------ multi-start L-BFGS state
class LbfgsState:
    """Device state of ``batch`` L-BFGS restarts advancing in lockstep (gpk_fit_init / gpk_fit_step /
    gpk_fit_current, include/gpk.h): owns the state buffer, ``x_trial`` [batch, n_par] and ``status`` [batch] int32.

    ``step(f, g, info)`` consumes the evaluation of ``x_trial`` (device tensors, read in place through their strides --
    e.g. the views sweep.native_batched_value_and_gradient returns) and writes the next ``x_trial``; nothing here
    synchronises with the host.  ``lo`` / ``hi``: [n_par] bounds shared by the members (None: unbounded)."""

    def __init__(self, x0: torch.Tensor, lo=None, hi=None, history: int = 8, max_iter: int = 200,
                 max_backtracks: int = 20, c1: float = 1e-4, gtol: float = 1e-5, ftol: float = 1e-9):
        self.L = nat.lib()
        if not nat.fit_supported(self.L):
            raise nat.NativeUnavailable("this libgpk.so was built before the gpk_fit_* entries existed: rebuild it")
        dev = device()
        x0 = as_device_f64(x0)
        if x0.dim() != 2:
            raise ValueError("x0 must be [batch, n_par]")
        self.batch, self.n_par = int(x0.shape[0]), int(x0.shape[1])
        self.opts = nat.GpkFitOpts(history, max_iter, max_backtracks, c1, gtol, ftol)
        nbytes = nat.fit_state_bytes(self.n_par, self.batch, self.opts)
        if nbytes == 0:
            raise ValueError("LbfgsState: %s" % nat.last_error())
        self.m = int(history)
        self.stride = nbytes // (8 * self.batch)
        inf = float("inf")
        self.lo = (torch.full((self.n_par,), -inf, dtype=torch.float64, device=dev) if lo is None
                   else as_device_f64(lo).reshape(-1))
        self.hi = (torch.full((self.n_par,), inf, dtype=torch.float64, device=dev) if hi is None
                   else as_device_f64(hi).reshape(-1))
        if self.lo.numel() != self.n_par or self.hi.numel() != self.n_par:
            raise ValueError("lo and hi must have n_par = %d values" % self.n_par)
        self.state = torch.empty((self.batch, self.stride), dtype=torch.float64, device=dev)
        self.x_trial = torch.empty((self.batch, self.n_par), dtype=torch.float64, device=dev)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.steps = 0
        nat.check(self.L.gpk_fit_init(self.n_par, self.batch, ctypes.byref(self.opts), nat.ptr(x0), self.n_par,
                                      nat.ptr(self.lo), nat.ptr(self.hi), nat.ptr(self.state), nat.ptr(self.x_trial),
                                      self.n_par, nat.stream_handle(dev)), "gpk_fit_init")

    @staticmethod
    def _strided(name: str, t: torch.Tensor, batch: int, row: Optional[int], dtype) -> int:
        """The row stride (elements) of a [batch] (row None) or [batch, row] device tensor whose rows are contiguous;
        the kernel reads batch rows blindly, so the extents are checked here."""
        if t.dtype != dtype or t.device.type != "cuda":
            raise ValueError("%s must be a %s device tensor" % (name, dtype))
        shape = (batch,) if row is None else (batch, row)
        if tuple(t.shape) != shape:
            raise ValueError("%s must have shape %s, not %s" % (name, list(shape), list(t.shape)))
        width = 1 if row is None else row
        if row is not None and row > 1 and t.stride(1) != 1:
            raise ValueError("%s: rows must be contiguous" % name)
        stride = int(t.stride(0)) if batch > 1 else max(int(t.stride(0)), width)
        if stride < width:
            raise ValueError("%s: row stride %d is smaller than the row (%d)" % (name, stride, width))
        return stride

    def step(self, f: torch.Tensor, g: torch.Tensor, info: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One gpk_fit_step launch; returns ``status`` (device int32, not synchronised)."""
        fs = self._strided("f", f, self.batch, None, torch.float64)
        gs = self._strided("g", g, self.batch, self.n_par, torch.float64)
        if info is not None and (info.dtype != torch.int32 or info.numel() != self.batch or not info.is_contiguous()
                                 or info.device.type != "cuda"):
            raise ValueError("info must be a contiguous int32 device tensor of %d values" % self.batch)
        nat.check(self.L.gpk_fit_step(self.n_par, self.batch, ctypes.byref(self.opts), nat.ptr(f), fs, nat.ptr(g), gs,
                                      nat.ptr(info), nat.ptr(self.state), nat.ptr(self.x_trial), self.n_par,
                                      nat.ptr(self.status), nat.stream_handle(self.state.device)), "gpk_fit_step")
        self.steps += 1
        return self.status

    def current(self):
        """(x [batch, n_par], f [batch], g [batch, n_par], iterations [batch] int32) of the accepted points."""
        dev = self.state.device
        x = torch.empty((self.batch, self.n_par), dtype=torch.float64, device=dev)
        g = torch.empty_like(x)
        f = torch.empty(self.batch, dtype=torch.float64, device=dev)
        it = torch.empty(self.batch, dtype=torch.int32, device=dev)
        nat.check(self.L.gpk_fit_current(self.n_par, self.batch, nat.ptr(self.state), nat.ptr(x), self.n_par,
                                         nat.ptr(f), nat.ptr(g), self.n_par, nat.ptr(it), nat.stream_handle(dev)),
                  "gpk_fit_current")
        return x, f, g, it

    # -- views of the state (include/gpk.h layout), for inspection --------------------------------
    def header(self) -> torch.Tensor:
        return self.state[:, :nat.FIT_HEADER]

    def _block(self, k: int) -> torch.Tensor:
        o = nat.FIT_HEADER + k * self.n_par
        return self.state[:, o:o + self.n_par]

    def ring(self):
        """(S [batch, m, n_par], Y [batch, m, n_par], rho [batch, m], pairs held [batch], next slot [batch])."""
        o = nat.FIT_HEADER + 5 * self.n_par
        rho = self.state[:, o:o + self.m]
        o += self.m
        S = self.state[:, o:o + self.m * self.n_par].view(self.batch, self.m, self.n_par)
        o += self.m * self.n_par
        Y = self.state[:, o:o + self.m * self.n_par].view(self.batch, self.m, self.n_par)
        return S, Y, rho, self.state[:, 4], self.state[:, 5]
