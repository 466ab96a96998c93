"""Time of one batched MSE value + gradient evaluation (gpk_mse_grad) against one -LML value + gradient evaluation
(gpk_nlml_grad) on the same training data (not part of bench.py): SE at D = 1, N = 4096 with m = 1024 test points and
16 candidates, and N = 256, m = 64, 64 candidates.  HIP events around each evaluation; the MSE evaluation is also
split into K build, factorisation, residual + right-hand sides, the two backward solves and the tile pass by running
the public entries one after the other (gpk_assemble, gpk_potrf_aug, gpk_mse_backward) and by gpk_timing_read's
classes for the pass.  Prints one JSON line per configuration and appends a table to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gaussianprocessfundamentals_amd.global_parameters as gp  # noqa: E402

gp.init(0)
from gaussianprocessfundamentals_amd import _native as nat  # noqa: E402
from gaussianprocessfundamentals_amd import engine, sweep  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics.BaseKernels import SquaredExponentialKernel  # noqa: E402


def timed(fn, reps, warmup):
    """[ms] of fn() per repetition, HIP events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ms):
    return "%.3f [%.3f - %.3f]" % (statistics.median(ms), min(ms), max(ms))


def config(n, m, B, reps, warmup):
    rng = np.random.default_rng(0)
    dev = engine.device()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    x, xs = np.sort(rng.uniform(0, 1, (n, 1)), axis=0), rng.uniform(0, 1, (m, 1))
    y, ys = np.sin(9 * x[:, 0]) + 0.1 * rng.standard_normal(n), np.sin(9 * xs[:, 0]) + 0.1 * rng.standard_normal(m)
    kernel = SquaredExponentialKernel(1)
    cands = t(np.column_stack([np.linspace(0.05, 0.3, B), np.full(B, 1e-2)])).contiguous()
    ev_mse = sweep.native_batched_mse_value_and_gradient(kernel, t(x), t(y), t(xs), t(ys))
    ev_lml = sweep.native_batched_value_and_gradient(kernel, t(x), t(y))
    res = {"n": n, "m": m, "batch": B, "reps": reps}
    res["mse_grad_ms"] = timed(lambda: ev_mse(cands), reps, warmup)
    res["nlml_grad_ms"] = timed(lambda: ev_lml(cands), reps, warmup)
    # the -LML evaluation without its gradient pass: K build + identity-augmented factorisation + read-out
    kd0 = engine.kernel_descriptor(kernel, 1)
    inv = engine.InverseFactorization(n, 1, B, torch.float64)
    c0, Xd, Yd = cands.reshape(-1), t(x), t(y).reshape(1, -1)
    res["nlml_inverse_ms"] = timed(lambda: inv.run(kd0, c0, 2, c0[1:], 2, Xd, 0, Yd, 0, gradient=False), reps, warmup)

    # the MSE evaluation's parts through the public entries on one factorisation object
    kd = engine.kernel_descriptor(kernel, 1)
    f = engine.AugmentedFactorization(n, 1, m, B, torch.float64)
    L, lay, s = f.L, f.layout, nat.stream_handle(dev)
    flat, w = cands.reshape(-1), kd.n_hyp + 1
    X, Y, Xs, Ys = t(x), t(y).reshape(1, -1), t(xs), t(ys).reshape(1, -1)

    def assemble():
        f._info.zero_()
        nat.check(L.gpk_assemble(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(flat), w, nat.ptr(flat[kd.n_hyp:]), w,
                                 nat.ptr(X), 0, nat.ptr(Xs), 0, None, 0, nat.ptr(Y), 0, nat.ptr(f._W), s), "assemble")

    def potrf():
        nat.check(L.gpk_potrf_aug(ctypes.byref(lay), nat.ptr(f._W), nat.ptr(f._Winv), nat.ptr(f._info), s), "potrf")

    f.run(kd, flat, w, flat[kd.n_hyp:], w, X, 0, Y, 0, Xs=Xs, xs_bstride=0)
    res["assemble_ms"] = timed(assemble, reps, warmup)
    # (the factorisation overwrites W: rebuild it before every timed factorisation, outside the events)
    pot = []
    for _ in range(reps + warmup):
        assemble()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        potrf()
        b.record()
        b.synchronize()
        pot.append(a.elapsed_time(b))
    res["potrf_ms"] = pot[warmup:]
    res["backward_ms"] = timed(lambda: f.mse_gradient(Ys, 0), reps, warmup)
    # the pass by launch class: "finalize" the residual kernel, "trsv" the two backward solves, "grad" the tile pass
    # and its reduction
    nat.timing_enable(True)
    nat.timing_reset()
    for _ in range(reps):
        f.mse_gradient(Ys, 0)
    torch.cuda.synchronize()
    tr = nat.timing_read()
    nat.timing_enable(False)
    res["pass_classes_ms_per_eval"] = {k: round(v["ms"] / reps, 4) for k, v in tr.items() if v["launches"] > 0}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    configs = [(256, 64, 64)] + ([] if a.small_only else [(4096, 1024, 16)])
    lines = []
    for n, m, B in configs:
        r = config(n, m, B, a.reps, a.warmup)
        print(json.dumps({k: (v if not isinstance(v, list) else [round(t, 4) for t in v]) for k, v in r.items()}),
              flush=True)
        lines.append("N = %d, m = %d, B = %d (ms, median [min - max] of %d)" % (n, m, B, a.reps))
        for key in ("mse_grad_ms", "nlml_grad_ms", "nlml_inverse_ms", "assemble_ms", "potrf_ms", "backward_ms"):
            lines.append("  %-14s %s" % (key[:-3], fmt(r[key])))
        lines.append("  pass by launch class (event-timed, ms per evaluation): %s"
                     % json.dumps(r["pass_classes_ms_per_eval"], default=str))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
