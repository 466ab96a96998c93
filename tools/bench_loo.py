"""Time of one batched leave-one-out value + gradient evaluation (gpk_loo_grad) against one -LML value + gradient
evaluation (gpk_nlml_grad) on the same data (not part of bench.py): SE at D = 1, fp64, N = 4096 with 16 candidates and
N = 256 with 64 candidates.  HIP events around each evaluation.  Also the value-only LOO call (grad_dev == NULL)
against the -LML evaluation without its gradient, the LOO pass alone (gpk_loo_backward) split by gpk_timing_read's
launch classes ("finalize" the read-out, "trsv" the matrix-vector product, "update" the cotangent kernel with its
flops, "grad" the tile pass), and the factorisation's own "update" class at the same N to set the cotangent kernel's
TFLOP/s against the trailing update's.  Prints one JSON line per configuration and appends a table to --out."""
import argparse
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


def classes(fn, reps):
    """gpk_timing_read per evaluation of fn(): {class: (ms, TFLOP/s or None)}."""
    nat.timing_enable(True)
    nat.timing_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    tr = nat.timing_read()
    nat.timing_enable(False)
    return {k: {"ms": round(v["ms"] / reps, 4),
                "tflops": round(v["flops"] / (v["ms"] * 1e9), 3) if v["flops"] > 0 and v["ms"] > 0 else None}
            for k, v in tr.items() if v["launches"] > 0}


def config(n, B, loss, reps, warmup):
    rng = np.random.default_rng(0)
    dev = engine.device()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    x = np.sort(rng.uniform(0, 1, (n, 1)), axis=0)
    y = np.sin(9 * x[:, 0]) + 0.1 * rng.standard_normal(n)
    kernel = SquaredExponentialKernel(1)
    cands = t(np.column_stack([np.linspace(0.05, 0.3, B), np.full(B, 1e-2)])).contiguous()
    ev_loo = sweep.native_batched_loo_value_and_gradient(kernel, t(x), t(y), loss)
    ev_lml = sweep.native_batched_value_and_gradient(kernel, t(x), t(y))
    res = {"n": n, "batch": B, "loss": "lpd" if loss == nat.LOO_LPD else "mse", "reps": reps}
    res["loo_grad_ms"] = timed(lambda: ev_loo(cands), reps, warmup)
    res["nlml_grad_ms"] = timed(lambda: ev_lml(cands), reps, warmup)
    kd = engine.kernel_descriptor(kernel, 1)
    inv = engine.InverseFactorization(n, 1, B, torch.float64)
    c0, Xd, Yd = cands.reshape(-1), t(x), t(y).reshape(1, -1)
    # value only: the LOO call with grad_dev == NULL against the -LML evaluation without its gradient
    res["loo_value_ms"] = timed(lambda: inv.run_loo(loss, kd, c0, 2, c0[1:], 2, Xd, 0, Yd, 0, gradient=False), reps,
                                warmup)
    res["nlml_value_ms"] = timed(lambda: inv.run(kd, c0, 2, c0[1:], 2, Xd, 0, Yd, 0, gradient=False), reps, warmup)
    res["factorisation_classes"] = classes(lambda: inv.run(kd, c0, 2, c0[1:], 2, Xd, 0, Yd, 0, gradient=False), reps)
    # the pass alone on that factorisation
    res["backward_ms"] = timed(lambda: inv.loo(loss, gradient=True), reps, warmup)
    res["pass_classes"] = classes(lambda: inv.loo(loss, gradient=True), reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--loss", default="lpd", choices=("lpd", "mse"))
    a = ap.parse_args()
    loss = nat.loo_loss_code(a.loss)
    configs = [(256, 64)] + ([] if a.small_only else [(4096, 16)])
    lines = []
    for n, B in configs:
        r = config(n, B, loss, a.reps, a.warmup)
        print(json.dumps({k: (v if not isinstance(v, list) else [round(t, 4) for t in v]) for k, v in r.items()}),
              flush=True)
        lines.append("N = %d, B = %d, loss %s (ms, median [min - max] of %d)" % (n, B, a.loss, a.reps))
        for key in ("loo_grad_ms", "nlml_grad_ms", "loo_value_ms", "nlml_value_ms", "backward_ms"):
            lines.append("  %-14s %s" % (key[:-3], fmt(r[key])))
        lines.append("  LOO pass by launch class (event-timed, per evaluation): %s" % json.dumps(r["pass_classes"]))
        lines.append("  factorisation by launch class (the same N and B):      %s"
                     % json.dumps(r["factorisation_classes"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
