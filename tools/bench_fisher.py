"""Time of the Fisher pass (InverseFactorization.fisher -> gpk_fisher) on one member (not part of bench.py): scaled SE
(P + 1 = 3) and ADD(SE, PER) (P + 1 = 4) at D = 1, fp64, N = 4096 and 8192.  Next to it, in the same run and in
alternating samples: the same number P of bare n x n x n gpk_dgemm calls (the floor of the direct route), the value +
gradient evaluation that precedes the pass (gpk_nlml_grad), and the P full derivative planes alone
(gpk_kernel_jacobian; the pass builds only their lower tiles).  HIP events around each; the median of the samples.
Prints one JSON line per configuration and writes all of them to --out."""
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
from gaussianprocessfundamentals_amd import engine  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def config(name, n, rounds, warmup):
    rng = np.random.default_rng(0)
    dev = engine.device()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    x = np.sort(rng.uniform(0, 1, (n, 1)), axis=0)
    y = np.sin(9 * x[:, 0]) + 0.1 * rng.standard_normal(n)
    if name == "SE_scaled":
        gp.p_scaled_base_kernel = True
        kernel, hyp = bk.SquaredExponentialKernel(1), [0.1, 1.3]
    else:
        gp.p_scaled_base_kernel = False
        kernel = ops.AdditionOperator(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1)])
        hyp = [0.1, 0.9, 0.5]
    kd = engine.kernel_descriptor(kernel, 1)
    P = kd.n_hyp
    H, nz, X, Y = t(hyp), t([1e-2]), t(x), t(y).reshape(1, -1)
    inv = engine.InverseFactorization(n, 1, 1, torch.float64)
    A, B = t(rng.standard_normal((n, n))), t(rng.standard_normal((P, n, n)))
    C = torch.empty_like(B)
    hl = [torch.tensor(v, dtype=torch.float64) for v in hyp]

    def value_and_gradient():
        inv.run(kd, H, 0, nz, 0, X, 0, Y, 0, gradient=True)

    def gemms():
        for p in range(P):
            engine.dgemm(A, B[p], C=C[p])

    steps = {"nlml_grad_ms": value_and_gradient, "fisher_ms": inv.fisher, "dgemm_floor_ms": gemms,
             "jacobian_full_ms": lambda: engine.kernel_jacobian(kernel, hl, X, X)}
    samples = {k: [] for k in steps}
    for r in range(warmup + rounds):   # alternating: one sample of each per round
        for k, fn in steps.items():
            ms = once(fn)
            if r >= warmup:
                samples[k].append(ms)
    inv.check_info()
    res = {"kernel": name, "n": n, "n_hyp_plus_noise": P + 1, "rounds": rounds}
    for k, v in samples.items():
        res[k] = round(statistics.median(v), 3)
        res[k + "_range"] = [round(min(v), 3), round(max(v), 3)]
    res["dgemm_tflops"] = round(2.0 * P * n ** 3 / (res["dgemm_floor_ms"] * 1e9), 2)
    res["fisher_over_dgemm_floor"] = round(res["fisher_ms"] / res["dgemm_floor_ms"], 3)
    res["fisher_over_nlml_grad"] = round(res["fisher_ms"] / res["nlml_grad_ms"], 3)
    res["workspace_mib"] = round(inv.work.numel() * 8 / 2 ** 20, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for n in a.sizes:
        for name in ("SE_scaled", "ADD(SE,PER)"):
            out.append(config(name, n, a.rounds, a.warmup))
            print(json.dumps(out[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
