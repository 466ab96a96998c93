"""Time of the fitted predictor's pass (InverseFactorization.predict -> gpk_predict; not part of bench.py): scaled SE
at D = 1, fp64, n training points and m new points.  Per (n, m), in one run and in alternating samples:
  (i)   the new pass, mean and variance (also the mean alone, the variance alone and the K build k(Xs, X) alone, from
        which the time of predict_norm_kernel is estimated: variance-only pass minus K build);
  (ii)  the same numbers the way they were computed before: get_posterior_mu + get_posterior_var_diag of
        HolisticAuxiliaryGpProperties on a fresh DataInput that carries the m points as test points (one augmented
        factorisation of (n_pad + m + 1)^2 doubles); "does not fit" where the matrix cannot be allocated;
  (iii) the floor of the route: one gpk_dgemm of [rows, n] x [n, n] per chunk of the pass -- the dense product whose
        upper-triangular half the pass computes.
and once per n the construction of the predictor (the one factorisation).  HIP events around each; the median of the
samples, min and max next to it.  Prints one JSON line per case and writes all of them to --out."""
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
from gaussianprocessfundamentals_amd.DataHandling.DataInput import DataInput  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk  # noqa: E402
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction  # noqa: E402
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import GaussianProcess  # noqa: E402
from gaussianprocessfundamentals_amd.Statistics.Predictor import PosteriorPredictor  # noqa: E402

NOISE = 1e-2
HYP = [0.1, 1.3]


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summarise(res, samples):
    for k, v in samples.items():
        res[k] = round(statistics.median(v), 3)
        res[k + "_range"] = [round(min(v), 3), round(max(v), 3)]


def case(n, m, rounds, warmup, old_limit_gib):
    rng = np.random.default_rng(0)
    dev = engine.device()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    x = np.sort(rng.uniform(0, 1, (n, 1)), axis=0)
    y = (np.sin(9 * x[:, 0]) + 0.1 * rng.standard_normal(n)).reshape(-1, 1)
    xs = rng.uniform(-0.1, 1.1, (m, 1))
    gp.p_scaled_base_kernel = True
    kernel = bk.SquaredExponentialKernel(1)
    hl = [torch.tensor(v, dtype=torch.float64) for v in HYP]
    zero = ZeroMeanFunction(1)
    train = DataInput(x, y, x[:1], y[:1])
    train.set_mean_function(zero)
    Xs, X = t(xs), t(x)

    def construct():
        return PosteriorPredictor(kernel, hl, NOISE, zero, None, train)

    p = construct()
    f = p.factorization
    lay = f.layout
    per_row = 8 * (lay.n_pad + 1 + (n + 63) // 64)
    rows = min(m, max(64, f.PREDICT_WORK_BYTES // per_row // 64 * 64))
    A = t(rng.standard_normal((rows, n)))
    B = t(rng.standard_normal((n, n)))
    C = torch.empty((rows, n), dtype=torch.float64, device=dev)

    def floor():
        for c0 in range(0, m, rows):
            mc = min(rows, m - c0)
            engine.dgemm(A[:mc], B, C=C[:mc])

    old_gib = 8.0 * (lay.n_pad + m + 1) ** 2 / 2 ** 30
    old_note = None

    def old_way():
        di = DataInput(x, y, xs, np.zeros((m, 1)))
        di.set_mean_function(zero)
        g = GaussianProcess(kernel, zero)
        g.set_data_input(di)
        mu = g.aux.get_posterior_mu(hl, NOISE)
        var = g.aux.get_posterior_var_diag(hl, NOISE)
        return mu, var

    steps = {"pass_ms": lambda: f.predict(Xs), "mu_only_ms": lambda: f.predict(Xs, want_var=False),
             "var_only_ms": lambda: f.predict(Xs, want_mu=False),
             "kbuild_ms": lambda: engine.kernel_matrix(kernel, hl, Xs, X), "dgemm_floor_ms": floor,
             "construct_ms": construct}
    if old_gib <= old_limit_gib:
        try:
            mu_o, var_o = old_way()
            mu_n, var_n = f.predict(Xs)
            err = (float((mu_o - mu_n).abs().max()), float((var_o - var_n).abs().max()))
            del mu_o, var_o
            steps["old_way_ms"] = old_way
        except torch.cuda.OutOfMemoryError:
            old_note = "does not fit: the augmented matrix needs %.1f GiB" % old_gib
            err = None
        torch.cuda.empty_cache()
    else:
        old_note = "not run: the augmented matrix needs %.1f GiB (limit of this run %.0f GiB)" % (old_gib, old_limit_gib)
        err = None
    samples = {k: [] for k in steps}
    for r in range(warmup + rounds):   # alternating: one sample of each per round
        for k, fn in steps.items():
            ms = once(fn)
            if r >= warmup:
                samples[k].append(ms)
    res = {"kernel": "SE_scaled", "n": n, "m": m, "rounds": rounds, "rows_per_pass": rows,
           "workspace_mib": round(rows * per_row / 2 ** 20, 1), "old_way_matrix_gib": round(old_gib, 2)}
    summarise(res, samples)
    flops_tri = float(m) * n * (n + 1)          # 2 m n (n + 1) / 2: the triangular product
    norm_ms = max(res["var_only_ms"] - res["kbuild_ms"], 1e-6)
    res["norm_kernel_est_ms"] = round(norm_ms, 3)
    res["norm_kernel_est_tflops"] = round(flops_tri / (norm_ms * 1e9), 2)
    res["dgemm_tflops"] = round(2.0 * m * n * n / (res["dgemm_floor_ms"] * 1e9), 2)
    res["pass_over_dgemm_floor"] = round(res["pass_ms"] / res["dgemm_floor_ms"], 3)
    if "old_way_ms" in res:
        res["pass_over_old_way"] = round(res["pass_ms"] / res["old_way_ms"], 4)
        res["construct_plus_pass_over_old_way"] = round((res["construct_ms"] + res["pass_ms"]) / res["old_way_ms"], 4)
        res["max_abs_diff_to_old_way"] = {"mu": err[0], "var": err[1]}
    else:
        res["old_way_ms"] = old_note
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--points", type=int, nargs="*", default=[64, 4096, 65536])
    ap.add_argument("--old-limit-gib", type=float, default=64.0,
                    help="largest augmented matrix the old way is run with (GiB)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for n in a.sizes:
        for m in a.points:
            out.append(case(n, m, a.rounds, a.warmup, a.old_limit_gib))
            print(json.dumps(out[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
