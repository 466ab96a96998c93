"""Time of the predictor's joint covariance (PosteriorPredictor.covariance -> gpk_predict_vt + gpk_predict_cov; not
part of bench.py): scaled SE at D = 1, fp64, n training points and m new points.  Per (n, m), in one run and in
alternating samples:
  (i)   covariance(x_new) with the predictor in hand, and its two steps alone: predict_vt (K build of (Xs, X) + V') and
        the symmetric gpk_predict_cov on a V' already computed (K build of (Xs, Xs) + the product); the K builds alone,
        from which the two MFMA kernels' own times are estimated; the two-set (full) product on the same operands;
  (ii)  the same matrix the way it was computed before: get_posterior_var of HolisticAuxiliaryGpProperties on a fresh
        DataInput that carries the m points as test points (one augmented factorisation of (n_pad + m + 1)^2 doubles);
  (iii) two dense floors from existing code on the same shapes: gpk_dgemm [m, n] x [n, n] (the dense product whose
        upper-triangular half V' is) and gpk_dgemm Va Va^T [m, n] x [n, m] (the full product whose lower half the
        symmetric mode computes);
and once per n the construction of the predictor (the one factorisation).  HIP events around each; the median of the
samples, min and max next to it.  Prints one JSON line per case and writes all of them to --out."""
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


def case(n, m, rounds, warmup):
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
    ld = int(lay.n_pad)
    L = f.L
    kd, hyp = f.kd, f._loo_operands[1]
    s = nat.stream_handle(dev)
    Va = f.predict_vt(Xs)                     # [m, n] view of [m, n_pad]
    C = torch.empty((m, m), dtype=torch.float64, device=dev)

    def cov_only(symmetric):
        nat.check(L.gpk_predict_cov(ctypes.byref(kd), 1, nat.ptr(hyp), nat.ptr(Xs), m,
                                           nat.ptr(Va), ld, nat.ptr(Xs), m, nat.ptr(Va), ld, n,
                                           nat.ptr(C), m, symmetric, s), "gpk_predict_cov")

    A = t(rng.standard_normal((m, n)))
    B = t(rng.standard_normal((n, n)))
    D = torch.empty((m, n), dtype=torch.float64, device=dev)
    Vd = Va.contiguous()
    G = torch.empty((m, m), dtype=torch.float64, device=dev)

    def old_way():
        di = DataInput(x, y, xs, np.zeros((m, 1)))
        di.set_mean_function(zero)
        g = GaussianProcess(kernel, zero)
        g.set_data_input(di)
        return g.aux.get_posterior_var(hl, NOISE)

    steps = {"covariance_ms": lambda: p.covariance(Xs), "predict_vt_ms": lambda: f.predict_vt(Xs),
             "cov_sym_ms": lambda: cov_only(1), "cov_full_ms": lambda: cov_only(0),
             "kbuild_sx_ms": lambda: engine.kernel_matrix(kernel, hl, Xs, X),
             "kbuild_ss_ms": lambda: engine.kernel_matrix(kernel, hl, Xs, Xs),
             "dgemm_vt_floor_ms": lambda: engine.dgemm(A, B, C=D),
             "dgemm_full_product_ms": lambda: engine.dgemm(Vd, Vd, trans_b=True, C=G),
             "construct_ms": construct, "old_way_ms": old_way}
    S_old = old_way()
    S_new = p.covariance(Xs)
    err = float((S_old - S_new).abs().max())
    del S_old, S_new
    torch.cuda.empty_cache()
    samples = {k: [] for k in steps}
    for r in range(warmup + rounds):   # alternating: one sample of each per round
        for k, fn in steps.items():
            ms = once(fn)
            if r >= warmup:
                samples[k].append(ms)
    res = {"kernel": "SE_scaled", "n": n, "m": m, "rounds": rounds,
           "old_way_matrix_gib": round(8.0 * (lay.n_pad + m + 1) ** 2 / 2 ** 30, 2)}
    summarise(res, samples)
    vt_ms = max(res["predict_vt_ms"] - res["kbuild_sx_ms"], 1e-6)
    sym_ms = max(res["cov_sym_ms"] - res["kbuild_ss_ms"], 1e-6)
    full_ms = max(res["cov_full_ms"] - res["kbuild_ss_ms"], 1e-6)
    res["vt_kernel_est_ms"] = round(vt_ms, 3)
    res["vt_kernel_est_tflops"] = round(float(m) * n * (n + 1) / (vt_ms * 1e9), 2)
    res["sym_product_est_ms"] = round(sym_ms, 3)
    res["sym_product_est_tflops"] = round(float(m) * (m + 1) * n / (sym_ms * 1e9), 2)
    res["full_product_est_ms"] = round(full_ms, 3)
    res["dgemm_vt_tflops"] = round(2.0 * m * n * n / (res["dgemm_vt_floor_ms"] * 1e9), 2)
    res["dgemm_full_product_tflops"] = round(2.0 * m * m * n / (res["dgemm_full_product_ms"] * 1e9), 2)
    res["vt_over_dgemm_floor"] = round(res["predict_vt_ms"] / res["dgemm_vt_floor_ms"], 3)
    res["sym_product_over_dgemm_full_product"] = round(sym_ms / res["dgemm_full_product_ms"], 3)
    res["cov_sym_over_dgemm_full_product"] = round(res["cov_sym_ms"] / res["dgemm_full_product_ms"], 3)
    res["covariance_over_old_way"] = round(res["covariance_ms"] / res["old_way_ms"], 4)
    res["construct_plus_covariance_over_old_way"] = round((res["construct_ms"] + res["covariance_ms"]) /
                                                          res["old_way_ms"], 4)
    res["max_abs_diff_to_old_way"] = err
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--points", type=int, nargs="*", default=[64, 1024, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for n in a.sizes:
        for m in a.points:
            out.append(case(n, m, a.rounds, a.warmup))
            print(json.dumps(out[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
