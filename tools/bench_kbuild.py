"""Kernel-matrix build (gpk_assemble into the augmented layout) on its own: time, HBM rate of the lower
tiles written, and element rate, for the SURVEY configs whose K build is not fused into the first
trailing update.

usage: python tools/bench_kbuild.py [case ...]   (cases: C5, C3, SE8192, LIN, RQ, CP; default C5 C3 SE8192)
C5: ADD(SE-ARD, PER standard) D=8, N=16384 fp64; C3: MAT52-ARD D=4, N=8192 fp32; SE8192: SE D=1, N=8192
fp64 batch 32 (the metric's inputs, built unfused).  Median, min and max of 10 launches, HIP events on the stream.
LIN: the single-node LIN build against the single-node SE build through the same plain assemble launch, N = 8192,
D = 1 and D = 8, fp64 and fp32 out (gpk_tune asm_f32_fast 0 for both, so SE's f32 build takes the same path): the
two kernels alternate inside one run, 20 samples of 10 launches each; median, min and max (the run's own spread).
RQ: the single-node RQ build against the single-node SE build by LIN's method, fp64 only (RQ programs have their own
instantiation of the assemble kernel, SE takes the single-node one: both through the plain assemble launch).
CP: the change-point device program (run_cp), same method.
"""
import ctypes
import hashlib
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import gaussianprocessfundamentals_amd.global_parameters as gp  # noqa: E402

gp.init(0)
import bench  # noqa: E402
from gaussianprocessfundamentals_amd import _native as nat  # noqa: E402
from gaussianprocessfundamentals_amd import engine  # noqa: E402


def run(case):
    cfg = {"C5": ("C5", 1), "C3": ("C3", 1), "SE8192": ("metric", 32)}[case]
    name, batch = cfg
    kname, d, n, noise, dtn, hyp = bench.CONFIGS[name]
    dtype = torch.float32 if dtn == "f32" else torch.float64
    dev = torch.device("cuda", 0)
    kern = bench.build_kernel(kname, d)
    kd = engine.kernel_descriptor(kern, d)
    f = engine.AugmentedFactorization(n, d, 0, batch, dtype)
    lay = f.layout
    g = torch.Generator().manual_seed(7)
    X = torch.rand(n, d, generator=g, dtype=torch.float64).to(dev).contiguous()
    Y = torch.rand(1, n, generator=g, dtype=torch.float64).to(dev).contiguous()
    H = (0.3 + torch.rand(batch, kd.n_hyp, generator=g, dtype=torch.float64)).to(dev).contiguous()
    NZ = torch.tensor([noise], dtype=torch.float64, device=dev)
    L = nat.lib()
    s = nat.stream_handle(dev)

    def asm():
        nat.check(L.gpk_assemble(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(H), kd.n_hyp, nat.ptr(NZ), 0,
                                 nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W), s), "gpk_assemble")

    for _ in range(3):
        asm()
    torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        asm()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ms = statistics.median(ts)
    w0 = f.w(0)
    digest = hashlib.sha256(torch.tril(w0[:lay.p, :lay.p]).cpu().numpy().tobytes()).hexdigest()[:16]
    es = 4 if dtype == torch.float32 else 8
    lower = batch * lay.p * (lay.p + 64) / 2
    return {"case": case, "n": n, "d": d, "batch": batch, "kernel": kname, "dtype": dtn, "ms": round(ms, 3),
            "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "GBps_lower_tiles": round(lower * es / (ms * 1e-3) / 1e9, 1),
            "Gelem_per_s": round(batch * n * (n + 1) / 2 / (ms * 1e-3) / 1e9, 2), "w0": digest}


def run_leaves(case="LIN", n=8192, samples=20, inner=10):
    """Rows for SE and the leaf ``case`` (LIN or RQ; one node each) at D = 1 / 8, fp64 / fp32 out (RQ: fp64 only),
    alternating inside each sample."""
    from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
    leaf = {"LIN": bk.LinearKernel, "RQ": bk.RationalQuadraticKernel}[case]
    dtypes = ((torch.float64, "f64"), (torch.float32, "f32")) if case == "LIN" else ((torch.float64, "f64"),)
    dev = torch.device("cuda", 0)
    L = nat.lib()
    s = nat.stream_handle(dev)
    rows = []
    old = nat.tune("asm_f32_fast", 0)
    try:
        for dtype, dtn in dtypes:
            for d in (1, 8):
                g = torch.Generator().manual_seed(7)
                X = torch.rand(n, d, generator=g, dtype=torch.float64).to(dev).contiguous()
                Y = torch.rand(1, n, generator=g, dtype=torch.float64).to(dev).contiguous()
                NZ = torch.tensor([0.1], dtype=torch.float64, device=dev)
                f = engine.AugmentedFactorization(n, d, 0, 1, dtype)
                lay = f.layout
                progs = {}
                for name, kern in (("SE", bk.SquaredExponentialKernel(d)), (case, leaf(d))):
                    kd = engine.kernel_descriptor(kern, d)
                    H = (0.3 + torch.rand(1, kd.n_hyp, generator=g, dtype=torch.float64)).to(dev).contiguous()
                    progs[name] = (kd, H)

                def asm(name):
                    kd, H = progs[name]
                    nat.check(L.gpk_assemble(ctypes.byref(kd), ctypes.byref(lay), nat.ptr(H), kd.n_hyp, nat.ptr(NZ), 0,
                                             nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W), s),
                              "gpk_assemble")

                for name in progs:
                    for _ in range(3):
                        asm(name)
                torch.cuda.synchronize()
                ts = {name: [] for name in progs}
                for _ in range(samples):
                    for name in progs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(inner):
                            asm(name)
                        e1.record()
                        torch.cuda.synchronize()
                        ts[name].append(e0.elapsed_time(e1) / inner)
                es = 4 if dtype == torch.float32 else 8
                lower = lay.p * (lay.p + 64) / 2
                for name in progs:
                    ms = statistics.median(ts[name])
                    rows.append({"case": case, "kernel": name, "n": n, "d": d, "dtype": dtn, "ms": round(ms, 4),
                                 "ms_min": round(min(ts[name]), 4), "ms_max": round(max(ts[name]), 4),
                                 "GBps_lower_tiles": round(lower * es / (ms * 1e-3) / 1e9, 1)})
    finally:
        nat.tune("asm_f32_fast", old)
    return rows


def run_cp(n=8192, samples=20, inner=10):
    """CP([SE, SE, SE], [1/3, 2/3]) on sorted uniform x in [0, 1], INDICATOR and SIGMOID masks: the one device program
    with gpk_tune cp_skip 1 and 0 (augmented layout: the lower tiles) against the single-node SE build through the
    same launch and against the operator's get_tf_tensor composition (three full n x n child matrices and the torch
    mask arithmetic: the full square, and the only way to this matrix without the device program).  All variants
    alternate inside every sample."""
    from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
    from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
    dev = torch.device("cuda", 0)
    L = nat.lib()
    s = nat.stream_handle(dev)
    g = torch.Generator().manual_seed(7)
    X = torch.sort(torch.rand(n, generator=g, dtype=torch.float64))[0].reshape(n, 1).to(dev).contiguous()
    Y = torch.rand(1, n, generator=g, dtype=torch.float64).to(dev).contiguous()
    NZ = torch.tensor([0.1], dtype=torch.float64, device=dev)
    f = engine.AugmentedFactorization(n, 1, 0, 1, torch.float64)
    lay = f.layout
    cps = [torch.tensor(1.0 / 3.0, dtype=torch.float64), torch.tensor(2.0 / 3.0, dtype=torch.float64)]
    hyp = cps + [torch.tensor(v, dtype=torch.float64) for v in (0.05, 0.1, 0.2)]
    cp_kernel = ops.ChangePointOperator(1, [bk.SquaredExponentialKernel(1) for _ in range(3)], cps)
    se_kd = engine.kernel_descriptor(bk.SquaredExponentialKernel(1), 1)
    se_h = torch.tensor([[0.1]], dtype=torch.float64, device=dev)
    rows = []
    old_skip = nat.tune("cp_skip", 1)
    old_mode = gp.p_cp_operator_type
    try:
        for mode in ("INDICATOR", "SIGMOID"):
            gp.p_cp_operator_type = gp.ChangePointOperatorType[mode]
            kd = engine.kernel_descriptor(cp_kernel, 1)
            H = engine.pack_hyper_parameter(hyp, kd.n_hyp).reshape(1, -1).contiguous()

            def asm(kdesc, hv):
                nat.check(L.gpk_assemble(ctypes.byref(kdesc), ctypes.byref(lay), nat.ptr(hv), kdesc.n_hyp, nat.ptr(NZ), 0,
                                         nat.ptr(X), 0, None, 0, None, 0, nat.ptr(Y), 0, nat.ptr(f.W), s), "gpk_assemble")

            def cp_build(skip):
                nat.tune("cp_skip", skip)
                asm(kd, H)

            variants = {"SE": lambda: asm(se_kd, se_h), "CP skip": lambda: cp_build(1), "CP no skip": lambda: cp_build(0),
                        "CP get_tf_tensor": lambda: cp_kernel.get_tf_tensor(hyp, X, X)}
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ts = {name: [] for name in variants}
            for _ in range(samples):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inner):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[name].append(e0.elapsed_time(e1) / inner)
            digests = {}
            for skip in (1, 0):
                cp_build(skip)
                torch.cuda.synchronize()
                digests[skip] = hashlib.sha256(torch.tril(f.w(0)[:n, :n]).cpu().numpy().tobytes()).hexdigest()[:16]
            for name in variants:
                ms = statistics.median(ts[name])
                rows.append({"case": "CP", "mode": mode, "variant": name, "n": n, "ms": round(ms, 4),
                             "ms_min": round(min(ts[name]), 4), "ms_max": round(max(ts[name]), 4),
                             "elements": "full square" if name == "CP get_tf_tensor" else "lower tiles",
                             "w0_skip": digests[1], "w0_no_skip": digests[0]})
    finally:
        nat.tune("cp_skip", old_skip)
        gp.p_cp_operator_type = old_mode
    return rows


if __name__ == "__main__":
    for c in sys.argv[1:] or ["C5", "C3", "SE8192"]:
        if c == "CP":
            for row in run_cp():
                print(json.dumps(row), flush=True)
        elif c in ("LIN", "RQ"):
            for row in run_leaves(c):
                print(json.dumps(row), flush=True)
        else:
            print(json.dumps(run(c)), flush=True)
