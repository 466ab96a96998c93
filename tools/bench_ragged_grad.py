"""-LML + gradient of members of different sizes: ONE ragged identity-augmented batch
(engine.RaggedInverseFactorization: gpk_assemble_inverse_ragged, gpk_potrf_aug_ragged_ex, gpk_finalize_ragged,
gpk_grad_ragged) against what the library offered for the same gradients before it: one
engine.InverseFactorization(batch = 1).run(gradient=True) per member (gpk_nlml_grad).

usage: python tools/bench_ragged_grad.py [--reps 15] [--warmup 3] [--out FILE]
Shapes: 8 segments between 600 and 1400 points; the 5 folds of n = 4096 (test_ratio 0.2: 819 points held out of each,
3277 training points).  SE, d = 1, fp64.  Both sides are warmed up, then timed alternately in the
same process with HIP events around the enqueue of one whole evaluation (operands already packed on the device; the
per-member side reuses one factorisation object per member); median [min - max] ms over the repetitions.  The results
are compared first (-LML and gradient of every member, ragged against per-member) and the worst differences printed.
"""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import gaussianprocessfundamentals_amd.global_parameters as gp  # noqa: E402

gp.init(0)
from gaussianprocessfundamentals_amd import _native as nat  # noqa: E402
from gaussianprocessfundamentals_amd import engine  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk  # noqa: E402

NOISE = 1e-2


def fold_sizes(n, test_ratio=0.2):
    """training points of the folds of Metrics/CrossValidation.get_data_inputs"""
    n_test = int(round(n * test_ratio))
    out, at = [], 0
    for _ in range(int(np.floor(1 / test_ratio))):
        out.append(n - (min(n, at + n_test) - at))
        at += n_test
    return out


def make_members(sizes, dev):
    kd = engine.kernel_descriptor(bk.SquaredExponentialKernel(1), 1)
    gen = torch.Generator(device="cpu").manual_seed(7)
    members = []
    for b, nb in enumerate(sizes):
        x = torch.sort(torch.rand(nb, 1, dtype=torch.float64, generator=gen), dim=0).values
        y = torch.sin(12.0 * x[:, 0]) + 0.1 * torch.randn(nb, dtype=torch.float64, generator=gen)
        h = torch.tensor([0.05 + 0.01 * b], dtype=torch.float64)
        members.append((kd, h.to(dev), x.to(dev).contiguous(), y.to(dev).contiguous()))
    return kd, members


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def run_case(name, sizes, reps, warmup):
    dev = engine.device()
    kd, members = make_members(sizes, dev)
    B, n = len(sizes), max(sizes)
    # ragged: operands packed once, run_packed per evaluation
    rag = engine.RaggedInverseFactorization(sizes, 1)
    X = torch.zeros((B, n, 1), dtype=torch.float64, device=dev)
    Y = torch.zeros((B, n), dtype=torch.float64, device=dev)
    H = torch.zeros((B, nat.MAX_HYP), dtype=torch.float64, device=dev)
    for b, (_, h, x, y) in enumerate(members):
        X[b, :sizes[b]], Y[b, :sizes[b]], H[b, :1] = x, y, h
    NZ = torch.full((B,), NOISE, dtype=torch.float64, device=dev)
    kds = [kd] * B

    def ragged():
        rag.run_packed(kds, H, NZ, X, Y, gradient=True)

    # per member: one InverseFactorization(batch 1) each, as before the ragged entries
    singles = [engine.InverseFactorization(nb, 1, 1) for nb in sizes]
    nz1 = NZ[:1].contiguous()
    ys = [m[3].reshape(1, -1).contiguous() for m in members]

    def per_member():
        for f, (_, h, x, _), y in zip(singles, members, ys):
            f.run(kd, h, 1, nz1, 0, x, 0, y, 0, gradient=True)

    for _ in range(warmup):
        ragged()
        per_member()
    torch.cuda.synchronize()
    # same results first
    d_nl = max(abs(float(rag.nlml()[b]) - float(singles[b].nlml()[0])) / abs(float(singles[b].nlml()[0]))
               for b in range(B))
    d_g = max(float((rag.gradient(b) - singles[b].gradient()[0]).abs().max()) /
              max(1.0, float(singles[b].gradient()[0].abs().max())) for b in range(B))
    info = int(rag.info.abs().max().item())
    t_r, t_s = [], []
    for _ in range(reps):     # alternating, one repetition each
        t_r += timed(ragged, 1)
        t_s += timed(per_member, 1)

    def stat(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    return {"case": name, "sizes": sizes, "reps": reps, "ragged": stat(t_r), "per_member": stat(t_s),
            "ratio_per_member_over_ragged": round(statistics.median(t_s) / statistics.median(t_r), 3),
            "max_rel_dnlml": d_nl, "max_scaled_dgrad": d_g, "info": info,
            "per_member_took_persistent_launch": bool(nat.last_factorisation_was_chain())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_grad needs the GPU: no timing is taken without one")
    seg = [int(v) for v in np.linspace(600, 1400, 8).round()]
    rows = [run_case("8 segments of 600 .. 1400", seg, args.reps, args.warmup),
            run_case("5 folds of n = 4096", fold_sizes(4096), args.reps, args.warmup)]
    text = "\n".join(json.dumps(r) for r in rows)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
