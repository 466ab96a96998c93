"""Time per iteration of the multi-start fitter (not part of bench.py): SE at D = 1, N = 256 with 64 starts and
N = 4096 with 16 starts.  Every iteration is split with HIP events into the batched value + gradient evaluation and
the step; the same loop runs once with the device step (gpk_fit_step) and once with the step restated in torch ops
(TorchStep below -- kept in this tool, not product code: the same state machine as masked batched tensor
operations, no host synchronisation either).  Prints one JSON line per configuration and appends a table to --out."""
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
from gaussianprocessfundamentals_amd import engine, sweep  # noqa: E402
from gaussianprocessfundamentals_amd.KernelBasics.BaseKernels import SquaredExponentialKernel  # noqa: E402
from gaussianprocessfundamentals_amd.Optimizer.Fitter import pack_bounds  # noqa: E402


class TorchStep:
    """include/gpk.h's state machine over [B, P] tensors; every branch is a torch.where on a [B] mask."""

    def __init__(self, x0, lo, hi, m=8, max_iter=200, max_backtracks=20, c1=1e-4, gtol=1e-5, ftol=1e-9):
        B, P = x0.shape
        dv, f64 = x0.device, torch.float64
        self.lo, self.hi, self.m, self.o = lo, hi, m, (max_iter, max_backtracks, c1, gtol, ftol)
        self.x = torch.minimum(torch.maximum(x0, lo), hi)
        self.x_trial = self.x.clone()
        z = lambda *s, dt=f64: torch.zeros(*s, dtype=dt, device=dv)  # noqa: E731
        self.f, self.fprev, self.t = z(B), z(B), z(B)
        self.g, self.d = z(B, P), z(B, P)
        self.S, self.Y, self.rho = z(B, m, P), z(B, m, P), z(B, m)
        i64 = torch.int64
        self.phase, self.status, self.iters, self.nback, self.cnt, self.head = (z(B, dt=i64) for _ in range(6))
        self.sd = z(B, dt=torch.bool)
        self.ar = torch.arange(B, device=dv)

    def _free(self, x, g):
        return (self.lo < self.hi) & ~((x == self.lo) & (g > 0)) & ~((x == self.hi) & (g < 0))

    def _descent(self, g, mask):
        d = torch.where(mask, -g, torch.zeros_like(g))
        return d, torch.clamp(1.0 / torch.sqrt((d * d).sum(1)), max=1.0)

    def _two_loop(self, q, cnt, head):
        m, ar = self.m, self.ar
        al = []
        for k in range(m):
            i = (head - 1 - k) % m
            live = (k < cnt)
            a = torch.where(live, self.rho[ar, i] * (self.S[ar, i] * q).sum(1), torch.zeros_like(self.f))
            al.append(a)
            q = q - a[:, None] * self.Y[ar, i]
        i0 = (head - 1) % m
        s0, y0 = self.S[ar, i0], self.Y[ar, i0]
        gam = torch.where(cnt > 0, (s0 * y0).sum(1) / (y0 * y0).sum(1), torch.ones_like(self.f))
        r = gam[:, None] * q
        for k in reversed(range(m)):
            i = (head - 1 - k) % m
            beta = torch.where(k < cnt, self.rho[ar, i] * (self.Y[ar, i] * r).sum(1), torch.zeros_like(self.f))
            r = r + (al[k] - beta)[:, None] * self.S[ar, i]
        return r

    def step(self, ft, gt, info):
        max_iter, max_back, c1, gtol, ftol = self.o
        W = torch.where
        run = self.status == 0
        bad = (info != 0) | ~torch.isfinite(ft) | ~torch.isfinite(gt).all(1)
        init = run & (self.phase == 0)
        srch = run & (self.phase == 1)
        s = self.x_trial - self.x
        gts = (self.g * s).sum(1)
        passed = srch & ~bad & (gts <= 0) & (ft <= self.f + c1 * gts)
        failed = srch & ~passed
        acc = passed | (init & ~bad)
        y = gt - self.g
        sy, ss, yy = (s * y).sum(1), (s * s).sum(1), (y * y).sum(1)
        push = passed & (sy > 2.2e-16 * (ss.sqrt() * yy.sqrt()))
        hd = self.head
        oh = torch.nn.functional.one_hot(hd, self.m).bool() & push[:, None]
        self.S = W(oh[:, :, None], s[:, None, :], self.S)
        self.Y = W(oh[:, :, None], y[:, None, :], self.Y)
        self.rho = W(oh, (1.0 / sy)[:, None], self.rho)
        drop = passed & ~push                       # a rejected pair clears the history
        head = W(push, (hd + 1) % self.m, W(drop, torch.zeros_like(hd), hd))
        cnt = W(push, torch.clamp(self.cnt + 1, max=self.m), W(drop, torch.zeros_like(self.cnt), self.cnt))
        fprev = W(passed, self.f, W(init, ft, self.fprev))
        x = W(acc[:, None], self.x_trial, self.x)
        f = W(acc, ft, self.f)
        g = W(acc[:, None], gt, self.g)
        iters = self.iters + passed.to(torch.int64)
        mask = self._free(x, g)
        pgn = (g.abs() * mask).amax(1)
        conv_g = passed & (pgn <= gtol)
        conv_f = passed & ~conv_g & (fprev - f <= ftol * torch.maximum(torch.ones_like(f), torch.maximum(f.abs(), fprev.abs())))
        maxit = passed & ~conv_g & ~conv_f & (iters >= max_iter)
        newdir = passed & ~conv_g & ~conv_f & ~maxit
        r = self._two_loop(W(mask, g, torch.zeros_like(g)), cnt, head)
        dq = W(mask, -r, torch.zeros_like(r))
        dsd, tsd = self._descent(g, mask)
        qn_bad = ~((dq * g).sum(1) < 0)
        nback = W(failed, self.nback + 1, torch.zeros_like(self.nback))
        over = failed & (nback > max_back)
        stall = over & self.sd
        restart = over & ~self.sd
        use_sd = init & ~bad | restart | (newdir & ((cnt == 0) | qn_bad))
        use_qn = newdir & ~use_sd
        clear = restart | (newdir & qn_bad)
        self.cnt, self.head = W(clear, torch.zeros_like(cnt), cnt), W(clear, torch.zeros_like(head), head)
        self.d = W(use_sd[:, None], dsd, W(use_qn[:, None], dq, self.d))
        self.t = W(use_sd, tsd, W(use_qn, torch.ones_like(f), W(failed & ~over, 0.5 * self.t, self.t)))
        self.sd = W(use_sd, torch.ones_like(self.sd), W(use_qn, torch.zeros_like(self.sd), self.sd))
        self.nback = W(use_sd | use_qn, torch.zeros_like(nback), W(run, nback, self.nback))
        st = self.status
        st = W(init & bad, torch.full_like(st, 5), st)
        st = W(conv_g, torch.full_like(st, 1), W(conv_f, torch.full_like(st, 2), W(maxit, torch.full_like(st, 3), st)))
        self.status = W(stall, torch.full_like(st, 4), st)
        self.x, self.f, self.g, self.fprev, self.iters = x, f, g, fprev, iters
        self.phase = W(run, torch.ones_like(self.phase), self.phase)
        trial = torch.minimum(torch.maximum(torch.addcmul(x, self.t[:, None], self.d), self.lo), self.hi)
        self.x_trial.copy_(W((self.status == 0)[:, None], trial, W(run[:, None], x, self.x_trial)))
        return self.status


def problem(n, starts, seed=0):
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, n).reshape(-1, 1)
    y = np.sin(9 * x[:, 0]) + 0.3 * np.cos(31 * x[:, 0]) + 0.1 * rng.standard_normal(n)
    kernel = SquaredExponentialKernel(1)
    x0 = np.column_stack([rng.uniform(0.03, 0.3, starts), rng.uniform(0.01, 0.2, starts)])
    gp.p_optimize_noise = True
    lo, hi = pack_bounds(kernel, [[0.0, 1.0]], n, True, True)
    return kernel, x, y, x0, np.array(lo), np.array(hi)


def timed_loop(evaluate, stepper, iters, warmup):
    dev = engine.device()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(iters + warmup)]
    for e0, e1, e2 in ev:
        e0.record()
        f, g, info = evaluate(stepper.x_trial)
        e1.record()
        stepper.step(f, g, info)
        e2.record()
    torch.cuda.synchronize(dev)
    ev = ev[warmup:]
    return [a.elapsed_time(b) for a, b, _ in ev], [b.elapsed_time(c) for _, b, c in ev]


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=0)
    args = ap.parse_args()
    lines = []
    for n, starts, iters in ((256, 64, 60), (4096, 16, 12)):
        iters = args.iters or iters
        kernel, x, y, x0, lo, hi = problem(n, starts)
        evaluate = sweep.native_batched_value_and_gradient(kernel, x, y)
        T = lambda a: torch.as_tensor(a, dtype=torch.float64, device=engine.device())  # noqa: E731
        res = {"n": n, "starts": starts, "iters": iters}
        for name in ("device", "torch"):
            # max_iter beyond the loop and zero tolerances: every member keeps stepping for the whole measurement
            if name == "device":
                st = engine.LbfgsState(T(x0), T(lo), T(hi), max_iter=10 ** 6, gtol=0.0, ftol=0.0)
            else:
                st = TorchStep(T(x0), T(lo), T(hi), max_iter=10 ** 6, gtol=0.0, ftol=0.0)
            te, ts = timed_loop(evaluate, st, iters, 4)
            res[name] = {"eval": stats(te), "step": stats(ts), "iteration": stats([a + b for a, b in zip(te, ts)])}
            if name == "device":
                res["f_device"] = float(st.current()[1].min())
            else:
                res["f_torch"] = float(st.f.min())
        print(json.dumps(res))
        lines.append(res)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("# tools/bench_fit.py on the MI355X (ms per iteration, HIP events: median [min - max])\n")
            for r in lines:
                for name in ("device", "torch"):
                    e, s, t = r[name]["eval"], r[name]["step"], r[name]["iteration"]
                    fh.write("N=%d starts=%d step=%-6s eval %.3f [%.3f - %.3f]  step %.3f [%.3f - %.3f]  iteration %.3f "
                             "[%.3f - %.3f]  (%d iterations)\n" % (
                                 r["n"], r["starts"], name, e["median_ms"], e["min_ms"], e["max_ms"], s["median_ms"],
                                 s["min_ms"], s["max_ms"], t["median_ms"], t["min_ms"], t["max_ms"], r["iters"]))
                fh.write("N=%d best f after the loop: device %.9f torch %.9f\n" % (r["n"], r["f_device"], r["f_torch"]))


if __name__ == "__main__":
    main()
