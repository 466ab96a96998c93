"""tools/bench_mean.py -- time gpk_mean_eval / gpk_mean_vjp at n = 8192, batch = 64, d = 4 for a LIN leaf and ADD(MUL(LIN, LOGIT), C),
against a torch-op restatement of the same trees on the same device (device events around back-to-back calls)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessfundamentals_amd.global_parameters as gp  # noqa: E402

gp.init(0)
from gaussianprocessfundamentals_amd import _native as nat, engine  # noqa: E402
from tests import mean_support as ms  # noqa: E402

N, B, D = 8192, 64, 4
ITERS, REPS = 3000, 5
dev = engine.device()
L = nat.lib()
s = nat.stream_handle(dev)
rng = np.random.default_rng(0)
X = torch.tensor(10.0 ** rng.uniform(-2, 0, (N, D)), device=dev)
y = torch.tensor(rng.standard_normal(N), device=dev)
g = torch.tensor(rng.standard_normal((B, N)), device=dev)


def timed(fn, iters=ITERS):
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return {"us_median": float(np.median(out)), "us_min": float(min(out)), "us_max": float(max(out))}


res = {"n": N, "batch": B, "d": D, "iters": ITERS, "reps": REPS}
for name, tree in (("LIN", ("LIN",)), ("ADD(MUL(LIN,LOGIT),C)", ms.NESTED)):
    mf = ms.make_mean(tree, D)
    md = engine.mean_descriptor(mf, D)
    hyp = torch.tensor(np.stack([ms.make_hyp(tree, D, 10 + b, 1.0 if b % 2 else -1.0) for b in range(B)]), device=dev)
    out = torch.empty((B, N), dtype=torch.float64, device=dev)
    grad = torch.empty((B, md.n_hyp), dtype=torch.float64, device=dev)
    wb = int(L.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), N, B))
    work = torch.empty(wb // 8, dtype=torch.float64, device=dev)
    mdp, hp, xp, yp, op, gpx, grp, wp = (ctypes.byref(md), nat.ptr(hyp), nat.ptr(X), nat.ptr(y), nat.ptr(out),
                                         nat.ptr(g), nat.ptr(grad), nat.ptr(work))

    def ev():
        L.gpk_mean_eval(mdp, hp, md.n_hyp, xp, N, 0, B, yp, 0, op, N, s)

    def vj():
        L.gpk_mean_vjp(mdp, hp, md.n_hyp, xp, N, 0, B, gpx, N, grp, wp, wb, s)

    def t_value(h):
        if name == "LIN":
            return torch.einsum("nd,bd->bn", X, h)
        lin = torch.einsum("nd,bd->bn", X, h[:, :D])
        sarg = torch.einsum("nd,bd->bn", X, h[:, D:2 * D]) - h[:, 2 * D:3 * D].sum(1, keepdim=True)
        return lin * (h[:, 3 * D:3 * D + 1] / (1 + torch.exp(sarg))) + h[:, 3 * D + 1:3 * D + 2]

    def t_ev():
        return y[None, :] - t_value(hyp)

    hreq = hyp.clone().requires_grad_(True)

    def t_vj():
        hreq.grad = None
        (t_value(hreq) * g).sum().backward()

    ev(); vj(); torch.cuda.synchronize()
    # sanity: the torch restatement and the device program agree
    assert torch.allclose(out, t_ev(), rtol=1e-12, atol=1e-12)
    t_vj()
    assert torch.allclose(grad, hreq.grad, rtol=1e-9, atol=1e-9)
    res[name] = {"gpk_mean_eval": timed(ev), "gpk_mean_vjp": timed(vj), "torch_eval": timed(t_ev, 500),
                 "torch_vjp": timed(t_vj, 300),
                 "engine.mean_vector": timed(lambda: engine.mean_vector(mf, hyp, X, y), 1000),
                 "engine.mean_vjp": timed(lambda: engine.mean_vjp(mf, hyp, X, g), 1000)}
    print(name, json.dumps(res[name]), flush=True)
os.makedirs("bench_out", exist_ok=True)
json.dump(res, open("bench_out/mean_timing.json", "w"), indent=1)
