"""What the launch path enqueues, as gpk_timing_read sees it, for an A/B of two builds of libgpk.so (selected with
GPK_LIB): per shape and class the launches and the flops / bytes sums as hex floats -- equal lines mean the same
launch sequence with the same accounting -- and, with --latency, the host-side enqueue time of one gpk_potrf_aug.

usage: python tools/launch_counters.py             the table (chain 0): N = 1024 / 4096 / 8192 single, 4096 x 32,
                                                   4096 identity-augmented, ragged 1 x 8192 + 15 x 4096
       python tools/launch_counters.py --latency   N = 1024, batch 1, chain 0: us per gpk_potrf_aug call (host time of
                                                   the call alone, stream idle before each), median / min of 300
"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessfundamentals_amd import _native as nat  # noqa: E402


def buffers(lay, eye):
    """K = I for every member (SPD whatever the member's size), identity extra rows for eye"""
    dev = torch.device("cuda", 0)
    W = torch.zeros((lay.batch, lay.p, lay.ld), dtype=torch.float64, device=dev)
    i = torch.arange(lay.n_pad, device=dev)
    W[:, i, i] = 1.0
    if eye:
        t = torch.arange(lay.n, device=dev)
        W[:, lay.n_pad + t, t] = 1.0
    return (W, torch.zeros(lay.batch * lay.inv_batch_stride, dtype=torch.float64, device=dev),
            torch.zeros(lay.batch, dtype=torch.int32, device=dev))


def factor(L, lay, eye, sizes, W, Winv, info):
    s = nat.stream_handle()
    if sizes is not None:
        n_dev = torch.tensor(sizes, dtype=torch.int64, device=W.device)
        return L.gpk_potrf_aug_ragged(ctypes.byref(lay), nat.ptr(W), nat.ptr(Winv), nat.ptr(info), nat.ptr(n_dev),
                                      None, s)
    return L.gpk_potrf_aug_ex(ctypes.byref(lay), nat.ptr(W), nat.ptr(Winv), nat.ptr(info),
                              nat.AUG_EXTRA_IDENTITY if eye else 0, s)


def table():
    L = nat.lib()
    cases = [("N=1024", 1, 1024, 0, False, None), ("N=4096", 1, 4096, 0, False, None),
             ("N=8192", 1, 8192, 0, False, None), ("N=4096 x 32", 32, 4096, 0, False, None),
             ("N=4096 eye", 1, 4096, 4096, True, None),
             ("ragged 1 x 8192 + 15 x 4096", 16, 8192, 0, False, [8192] + [4096] * 15)]
    for name, batch, n, m, eye, sizes in cases:
        lay = nat.plan(nat.GPK_F64, batch, n, m, 1)
        W, Winv, info = buffers(lay, eye)
        with nat.thread_tune(chain=0):
            nat.timing_enable(True)
            nat.timing_reset()
            nat.check(factor(L, lay, eye, sizes, W, Winv, info), name)
            got = nat.timing_read()
            nat.timing_enable(False)
            nat.timing_reset()
        torch.cuda.synchronize()
        print(json.dumps({"case": name, "info": int(info.abs().max()),
                          **{c: [got[c]["launches"], float(got[c]["flops"]).hex(), float(got[c]["bytes"]).hex()]
                             for c in ("diag", "trsm", "update")}}), flush=True)
        del W, Winv, info


def latency():
    L = nat.lib()
    lay = nat.plan(nat.GPK_F64, 1, 1024, 0, 1)
    W0, Winv, info = buffers(lay, False)
    W = W0.clone()
    ts = []
    with nat.thread_tune(chain=0):
        for it in range(320):
            W.copy_(W0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = factor(L, lay, False, None, W, Winv, info)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            nat.check(rc, "gpk_potrf_aug")
            if it >= 20:
                ts.append((t1 - t0) * 1e6)
    print(json.dumps({"case": "enqueue N=1024", "median_us": round(statistics.median(ts), 2),
                      "min_us": round(min(ts), 2), "calls": len(ts), "info": int(info.abs().max())}), flush=True)


if __name__ == "__main__":
    latency() if "--latency" in sys.argv[1:] else table()
