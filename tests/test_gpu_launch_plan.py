"""gpk_launch_plan is what the launch path enqueues (needs the MI355X): with event timing on and the persistent launch
off, the launches, flops and bytes gpk_timing_read accumulates per class for one gpk_potrf_aug / _ex / _ragged call
equal the sums over nat.launch_plan's steps for the same arguments -- counts exactly, the doubles to rel 1e-12."""
import ctypes

import pytest
import torch

from gaussianprocessfundamentals_amd import engine

pytestmark = pytest.mark.gpu
nat = engine.nat

CLASSES = {1: "diag", 2: "trsm", 3: "update"}


def _identity_w(lay, eye):
    """W of K = I for every member (SPD whatever the member's size), identity extra rows for eye"""
    dev = engine.device()
    W = torch.zeros((lay.batch, lay.p, lay.ld), dtype=torch.float64, device=dev)
    i = torch.arange(lay.n_pad, device=dev)
    W[:, i, i] = 1.0
    if eye:
        t = torch.arange(lay.n, device=dev)
        W[:, lay.n_pad + t, t] = 1.0
    assert W.numel() == lay.batch * lay.w_batch_stride
    Winv = torch.zeros(lay.batch * lay.inv_batch_stride, dtype=torch.float64, device=dev)
    info = torch.zeros(lay.batch, dtype=torch.int32, device=dev)
    return W, Winv, info


@pytest.mark.parametrize("case", ["plain", "eye", "ragged"])
def test_timing_counters_equal_the_plan(case):
    L = nat.lib()
    dev = engine.device()
    if case == "plain":
        lay, eye, knobs, sizes = nat.plan(nat.GPK_F64, 3, 300, 77, 1), False, {}, None
    elif case == "eye":
        lay, eye, knobs, sizes = nat.plan(nat.GPK_F64, 1, 257, 257, 1), True, {"lookahead": 1, "group": 2}, None
    else:
        lay, eye, knobs, sizes = nat.plan(nat.GPK_F64, 2, 640, 0, 1), False, {"ingroup": 2}, [640, 130]
    W, Winv, info = _identity_w(lay, eye)
    s = nat.stream_handle()
    with nat.thread_tune(chain=0, **knobs):
        # (torch's current stream is an ordinary one: it has the fused panel solve's counters)
        steps = nat.launch_plan(lay, eye=eye, counters=True)
        nat.timing_enable(True)
        try:
            nat.timing_reset()
            if case == "plain":
                rc = L.gpk_potrf_aug(ctypes.byref(lay), nat.ptr(W), nat.ptr(Winv), nat.ptr(info), s)
            elif case == "eye":
                rc = L.gpk_potrf_aug_ex(ctypes.byref(lay), nat.ptr(W), nat.ptr(Winv), nat.ptr(info),
                                        nat.AUG_EXTRA_IDENTITY, s)
            else:
                n_dev = torch.tensor(sizes, dtype=torch.int64, device=dev)
                rc = L.gpk_potrf_aug_ragged(ctypes.byref(lay), nat.ptr(W), nat.ptr(Winv), nat.ptr(info),
                                            nat.ptr(n_dev), None, s)
            nat.check(rc, "gpk_potrf_aug (%s)" % case)
            got = nat.timing_read()
        finally:
            nat.timing_enable(False)
            nat.timing_reset()
    torch.cuda.synchronize()
    assert not nat.last_factorisation_was_chain()
    assert int(info.abs().max()) == 0
    for cls, name in CLASSES.items():
        mine = steps[steps["cls"] == cls]
        print(case, name, got[name]["launches"], got[name]["flops"], got[name]["bytes"],
              len(mine), float(mine["flops"].sum()), float(mine["bytes"].sum()))
        assert got[name]["launches"] == len(mine)
        assert len(mine) > 0 or name == "trsm"  # (every panel solve may be fused into its diagonal launch)
        assert got[name]["flops"] == pytest.approx(float(mine["flops"].sum()), rel=1e-12, abs=0)
        assert got[name]["bytes"] == pytest.approx(float(mine["bytes"].sum()), rel=1e-12, abs=0)
    for name in ("assemble", "finalize", "trsv", "grad"):
        assert got[name]["launches"] == 0
