"""The change-point operator's device program on the host: descriptor, validation, and the test restatement of
tests/cp_support.py pinned against oracle.gp_oracle.change_point_matrix and closed forms (no GPU).

Reference (paths relative to gpbasics/): KernelBasics/Operators.py:379-476."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gp_oracle as o
from tests import cp_support as cs
from tests.lin_support import LIN, lin_oracle  # noqa: F401

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Kernel as kk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops

SE, PER, MAT52, MAT32 = ("SE", {}), ("PER", {}), ("MAT52", {}), ("MAT32", {})
CP3 = ("CP", [SE, PER, MAT52])
HYP3 = [0.31, 0.62, 0.2, 0.9, 0.35, 0.3]          # cp_0, cp_1, l_SE, l_PER, p_PER, l_MAT52
W, MUL, ADD = nat.OP_CPW, (nat.OP_MUL, 0, -1, 0), (nat.OP_ADD, 0, -1, 0)
LO, HI, SIG, APX = nat.NODE_CP_LO, nat.NODE_CP_HI, nat.NODE_CP_SIGMOID, nat.NODE_CP_APPROX


@pytest.fixture(autouse=True)
def _restore_mode():
    old = gp.p_cp_operator_type
    yield
    gp.p_cp_operator_type = old


def _nodes(kd):
    return [(kd.nodes[i].op, kd.nodes[i].hyp_offset, kd.nodes[i].ard_slot, kd.nodes[i].flags)
            for i in range(kd.n_nodes)]


def _cp3_kernel():
    return ops.ChangePointOperator(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1), bk.MaternKernel5_2(1)],
                                   [torch.tensor(0.3, dtype=torch.float64), torch.tensor(0.65, dtype=torch.float64)])


# ------------------------------------------------------------------------------ descriptor
@pytest.mark.parametrize("scaled", [False, True])
def test_descriptor_of_a_three_child_tree(scaled):
    """W_0 K_0 MUL  W_1 K_1 MUL ADD  W_2 K_2 MUL ADD: windows at hyp_offset 0 / 0 / 1 (adjacent windows share a
    slot), children after the two change points."""
    assert nat.OP_CPW == kk.KernelManifestation.CP.value == 203 and nat.GPK_ABI_VERSION == 7
    gp.p_scaled_base_kernel = scaled
    kd = engine.kernel_descriptor(_cp3_kernel(), 1)
    s = nat.NODE_SCALED if scaled else 0
    c0, c1, c2 = (2, 4, 7) if scaled else (2, 3, 5)
    assert _nodes(kd) == [(W, 0, -1, HI), (nat.OP_SE, c0, -1, s), MUL,
                          (W, 0, -1, LO | HI), (nat.OP_PER, c1, -1, s), MUL, ADD,
                          (W, 1, -1, LO), (nat.OP_MAT52, c2, -1, s), MUL, ADD]
    assert kd.n_hyp == (9 if scaled else 6) and kd.n_ard == 0 and kd.dim == 1


def test_descriptor_inside_an_add_and_with_a_lin_child():
    """ADD(SE, CP([LIN, SE], [cp])): every offset shifted by the SE's one value; the LIN child has its one offset."""
    k = ops.AdditionOperator(1, [bk.SquaredExponentialKernel(1),
                                 ops.ChangePointOperator(1, [bk.LinearKernel(1), bk.SquaredExponentialKernel(1)],
                                                         [torch.tensor(0.5, dtype=torch.float64)])])
    kd = engine.kernel_descriptor(k, 1)
    assert _nodes(kd) == [(nat.OP_SE, 0, -1, 0),
                          (W, 1, -1, HI), (nat.OP_LIN, 2, -1, 0), MUL,
                          (W, 1, -1, LO), (nat.OP_SE, 3, -1, 0), MUL, ADD, ADD]
    assert kd.n_hyp == 4
    # an ADD inside a change point
    k2 = ops.ChangePointOperator(1, [ops.AdditionOperator(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1)]),
                                     bk.MaternKernel3_2(1)], [torch.tensor(0.5, dtype=torch.float64)])
    assert _nodes(engine.kernel_descriptor(k2, 1)) == [
        (W, 0, -1, HI), (nat.OP_SE, 1, -1, 0), (nat.OP_PER, 2, -1, 0), ADD, MUL,
        (W, 0, -1, LO), (nat.OP_MAT32, 4, -1, 0), MUL, ADD]
    # the one-child form keeps delegating
    k1 = ops.ChangePointOperator(1, [bk.SquaredExponentialKernel(1)], [])
    assert _nodes(engine.kernel_descriptor(k1, 1)) == [(nat.OP_SE, 0, -1, 0)]


def test_descriptor_limits_and_settings():
    se = bk.SquaredExponentialKernel
    cps = [torch.tensor(v, dtype=torch.float64) for v in (0.2, 0.4, 0.6, 0.8)]
    four = ops.ChangePointOperator(1, [se(1) for _ in range(4)], cps[:3])
    assert engine.kernel_descriptor(four, 1).n_nodes == 15
    with pytest.raises(ValueError):                                     # 19 nodes > GPK_MAX_NODES
        engine.kernel_descriptor(ops.ChangePointOperator(1, [se(1) for _ in range(5)], cps), 1)
    with pytest.raises(NotImplementedError, match="1-D"):
        engine.kernel_descriptor(ops.ChangePointOperator(2, [se(2), se(2)], cps[:1]), 2)
    k = _cp3_kernel()
    for mode, bit in (("INDICATOR", 0), ("SIGMOID", SIG), ("APPROX_INDICATOR", APX), ("INDICATOR", 0)):
        cs.set_mode(mode)                                               # read at emission: no descriptor is cached
        fl = [n[3] for n in _nodes(engine.kernel_descriptor(k, 1)) if n[0] == W]
        assert fl == [HI | bit, LO | HI | bit, LO | bit]


# ------------------------------------------------------------------------------ valid_kdesc (host code)
def _program(window, n_hyp=3, dim=1):
    """[window, SE, MUL] with the SE's length scale in the last slot"""
    kd = nat.GpkKdesc()
    kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 3, n_hyp, dim, 0
    for i, (op, off, slot, fl) in enumerate([window, (nat.OP_SE, n_hyp - 1, -1, 0), MUL]):
        kd.nodes[i].op, kd.nodes[i].hyp_offset, kd.nodes[i].ard_slot, kd.nodes[i].flags = op, off, slot, fl
    return kd


def test_descriptor_validation_on_the_host():
    """valid_kdesc runs before anything touches the device: every malformed window node gives -1 (argument 1); a valid
    program gets past it to the next argument check (-5: X)."""
    L = nat.load_library()
    hyp = (ctypes.c_double * 8)()

    def call(kd):
        return L.gpk_kernel_matrix(ctypes.byref(kd), ctypes.cast(hyp, ctypes.c_void_p), nat.GPK_F64, 0, None, 10, None,
                                   10, kd.dim, 0.0, None, 10, None)

    bad = [_program((W, 0, -1, 0)),                        # no bound
           _program((W, 0, -1, SIG)),
           _program((W, 0, -1, HI | SIG | APX)),           # both form bits
           _program((W, 0, -1, HI | nat.NODE_SCALED)),
           _program((W, 0, -1, HI | nat.NODE_ARD)),
           _program((W, 0, -1, HI | nat.NODE_SE_EXPANDED)),
           _program((W, 0, -1, HI | nat.NODE_STANDARD)),
           _program((W, 0, 0, HI)),                        # an ARD slot
           _program((W, 3, -1, HI)),                       # the bound past n_hyp
           _program((W, 2, -1, LO | HI)),                  # the second bound past n_hyp
           _program((W, -1, -1, HI)),
           _program((W, 0, -1, HI), dim=2)]
    for kd in bad:
        assert call(kd) == -1, _nodes(kd)
    for fl in (HI, LO, LO | HI, HI | SIG, LO | HI | APX):
        assert call(_program((W, 0, -1, fl))) == -5
    assert call(_program((W, 1, -1, LO | HI))) == -5       # bounds in slots 1, 2 of 3
    assert L.gpk_op_supported(203) == 1 and L.gpk_op_supported(999) == 0
    assert all(L.gpk_op_supported(op) == 1 for op in (102, 104, 105, 107, 108, 201, 202))
    assert nat.op_supported(nat.OP_CPW) and not nat.op_supported(999)


def test_cp_skip_knob():
    assert nat.tune("cp_skip", 1) == 1                     # default on; (host-only call)


# ------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("mode", cs.MODES)
def test_restatement_matches_the_oracle(mode):
    """cp_torch (separable: w_i(x) w_i(y) K_i) against change_point_matrix (masks as outer products, child by child) at
    1e-15 of the largest entry, 200 x 77 points with some inside every transition zone."""
    x, _, xs = cs.cp_inputs(200, 5, HYP3[:2], m=77)
    ref = cs.cp_numpy(CP3, HYP3, x, xs, mode)
    got = cs.cp_torch(CP3, cs.as_params(HYP3, False), torch.as_tensor(x), torch.as_tensor(xs), mode).numpy()
    assert ref.shape == (200, 77)
    assert np.max(np.abs(got - ref)) <= 1e-15 * np.max(np.abs(ref))
    if mode != "APPROX_INDICATOR":                          # (the rising mask all but empties the inner child)
        assert np.count_nonzero(ref) > 0.2 * ref.size


def test_restatement_closed_forms():
    """Under the hard mask every weight is exactly 0 or 1, so the operator's matrix is made of the children's own
    entries and exact zeros.  The children's matrices come from the same torch leaf code (bitwise comparable on any
    machine) and are themselves checked against the numpy oracle at 1e-15."""
    x = np.sort(np.random.default_rng(6).uniform(0, 1, 90)).reshape(-1, 1)
    X = torch.as_tensor(x)

    def child(t, h):
        k = cs.cp_torch(t, cs.as_params(h, False), X, X, "INDICATOR").numpy()
        assert np.max(np.abs(k - o.kernel_matrix(t, h, x, x))) <= 1e-15
        return k

    k_se, k_per, k_m52, k_m32 = child(SE, [0.2]), child(PER, [0.9, 0.35]), child(MAT52, [0.3]), child(MAT32, [0.3])
    K = cs.cp_torch(CP3, cs.as_params(HYP3, False), X, X, "INDICATOR").numpy()
    seg = np.searchsorted(HYP3[:2], x[:, 0], side="right")            # [x < cp]: x == cp falls right of it
    assert len(set(seg)) == 3
    blocks = np.zeros_like(K)
    for i, k in enumerate((k_se, k_per, k_m52)):
        a = seg == i
        blocks[np.ix_(a, a)] = k[np.ix_(a, a)]
    assert np.array_equal(K, blocks)                                   # block diagonal, the children's blocks
    # a change point below the data empties child 0
    K = cs.cp_torch(("CP", [SE, MAT32]), cs.as_params([-0.5, 0.2, 0.3], False), X, X, "INDICATOR").numpy()
    assert np.array_equal(K, k_m32)
    # cp_1 < cp_0 empties the middle child: [x >= cp_0][x < cp_1] = 0
    h = [0.6, 0.4, 0.2, 0.9, 0.35, 0.3]
    K = cs.cp_torch(CP3, cs.as_params(h, False), X, X, "INDICATOR").numpy()
    lo, hi = x[:, 0] < 0.6, x[:, 0] >= 0.4
    assert np.array_equal(K, np.outer(lo, lo) * k_se + np.outer(hi, hi) * k_m52)


# ------------------------------------------------------------------------------ non-vacuity of the gradient tests
def test_change_point_gradients_are_not_vacuous():
    """On cp_inputs(200, .., [0.31, 0.62]) the SIGMOID -LML gradient of every change point exceeds the largest child
    component (the GPU gradient tests rely on it: without points inside the transition they would test nothing), and
    the hard mask passes no gradient at all."""
    x, y, _ = cs.cp_inputs(200, 11, HYP3[:2])
    _, g, _ = cs.cp_nlml_and_grad(CP3, HYP3, 1e-2, x, y, "SIGMOID")
    print("SIGMOID d(-LML)/d(cp, children):", g)
    assert np.all(np.isfinite(g))
    assert min(abs(g[0]), abs(g[1])) > np.max(np.abs(g[2:]))
    _, g, _ = cs.cp_nlml_and_grad(CP3, HYP3, 1e-2, x, y, "INDICATOR")
    assert g[0] == 0.0 and g[1] == 0.0 and np.max(np.abs(g[2:])) > 0.0


def test_restatement_with_a_lin_child(lin_oracle):
    tree, hyp = ("CP", [LIN, SE]), [0.5, [0.3], 0.2]
    x, _, xs = cs.cp_inputs(60, 7, [0.5], m=20)
    for mode in cs.MODES:
        ref = cs.cp_numpy(tree, hyp, x, xs, mode)
        got = cs.cp_torch(tree, cs.as_params(hyp, False), torch.as_tensor(x), torch.as_tensor(xs), mode).numpy()
        assert np.max(np.abs(got - ref)) <= 1e-15 * np.max(np.abs(ref))
    k = cs.make_kernel(tree, hyp)
    assert isinstance(k, ops.ChangePointOperator) and k.get_number_of_hyper_parameter() == 3
