"""LinearKernel on the host: device descriptor, hyperparameter plumbing and the test restatement (no GPU).

Expected values are worked out by hand from the reference (gpbasics/KernelBasics/BaseKernels.py:110-270);
the restatement of tests/lin_support.py is pinned by closed forms, in the spirit of oracle.known_answers()."""
import math

import numpy as np
import pytest
import torch

from oracle import gp_autodiff as ad
from oracle import gp_oracle as o
from tests.lin_support import (LIN, kernel_and_bound, lin_nlml_closed_form, lin_numpy, lin_oracle,  # noqa: F401
                               lin_torch, make_kernel, with_sg)

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Kernel as kk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops

SE = ("SE", {})
PER = ("PER", {})


def _nodes(kd):
    return [(kd.nodes[i].op, kd.nodes[i].hyp_offset, kd.nodes[i].ard_slot, kd.nodes[i].flags)
            for i in range(kd.n_nodes)]


# ------------------------------------------------------------------------------ descriptor
def test_descriptor_add_se_lin():
    assert nat.OP_LIN == kk.KernelManifestation.LIN.value == 102 and nat.GPK_ABI_VERSION == 7
    k = ops.AdditionOperator(3, [bk.SquaredExponentialKernel(3), bk.LinearKernel(3)])
    kd = engine.kernel_descriptor(k, 3)
    assert _nodes(kd) == [(nat.OP_SE, 0, -1, 0), (nat.OP_LIN, 1, -1, 0), (nat.OP_ADD, 0, -1, 0)]
    assert kd.n_hyp == 4 and kd.n_ard == 0 and kd.dim == 3
    gp.p_scaled_base_kernel = True
    kd = engine.kernel_descriptor(k, 3)
    assert _nodes(kd)[:2] == [(nat.OP_SE, 0, -1, nat.NODE_SCALED), (nat.OP_LIN, 2, -1, nat.NODE_SCALED)]
    assert kd.n_hyp == 6


def test_descriptor_single_lin_and_no_ard():
    kd = engine.kernel_descriptor(bk.LinearKernel(16), 16)
    assert _nodes(kd) == [(nat.OP_LIN, 0, -1, 0)] and kd.n_hyp == 16
    gp.p_stationary_distance, old = "standard", gp.p_stationary_distance
    gp.p_se_expanded_norm = True
    try:   # neither the standard-distance nor the expanded-norm option touches a LIN node
        assert _nodes(engine.kernel_descriptor(bk.LinearKernel(2), 2)) == [(nat.OP_LIN, 0, -1, 0)]
    finally:
        gp.p_stationary_distance = old
    with pytest.raises(ValueError):
        bk.LinearKernel(2, ard=True)


# ------------------------------------------------------------------------------ hyperparameter plumbing
def test_counts_dimensionalities_names():
    k = bk.LinearKernel(3)
    assert k.get_number_of_hyper_parameter() == 1 and k.get_hyper_parameter_dimensionalities() == [[3]]
    assert k.get_hyper_parameter_names() == ["LIN_c"] and k.get_hyper_parameter_names(4) == ["LIN_4_c"]
    assert k.get_number_base_kernels() == 1 and k.get_number_of_child_nodes() == 1
    assert k.get_string_representation() == "LIN" and k.get_string_representation_weight() == 2
    gp.p_scaled_base_kernel = True
    assert k.get_number_of_hyper_parameter() == 2 and k.get_hyper_parameter_dimensionalities() == [[3], []]
    assert k.get_hyper_parameter_names() == ["LIN_c", "LIN_sg"]
    assert k.get_hyper_parameter_names(0) == ["LIN_0_c", "LIN_0_sg"]
    # kernel ids through an operator (K/Operators.py: one running id per base kernel)
    add = ops.AdditionOperator(3, [bk.LinearKernel(3), bk.SquaredExponentialKernel(3)])
    assert add.get_hyper_parameter_names(0)[:2] == ["LIN_0_c", "LIN_0_sg"]


def test_defaults_bounds_distribution():
    xr = [[0.0, 2.0], [-1.0, 3.0]]
    k = bk.LinearKernel(2)
    gp.p_scaled_base_kernel = True
    c, sg = k.get_default_hyper_parameter(xr, 100)                       # BaseKernels.py:168-176
    assert c.dtype == torch.float64 and c.tolist() == [0.01, 0.01] and float(sg) == 0.1 and sg.shape == ()
    assert [t.tolist() for t in k.get_default_hyper_parameter_fixed(xr, 100)] == [[0.01, 0.01], 0.1]
    (clo, chi), (slo, shi) = k.get_hyper_parameter_bounds(xr, 100)       # :136-151
    assert clo.tolist() == [-math.inf] * 2 and chi.tolist() == [math.inf] * 2
    assert float(slo) == pytest.approx(100 * 1e-8, rel=1e-15) and float(shi) == math.inf
    dc, dsg = k.get_hyper_parameter_distribution_definition(xr, 100)    # :198-212
    assert dc["type"] == "random_uniform" and dc["shape"] == [2]
    assert torch.as_tensor(dc["minval"]).tolist() == [-2.0, -5.0]        # x_min - range per dimension
    assert torch.as_tensor(dc["maxval"]).tolist() == [4.0, 7.0]          # x_max + range
    assert dsg == {"shape": [], "mean": 0.1, "stddev": 0.2, "type": "random_normal"}
    torch.manual_seed(0)
    for _ in range(5):                                                   # :178-196: min / max over the dimensions
        rc, rsg = k.get_default_hyper_parameter(xr, 100, from_distribution=True)
        assert rc.shape == (2,) and bool(torch.all((rc >= -5.0) & (rc <= 7.0))) and float(rsg) >= 0.0
    gp.p_scaled_base_kernel = False
    assert len(k.get_default_hyper_parameter(xr, 100)) == 1 and len(k.get_hyper_parameter_bounds(xr, 100)) == 1
    assert len(k.get_hyper_parameter_distribution_definition(xr, 100)) == 1


def test_last_hyper_parameter_affine_rescale_and_no_abs():
    gp.p_scaled_base_kernel = True
    k = bk.LinearKernel(2)
    c = torch.tensor([-0.5, 0.25], dtype=torch.float64)
    k.set_last_hyper_parameter([c, torch.tensor(0.7, dtype=torch.float64)])
    got = k.get_last_hyper_parameter()
    assert got[0].tolist() == [-0.5, 0.25] and float(got[1]) == 0.7       # signed: no |.| (unlike the length scales)
    shift, scale = 3.0, 2.0                                              # :259-269: c scale + shift, sg unchanged
    got = k.get_last_hyper_parameter([shift, scale])
    assert got[0].tolist() == [2.0, 3.5] and float(got[1]) == 0.7
    with pytest.raises(AssertionError):
        k.set_last_hyper_parameter([c])
    with pytest.raises(Exception):
        k.set_last_hyper_parameter(c)


def test_deepcopy_compare_json():
    k = bk.LinearKernel(2)
    k.set_last_hyper_parameter([torch.tensor([0.1, -0.2], dtype=torch.float64)])
    k.set_noise(torch.tensor(0.05))
    c = k.deepcopy()
    assert isinstance(c, bk.LinearKernel) and c is not k and c.input_dimensionality == 2
    assert c.get_last_hyper_parameter()[0].tolist() == [0.1, -0.2] and float(c.get_noise()) == pytest.approx(0.05)
    c.set_last_hyper_parameter([torch.tensor([9.0, 9.0], dtype=torch.float64)])
    assert k.get_last_hyper_parameter()[0].tolist() == [0.1, -0.2]
    assert k.type_compare_to(c) and not k.type_compare_to(bk.SquaredExponentialKernel(2))
    assert not bk.SquaredExponentialKernel(2).type_compare_to(k)
    assert k.get_json() == {"type": "LIN", "hyper_param": [[0.1, -0.2]]}


def test_constant_kernel_raises_like_the_reference():
    with pytest.raises(Exception, match="Not up to date. Implementation for ConstantKernel is not available."):
        bk.ConstantKernel(1)
    assert not hasattr(bk, "WhiteNoiseKernel")


@pytest.mark.parametrize("op", [ops.AdditionOperator, ops.MultiplicationOperator])
def test_operator_sorting_puts_lin_first(op):
    k = op(1, [bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1), bk.LinearKernel(1)])
    k.sort_child_nodes()
    assert [c.get_string_representation() for c in k.child_nodes] == ["LIN", "PER", "SE"]


def test_operator_simplification_accepts_lin():
    lin, se, per = bk.LinearKernel(1), bk.SquaredExponentialKernel(1), bk.PeriodicKernel(1)
    s = ops.MultiplicationOperator(1, [ops.AdditionOperator(1, [se, per]), lin]).get_simplified_version()
    assert s.get_string_representation() == "((LIN x SE) + (LIN x PER))"
    cp = ops.ChangePointOperator(1, [bk.LinearKernel(1), bk.SquaredExponentialKernel(1)], [0.5])
    assert cp.get_number_of_hyper_parameter() == 3


# ------------------------------------------------------------------------------ the restatement
def test_restatement_closed_forms():
    x = np.array([[1.0], [2.0], [3.0]])
    np.testing.assert_array_equal(lin_numpy([[0.0]], x, x), np.outer([1, 2, 3], [1, 2, 3]))
    np.testing.assert_array_equal(lin_numpy([[0.0], 0.5], x, x, scaled=True), 0.5 * np.outer([1, 2, 3], [1, 2, 3]))
    xd = np.array([[0.3, -1.2], [0.5, 0.25]])
    assert np.all(lin_numpy([xd[0]], xd[:1], xd) == 0.0)                  # x = c: a zero row
    np.testing.assert_allclose(lin_torch([torch.tensor(xd[1])], torch.tensor(xd), torch.tensor(xd)).numpy(),
                               lin_numpy([xd[1]], xd, xd), rtol=1e-15, atol=0)
    # D = 2 by hand: (0.3 - 0.1)(0.5 - 0.1) + (-1.2 - 0.2)(0.25 - 0.2)
    assert lin_numpy([[0.1, 0.2]], xd[:1], xd[1:])[0, 0] == pytest.approx(0.2 * 0.4 + -1.4 * 0.05, rel=1e-14)


def test_tree_bound_propagation():
    rng = np.random.default_rng(1)
    x, z = rng.uniform(-1, 1, (5, 2)), rng.uniform(-1, 1, (4, 2))
    K, B = kernel_and_bound(("MUL", [LIN, LIN]), [[0.1, 0.2], [0.3, -0.4]], x, z)
    a, b = lin_numpy([[0.1, 0.2]], x, z), lin_numpy([[0.3, -0.4]], x, z)
    np.testing.assert_allclose(K, a * b, rtol=1e-15)
    da = 1e-12 * (np.abs(x - [0.1, 0.2]) @ np.abs(z - [0.1, 0.2]).T) + 1e-13
    db = 1e-12 * (np.abs(x - [0.3, -0.4]) @ np.abs(z - [0.3, -0.4]).T) + 1e-13
    np.testing.assert_allclose(B, np.abs(a) * db + np.abs(b) * da, rtol=1e-12)
    K, B = kernel_and_bound(("ADD", [SE, LIN]), [0.5, [0.1, 0.2]], x, z)
    np.testing.assert_allclose(B, (1e-12 * np.abs(o.kernel_matrix(SE, [0.5], x, z)) + 1e-13) + da, rtol=1e-12)


def test_patched_oracle_closed_form_nlml(lin_oracle):
    """D = 1, sg LIN + s2 I: the oracle's Cholesky -LML against the determinant lemma / Sherman-Morrison."""
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (300, 1))
    y = 0.7 * x[:, 0] + 0.3 * rng.standard_normal(300)
    for c, sg, s2 in ((0.0, 1.0, 0.1), (0.25, 0.4, 0.05), (-2.0, 1.7, 0.3)):
        got = lin_oracle.nlml(LIN, [[c], sg], s2, x, y, scaled=True)
        assert abs(got - lin_nlml_closed_form(x, y, c, sg, s2)) <= 1e-12 * abs(got)
    got = lin_oracle.nlml(LIN, [[0.25]], 0.1, x, y)
    assert abs(got - lin_nlml_closed_form(x, y, 0.25, 1.0, 0.1)) <= 1e-12 * abs(got)


def test_patched_oracle_understands_trees(lin_oracle):
    rng = np.random.default_rng(3)
    x, z = rng.uniform(-1, 1, (6, 3)), rng.uniform(-1, 1, (4, 3))
    tree, hyp = ("ADD", [("MUL", [SE, LIN]), ("MAT52", {})]), [0.5, [0.1, 0.2, 0.3], 0.8]
    exp = o.kernel_matrix(SE, [0.5], x, z) * lin_numpy([[0.1, 0.2, 0.3]], x, z) + \
        o.kernel_matrix(("MAT52", {}), [0.8], x, z)
    np.testing.assert_allclose(lin_oracle.kernel_matrix(tree, hyp, x, z), exp, rtol=1e-15)
    assert lin_oracle.n_hyp(tree, True, 3) == 6 and ad._n_hyp(tree, False) == 3
    hs = with_sg(tree, hyp, [1.1, 1.2, 1.3])
    assert len(hs) == 6 and hs[2] is hyp[1]
    Kt = ad.kernel_matrix_t(tree, [torch.tensor(np.asarray(h, dtype=np.float64)) for h in hs], torch.tensor(x),
                            torch.tensor(z), scaled=True)
    np.testing.assert_allclose(Kt.numpy(), lin_oracle.kernel_matrix(tree, hs, x, z, scaled=True), rtol=1e-14)


def test_oracle_is_restored_after_the_fixture():
    with pytest.raises(ValueError):
        o.eval_base("LIN", {}, [[0.0]], np.zeros((1, 1)), np.zeros((1, 1)), False, False)


@pytest.mark.parametrize("tree,hyp,d,scaled", [
    (LIN, [[0.2, -0.1, 0.4], 0.6], 3, True),
    (("ADD", [SE, LIN]), [0.7, [0.1, 0.3]], 2, False),
    (("MUL", [LIN, PER]), [[0.3], 1.1, 0.8], 1, False),
    (("MUL", [LIN, LIN]), [[0.3, -0.6], 0.5, [1.2, 0.1], 0.9], 2, True),
])
def test_torch_restatement_gradient_matches_finite_differences(lin_oracle, tree, hyp, d, scaled):
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (40, d))
    y = np.sin(2 * x[:, 0]) + 0.5 * x[:, -1]
    noise = 0.2
    nl, g, gn = ad.nlml_and_grad(tree, hyp, noise, x, y, scaled)
    assert abs(nl - lin_oracle.nlml(tree, hyp, noise, x, y, scaled)) <= 1e-11 * abs(nl)
    fd, fdn = ad.finite_difference(lambda h, s: lin_oracle.nlml(tree, h, s, x, y, scaled), hyp, noise)
    scale = max(1.0, max(float(np.max(np.abs(v))) for v in g))
    for a, b in zip(list(g) + [gn], list(fd) + [fdn]):
        np.testing.assert_allclose(np.asarray(a), np.asarray(b).reshape(np.shape(a)), rtol=0, atol=2e-6 * scale)


# ------------------------------------------------------------------------------ descriptor validation (host code)
def test_descriptor_validation_on_the_host():
    """valid_kdesc runs before anything touches the device: a LIN node with an ARD / expanded / standard flag, an ARD
    slot, or too few hyperparameters gives -1 (argument 1); a valid one gets past it to the next argument check (-5: X)."""
    import ctypes
    L = nat.load_library()
    d = 3

    def kdesc(n_hyp, flags=0, slot=-1, n_ard=0):
        kd = nat.GpkKdesc()
        kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 1, n_hyp, d, n_ard
        kd.nodes[0].op, kd.nodes[0].hyp_offset, kd.nodes[0].ard_slot, kd.nodes[0].flags = nat.OP_LIN, 0, slot, flags
        return kd

    hyp = (ctypes.c_double * 8)()

    def call(kd):
        return L.gpk_kernel_matrix(ctypes.byref(kd), ctypes.cast(hyp, ctypes.c_void_p), nat.GPK_F64, 0, None, 10, None,
                                   10, d, 0.0, None, 10, None)

    for kd in (kdesc(d, nat.NODE_ARD, 0, 1), kdesc(d, nat.NODE_SE_EXPANDED), kdesc(d, nat.NODE_STANDARD), kdesc(d - 1),
               kdesc(d, nat.NODE_SCALED), kdesc(d, 0, 0)):
        assert call(kd) == -1
    assert call(kdesc(d)) == -5 and call(kdesc(d + 1, nat.NODE_SCALED)) == -5
