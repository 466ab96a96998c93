"""Mean functions without a GPU: the classes' plumbing against the reference's behaviour
(gpbasics/MeanFunctionBasics/BaseMeanFunctions.py, Operators.py), the device programs ``_emit`` writes, and the
host-only entries of the C ABI (gpk_mean_op_supported, gpk_mean_vjp_workspace_bytes and its descriptor checks)."""
import ctypes
import math
import os
import re

import pytest
import torch

from gaussianprocessfundamentals_amd import _build, _native as nat, engine
from gaussianprocessfundamentals_amd.MeanFunctionBasics import BaseMeanFunctions as bmf
from gaussianprocessfundamentals_amd.MeanFunctionBasics import MeanFunction as mfm
from gaussianprocessfundamentals_amd.MeanFunctionBasics import Operators as mops

from tests import mean_support as ms

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpk.h")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return nat.load_library()


# ---------------------------------------------------------------------------------------------- classes
@pytest.mark.parametrize("d", [1, 3])
def test_leaf_hyperparameter_counts_shapes_and_defaults(d):
    lin, ex, lo = bmf.LinearMeanFunction(d), bmf.ExponentialMeanFunction(d), bmf.LogitMeanFunction(d)
    assert lin.get_hyper_parameter_dimensionalities() == [[d]]
    assert ex.get_hyper_parameter_dimensionalities() == [[d], [d], []]
    assert lo.get_hyper_parameter_dimensionalities() == [[d], [d], []]
    assert (lin.get_number_of_hyper_parameter(), ex.get_number_of_hyper_parameter(),
            lo.get_number_of_hyper_parameter()) == (1, 3, 3)
    for f in (lin, ex, lo):
        hyp = f.get_default_hyper_parameter()
        assert [list(h.shape) for h in hyp] == f.get_hyper_parameter_dimensionalities()
        assert all(h.dtype == torch.float64 for h in hyp)
        assert f.get_number_base_mean_function() == 1
    assert lin.get_default_hyper_parameter()[0].tolist() == [1 / d] * d
    a, b, base = ex.get_default_hyper_parameter()
    assert a.tolist() == [1.0] * d and b.tolist() == [0.0] * d and float(base) == math.e
    a, b, c = lo.get_default_hyper_parameter()
    assert a.tolist() == [-1.0] * d and b.tolist() == [0.0] * d and float(c) == 1.0


def test_names_weights_manifestations_and_deepcopy():
    d = 2
    leaves = [bmf.ConstantMeanFunction(d), bmf.LinearMeanFunction(d), bmf.ExponentialMeanFunction(d),
              bmf.LogitMeanFunction(d)]
    assert [f.get_string_representation() for f in leaves] == ["C", "LIN", "EXP", "LOGIT"]
    assert [f.get_string_representation_weight() for f in leaves] == [1, 2, 3, 4]
    assert [f.manifestation.value for f in leaves] == [101, 102, 103, 104]
    assert bmf.ZeroMeanFunction(d).get_string_representation() == "ZERO_MEAN"
    for f in leaves[1:]:
        assert f.get_mean_function_type() is mfm.MeanFunctionType.BASE_MEAN_FUNCTION
        hyp = f.get_default_hyper_parameter()
        f.set_last_hyper_parameter(hyp)
        c = f.deepcopy()
        assert type(c) is type(f) and c is not f and c.input_dimensionality == d
        assert c.get_last_hyper_parameter() is hyp
        with pytest.raises(AssertionError):
            f.set_last_hyper_parameter(hyp + hyp)


def test_operator_plumbing():
    d = 3
    lin, lo, c = bmf.LinearMeanFunction(d), bmf.LogitMeanFunction(d), bmf.ConstantMeanFunction(d)
    add = mops.AdditionOperator([lo, c], d)
    assert add.manifestation is mfm.MeanFunctionManifestation.ADD
    assert add.get_mean_function_type() is mfm.MeanFunctionType.OPERATOR
    assert add.get_number_of_hyper_parameter() == 4 and add.get_number_base_mean_function() == 2
    assert add.get_number_of_child_nodes() == 2
    assert add.get_string_representation() == "(LOGIT + C)"
    assert add.get_string_representation_weight() == 5
    assert add.get_hyper_parameter_dimensionalities() == [[d], [d], [], []]
    add.add_child_mean_function(lin)
    assert add.get_number_of_hyper_parameter() == 5
    # children sorted by weight (LIN 2, LOGIT 4, C 1), nested operators too
    mul = mops.MultiplicationOperator([add, bmf.ExponentialMeanFunction(d)], d)
    mul.sort_child_nodes()
    assert mul.get_string_representation() == "(EXP x (C + LIN + LOGIT))"
    assert [type(n) for n in add.child_nodes] == [bmf.ConstantMeanFunction, bmf.LinearMeanFunction,
                                                  bmf.LogitMeanFunction]
    # the last-hyperparameter round trip slices by child
    hyp = [torch.full([] if not s else s, float(i)) for i, s in enumerate(mul.get_hyper_parameter_dimensionalities())]
    assert len(hyp) == mul.get_number_of_hyper_parameter() == 8
    mul.set_last_hyper_parameter(hyp)
    assert mul.child_nodes[0].get_last_hyper_parameter() == hyp[:3]
    assert add.child_nodes[0].get_last_hyper_parameter() == hyp[3:4]
    assert add.child_nodes[2].get_last_hyper_parameter() == hyp[5:8]
    got = mul.get_last_hyper_parameter()
    assert len(got) == 8 and all(a is b for a, b in zip(got, hyp))
    with pytest.raises(AssertionError):
        mul.set_last_hyper_parameter(hyp[:-1])
    # defaults concatenate, replace_child_node swaps, deepcopy copies the tree
    assert len(mul.get_default_hyper_parameter()) == 8
    mul.replace_child_node(0, bmf.ConstantMeanFunction(d))
    assert mul.get_string_representation() == "(C x (C + LIN + LOGIT))"
    with pytest.raises(AssertionError):
        mul.replace_child_node(2, c)
    mul.set_last_hyper_parameter(mul.get_default_hyper_parameter())   # (a leaf copies its last values, as upstream)
    cp = mul.deepcopy()
    assert cp.child_nodes[1].child_nodes[1].get_last_hyper_parameter()[0].tolist() == [1 / d] * d
    assert type(cp) is mops.MultiplicationOperator and cp.child_nodes[1] is not add
    assert cp.get_string_representation() == mul.get_string_representation()
    single = mops.AdditionOperator([lin], d)
    assert single.get_string_representation() == "LIN"


# --------------------------------------------------------------------------------------------- programs
def _program(md):
    return [(md.nodes[i].op, md.nodes[i].hyp_offset, md.nodes[i].ard_slot, md.nodes[i].flags)
            for i in range(md.n_nodes)]


def test_emit_programs(lib):
    d = 3
    md = engine.mean_descriptor(bmf.LogitMeanFunction(d))
    assert (md.n_nodes, md.n_hyp, md.dim, md.reserved) == (1, 7, 3, 0)
    assert _program(md) == [(104, 0, -1, 0)]
    md = engine.mean_descriptor(bmf.ZeroMeanFunction(d))
    assert _program(md) == [(101, 0, -1, 0)] and md.n_hyp == 1
    flat = ms.make_mean(("ADD", [("LIN",), ("EXP",), ("C",)]), d)
    md = engine.mean_descriptor(flat)
    assert md.n_hyp == 3 + 7 + 1
    assert _program(md) == [(102, 0, -1, 0), (103, 3, -1, 0), (201, 0, -1, 0), (101, 10, -1, 0), (201, 0, -1, 0)]
    md = engine.mean_descriptor(ms.make_mean(ms.NESTED, d))
    assert _program(md) == [(102, 0, -1, 0), (104, 3, -1, 0), (202, 0, -1, 0), (101, 10, -1, 0), (201, 0, -1, 0)]
    assert md.n_hyp == 11
    # the largest program that fits GPK_MAX_NODES = 16: L leaves take L - 1 binary ops, 2 L - 1 nodes, so eight
    # leaves fill 15 of the 16 slots and a ninth leaf needs 17
    eight = ("ADD", [("MUL", [("C",), ("LIN",)]), ("MUL", [("C",), ("LIN",)]), ("MUL", [("C",), ("LIN",)]),
                     ("MUL", [("C",), ("LIN",)])])
    md = engine.mean_descriptor(ms.make_mean(eight, 2))
    assert md.n_nodes == 15 and md.n_hyp == 4 * 3
    assert [p[0] for p in _program(md)] == [101, 102, 202, 101, 102, 202, 201, 101, 102, 202, 201, 101, 102, 202, 201]
    assert [p[1] for p in _program(md) if p[0] < 200] == [0, 1, 3, 4, 6, 7, 9, 10]
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), 100, 1) > 0
    with pytest.raises(ValueError):
        engine.mean_descriptor(ms.make_mean(("ADD", [("C",)] * 9), 1))
    with pytest.raises(ValueError):
        engine.mean_descriptor(ms.make_mean(("ADD", [("EXP",), ("EXP",)]), 16))   # 66 hyperparameters
    with pytest.raises(ValueError):
        engine.mean_descriptor(bmf.LinearMeanFunction(17))


# -------------------------------------------------------------------------------------------------- ABI
def test_mdesc_size_matches_header(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} gpk_mdesc;", src).group(1)
    assert len(re.findall(r"\bint32_t\s+\w+;", body)) == 4 and "gpk_node nodes[GPK_MAX_NODES];" in body
    assert ctypes.sizeof(nat.GpkMdesc) == 4 * 4 + nat.MAX_NODES * ctypes.sizeof(nat.GpkNode) == 272
    assert int(re.search(r"#define GPK_MEAN_POINTS_PER_WG (\d+)", src).group(1)) == nat.MEAN_POINTS_PER_WG
    assert int(re.search(r"#define GPK_ABI_VERSION (\d+)", src).group(1)) == 7


def test_mean_op_supported(lib):
    for op in (101, 102, 103, 104, 201, 202):
        assert lib.gpk_mean_op_supported(op) == 1 and nat.mean_op_supported(op)
    for op in (0, 100, 105, 203, 204, -1):
        assert lib.gpk_mean_op_supported(op) == 0
    assert {"gpk_mean_op_supported", "gpk_mean_eval", "gpk_mean_vjp_workspace_bytes", "gpk_mean_vjp"} <= set(nat.EXPORTS)


def _md(nodes, n_hyp, dim):
    md = nat.GpkMdesc()
    md.n_nodes, md.n_hyp, md.dim, md.reserved = len(nodes), n_hyp, dim, 0
    for i, nd in enumerate(nodes):
        op, off, slot, flags = (nd + (-1, 0))[:4] if len(nd) == 2 else nd
        md.nodes[i].op, md.nodes[i].hyp_offset, md.nodes[i].ard_slot, md.nodes[i].flags = op, off, slot, flags
    return md


INVALID = {
    "stack underflow": _md([(102, 0), (201, 0)], 2, 2),
    "leftover operands": _md([(102, 0), (101, 2)], 3, 2),
    "n_hyp too small": _md([(103, 0)], 4, 2),
    "n_hyp too large": _md([(103, 0)], 6, 2),
    "unknown op": _md([(105, 0)], 1, 1),
    "change-point op": _md([(101, 0), (101, 1), (203, 0)], 2, 1),
    "non-zero flags": _md([(102, 0, -1, 1)], 2, 2),
    "dim 17": _md([(101, 0)], 1, 17),
    "dim 0": _md([(101, 0)], 1, 0),
    "offsets out of order": _md([(101, 1), (101, 0), (201, 0)], 2, 1),
    "no nodes": _md([], 0, 1),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_workspace_bytes_is_zero_for_invalid_programs(lib, name):
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(INVALID[name]), 100, 2) == 0


def test_workspace_bytes_for_valid_programs(lib):
    P = nat.MEAN_POINTS_PER_WG
    md = _md([(102, 0), (104, 2), (202, 0), (101, 7), (201, 0)], 8, 2)
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), 1, 1) == 8 * 8
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), P, 3) == 3 * 8 * 8
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), 2 * P + 1, 3) == 3 * 3 * 8 * 8
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), 0, 1) == 0
    assert lib.gpk_mean_vjp_workspace_bytes(ctypes.byref(md), 10, 0) == 0
    assert lib.gpk_mean_vjp_workspace_bytes(None, 10, 1) == 0


def test_restatements_agree_with_each_other():
    """numpy, torch and mpmath restatements of the nested tree give the same values, and forward()'s partials
    are torch autograd's."""
    d, n = 3, 7
    x = ms.make_x(n, d, 1)
    for tree, sign in ((ms.NESTED, 1.0), (("ADD", [("EXP",), ("MUL", [("LIN",), ("EXP",)])]), -1.0)):
        flat = ms.make_hyp(tree, d, 2, sign)
        m, g = ms.forward(tree, flat, x)
        mm, gm = ms.forward_mp(tree, flat, x)
        ft = torch.tensor(flat, requires_grad=True)
        mt = ms.value_torch(tree, ft, torch.tensor(x))
        assert abs(m - ms.to_f64(mm)).max() <= 1e-14 * abs(m).max()
        assert abs(m - mt.detach().numpy()).max() <= 1e-14 * abs(m).max()
        w = torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
        (mt * w).sum().backward()
        exp = (w.numpy()[:, None] * g).sum(0)
        assert abs(ft.grad.numpy() - exp).max() <= 1e-13 * max(1.0, abs(exp).max())
        assert abs(ms.to_f64(gm) - g).max() <= 1e-13 * max(1.0, abs(g).max())
