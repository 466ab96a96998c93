"""The derivative matrices d K / d theta on the HIP path (gpk_kernel_jacobian, needs the MI355X) against the autodiff
restatement (tests/fisher_support.jacobian_ref) and against gpk_kernel_vjp, which sums the same per-element partials.

Bar against the restatement: the project's gradient tolerance |got - ref| <= 1e-7 max(1, max|ref|)
(tests/test_gpu_grad.py::_check_grad) -- a ceiling, not an error model; the largest error per leaf is printed.
One reference per (tree, scaled, d) at the largest shape; the smaller shapes are its leading blocks (the planes are
elementwise in the points)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _native as nat
from gaussianprocessfundamentals_amd import engine
from tests import cp_support as cs
from tests import fisher_support as fs
from tests import rq_support as rs
from tests.helpers import hyp_list, set_flags
from tests.test_grad_oracle import _inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (63, 64), (65, 33), (64, 130)]
N_MAX, M_MAX = 65, 130
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True)
def _cp_mode():
    yield
    cs.set_mode("INDICATOR")


def _vec(d, lo, hi):
    return [float(v) for v in np.linspace(lo, hi, d)]


def _leaf(name, d):
    """(tree, unscaled hyperparameter list, expanded) of a leaf at dimension d"""
    return {
        "SE": (("SE", {}), [0.3], False),
        "SE_expanded": (("SE", {}), [0.45], True),
        "SE_ARD": (("SE", {"ard": True}), [_vec(d, 0.4, 0.9)], False),
        "PER": (("PER", {}), [0.8, 0.6], False),
        "MAT32": (("MAT32", {}), [-0.35], False),       # (a negative l: |l| differentiates to sign(l))
        "MAT52": (("MAT52", {}), [0.4], False),
        "LIN": (("LIN", {}), [_vec(d, 0.2, -0.3)], False),
        "RQ": (("RQ", {}), [0.4, 1.3], False),
    }[name]


LEAVES = ["SE", "SE_expanded", "SE_ARD", "PER", "MAT32", "MAT52", "LIN", "RQ"]
TREES = {
    "ADD(SE,PER)": (("ADD", [("SE", {}), ("PER", {})]), [0.3, 0.9, 0.5], 1),
    "MUL(SE,PER)": (("MUL", [("SE", {}), ("PER", {})]), [0.3, 0.9, 0.5], 1),
    "MUL(ADD(SE,MAT52),PER)": (("MUL", [("ADD", [("SE", {}), ("MAT52", {})]), ("PER", {})]), [0.4, 0.7, 1.0, 0.8], 1),
    "MUL(SE_ARD,MAT52_ARD)@16": (("MUL", [("SE", {"ard": True}), ("MAT52", {"ard": True, "standard": True})]),
                                 [_vec(16, 1.5, 3.0), _vec(16, 2.0, 4.0)], 16),
}
CP3 = ("CP", [("SE", {}), ("SE", {}), ("SE", {})])
CP3_HYP = [0.35, 0.7, 0.2, 0.3, 0.4]


def _has(tree, op):
    return tree[0] == op or (tree[0] in ("ADD", "MUL", "CP") and any(_has(c, op) for c in tree[1]))


def _kernel(tree, hyp, d):
    if _has(tree, "RQ"):
        return rs.make_kernel(tree, d)
    return cs.make_kernel(tree, hyp, d)


def _points(d, seed, cps=None):
    if cps is not None:   # points inside the transition zones of the change points
        x = cs.cp_inputs(N_MAX, seed, cps)[0]
        z = cs.cp_inputs(M_MAX, seed + 1, cps)[0]
        return x, z
    return _inputs(N_MAX, d, seed)[0], _inputs(M_MAX, d, seed + 1)[0]


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(tree, hyp, d, scaled, expanded, mode, x, z, planes [P, N_MAX, M_MAX]) for a case key; computed once"""
    kind, name, scaled, d, mode = key
    if kind == "leaf":
        tree, hyp, expanded = _leaf(name, d)
        if scaled:
            hyp = hyp + [1.7]
        x, z = _points(d, 40 + LEAVES.index(name))
    elif kind == "tree":
        tree, hyp, d = TREES[name]
        expanded = False
        x, z = _points(d, 60)
    else:
        tree, hyp, expanded = CP3, CP3_HYP, False
        x, z = _points(1, 70, cps=CP3_HYP[:2])
    J = fs.jacobian_ref(tree, hyp, x, z, scaled, expanded, mode or "SIGMOID")
    J.setflags(write=False)
    return tree, hyp, d, scaled, expanded, mode, x, z, J


def _device_planes(ref, n, m):
    tree, hyp, d, scaled, expanded, mode, x, z, _ = ref
    set_flags(scaled=scaled, expanded=expanded)
    if mode:
        cs.set_mode(mode)
    return engine.kernel_jacobian(_kernel(tree, hyp, d), hyp_list(hyp), x[:n], z[:m])


def _check(got, ref, label):
    scale = max(1.0, float(np.max(np.abs(ref)))) if ref.size else 1.0
    err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    print("JACERR %s max|got-ref| = %.3e  rel to max|ref| = %.3e" % (label, err, err / max(float(np.max(np.abs(ref))), 1e-300)))
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got))
    assert err <= 1e-7 * scale, (label, err, scale)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", LEAVES)
def test_every_leaf_against_autodiff(name, scaled, d, shape):
    n, m = shape
    ref = _reference(("leaf", name, scaled, d, None))
    got = _device_planes(ref, n, m).cpu().numpy()
    _check(got, ref[-1][:, :n, :m], "%s%s d=%d %dx%d" % (name, " scaled" if scaled else "", d, n, m))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(TREES))
def test_adjoint_masks_against_autodiff(name, shape):
    n, m = shape
    ref = _reference(("tree", name, False, 0, None))
    got = _device_planes(ref, n, m).cpu().numpy()
    _check(got, ref[-1][:, :n, :m], "%s %dx%d" % (name, n, m))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mode", ["SIGMOID", "APPROX_INDICATOR"])
def test_change_points_share_a_bound(mode, shape):
    """CP([SE, SE, SE]): cp_0 is the upper bound of window 0 and the lower bound of window 1, cp_1 likewise."""
    n, m = shape
    ref = _reference(("cp", "CP3", False, 1, mode))
    got = _device_planes(ref, n, m).cpu().numpy()
    _check(got, ref[-1][:, :n, :m], "CP3 %s %dx%d" % (mode, n, m))
    if n > 1:   # both windows contribute to the shared bound: the plane is not one window's alone
        assert np.abs(ref[-1][0, :n, :m]).max() > 1.0 and np.abs(ref[-1][1, :n, :m]).max() > 1.0


VJP_CASES = [
    (("ADD", [("SE", {}), ("PER", {})]), [0.3, 0.9, 0.5], 1, False, None),
    (("MUL", [("ADD", [("SE", {}), ("MAT52", {})]), ("PER", {})]), [0.4, 0.7, 1.0, 0.8], 1, False, None),
    (("SE", {"ard": True}), [[0.4, 0.7, 0.9], 1.5], 3, True, None),
    (("RQ", {}), [0.4, 1.3, 0.8], 2, True, None),
    (CP3, CP3_HYP, 1, False, "SIGMOID"),
]


@pytest.mark.parametrize("case", range(len(VJP_CASES)))
def test_planes_contract_to_kernel_vjp(case):
    """sum_ij G_ij J_p[i, j], summed exactly on the host (math.fsum) from the device planes, against kernel_vjp's
    p-th adjoint: both come from base_partials, so they differ by the rounding of a sum of n m terms in any order,
    2 n m eps sum|G_ij J_p[i, j]|."""
    tree, hyp, d, scaled, mode = VJP_CASES[case]
    n, m = 150, 40
    set_flags(scaled=scaled)
    if mode:
        cs.set_mode(mode)
        x, z = cs.cp_inputs(n, 5, hyp[:2])[0], cs.cp_inputs(m, 6, hyp[:2])[0]
    else:
        x, z = _inputs(n, d, 5)[0], _inputs(m, d, 6)[0]
    k = _kernel(tree, hyp, d)
    G = np.random.default_rng(case).standard_normal((n, m))
    Gd = torch.as_tensor(G, device=engine.device())
    J = engine.kernel_jacobian(k, hyp_list(hyp), x, z).cpu().numpy()
    gh, _ = engine.kernel_vjp(k, hyp_list(hyp), x, z, G=Gd)
    gh = gh.cpu().numpy()
    assert J.shape[0] == gh.shape[0]
    for p in range(J.shape[0]):
        terms = (G * J[p]).reshape(-1)
        exact = math.fsum(terms.tolist())
        bound = 2.0 * n * m * EPS * math.fsum(np.abs(terms).tolist())
        print("VJP case %d p %d |diff| %.3e bound %.3e" % (case, p, abs(exact - gh[p]), bound))
        assert abs(exact - gh[p]) <= bound, (p, exact, gh[p], bound)


def test_batch_through_the_abi_equals_single_calls_bit_for_bit():
    tree, d = ("MUL", [("ADD", [("SE", {}), ("MAT52", {})]), ("PER", {})]), 1
    hyps = [[0.4, 0.7, 1.0, 0.8], [0.25, 0.5, 0.6, 1.1], [0.9, -0.3, 1.4, 0.45]]
    n, m = 65, 130
    x, z = _inputs(n, d, 11)[0], _inputs(m, d, 12)[0]
    k = _kernel(tree, hyps[0], d)
    singles = [engine.kernel_jacobian(k, hyp_list(h), x, z) for h in hyps]
    again = engine.kernel_jacobian(k, hyp_list(hyps[1]), x, z)
    assert torch.equal(again, singles[1])                       # two calls, the same bits
    L, dev = nat.lib(), engine.device()
    kd = engine.kernel_descriptor(k, d)
    P = kd.n_hyp
    H = torch.tensor(hyps, dtype=torch.float64, device=dev)
    X, Z = torch.as_tensor(x, device=dev).contiguous(), torch.as_tensor(z, device=dev).contiguous()
    # a padded row stride and padded plane / member strides, filled with a marker nothing may overwrite
    ldj, ps = m + 3, n * (m + 3) + 5
    bs = P * ps + 7
    J = torch.full((3 * bs,), -7.0, dtype=torch.float64, device=dev)
    assert L.gpk_kernel_jacobian_workspace_bytes(ctypes.byref(kd), n, m, d) == 0
    nat.check(L.gpk_kernel_jacobian(ctypes.byref(kd), nat.ptr(H), P, 3, nat.ptr(X), n, 0, nat.ptr(Z), m, 0, d,
                                    nat.ptr(J), ldj, ps, bs, None, 0, nat.stream_handle(dev)), "gpk_kernel_jacobian")
    Jh = J.cpu()
    written = torch.zeros(3 * bs, dtype=torch.bool)
    for b in range(3):
        for p in range(P):
            plane = Jh[b * bs + p * ps: b * bs + p * ps + n * ldj].reshape(n, ldj)
            assert torch.equal(plane[:, :m], singles[b][p].cpu())
            w = written[b * bs + p * ps: b * bs + p * ps + n * ldj].reshape(n, ldj)
            w[:, :m] = True
    assert bool((Jh[~written] == -7.0).all())                  # nothing outside i < n, j < m is touched


def test_argument_checks():
    L, dev = nat.lib(), engine.device()
    k = _kernel(("SE", {}), [0.3], 1)
    kd = engine.kernel_descriptor(k, 1)
    t = torch.zeros(64, dtype=torch.float64, device=dev)
    s = nat.stream_handle(dev)

    def call(hyp=t, hs=0, batch=1, X=t, n=4, xs=0, Z=t, m=4, zs=0, d=1, J=t, ldj=4, ps=16, bs=16):
        return L.gpk_kernel_jacobian(ctypes.byref(kd), nat.ptr(hyp), hs, batch, nat.ptr(X), n, xs, nat.ptr(Z), m, zs, d,
                                     nat.ptr(J), ldj, ps, bs, None, 0, s)
    assert call() == 0
    assert call(d=2) == -1 and call(hyp=None) == -2 and call(batch=0) == -4 and call(X=None) == -5
    assert call(n=0) == -6 and call(Z=None) == -8 and call(m=0) == -9 and call(J=None) == -12
    assert call(ldj=3) == -13 and call(batch=2, bs=15) == -15 and call(batch=2, xs=3) == -7
    assert "j_bstride" in nat.last_error() or "x_bstride" in nat.last_error()


def test_hard_indicator_planes_and_coincident_points_are_exact_zeros():
    cs.set_mode("INDICATOR")
    x, z = cs.cp_inputs(70, 3, CP3_HYP[:2])[0], cs.cp_inputs(65, 4, CP3_HYP[:2])[0]
    J = engine.kernel_jacobian(_kernel(CP3, CP3_HYP, 1), hyp_list(CP3_HYP), x, z)
    assert bool((J[:2] == 0.0).all())                           # d K / d cp of the hard mask
    assert float(J[2:].abs().max()) > 0.1
    # coincident points: the distance terms differentiate to exactly 0 on the diagonal of K(x, x)
    for tree, hyp, d, planes in [(("SE", {}), [0.3], 1, [0]), (("SE", {"ard": True}), [[0.4, 0.7]], 2, [0, 1]),
                                 (("MAT32", {}), [-0.35], 1, [0]), (("MAT52", {"standard": True}), [0.4], 2, [0]),
                                 (("MAT52", {"ard": True, "standard": True}), [[0.5, 0.9]], 2, [0, 1]),
                                 (("PER", {}), [0.8, 0.6], 1, [0, 1]), (("RQ", {}), [0.4, 1.3], 2, [0, 1])]:
        set_flags()
        xx = _inputs(70, d, 9)[0]
        Jd = engine.kernel_jacobian(_kernel(tree, hyp, d), hyp_list(hyp), xx, xx)
        for p in planes:
            assert bool((torch.diagonal(Jd[p]) == 0.0).all()), (tree, p)
            assert float(Jd[p].abs().max()) > 1e-3


@pytest.mark.parametrize("case", ["scalar", "ard", "operator", "cp"])
def test_get_derivative_matrices(case):
    n, m = 65, 33
    if case == "scalar":
        tree, hyp, d, scaled = ("SE", {}), [0.3, 1.7], 1, True
    elif case == "ard":
        tree, hyp, d, scaled = ("SE", {"ard": True}), [[0.4, 0.7, 0.9], 1.5], 3, True
    elif case == "operator":
        tree, hyp, d, scaled = ("MUL", [("SE", {"ard": True}), ("PER", {})]), [[0.4, 0.7], 0.9, 0.5], 2, False
    else:
        tree, hyp, d, scaled = CP3, CP3_HYP, 1, False
        cs.set_mode("SIGMOID")
    set_flags(scaled=scaled)
    x, z = _inputs(n, d, 21)[0], _inputs(m, d, 22)[0]
    k = _kernel(tree, hyp, d)
    hl = hyp_list(hyp)
    K = k.get_tf_tensor(hl, x, z)
    K0 = K.clone()
    out = k.get_derivative_matrices(hl, x, z)
    assert isinstance(out, list) and len(out) == len(hl)
    for o, h in zip(out, hl):
        assert tuple(o.shape) == tuple(h.shape) + (n, m) and o.dtype == torch.float64 and o.is_cuda
    flat = torch.cat([o.reshape(-1, n, m) for o in out])
    assert torch.equal(flat, engine.kernel_jacobian(k, hl, x, z))
    assert torch.equal(K, K0) and torch.equal(k.get_tf_tensor(hl, x, z), K0)
    ref = fs.jacobian_ref(tree, hyp, x, z, scaled, False, "SIGMOID")
    _check(flat.cpu().numpy(), ref, "get_derivative_matrices %s" % case)
