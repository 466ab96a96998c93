"""Folded in-group columns (gpk_tune "ingroup" = 4, needs the MI355X): a column k of the two-level scheme with d > 0
earlier panels in its half is solved as  X = [A | C] [ -L^-1 B | L^-1 ]^T  in one panel-solve launch of depth
128 (d + 1) (prep_kernel forms the right operand), instead of a thin update of the column followed by its solve.

The same operations in another association: against ingroup = 3 the read-outs agree to rel <= 1e-12 (the project's bar
between in-group schedules, tests/test_gpu_diag_versions.py; a numpy restatement of both schemes on these inputs --
SURVEY section 8d generator, noise 1e-2 -- agrees to 2.4e-14), not bitwise.  Against the fp64 oracle: -LML rel <= 1e-9
(SURVEY section 8d), posterior mean and variance max-abs <= 1e-8 (tests/test_gpu_parity.py's C2 bounds).  Two runs of
mode 4 are bitwise equal.

Shapes (batch 3, fuse_trsm = 0 so that no panel solve runs inside the diagonal launch -- those columns keep mode 3):
  n =  640, group 4          d = 1 only
  n = 1280, group 8          d = 1 .. 3, a short last group
  n = 1100, group 8          identity padding under the last panel
  n = 1280, m = 77, group 8  test rows
each with the look-ahead off / on, the fused K build off / on, upd_tri 0 / 1, and with the launches on 64-row tiles
(these batches' own choice) and forced onto the 128-row tile kernels (trsm_t128_min = upd_t128_min = 0).
"""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as o
from tests.helpers import make_kernel
from tests.test_gpu_segmented import ragged_members
from tests.test_gpu_update_triangle import _Knobs, _assert_bitwise, _host

from gaussianprocessfundamentals_amd import engine

pytestmark = pytest.mark.gpu

SE = ("SE", {"ard": False})
MAT52 = ("MAT52", {})
LS = (0.1, 0.163, 0.13)
NOISE = 1e-2
SHAPES = [(640, 4, 0), (1280, 8, 0), (1100, 8, 0), (1280, 8, 77)]


def _problem(n, m, noise=(NOISE,), dtype=None):
    x, y = o.make_inputs("metric", n=n, seed=5)
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(SE, 1), 1)
    H = torch.tensor([[l] for l in LS], dtype=torch.float64, device=dev)
    NZ = torch.tensor(list(noise), dtype=torch.float64, device=dev)
    X = torch.tensor(x, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
    Y = torch.tensor(y, dtype=torch.float64, device=dev).reshape(1, -1).contiguous()
    xs = np.linspace(-0.1, 1.1, max(m, 1)).reshape(-1, 1)
    Xs = torch.tensor(xs, dtype=torch.float64, device=dev) if m else None

    def run():
        f = engine.AugmentedFactorization(n, 1, m, len(LS), dtype)
        f.W.zero_()
        f.run(kd, H, H.shape[1], NZ, 1 if len(noise) > 1 else 0, X, 0, Y, 0, Xs, 0)
        if not m:
            return f, []
        return f, [torch.stack([f.posterior_mu(b) for b in range(len(LS))]),
                   torch.stack([f.posterior_var_diag(b) for b in range(len(LS))])]
    return run, x, y, xs


@pytest.fixture(scope="module", params=SHAPES, ids=lambda c: "n%d-g%d-m%d" % c)
def shape(request):
    """The problem and the oracle's answers, computed once per shape."""
    n, group, m = request.param
    run, x, y, xs = _problem(n, m)
    ref = []
    for l in LS:
        c = o.nlml_components(SE, [l], NOISE, x, y)
        mu, var = o.posterior(SE, [l], NOISE, x, y, xs) if m else (None, None)
        ref.append((c["nlml"], mu, None if var is None else np.diag(var)))
    return n, group, m, run, ref


def _run(run, ingroup, **knobs):
    with _Knobs(chain=0, fuse_trsm=0, ingroup=ingroup, **knobs):
        f, more = run()
        return _host(f, more), f.layout


def _has_fold(lay, **knobs):
    with engine.nat.thread_tune(fuse_trsm=0, ingroup=4, **knobs):
        steps = engine.nat.launch_plan(lay)
    return bool((steps["kind"] == 5).any())


def _rel(a, b):
    return np.max(np.abs(a - b) / np.abs(b))


@pytest.mark.parametrize("t128", [0, 1])
@pytest.mark.parametrize("tri", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("lookahead", [0, 1])
def test_folded_columns_agree_with_the_two_level_schedule_and_the_oracle(shape, lookahead, fuse, tri, t128):
    n, group, m, run, ref = shape
    knobs = dict(group=group, group_first=group, lookahead=lookahead, fuse_kbuild=fuse, upd_tri=tri)
    if t128:
        knobs.update(trsm_t128_min=0, upd_t128_min=0)
    a, lay = _run(run, 4, **knobs)
    a2, _ = _run(run, 4, **knobs)
    b, _ = _run(run, 3, **knobs)
    assert _has_fold(lay, **{k: v for k, v in knobs.items() if k != "upd_tri"})  # (the folded steps really ran)
    assert not a[2].any() and not b[2].any()                    # info == 0
    _assert_bitwise(a, a2, lower_only=False)                    # two runs of mode 4: the same bits
    out4, out3 = a[1].reshape(-1, 4), b[1].reshape(-1, 4)
    print("n %d m %d la %d fuse %d tri %d t128 %d: vs ingroup 3 nlml %.2e fit %.2e logdet %.2e; vs oracle %.2e"
          % (n, m, lookahead, fuse, tri, t128, _rel(out4[:, 0], out3[:, 0]), _rel(out4[:, 1], out3[:, 1]),
             _rel(out4[:, 2], out3[:, 2]), _rel(out4[:, 0], np.array([r[0] for r in ref]))))
    for c in range(3):                                          # -LML, fit, logdet against the two-level schedule
        assert _rel(out4[:, c], out3[:, c]) <= 1e-12
    assert _rel(out4[:, 0], np.array([r[0] for r in ref])) <= 1e-9
    if m:
        for i, (_, mu, vd) in enumerate(ref):
            assert np.max(np.abs(a[3][i] - mu)) <= 1e-8
            assert np.max(np.abs(a[4][i] - vd)) <= 1e-8


@pytest.mark.parametrize("lookahead", [0, 1])
def test_a_member_that_is_not_positive_definite(lookahead):
    """Member 1 at noise -0.5: its info is mode 3's, and the other members' results are bit for bit what they are in
    a batch without it."""
    n, group = 1280, 8
    knobs = dict(group=group, group_first=group, lookahead=lookahead, fuse_kbuild=0)
    bad, _ = _run(_problem(n, 0, noise=(NOISE, -0.5, NOISE))[0], 4, **knobs)
    bad3, _ = _run(_problem(n, 0, noise=(NOISE, -0.5, NOISE))[0], 3, **knobs)
    good, _ = _run(_problem(n, 0, noise=(NOISE, NOISE, NOISE))[0], 4, **knobs)
    assert np.array_equal(bad[2], bad3[2]) and bad[2][1] > 0 and bad[2][0] == 0 and bad[2][2] == 0
    for i in (0, 2):
        _assert_bitwise([bad[0][i], bad[1].reshape(-1, 4)[i]], [good[0][i], good[1].reshape(-1, 4)[i]],
                        lower_only=False)


def _mode4_is_mode3(fn, **knobs):
    out = {}
    for mode in (4, 3):
        with _Knobs(chain=0, fuse_trsm=0, ingroup=mode, lookahead=0, **knobs):
            f, more = fn()
            out[mode] = _host(f, more)
    _assert_bitwise(out[4], out[3], lower_only=False)


def test_f32_keeps_the_two_level_schedule():
    run = _problem(1280, 0, dtype=torch.float32)[0]
    _mode4_is_mode3(run, group=8, group_first=8)


def test_identity_augmented_layout_keeps_the_two_level_schedule():
    x, y = o.make_inputs("metric", n=1100, seed=5)
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(SE, 1), 1)
    X = torch.tensor(x, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
    Y = torch.tensor(y, dtype=torch.float64, device=dev).reshape(1, -1).contiguous()
    H = torch.tensor([[l] for l in LS], dtype=torch.float64, device=dev)
    NZ = torch.tensor([NOISE], dtype=torch.float64, device=dev)

    def run():
        f = engine.InverseFactorization(len(x), 1, len(LS))
        f.W.zero_()
        f.run(kd, H, 1, NZ, 0, X, 0, Y, 0)
        return f, [f.gradient()]
    _mode4_is_mode3(run, group_eye=4)


def test_ragged_batch_keeps_the_two_level_schedule():
    sizes, tsz = [1280, 1000, 700, 129], [10, 0, 33, 5]
    members, _ = ragged_members([(SE, [0.1]), (MAT52, [0.3])], sizes, tsz)

    def run():
        f = engine.RaggedFactorization(sizes, 1, tsz)
        f.W.zero_()
        f.run(members, NOISE)
        return f, [f.mu, f.var]
    _mode4_is_mode3(run, group=8, group_first=8)
