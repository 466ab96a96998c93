"""Software-pipelined K loop of the f64 128 x 128 trailing-update tile (gemm_kernel) vs the 64 x 64 update
tile, which runs the plain loop of the shared tile core (needs the MI355X).

The rotated loop carries the last k-step of every chunk across the chunk barrier and reorders the fragment
reads, but per accumulator element the k-steps still come in the same order onto C loaded first, so the whole
augmented matrix, the read-outs and info must agree BIT FOR BIT with the 64-tile kernel.  Every case runs the
launch path (chain 0, lookahead 0) twice: upd_t128_min = 1 (the 128-tile kernel on every trailing update) and
upd_t128_min = 2^30 (the 64-tile kernel on every one).  Both equal the persistent launch, whose tile task runs
the plain loop on 128 x 128 tiles.

The same comparison is made between the two panel-solve tile heights (trsm_t128_min = 1 and 2^30, 128 and 64
rows) and, for an f32 factorisation, between the tile sizes of both kernels: instantiations of the plain loop
that no other bitwise test singles out.

W is compared on the lower triangle (row >= column) of every member's whole augmented matrix -- L, z, V^T, the
Schur corner, K^-1 -- which is all the factorisation defines.  Above the diagonal the two tile sizes differ by
design, with either loop: a 128 x 128 diagonal tile also updates its upper 64 x 64 quarter, which no 64 x 64
tile covers (measured with the plain loop: n = 300, m = 0 differs in exactly the 4096 words of rows 128..191,
columns 192..255, and in none with row >= column).

Shapes: the smallest at which the loop can go wrong -- the three row-block forms side by side in one workgroup
(tiles of the y row's block: n = 300 with m = 0, 40, 100 gives the waves forms 1 + 0, MB + 0, MB + MB), every
chunk count from 8 to 128 (group 1 .. 16) under every in-group schedule, the fused-K-build instantiations,
a ragged batch (zero-row tiles skipped), the identity-augmented layout, and a batch with test rows."""
import numpy as np
import pytest
import torch

from oracle import gp_oracle as o
from tests.helpers import make_kernel

from gaussianprocessfundamentals_amd import engine
from tests.test_gpu_segmented import ragged_members

pytestmark = pytest.mark.gpu

SE = ("SE", {"ard": False})
MAT52 = ("MAT52", {})
T128, T64 = 1, 2 ** 30


class _Knobs:
    """gpk_tune knobs set for a block, each restored on the way out."""

    def __init__(self, **kv):
        self.kv, self.old = kv, []

    def __enter__(self):
        for k, v in self.kv.items():
            self.old.append((k, engine.nat.tune(k, v)))
        return self

    def __exit__(self, *exc):
        for k, v in reversed(self.old):
            engine.nat.tune(k, v)
        return False


def _lower(f):
    """The lower triangles (row >= column) of every member's augmented matrix, [batch, p, ld]."""
    return torch.stack([torch.tril(f.w(b)) for b in range(f.batch)])


def _both(fn, vary="upd_t128_min", **knobs):
    """fn() -> (factorisation, further results) on the launch path with 128-tile and with 64-tile updates (or
    panel solves: vary = "trsm_t128_min") -> two lists of host arrays: W's lower triangles, out, info, then the
    further results."""
    out = {}
    for t in (T128, T64):
        with _Knobs(chain=0, lookahead=0, **{vary: t}, **knobs):
            f, more = fn()
            torch.cuda.synchronize()
            out[t] = [np.array(r.detach().cpu().numpy(), copy=True) for r in [_lower(f), f.out, f.info] + list(more)]
    return out[T128], out[T64]


def _assert_bitwise(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype
        bits = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(u.dtype)
        assert np.array_equal(u.view(bits) if bits else u, v.view(bits) if bits else v)


def _plain(n, m, batch, tree=SE, hyps=None, seed=3, dtype=torch.float64, noise=1e-2):
    x, y = o.make_inputs("C1", n=n, seed=seed)
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(tree, 1), 1)
    hyps = hyps or [[0.1]] * batch
    H = torch.tensor(hyps, dtype=torch.float64, device=dev)
    NZ = torch.tensor([noise], dtype=torch.float64, device=dev)
    X = torch.tensor(x, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
    Y = torch.tensor(y, dtype=torch.float64, device=dev).reshape(1, -1).contiguous()
    Xs = torch.linspace(-0.1, 1.1, max(m, 1), dtype=torch.float64, device=dev).reshape(-1, 1) if m else None

    def run():
        f = engine.AugmentedFactorization(n, 1, m, batch, dtype)
        f.W.zero_()
        f.run(kd, H, H.shape[1], NZ, 0, X, 0, Y, 0, Xs, 0)
        return f, ([f.mu, f.var] if m else [])
    return run


@pytest.mark.parametrize("m", [0, 40, 100])
def test_row_block_forms_side_by_side(m):
    """n = 300: the y row's block gives the wr = 0 waves one or MB live row blocks and the wr = 1 waves none or MB."""
    a, b = _both(_plain(300, m, 1))
    _assert_bitwise(a, b)


def test_batch_with_test_rows():
    a, b = _both(_plain(777, 64, 3, hyps=[[0.05 + 0.03 * i] for i in range(3)]))
    _assert_bitwise(a, b)


@pytest.mark.parametrize("n,m,batch", [(300, 0, 1), (300, 100, 1), (777, 64, 3)])
def test_panel_solve_tile_heights(n, m, batch):
    """128-row vs 64-row panel-solve tiles (update tiles fixed at 128): the y row's block gives the MB / 1 / 0 forms.
    fuse_trsm = 0: with the look-ahead off, the diagonal-block kernel would otherwise solve the panels of matrices
    this small itself and gemm_kernel<TRSM> would not be launched at all."""
    a, b = _both(_plain(n, m, batch, hyps=[[0.05 + 0.03 * i] for i in range(batch)]), vary="trsm_t128_min",
                 upd_t128_min=T128, fuse_trsm=0)
    _assert_bitwise(a, b)


@pytest.mark.parametrize("vary,fixed", [("upd_t128_min", {}), ("trsm_t128_min", {"upd_t128_min": T128})])
@pytest.mark.parametrize("n,m", [(300, 0), (300, 100), (1000, 37)])
def test_f32_tile_sizes(n, m, vary, fixed):
    """The f32 launch path (the factorisation tests/test_gpu_chain_f32.py compares the persistent launch with):
    128- vs 64-tile updates, and 128- vs 64-row panel solves."""
    a, b = _both(_plain(n, m, 1, dtype=torch.float32, noise=1e-1), vary=vary, **fixed)
    _assert_bitwise(a, b)


@pytest.fixture(scope="module")
def grouped():
    return _plain(2100, 100, 2, tree=MAT52, hyps=[[0.2], [0.4]])


@pytest.mark.parametrize("ingroup", [1, 2, 3])
@pytest.mark.parametrize("group", [1, 2, 3, 8, 16])
def test_every_chunk_count_and_in_group_schedule(grouped, group, ingroup):
    """K = 128 group: 8 .. 128 chunks per update, and the in-group left-looking updates of every depth below it."""
    a, b = _both(grouped, group=group, ingroup=ingroup)
    _assert_bitwise(a, b)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("tree,hyp", [(SE, [0.1]), (MAT52, [0.3])])
def test_fused_kbuild_instantiations(tree, hyp, fuse):
    """group 2 at n = 600 (5 panels): the first trailing update is the one that evaluates its C tiles."""
    a, b = _both(_plain(600, 0, 2, tree=tree, hyps=[hyp, [1.3 * hyp[0]]]), group=2, group_first=2, fuse_kbuild=fuse)
    _assert_bitwise(a, b)
    assert not a[2].any()


def test_ragged_batch():
    sizes, tsz = [300, 1000, 129, 1], [10, 0, 33, 5]
    members, _ = ragged_members([(SE, [0.1]), (MAT52, [0.3])], sizes, tsz)

    def run():
        f = engine.RaggedFactorization(sizes, 1, tsz)
        f.W.zero_()
        f.run(members, 1e-2)
        return f, [f.mu, f.var]
    a, b = _both(run)
    _assert_bitwise(a, b)


def test_identity_augmented_layout():
    x, y = o.make_inputs("C1", n=500, seed=21)
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(SE, 1), 1)
    X = torch.tensor(x, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
    Y = torch.tensor(y, dtype=torch.float64, device=dev).reshape(1, -1).contiguous()
    H = torch.tensor([[0.07]], dtype=torch.float64, device=dev)
    NZ = torch.tensor([1e-2], dtype=torch.float64, device=dev)

    def run():
        f = engine.InverseFactorization(len(x), 1, 1)
        f.W.zero_()
        f.run(kd, H, 1, NZ, 0, X, 0, Y, 0)
        return f, [f.gradient()]
    a, b = _both(run)
    _assert_bitwise(a, b)


def test_nlml_matches_oracle_on_the_128_tile_path():
    n = 700
    x, y = o.make_inputs("C1", n=n, seed=4)
    with _Knobs(chain=0, lookahead=0, upd_t128_min=T128, group=2, group_first=2):
        f, _ = _plain(n, 0, 1, seed=4)()
        got = float(f.nlml()[0])
        assert int(f.info[0]) == 0
    exp = o.nlml(SE, [0.1], 1e-2, x, y)
    assert abs(got - exp) <= 1e-9 * abs(exp)
