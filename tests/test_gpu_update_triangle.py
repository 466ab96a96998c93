"""The f64 trailing update split by tile class (gpk_tune "upd_tri", needs the MI355X): gemm_kernel on the strictly lower
128 x 128 tiles and update_tri_kernel on the lower 16 x 16 blocks of the diagonal tiles (plus, when the y row's tile row
has a single live 16-row block, that block's row) against one gemm_kernel launch over all tiles (upd_tri = 0).

update_tri_kernel stages like the shared tile core and feeds every accumulator element its k-steps in the same order
onto C loaded first, so everything the factorisation defines must agree BIT FOR BIT between the two: the lower triangle
(row >= column) of every member's augmented matrix, the read-outs (nlml, fit, logdet) and info.  Above the diagonal the
two differ by design: the 28 blocks strictly above the diagonal of a diagonal tile are no longer written.

Shapes: group = 2 (4 where the two-level in-group schedule needs it) and upd_t128_min = 0 put several group updates on
the 128-tile path at N of a few hundred:
  n = 640, m = 0   the plain case: the y row's block folded into the diagonal tiles' workgroups
  n = 700, m = 0   identity padding rows in the last block of K
  n = 640, m = 5   test rows and y in one 16-row block: folded
  n = 640, m = 20  two live 16-row blocks in the last tile row: not folded, triangles only (its own diagonal tile partial)
  n = 384, batch 3 a single trailing column after the first group
each under in-group schedules 1 and 3, with the look-ahead off and on (LOOKAHEAD and BULK launches, c_lo > 0) and with
the fused K build off and on (its launch keeps the single kernel).
"""
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


def _host(f, more=()):
    """Host copies: every member's whole W [batch, p, ld], out, info, then the further results."""
    torch.cuda.synchronize()
    W = torch.stack([f.w(b) for b in range(f.batch)])
    return [np.array(r.detach().cpu().numpy(), copy=True) for r in [W, f.out, f.info] + list(more)]


def _both(fn, **knobs):
    """fn() -> (factorisation, further results) on the launch path with upd_tri = 1 and 0."""
    out = {}
    for tri in (1, 0):
        with _Knobs(chain=0, upd_t128_min=0, upd_tri=tri, **knobs):
            f, more = fn()
            out[tri] = _host(f, more)
    return out[1], out[0]


def _bits(u):
    kind = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}.get(u.dtype)
    return u.view(kind) if kind else u


def _assert_bitwise(a, b, lower_only=True):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype
        if k == 0 and lower_only:
            u, v = np.tril(u), np.tril(v)
        assert np.array_equal(_bits(u), _bits(v))


def _plain(n, m, batch, tree=SE, seed=3, noise=1e-2):
    x, y = o.make_inputs("C1", n=n, seed=seed)
    dev = engine.device()
    kd = engine.kernel_descriptor(make_kernel(tree, 1), 1)
    H = torch.tensor([[0.05 + 0.03 * i] for i in range(batch)], dtype=torch.float64, device=dev)
    NZ = torch.tensor([noise], dtype=torch.float64, device=dev)
    X = torch.tensor(x, dtype=torch.float64, device=dev).reshape(-1, 1).contiguous()
    Y = torch.tensor(y, dtype=torch.float64, device=dev).reshape(1, -1).contiguous()
    Xs = torch.linspace(-0.1, 1.1, max(m, 1), dtype=torch.float64, device=dev).reshape(-1, 1) if m else None

    def run():
        f = engine.AugmentedFactorization(n, 1, m, batch)
        f.W.zero_()
        f.run(kd, H, H.shape[1], NZ, 0, X, 0, Y, 0, Xs, 0)
        return f, ([f.mu, f.var] if m else [])
    return run


CASES = [(640, 2, 0), (700, 2, 0), (640, 2, 5), (640, 2, 20), (384, 3, 0)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "n%d-b%d-m%d" % c)
def case(request):
    n, batch, m = request.param
    return n, _plain(n, m, batch)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("group,ingroup", [(2, 1), (2, 3), (4, 3)])
def test_split_update_writes_the_same_bits(case, group, ingroup, lookahead, fuse):
    """(group 4, ingroup 3: the two-level schedule's HALF update, which group 2 is too short for.)"""
    n, run = case
    a, b = _both(run, group=group, group_first=group, ingroup=ingroup, lookahead=lookahead, fuse_kbuild=fuse)
    _assert_bitwise(a, b)
    assert not a[2].any()
    if n >= 640 and group == 2:
        # the split really ran: a later group's diagonal tile (rows 512 ..) keeps its blocks above the diagonal
        assert not np.array_equal(_bits(np.triu(a[0], 1)), _bits(np.triu(b[0], 1)))


def test_diagonal_tiles_first():
    """upd_tri = 2: the same two kernels in the other order."""
    run = _plain(640, 5, 2)
    with _Knobs(chain=0, upd_t128_min=0, upd_tri=2, group=2, group_first=2, fuse_kbuild=0, lookahead=0):
        f, more = run()
        a = _host(f, more)
    with _Knobs(chain=0, upd_t128_min=0, upd_tri=0, group=2, group_first=2, fuse_kbuild=0, lookahead=0):
        f, more = run()
        b = _host(f, more)
    _assert_bitwise(a, b)


def test_ragged_batch_keeps_the_single_kernel():
    sizes, tsz = [300, 1000, 129, 1], [10, 0, 33, 5]
    members, _ = ragged_members([(SE, [0.1]), (MAT52, [0.3])], sizes, tsz)

    def run():
        f = engine.RaggedFactorization(sizes, 1, tsz)
        f.W.zero_()
        f.run(members, 1e-2)
        return f, [f.mu, f.var]
    a, b = _both(run, group=2, group_first=2, lookahead=0)
    _assert_bitwise(a, b, lower_only=False)


def test_identity_augmented_layout_keeps_the_single_kernel():
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
    a, b = _both(run, group_eye=2, lookahead=0)
    _assert_bitwise(a, b, lower_only=False)


def _first_bad_pivot(K):
    """1-based column of the first non-positive pivot of an unblocked Cholesky factorisation of K."""
    A = np.array(K, dtype=np.float64, copy=True)
    for k in range(A.shape[0]):
        if not A[k, k] > 0.0:
            return k + 1
        A[k + 1:, k] /= np.sqrt(A[k, k])
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return 0


def test_not_positive_definite_reports_the_first_bad_pivot():
    n, noise = 640, -0.5
    a, b = _both(_plain(n, 0, 2, noise=noise), group=2, group_first=2, lookahead=0, fuse_kbuild=0)
    assert np.array_equal(a[2], b[2])
    x, _ = o.make_inputs("C1", n=n, seed=3)
    for i in range(2):
        K = o.k_noised(SE, [0.05 + 0.03 * i], noise, x.reshape(-1, 1))
        want = _first_bad_pivot(K)
        assert want > 0 and int(a[2][i]) == want


def test_persistent_launch_matches_the_split_launch_path():
    """The chain-vs-launch bitwise contract with the split on."""
    run = _plain(640, 0, 1)
    with _Knobs(chain=2):
        before = engine.nat.chain_stats()["launches"]
        f, more = run()
        c = _host(f, more)
        assert engine.nat.chain_stats()["launches"] > before
    with _Knobs(chain=0, upd_t128_min=0, upd_tri=1, group=2, group_first=2, lookahead=0):
        f, more = run()
        l = _host(f, more)
    yr = f.layout.y_row  # (what the contract covers: L, z and the Schur corner, as tests/test_gpu_chain.py)
    c[0], l[0] = c[0][:, :yr + 1, :yr + 1], l[0][:, :yr + 1, :yr + 1]
    _assert_bitwise(c, l)
