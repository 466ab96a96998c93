"""Host-side checks of the launch path's schedule (gpk_launch_plan; no GPU): the steps gpk_potrf_aug / _ex / _ragged
enqueue -- launches and event edges, in issue order -- taken from nat.launch_plan alone.

Coverage: every (tile, panel) update exactly once and before the tile's block column is factored / solved, tiles the
band compression leaves out wholly inside the step's zero band.  Ordering: any two launches that touch a common tile
(write / write or read / write) are ordered by per-stream program order plus the record -> wait edges.  Replay: the
steps executed in list order in numpy reproduce numpy's Cholesky factor, solves and Schur corner.  Accounting: the
flops per class sum to the closed forms over padded blocks.
"""
import itertools

import numpy as np
import pytest

from gaussianprocessfundamentals_amd import _build, _native as nat

NB = 128
DIAG, TRSM, UPDATE, RECORD, WAIT = range(5)
CALLER, PANEL, BULK = range(3)
EPS = np.finfo(np.float64).eps

BLOCKS = (3, 5, 9)
GROUPS = (2, 4)
KINDS = ("m0", "m77", "eye")
# the panel solve fused into the diagonal launch (with a bound that leaves the first panels of 9 blocks unfused) or not
FUSE = ({"fuse_trsm": 0}, {"fuse_trsm": 2, "fuse_trsm_max": 24})
CASES = list(itertools.product(BLOCKS, GROUPS, KINDS, (1, 2, 3), (0, 1), (0, 1)))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    _build.build()


def layout(nblk, kind, batch=1, dtype=nat.GPK_F64):
    n = nblk * NB - 28  # (not a multiple of the block: identity padding under the last panel)
    return nat.plan(dtype, batch, n, {"m0": 0, "m77": 77, "eye": n}[kind], 1)


def plan_of(nblk, group, kind, ingroup, la, fuse, batch=1, **kw):
    lay = layout(nblk, kind, batch)
    knobs = dict(ingroup=ingroup, lookahead=la, group=group, group_eye=group, group_first=group, **FUSE[fuse])
    knobs.update(kw)
    with nat.thread_tune(**knobs):
        return lay, nat.launch_plan(lay, eye=kind == "eye", counters=True)


# ------------------------------------------------------------------------------------------ what a step touches
def zero_rows(s, r0, r1):
    """gemm_kernel's own skip (uniform batches): rows wholly inside the step's zero band"""
    return r0 >= s["zlo"] and r1 <= s["zhi"]


def expand(s, t):
    """compressed tile index -> tile index from row0 (the grid leaves out the bzn tiles from bz0)"""
    return t + s["bzn"] if s["bzn"] and t >= s["bz0"] else t


def update_tiles(s):
    """(row, column) of every tile the UPDATE launch enumerates, as element offsets (tile edge s['tile'])"""
    T = int(s["tile"])
    for tj in range(int(s["c_lo"]), int(s["c_hi"])):
        for ti in range(tj, int(s["nt"])):
            yield int(s["row0"]) + expand(s, ti) * T, int(s["row0"]) + expand(s, tj) * T


def solve_tiles(s):
    """first rows of the row tiles a panel solve covers (TRSM step, or a DIAG step with the solve fused), tile edge"""
    if s["kind"] == DIAG:
        return [int(s["row0"]) + 64 * t for t in range(int(s["trsm_tiles"]))], 64
    T = int(s["tile"])
    return [int(s["row0"]) + expand(s, t) * T for t in range(int(s["nt"]))], T


def is_solve(s):
    return s["kind"] == TRSM or (s["kind"] == DIAG and s["trsm_tiles"] > 0)


# ------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("nblk,group,kind,ingroup,la,fuse", CASES)
def test_every_tile_receives_every_panel_once_before_it_is_used(nblk, group, kind, ingroup, la, fuse):
    lay, steps = plan_of(nblk, group, kind, ingroup, la, fuse)
    p, n_pad = lay.p, lay.n_pad
    R = p // NB
    assert n_pad == nblk * NB
    diag_at, solve_at = {}, {}
    for i, s in enumerate(steps):
        if s["kind"] == DIAG:
            c = int(s["kblk"])
            assert c not in diag_at and s["j0"] == c * NB
            diag_at[c] = i
        if is_solve(s):
            c = int(s["j0"]) // NB
            assert c not in solve_at and s["row0"] == (c + 1) * NB
            assert i >= diag_at[c]  # (the block is factored by then: same launch, or a later one)
            solve_at[c] = i
            rows, T = solve_tiles(s)
            got = set()
            for r0 in rows:
                assert r0 % T == 0 and r0 + T <= p and r0 not in got
                got.add(r0)
            for r0 in range((c + 1) * NB, p, T):  # every row tile below the block, or wholly in the zero band
                assert r0 in got or zero_rows(s, r0, r0 + T), (c, r0)
    assert sorted(diag_at) == sorted(solve_at) == list(range(nblk))
    if not fuse:
        assert all(s["trsm_tiles"] == 0 for s in steps)
    else:
        assert any(s["kind"] == DIAG and s["trsm_tiles"] > 0 for s in steps)
        assert sum(s["kind"] == TRSM for s in steps) + sum(s["kind"] == DIAG and s["trsm_tiles"] > 0 for s in steps) == nblk

    # 64 x 64 cells (i, j), j < n_pad / 64: seen[i, j, q] = updates of the cell with panel q
    H = 64
    seen = np.zeros((p // H, n_pad // H, nblk), dtype=np.int32)
    last = np.full((p // H, n_pad // H), -1, dtype=np.int64)
    for i, s in enumerate(steps):
        if s["kind"] != UPDATE:
            continue
        T, row0, j0, kd = int(s["tile"]), int(s["row0"]), int(s["j0"]), int(s["kdepth"])
        assert T in (64, 128) and j0 % NB == 0 and kd % NB == 0 and kd > 0 and row0 == j0 + kd
        q0, q1 = j0 // NB, (j0 + kd) // NB
        cols = {}
        for r0, c0 in update_tiles(s):
            assert r0 + T <= p and c0 + T <= p and r0 >= c0
            cols.setdefault(c0, set()).add(r0)
            if c0 >= n_pad:
                continue
            for di in range(T // H):
                for dj in range(T // H):
                    if r0 // H + di >= c0 // H + dj:  # (lower cells: the diagonal block is read as a lower triangle)
                        seen[r0 // H + di, c0 // H + dj, q0:q1] += 1
                        last[r0 // H + di, c0 // H + dj] = i
        # a tile the band compression leaves out lies wholly inside [zlo, zhi): below every enumerated column, the
        # rows from the column's own tile to the end are enumerated or in the band (no factored column is)
        for c0, rows in cols.items():
            assert not zero_rows(s, c0, c0 + T) or c0 >= n_pad
            for r0 in range(c0, p, T):
                assert r0 in rows or zero_rows(s, r0, r0 + T), (i, r0, c0)
        assert s["nt"] == (p - row0) // T - s["bzn"]
        if s["bzn"]:
            assert kind == "eye"
            b0, b1 = row0 + int(s["bz0"]) * T, row0 + int(s["bz0"] + s["bzn"]) * T
            assert s["zlo"] <= b0 and b1 <= s["zhi"]
    if kind == "eye":
        assert any(s["bzn"] > 0 for s in steps)  # (the compression is exercised)
    for i64 in range(p // H):
        for j64 in range(min(i64 + 1, n_pad // H)):
            r, c = i64 // 2, j64 // 2
            # identity rows: row n_pad + t of E L^-T is zero left of column t, so its cells receive nothing from
            # the panels left of the row's own block -- those are the cells a step may leave out
            structurally_zero = kind == "eye" and n_pad <= i64 * H < lay.y_row and (i64 * H + H) <= lay.y_row
            for q in range(c):
                if structurally_zero and (q + 1) * NB <= i64 * H - n_pad:
                    assert seen[i64, j64, q] <= 1
                else:
                    assert seen[i64, j64, q] == 1, (i64, j64, q, seen[i64, j64, q])
            assert not seen[i64, j64, c:].any()
            if c > 0 and last[i64, j64] >= 0:
                assert last[i64, j64] < (diag_at[c] if r == c else solve_at[c]), (i64, j64)
            assert r < R


# ------------------------------------------------------------------------------------------------- ordering
def happens_before(steps):
    """anc[i]: bit mask of the steps that precede step i -- per-stream program order plus record -> wait edges, a
    wait bound to the latest earlier record of its event (as HIP binds it at enqueue time)"""
    anc = [0] * len(steps)
    last_on = {}
    recorded = {}
    for i, s in enumerate(steps):
        preds = []
        if int(s["stream"]) in last_on:
            preds.append(last_on[int(s["stream"])])
        last_on[int(s["stream"])] = i
        if s["kind"] == RECORD:
            recorded[int(s["event"])] = i
        elif s["kind"] == WAIT:
            assert int(s["event"]) in recorded, "wait for an event never recorded"
            preds.append(recorded[int(s["event"])])
        for q in preds:
            anc[i] |= anc[q] | (1 << q)
    return anc


def touches(lay, s):
    """(read mask, write mask) over 64 x 64 cells of W (bit i * nc + j) plus one bit per inverted diagonal block"""
    H, nc = 64, lay.p // 64
    inv0 = nc * nc

    def cells(r0, r1, c0, c1):
        m = 0
        for i in range(r0 // H, r1 // H):
            for j in range(c0 // H, c1 // H):
                m |= 1 << (i * nc + j)
        return m

    rd = wr = 0
    j0 = int(s["j0"])
    if s["kind"] == DIAG:
        wr |= cells(j0, j0 + NB, j0, j0 + NB) | 1 << (inv0 + j0 // NB)
    if is_solve(s):
        rd |= 1 << (inv0 + j0 // NB)
        rows, T = solve_tiles(s)
        for r0 in rows:
            if not zero_rows(s, r0, r0 + T):
                wr |= cells(r0, r0 + T, j0, j0 + NB)
    if s["kind"] == UPDATE:
        T, kd = int(s["tile"]), int(s["kdepth"])
        for r0, c0 in update_tiles(s):
            if zero_rows(s, r0, r0 + T) or zero_rows(s, c0, c0 + T):
                continue
            rd |= cells(r0, r0 + T, j0, j0 + kd) | cells(c0, c0 + T, j0, j0 + kd)
            wr |= cells(r0, r0 + T, c0, c0 + T)
    return rd | wr, wr  # (every written cell is read first)


@pytest.mark.parametrize("nblk,group,kind,ingroup,la,fuse", CASES)
def test_conflicting_launches_are_ordered_across_streams(nblk, group, kind, ingroup, la, fuse):
    lay, steps = plan_of(nblk, group, kind, ingroup, la, fuse)
    ev = [s for s in steps if s["kind"] in (RECORD, WAIT)]
    if not la:
        assert not ev and all(s["stream"] == CALLER for s in steps)
        return
    # forced on: the panel chain and the bulk updates leave the caller's stream
    launches = [i for i, s in enumerate(steps) if s["kind"] <= UPDATE]
    on = {int(steps[i]["stream"]) for i in launches}
    # (a bulk part exists where the first group's trailing matrix has more block columns than the look-ahead takes)
    assert PANEL in on and on <= {PANEL, BULK} and (BULK in on) == (lay.p // NB - min(group, nblk) > group)
    ngroups = -(-nblk // group)
    assert sum(s["kind"] == RECORD and s["event"] == 2 for s in steps) == ngroups  # one `bulk` event, reused per group
    assert sum(s["kind"] == RECORD and s["event"] == 1 for s in steps) == ngroups
    anc = happens_before(steps)
    # the caller's stream before the fork precedes everything, everything precedes the caller's stream after the joins
    assert steps[0]["kind"] == RECORD and steps[0]["stream"] == CALLER and steps[0]["event"] == 0
    assert steps[-1]["kind"] == WAIT and steps[-1]["stream"] == CALLER
    for i in launches:
        assert anc[i] & 1, i
        assert anc[len(steps) - 1] >> i & 1, i
    tw = {i: touches(lay, steps[i]) for i in launches}
    for a, b in itertools.combinations(launches, 2):
        (ra, wa), (rb, wb) = tw[a], tw[b]
        if (wa & rb) or (wb & ra):
            assert anc[b] >> a & 1, (a, b, steps[a], steps[b])  # (a < b in issue order: b must come after a)


def test_four_groups_reuse_the_bulk_and_panel_events():
    """9 blocks in groups of 2: five groups, so the single `bulk` / `panel` events are re-recorded four times, and
    from the second group on the panel stream waits for the previous bulk update before its look-ahead update."""
    lay, steps = plan_of(9, 2, "m0", 1, 1, 0)
    waits_bulk = [i for i, s in enumerate(steps) if s["kind"] == WAIT and s["event"] == 2]
    assert len(waits_bulk) == 4 and all(steps[i]["stream"] == PANEL for i in waits_bulk)
    rec_bulk = [i for i, s in enumerate(steps) if s["kind"] == RECORD and s["event"] == 2]
    assert len(rec_bulk) == 5 and all(steps[i]["stream"] == BULK for i in rec_bulk)
    for w, r in zip(waits_bulk, rec_bulk):  # each wait binds to the previous group's record
        assert r < w and not any(r < x < w for x in rec_bulk)


# --------------------------------------------------------------------------------------------------- replay
def se(a, b, ell=0.7):
    return np.exp(-0.5 * ((a[:, None] - b[None, :]) / ell) ** 2)


_problem_cache = {}


def problem(lay, kind):
    """W of K + I for a random SE kernel (well conditioned) with its extra rows, and numpy's answers"""
    key = (lay.n, lay.m, kind)
    if key in _problem_cache:
        return _problem_cache[key]
    rng = np.random.default_rng(lay.n + 7 * lay.m)
    n, n_pad, y_row, p = lay.n, lay.n_pad, lay.y_row, lay.p
    x = np.sort(rng.uniform(0.0, 40.0, n))
    K = np.eye(n_pad)
    K[:n, :n] = se(x, x) + np.eye(n)
    W = np.zeros((p, p))
    W[:n_pad, :n_pad] = K
    if kind == "eye":
        W[n_pad + np.arange(n), np.arange(n)] = 1.0
    elif lay.m:
        xs = rng.uniform(0.0, 40.0, lay.m)
        W[n_pad:y_row, :n] = se(xs, x)
        W[n_pad:y_row, n_pad:y_row] = se(xs, xs)
    W[y_row, :n] = rng.standard_normal(n)
    L = np.linalg.cholesky(K)
    B = W[n_pad:y_row + 1, :n_pad].copy()           # extra rows and the y row
    BLt = np.linalg.solve(L, B.T).T                  # B L^-T: the test / identity rows and z
    corner = W[n_pad:y_row + 1, n_pad:y_row + 1] - BLt @ BLt.T
    W.setflags(write=False)
    _problem_cache[key] = (W, K, L, BLt, corner)
    return _problem_cache[key]


def replay(lay, steps, W):
    inv = {}
    for s in steps:
        j0 = int(s["j0"])
        if s["kind"] == DIAG:
            A = np.tril(W[j0:j0 + NB, j0:j0 + NB])
            Lk = np.linalg.cholesky(A + np.tril(A, -1).T)
            W[j0:j0 + NB, j0:j0 + NB] = Lk
            inv[j0 // NB] = np.linalg.inv(Lk)
        if is_solve(s):
            rows, T = solve_tiles(s)
            for r0 in rows:
                if not zero_rows(s, r0, r0 + T):
                    W[r0:r0 + T, j0:j0 + NB] = W[r0:r0 + T, j0:j0 + NB] @ inv[j0 // NB].T
        if s["kind"] == UPDATE:
            T, kd = int(s["tile"]), int(s["kdepth"])
            for r0, c0 in update_tiles(s):
                if zero_rows(s, r0, r0 + T) or zero_rows(s, c0, c0 + T):
                    continue
                W[r0:r0 + T, c0:c0 + T] -= W[r0:r0 + T, j0:j0 + kd] @ W[c0:c0 + T, j0:j0 + kd].T
    return W


@pytest.mark.parametrize("nblk,group,kind,ingroup,la,fuse", CASES)
def test_replay_reproduces_the_factor_the_solves_and_the_schur_corner(nblk, group, kind, ingroup, la, fuse):
    lay, steps = plan_of(nblk, group, kind, ingroup, la, fuse)
    W0, K, L, BLt, corner = problem(lay, kind)
    W = replay(lay, steps, W0.copy())
    n, n_pad, y_row = lay.n, lay.n_pad, lay.y_row
    tol = 8 * n_pad * EPS * np.abs(K).max()  # the factor bound, normwise
    assert np.abs(np.tril(W[:n_pad, :n_pad]) - L).max() <= tol
    assert np.abs(W[n_pad:y_row + 1, :n_pad] - BLt).max() <= tol          # test / identity rows, and z in the y row
    got = np.tril(W[n_pad:y_row + 1, n_pad:y_row + 1])
    assert np.abs(got - np.tril(corner)).max() <= tol                      # Schur corner (with -z z^T in the y row)
    if kind == "eye":
        Kinv = np.linalg.inv(K[:n, :n])
        assert np.abs(np.tril(W[n_pad:n_pad + n, n_pad:n_pad + n]) + np.tril(Kinv)).max() <= tol


# ----------------------------------------------------------------------------------------------- accounting
@pytest.mark.parametrize("nblk,group,kind,ingroup,la,fuse",
                         [c for c in CASES if c[2] != "eye"])
def test_flops_per_class_sum_to_the_closed_forms(nblk, group, kind, ingroup, la, fuse):
    """Plain layouts.  Diagonal blocks: NB^3 / 3 each.  Panel solve of block k: NB^2 per row that is nonzero in the
    panel, the n_pad - (k + 1) NB rows of K below the block and the m test rows (counted in the diagonal class where
    the solve is fused).  Updates: 2 NB per (lower element, panel) pair -- column a of the n_pad + m rows of K and the
    test rows holds n_pad + m - a lower elements (its own included) and receives the min(a // NB, nblk) panels left
    of its block.  The y row and the padding below it are not counted.  Exact in integers; the plan sums doubles."""
    batch = 3
    lay, steps = plan_of(nblk, group, kind, ingroup, la, fuse, batch=batch)
    n_pad, m = lay.n_pad, lay.m
    by_cls = {c: sum(float(s["flops"]) for s in steps if s["cls"] == c) for c in (1, 2, 3)}
    solve = [NB * NB * (n_pad - (k + 1) * NB + m) for k in range(nblk)]
    fused = {int(s["kblk"]) for s in steps if s["kind"] == DIAG and s["trsm_tiles"] > 0}
    want_diag = batch * (nblk * NB ** 3 / 3.0 + sum(f for k, f in enumerate(solve) if k in fused))
    want_trsm = batch * sum(f for k, f in enumerate(solve) if k not in fused)
    want_upd = batch * 2 * NB * sum((n_pad + m - a) * min(a // NB, nblk) for a in range(n_pad + m))
    assert by_cls[1] == pytest.approx(want_diag, rel=1e-12)
    assert by_cls[2] == pytest.approx(want_trsm, rel=1e-12, abs=0)
    assert by_cls[3] == pytest.approx(want_upd, rel=1e-12)
    if m == 0:  # N^3 / 3 over padded blocks: NB^3 (nblk / 3 + nblk (nblk - 1) / 2 + sum_c c (2 (nblk - c) - 1 + 1 / NB))
        total = NB ** 3 * (nblk / 3.0 + nblk * (nblk - 1) / 2.0 +
                           sum(c * (2 * (nblk - c) - 1 + 1.0 / NB) for c in range(nblk)))
        assert sum(by_cls.values()) == pytest.approx(batch * total, rel=1e-12)
    assert all(s["bytes"] == 0 for s in steps if s["cls"] in (1, 2))
    es = 8
    for s in steps:
        if s["kind"] == UPDATE and s["role"] == 5:  # a whole trailing update: its lower triangle read + written once
            rows = lay.p - int(s["row0"])
            assert s["bytes"] == batch * es * (2.0 * (rows * (rows + 1) / 2.0) + rows * float(s["kdepth"]))


# ------------------------------------------------------------------------------------------- gpk_nlml's limit
@pytest.mark.parametrize("nblk", BLOCKS)
@pytest.mark.parametrize("group,first", [(2, 1), (2, 8), (4, 2), (8, 8), (8, 3)])
@pytest.mark.parametrize("la", [0, 1])
def test_first_group_is_what_the_fused_k_build_finds_assembled(nblk, group, first, la):
    lay = layout(nblk, "m0")
    with nat.thread_tune(group=group, group_first=first, lookahead=la):
        steps, g0 = nat.launch_plan(lay, counters=True, kbuild=True, first_group=True)
        plain = nat.launch_plan(lay, counters=True, kbuild=False)
    assert g0 == min(first, group, nblk)
    kb = np.flatnonzero(steps["kbuild"])
    # (look-ahead on: both parts of the first trailing update, if its nblk - g0 + 1 block columns exceed the look-ahead's)
    assert len(kb) == (2 if la and nblk - g0 + 1 > group else 1)
    assert np.count_nonzero(steps["kind"][:kb[0]] == DIAG) == g0
    assert all(steps[i]["kind"] == UPDATE and steps[i]["j0"] == 0 and steps[i]["kdepth"] == g0 * NB for i in kb)
    # nothing else moves: the same steps as the unfused factorisation
    assert len(steps) == len(plain) and not plain["kbuild"].any()
    assert all(np.array_equal(steps[f], plain[f]) for f in steps.dtype.names if f != "kbuild")


def test_rejects_bad_arguments():
    import ctypes
    L = nat.load_library()
    lay = layout(3, "m77")
    ns = ctypes.c_int64(0)
    assert L.gpk_launch_plan(None, 0, 1, 0, None, 0, ctypes.byref(ns), None) == -1
    assert L.gpk_launch_plan(ctypes.byref(lay), 2, 1, 0, None, 0, ctypes.byref(ns), None) == -2
    assert L.gpk_launch_plan(ctypes.byref(lay), 1, 1, 0, None, 0, ctypes.byref(ns), None) == -1   # eye needs m = n
    assert L.gpk_launch_plan(ctypes.byref(lay), 0, 1, 0, None, 0, None, None) == -7
    assert L.gpk_launch_plan(ctypes.byref(lay), 0, 1, 0, None, 0, ctypes.byref(ns), None) == 0 and ns.value > 0
    buf = (ctypes.c_int64 * nat.LAUNCH_STEP_WORDS)()
    assert L.gpk_launch_plan(ctypes.byref(lay), 0, 1, 0, buf, 1, ctypes.byref(ns), None) == -6   # cap below the count
