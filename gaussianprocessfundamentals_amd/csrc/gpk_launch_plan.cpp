// The launch path's schedule (gpk_launch_plan.h): decisions, band compression and the per-launch accounting.
// Host arithmetic only -- plain C++17, no HIP header -- so it builds and runs without the HIP toolchain
// (tests/native/launch_plan_main.cpp).
#include "gpk_launch_plan.h"

#include <algorithm>

#include "gpk_const.h"

namespace gpk {

// The panel chain (diag, panel solve, thin and look-ahead updates) runs on a high-priority
// stream, the bulk of each trailing update on a CU-masked stream concurrently with the next
// panel pair's chain; both fork from and join back into the caller's stream.
// GPK_LOOKAHEAD=0 puts everything on the caller's stream.
// Auto (2): on when the augmented matrix has at least la_min_blocks 128-blocks.  Below that the
// whole factorisation is faster on the caller's stream alone: each launch on the side streams costs
// ~5 us more than back to back on one queue, more than the overlap of the short trailing updates
// saves.  ms per call, look-ahead off / on (profiles/r02s_lookahead.txt): one member N = 1024
// 0.45 / 0.55, 2048 0.92 / 1.09, 4096 2.10 / 2.29, 6144 3.98 / 4.03, 8192 6.53 / 6.40, 12288
// 15.3 / 14.5; batches of 8 at N = 4096 5.13 / 5.26; the 128-candidate C4 sweep 52.7 / 54.2;
// -LML + gradient (identity rows: twice the width) N = 4096 3.44 / 3.28.  With the panel solve fused
// (look-ahead off only): N = 6144 3.89 / 4.02, 7168 5.01 / 5.05, 8192 6.43 / 6.39 -> 64 blocks.
bool launch_lookahead(const Tune& tn, int64_t p) {
  return tn.lookahead == 1 || (tn.lookahead == 2 && p / NB >= tn.la_min_blocks);
}

namespace {

// Groups of G 128-column panels per trailing update (K = 128 G): inside the group, block column k
// is brought up to date with the group's earlier panels (one left-looking update of depth
// 128 (k - g0)) and then factored and solved, ..., then update the trailing
// matrix with all G panels at once -- its first G block columns (look-ahead, on the panel
// stream: the next group's panels) and the rest (bulk stream, overlapping the next group's
// panel chain).  A deeper K halves the read-modify-write passes over the trailing matrix per
// doubling of G.  The first group has G0 <= G panels: its chain is exposed (nothing to overlap
// yet), so a short one lets the first bulk update start early.
// identity-augmented (gradient / inverse) factorisations: groups of group_eye panels -- their
// trailing matrix carries the K^-1 corner, and 4-panel groups measured faster there at every batch
int64_t group_size(const Tune& tn, bool eye) {
  return std::max<int64_t>(1, std::min<int64_t>(eye ? tn.group_eye : tn.group, 16));
}

// identity extra rows: the tiles wholly inside the zero band [zlo, zhi) are left out of the grid
// (launched and exiting at once they would also crowd the live tiles onto a few XCDs, since
// xcd_remap hands each XCD a contiguous run of tile ids).  Tiles [bz0, bz0 + bzn), in units of `tile` rows from row0.
struct Band {
  int64_t bz0 = 0, bzn = 0;
  // c: a tile index from row0 -> its index in the compressed enumeration
  int64_t compress(int64_t c) const { return bzn == 0 || c < bz0 ? c : (c >= bz0 + bzn ? c - bzn : bz0); }
};

struct Planner {
  const LaunchShape& sh;
  const bool eye, counters, kbuild;
  const Tune& tn;
  const bool la;
  std::vector<LaunchStep>& out;

  LaunchStep step(int kind, int stream, int cls) const {
    LaunchStep s{};
    s.kind = kind;
    s.stream = stream;
    s.event = -1;
    s.cls = cls;
    return s;
  }

  void event(int kind, int ev, int stream) {
    LaunchStep s = step(kind, stream, -1);
    s.event = ev;
    out.push_back(s);
  }

  // extra rows that are nonzero in panel columns left of c: all test rows, or the identity rows
  // t < c (row n_pad + t of E L^-T is zero left of column t)
  double extra_nonzero(int64_t c) const { return (double)(eye ? std::min<int64_t>(sh.m, c) : sh.m); }

  Band band_of(const LaunchStep& s, int tile) const {
    Band b;
    if (!eye || !tn.band_skip) return b;
    const int64_t b0 = (s.zlo - s.row0) / tile, b1 = (s.zhi - s.row0) / tile;
    if (b1 > b0) {
      b.bz0 = b0;
      b.bzn = b1 - b0;
    }
    return b;
  }

  // Small grids (f64): the panel solve of block k runs inside the diagonal-block launch -- one
  // workgroup per 64-row tile (plus the one that writes L and L^-1), each factoring the block
  // redundantly (the chip is otherwise idle there) and solving its rows against L^-1 in LDS, bitwise
  // the separate gemm<TRSM>; one launch fewer on the chain per panel.
  int64_t fused_tiles(int64_t k) const {
    const int64_t rows = sh.p - (k + 1) * NB;
    if (!counters) return 0;  // no counters for this stream: the separate panel-solve launch
    // (the timing-only ablations of the diagonal kernel skip the writer's counter reset: never fused)
    if (sh.f32 || !tn.fuse_trsm || tn.diag_version == 1 || tn.diag_dbg != 0 || rows <= 0) return 0;
    if (la && tn.fuse_trsm != 2) return 0;  // beside the look-ahead's bulk updates the extra workgroups
                                             // cost more than the launch saves (N = 8192: 6.39 -> 6.43 ms)
    const int64_t t64 = rows / 64;
    return (t64 + 1) * sh.batch <= tn.fuse_trsm_max && sh.batch <= kFuseCtr ? t64 : 0;
  }

  // diagonal block k: factor + invert
  void diag(int64_t k, int stream) {
    LaunchStep s = step(LP_DIAG, stream, 1);
    s.kblk = k;
    s.j0 = k * NB;
    s.trsm_tiles = fused_tiles(k);
    s.flops = (double)sh.batch * NB * NB * NB / 3.0;
    if (s.trsm_tiles > 0) {
      s.row0 = (k + 1) * NB;
      s.zlo = eye ? sh.n_pad + s.row0 : 0;  // identity rows t >= j0 + nb are still zero
      s.zhi = eye ? sh.y_row : 0;
      s.flops += (double)sh.batch * ((double)(sh.n_pad - s.row0) + extra_nonzero(s.row0)) * NB * NB;
    }
    out.push_back(s);
  }

  // the right operand of block column k's folded panel solve, from L_kk^-1 and block row k's columns [h0 NB, k NB):
  // a triangular 128 x 128 times a 128 x 128 d product per member (its own flops, in the diagonal class)
  void prep(int64_t k, int64_t h0, int stream) {
    LaunchStep s = step(LP_PREP, stream, 1);
    s.kblk = k;
    s.j0 = h0 * NB;
    s.row0 = k * NB;
    s.kdepth = (k - h0) * NB;
    s.flops = (double)sh.batch * NB * (NB + 1) * (double)s.kdepth;
    out.push_back(s);
  }

  // panel solve of block k: every row below the block (the y / test rows included).  fold_depth > 0: the launch also
  // applies the in-group update of the rows below the diagonal tile with the fold_depth columns left of the block
  // (fold_flops: that update's algorithmic flops)
  void trsm(int64_t k, int stream, int64_t fold_depth = 0, double fold_flops = 0.0) {
    if (fused_tiles(k) > 0) return;  // solved by the diagonal-block launch
    LaunchStep s = step(LP_TRSM, stream, 2);
    s.j0 = k * NB;
    s.row0 = s.j0 + NB;
    const int64_t rows = sh.p - s.row0;
    if (rows <= 0) return;
    s.kdepth = NB + fold_depth;
    s.row_end = tn.skip_zero_rows ? sh.y_row + 1 : 0;  // rows below the y row are zero
    if (eye) {  // identity rows t >= j0 + nb are still zero in this panel
      s.zlo = sh.n_pad + s.j0 + NB;
      s.zhi = sh.y_row;
    }
    s.tile = (band_of(s, 128).compress(rows / NB) * sh.batch >= tn.trsm_t128_min) ? 128 : 64;
    const Band b = band_of(s, (int)s.tile);
    s.bz0 = b.bz0;
    s.bzn = b.bzn;
    s.nt = b.compress(rows / s.tile);
    // algorithmic: rows that are nonzero in the panel (K part + extra rows) x nb^2
    const double rK = (double)(sh.n_pad - s.row0) + extra_nonzero(s.j0 + NB);
    s.flops = (double)sh.batch * rK * NB * NB + fold_flops;
    out.push_back(s);
  }

  // trailing update from panel columns [j0, j0 + kdepth) of the lower tiles whose 128-column
  // block lies in [c_lo, c_hi) (relative to row0 = j0 + kdepth; c_hi < 0: to the end).  cap128 > 0: only the first
  // cap128 block rows from row0 (the folded schedule's diagonal tile; plain layouts); returns the algorithmic flops of
  // the rows the cap leaves out
  double update(int64_t j0, int64_t kdepth, int64_t c_lo, int64_t c_hi, int stream, int role, bool fused_k = false,
                int64_t cap128 = 0) {
    LaunchStep s = step(LP_UPDATE, stream, 3);
    s.role = role;
    s.kbuild = fused_k && kbuild;  // first trailing update: C is evaluated, not loaded (gpk_nlml's fused K build)
    s.j0 = j0;
    s.row0 = j0 + kdepth;
    s.kdepth = kdepth;
    s.row_end = tn.skip_zero_rows ? sh.y_row + 1 : 0;
    const int64_t rows_all = sh.p - s.row0;
    if (rows_all <= 0) return 0.0;
    const int64_t rows = cap128 > 0 ? std::min(rows_all, cap128 * NB) : rows_all;
    const int64_t t128 = rows / NB;
    if (c_hi < 0 || c_hi > t128) c_hi = t128;
    if (c_lo >= c_hi) return 0.0;
    if (eye) {  // identity rows t >= j0 + kdepth are zero in the panel columns
      s.zlo = sh.n_pad + j0 + kdepth;
      s.zhi = sh.y_row;
    }
    const Band b128 = band_of(s, 128);
    const int64_t w128 = b128.compress(c_hi) - b128.compress(c_lo);
    if (w128 <= 0) return 0.0;
    const int64_t tiles128 = w128 * (w128 + 1) / 2 + (b128.compress(t128) - b128.compress(c_hi)) * w128;
    s.tile = (tiles128 * sh.batch >= tn.upd_t128_min) ? 128 : 64;
    const int64_t scale = NB / s.tile;
    const Band b = band_of(s, (int)s.tile);
    s.bz0 = b.bz0;
    s.bzn = b.bzn;
    s.nt = b.compress(rows / s.tile);
    s.c_lo = b.compress(c_lo * scale);
    s.c_hi = b.compress(c_hi * scale);
    s.band = std::max<int64_t>(0, tn.upd_band);
    // algorithmic flops: 2 kdepth x (lower-triangle elements in the column range of the rows that
    // are nonzero in the panel: the K part, then the extra rows, which follow it contiguously)
    const double rK_all = (double)(sh.n_pad - s.row0) + extra_nonzero(j0 + kdepth);
    const double rK = std::min(rK_all, (double)rows);
    const double cl = std::min(rK, (double)(c_lo * NB)), ch = std::min(rK, (double)(c_hi * NB));
    const double elems = (ch - cl) * rK - (cl + ch - 1.0) * (ch - cl) / 2.0;
    const double elems_left_out = (ch - cl) * (rK_all - rK);  // (whole rows below the cap: cl, ch <= rK)
    // algorithmic bytes: the updated tiles' elements read + written once (y / test rows too)
    // and the panel rows read once
    const double es = sh.f32 ? 4.0 : 8.0;
    const double rA = (double)rows;
    const double ca = (double)(c_lo * NB), cb = (double)(c_hi * NB);
    const double elems_all = (cb - ca) * rA - (ca + cb - 1.0) * (cb - ca) / 2.0;
    s.flops = (double)sh.batch * 2.0 * kdepth * std::max(0.0, elems);
    s.bytes = (double)sh.batch * es * (2.0 * elems_all + rA * kdepth);
    out.push_back(s);
    return (double)sh.batch * 2.0 * kdepth * std::max(0.0, elems_left_out);
  }

  void run() {
    const int64_t nblk = sh.n_pad / NB;
    const int64_t G = group_size(tn, eye);
    const int sp = la ? LP_PANEL : LP_CALLER, sb = la ? LP_BULK : LP_CALLER;
    if (la) {
      event(LP_RECORD, LP_EV_FORK, LP_CALLER);
      event(LP_WAIT, LP_EV_FORK, sp);
      event(LP_WAIT, LP_EV_FORK, sb);
    }
    // In-group updates.  Left-looking (throughput): block column k receives the group's earlier
    // panels in ONE update of depth 128 (k - g0) right before its diagonal block is factored
    // (right-looking updates read and write the group's columns once per panel).  Right-looking
    // (latency, small batches whose thin launches cannot fill the chip): after panel k, the group's
    // remaining columns receive panel k at depth 128 -- the chain to diag(k + 1) then carries one
    // short update instead of one of depth up to 128 (G - 1).
    // Two-level left-looking (ingroup 3): the group is split in halves; each half is left-looking
    // within itself, and between the halves ONE update of the second half's columns with the first
    // half's panels (depth 128 G/2) -- the thin launches re-read the half's panels instead of the
    // group's, 36 instead of 42 panel-column reads + writes per group of 8 (they are HBM-bound).
    const int64_t rows128 = sh.p / NB;
    const bool right_looking = tn.ingroup == 2 || (tn.ingroup == 0 && sh.batch * rows128 < tn.rl_max_tiles);
    const bool two_level = !right_looking && (tn.ingroup == 3 || tn.ingroup == 4 || tn.ingroup == 0) && G >= 4;
    // Folded columns (ingroup 4; f64 uniform plain batches): a column k of the two-level scheme with d = k - h0 > 0
    // earlier panels in its half is not updated and then solved -- two launches that each stream the block column
    // through HBM -- but solved against a deeper operand: with A the row tile's d earlier panels, B block row k's and C
    // the row tile's part of column k,  (C - A B^T) L^-T = [A | C] [-L^-1 B | L^-1]^T.  Only the diagonal tile takes the
    // thin update (diag(k) needs it); PREP forms the right operand once per member; the solve then runs at K = 128 (d +
    // 1) over columns that lie contiguously in W.  d + 2 instead of d + 4 passes over the column, one launch of
    // 64-row-tile grids less on the chain.  Same operations in another association: results agree with modes 1-3 to
    // summation order, not bitwise.  Columns whose solve runs inside the diagonal launch keep mode 3's steps.
    const bool fold = two_level && (tn.ingroup == 4 || tn.ingroup == 0) && !sh.f32 && !sh.ragged && !sh.no_fold && !eye;
    bool bulk_pending = false;
    for (int64_t g0 = 0, gsize = launch_first_group(tn, eye, sh.n_pad); g0 < nblk; g0 += gsize, gsize = G) {
      const int64_t gend = std::min(g0 + gsize, nblk);
      const int64_t gmid = two_level ? std::min(g0 + (gend - g0 + 1) / 2, gend) : gend;
      for (int64_t k = g0; k < gend; ++k) {
        const int64_t h0 = k < gmid ? g0 : gmid;  // first panel of k's half
        if (two_level && k == gmid && gmid > g0) update(g0 * NB, (gmid - g0) * NB, 0, gend - gmid, sp, LP_ROLE_HALF);
        if (fold && k > h0 && fused_tiles(k) == 0) {
          const double rest = update(h0 * NB, (k - h0) * NB, 0, 1, sp, LP_ROLE_THIN, false, 1);
          diag(k, sp);
          prep(k, h0, sp);
          trsm(k, sp, (k - h0) * NB, rest);
          continue;
        }
        if (!right_looking && k > h0) update(h0 * NB, (k - h0) * NB, 0, 1, sp, LP_ROLE_THIN);
        diag(k, sp);
        trsm(k, sp);
        if (right_looking && k + 1 < gend) update(k * NB, NB, 0, gend - k - 1, sp, LP_ROLE_THIN);
      }
      const int64_t kd = (gend - g0) * NB;
      if (!la) {
        update(g0 * NB, kd, 0, -1, LP_CALLER, LP_ROLE_GROUP, g0 == 0);
        continue;
      }
      event(LP_RECORD, LP_EV_PANEL, sp);  // panels g0 .. gend-1 solved
      if (bulk_pending) event(LP_WAIT, LP_EV_BULK, sp);
      update(g0 * NB, kd, 0, G, sp, LP_ROLE_LOOKAHEAD, g0 == 0);
      event(LP_WAIT, LP_EV_PANEL, sb);
      update(g0 * NB, kd, G, -1, sb, LP_ROLE_BULK, g0 == 0);
      event(LP_RECORD, LP_EV_BULK, sb);
      bulk_pending = true;
    }
    if (la) {
      event(LP_RECORD, LP_EV_JOIN_P, sp);
      event(LP_RECORD, LP_EV_JOIN_B, sb);
      event(LP_WAIT, LP_EV_JOIN_P, LP_CALLER);
      event(LP_WAIT, LP_EV_JOIN_B, LP_CALLER);
    }
  }
};

}  // namespace

int64_t launch_first_group(const Tune& tn, bool eye, int64_t n_pad) {
  const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(tn.group_first, group_size(tn, eye)));
  return std::min<int64_t>(G0, n_pad / NB);
}

// (sized for the deepest operand any plan of this batch and group size can hold -- a half of ceil(G / 2) panels -- not
// for this plan's own deepest, so that a stream's block does not grow from one shape to the next)
int64_t launch_fold_bytes(const LaunchShape& sh, bool eye, const Tune& tn, const std::vector<LaunchStep>& steps) {
  for (const LaunchStep& s : steps)
    if (s.kind == LP_PREP) return sh.batch * NB * NB * ((group_size(tn, eye) + 1) / 2) * (int64_t)sizeof(double);
  return 0;
}

void launch_plan(const LaunchShape& sh, bool eye, bool counters, bool kbuild, const Tune& tn,
                 std::vector<LaunchStep>& out) {
  out.clear();
  Planner{sh, eye, counters, kbuild, tn, launch_lookahead(tn, sh.p), out}.run();
}

}  // namespace gpk
