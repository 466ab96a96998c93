// The planner of the persistent factorisation: the order in which chain_kernel's workgroups claim their tasks.
// Host arithmetic only -- plain C++17, no HIP header -- so it builds and runs without the HIP toolchain
// (tests/native/chain_plan_main.cpp).
#include "gpk_chain_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <functional>
#include <queue>
#include <utility>

#include "gpk_const.h"

namespace gpk {

namespace {

// panels per deferred tile update: the knob, or (0) 4 below 80 diagonal blocks and 8 from there -- the deep
// updates' MFMA rate starts to matter more than the columns they hold back (N = 8192 4.46 / 4.49 ms with 4 / 8,
// 10240 7.74 / 7.62, 12288 12.56 / 12.17, profiles/r04af_chain_group_large.jsonl)
int chain_group_for(int64_t knob, int64_t n_pad, bool f32) {
  if (knob > 0) return (int)knob;
  // (f32: 8 -- C3 at 8 persistent launches in flight 426 / 436 / 427 / 417 evals/s at 4 / 8 / 12 / 16,
  // profiles/r06j_c3_f32_chain_sweep.txt)
  return n_pad / NB >= 80 || f32 ? 8 : 4;
}

// list-scheduling durations (us) of D / S / U32 / BLK: the measured per-task run times (round 4, profiles/r04y_*;
// UQ: half of U32); GPK_CHAIN_DUR="d,s,u,b" overrides them (A/B), read once per process
const float* chain_durations() {
  static const std::array<float, 4> dur = [] {
    std::array<float, 4> d = {28.f, 6.5f, 12.f, 22.5f};
    if (const char* e = getenv("GPK_CHAIN_DUR")) sscanf(e, "%f,%f,%f,%f", &d[0], &d[1], &d[2], &d[3]);
    return d;
  }();
  return dur.data();
}

}  // namespace

ChainKnobs chain_knobs(const Tune& tn, int64_t n_pad, bool eye, bool f32, int grid) {
  ChainKnobs k;
  const int64_t gk = eye && tn.chain_group_eye > 0 ? tn.chain_group_eye : tn.chain_group;
  k.group = std::max(1, std::min(chain_group_for(gk, n_pad, f32), 16));
  // (f32: one U32 task per slice -- chain_kernel<float> has no quarter-task bodies)
  k.uq = f32 ? 0 : (int)std::max<int64_t>(0, std::min<int64_t>(2, tn.chain_uq));
  k.group_corner = (int)std::max<int64_t>(1, std::min<int64_t>(tn.chain_group_corner, 16));
  k.corner_tail = (int)std::max<int64_t>(0, tn.chain_corner_tail);
  k.group_la = (int)std::max<int64_t>(1, tn.chain_group_la);
  k.group_near = (int)std::max<int64_t>(1, std::min<int64_t>(tn.chain_group_near, k.group));
  k.near_la = (int)std::max<int64_t>(1, tn.chain_near_la);
  // (auto: slice updates only for short chains on a full grid -- single N = 4096 on 256 workgroups 1.577 vs 1.595 ms;
  // C2's 64-workgroup launches 1726 -> 1863 evals/s, N = 8192 4.50 -> 4.31 ms, C3 f32 persistent 442 -> 470,
  // profiles/r06r_chain_u128_ab.txt)
  k.u128 = tn.chain_u128 == 1 || (tn.chain_u128 == 2 && (n_pad / NB >= 48 || grid <= 2 * (n_pad / NB))) ? 1 : 0;
  // (auto: the CU-share launches only -- C3 on 8 f32 launches of 64 workgroups 476 -> 495 evals/s, C2 neutral, while a
  // single N = 8192 on 256 workgroups lost 2 %: 4.27 -> 4.37 ms, profiles/r06x_chain_s128_ab.txt)
  // and the long identity-augmented plans (value + gradient N = 8192 10.43-10.48 -> 10.32-10.35 ms)
  k.s128 = tn.chain_s128 == 1 ||
                   (tn.chain_s128 == 2 && ((grid > 0 && grid <= 2 * (n_pad / NB)) || (eye && n_pad / NB >= 64)))
               ? 1 : 0;
  return k;
}

// chain_xcd: the diagonal chain's tasks -- D, the panel solves of the next diagonal block's slices (S / SQ), its
// quarter updates (UQ) or, without quarters, its per-slice updates (U32 of block column k + 1 on its own rows) --
// move to list B, in their order; the rest stays list A.  Both lists keep the topological order.  Returns nb.
int32_t chain_split_lists(std::vector<int32_t>& ord) {
  std::vector<int32_t> la, lb;
  la.reserve(ord.size());
  for (size_t t = 0; t + 3 < ord.size(); t += 4) {
    const int tyg = ord[t], ty = tyg & kChainTypeMask, g = ((tyg >> kChainGShift) & kChainGMask) + 1,
              k = ord[t + 1], r = ord[t + 2], j = ord[t + 3];
    const bool chain = ty == CH_D || (ty == CH_S && (r >> 2) == k + 1) ||
                       (ty == CH_U32 && (g > 1 || (j == k + 1 && (r >> 2) == k + 1)));
    std::vector<int32_t>& dst = chain ? lb : la;
    dst.insert(dst.end(), ord.begin() + t, ord.begin() + t + 4);
  }
  const int32_t nb = (int32_t)(lb.size() / 4);
  ord.assign(la.begin(), la.end());
  ord.insert(ord.end(), lb.begin(), lb.end());
  return nb;
}

// eye: identity extra rows (m = n, gpk_potrf_aug_ex GPK_AUG_EXTRA_IDENTITY).  Extra row t (row n_pad + t) of
// E L^-T is zero left of column t, so block i >= nblk (extra block e = i - nblk) is zero in every panel q < e
// (its rows' panel columns are zero until panel e, where its identity entries are solved): the list leaves out
// every task that would only move zeros -- the panel solves of such slices and the tile updates where either
// block is still zero -- so the factorisation does n^3 flops (potrf + trtri + lauum) like the launch path's
// band skip.  The block holding the y row is live in every panel.
// Returns the task words (four per task); empty if the graph exceeds a bound of the device tasks (the caller
// reports that as an error -- never reached for graphs built here, whose in-degrees are bounded by construction).
std::vector<int32_t> chain_order(int64_t n_pad, int64_t y_row, int grid, int nmem, const ChainKnobs& kn,
                                 bool eye) {
  const int group = kn.group, chain_uq = kn.uq;
  const int nblk = (int)(n_pad / NB), yb = (int)(y_row / NB), rlast = (int)(y_row / 32);
  // block i holds a nonzero row in the columns of panel q (monotone in q): from panel live_from(i) on
  auto live_from = [&](int i) { return (!eye || i < nblk || i == yb) ? 0 : i - nblk; };
  auto live = [&](int i, int q) { return live_from(i) <= q; };
  // (flat storage: the lists reach 70 000+ tasks for the identity-augmented N = 8192 -- a vector per task's
  // dependencies and a map per tile made the first call of a shape cost ~30 ms of host time there)
  constexpr int MAXDEP = 16;  // D: up to 10 quarter tasks; BLK: 4 + 4 slices + the tile's last update
  struct Task {
    int ty, k, r, j;
    float dur;
    int nd;
    int deps[MAXDEP];
    void dep(int d) {
      if (nd < MAXDEP) deps[nd] = d;
      ++nd;
    }
  };
  std::vector<Task> T;
  T.reserve(4096);
  const int nr = rlast + 1;
  std::vector<int> D(nblk, -1), S((size_t)nblk * nr, -1), U((size_t)nblk * nr, -1);
  const int nbt = yb + 1;
  std::vector<int> last_upd((size_t)nbt * nbt, -1);  // tile (i, j) -> its latest update task so far
  auto mk = [](int ty, int k, int r, int j, float du) {
    Task t;
    t.ty = ty;
    t.k = k;
    t.r = r;
    t.j = j;
    t.dur = du;
    t.nd = 0;
    return t;
  };
  auto s_of = [&](int k, int r) { return S[(size_t)k * nr + r]; };
  auto u_of = [&](int k, int r) { return U[(size_t)k * nr + r]; };
  // list-scheduling durations (chain_durations); a tile update over g panels is estimated at b (0.25 + 0.75 g):
  // the C read / write and the pipeline fill are paid once per task
  const float* dur = chain_durations();
  // Deferred tile updates: the panels of group [q0, q1) (G panels) are applied to a tile of block column j
  // by ONE task of depth 128 (q1 - q0) when j >= q1 + L -- the column is not needed until L steps after
  // the group's last panel solve; the columns nearer the diagonal take each panel on its own (depth 128),
  // so the diagonal chain never waits for a deep update.  G = 1 disables it.
  const int G = group, Gc = kn.group_corner, tail_c = kn.corner_tail, LA = kn.group_la, Gn = kn.group_near;
  bool overflow = false;  // a task with more than MAXDEP dependencies (unreachable: bounded by construction)
  auto add = [&](const Task& t) {
    if (t.nd > MAXDEP) overflow = true;
    T.push_back(t);
    return (int)T.size() - 1;
  };
  // BLK tasks carry ty = 3 | (g - 1) << 2 for an update over the g panels k .. k + g - 1
  auto blk = [&](int q0, int g, int i, int jj) {
    const int ql = q0 + g - 1;  // (S(ql, r) done implies S(q, r) done for every q < ql that has an S task)
    if (!live(i, ql) || !live(jj, ql)) return;  // (identity rows: zero in every panel of the group)
    // (identity rows: the group's leading panels in which either block is still zero are left out -- their
    // products are exact zeros, so the tile's bits are those of the launch path, which includes or skips them)
    const int f = std::max(live_from(i), live_from(jj));
    if (f > q0) {
      g -= f - q0;
      q0 = f;
    }
    Task t = mk(CH_BLK | ((g - 1) << kChainGShift), q0, i, jj, dur[3] * (0.25f + 0.75f * (float)g));
    for (int s = 4 * i; s <= std::min(4 * i + 3, rlast); ++s) t.dep(s_of(ql, s));
    if (jj != i)
      for (int s = 4 * jj; s <= std::min(4 * jj + 3, rlast); ++s) t.dep(s_of(ql, s));
    int& lu = last_upd[(size_t)i * nbt + jj];
    if (lu >= 0)
      t.dep(lu);
    else if (q0 > 0)
      t.ty |= kChainFirst;
    lu = add(t);
  };
  // the next diagonal block's update by panel k, split by 32-column quarter (UQ: U32 with the quarter + 1 in
  // the type word's bits 2..7): 10 tasks of 32 x 32 x 128 on the chain to D(k + 1) instead of 4 of 32 x 128 x
  // 128, each loading 64 KB of panel instead of 160 (chain_uq; 0: one U32 per slice)
  const bool uq = chain_uq != 0, sq = chain_uq == 2;
  std::vector<std::vector<int>> uq_of(nr);  // slice s of diagonal block k + 1 -> its UQ tasks (panel k)
  for (int k = 0; k < nblk; ++k) {
    Task d = mk(CH_D, k, 0, k, dur[0]);
    if (k > 0)
      for (int s = 4 * k; s <= std::min(4 * k + 3, rlast); ++s) {
        if (uq)
          for (int t : uq_of[s]) d.dep(t);
        else
          d.dep(u_of(k - 1, s));
      }
    D[k] = add(d);
    for (int r = 4 * (k + 1); r <= rlast; ++r) {
      if (!live(r / 4, k)) continue;
      if (kn.s128 && r >= 4 * (k + 2)) {
        // chain_s128: below the next diagonal block, a block row's slices take ONE panel-solve task (S with g = the
        // slice count in the type word's bits 2..5: the slices solved one after another, each as its own S task would)
        if (r % 4 != 0) continue;
        const int g = std::min(4, rlast - r + 1);
        Task t = mk(CH_S | ((g - 1) << kChainGShift), k, r, 0, dur[1] * (0.5f + 0.5f * (float)g));
        t.dep(D[k]);
        if (k > 0 && live(r / 4, k - 1)) {
          for (int s2 = r; s2 < r + g; ++s2) {
            const int u = u_of(k - 1, s2);
            bool dup = false;
            for (int e = 0; e < t.nd && e < MAXDEP; ++e) dup = dup || t.deps[e] == u;
            if (!dup) t.dep(u);
          }
        } else if (k > 0) {
          t.ty |= kChainFirst;
        }
        const int id = add(t);
        for (int s2 = r; s2 < r + g; ++s2) S[(size_t)k * nr + s2] = id;
        continue;
      }
      // chain_uq 2: the next diagonal block's slices take SQ tasks -- the panel solve followed by the slice's lower
      // quarters of that block (chain_sq), which need the siblings' solved rows (claimed before: lower slices first)
      const bool sqt = sq && k + 1 < nblk && r < 4 * (k + 2);
      Task t = mk(CH_S | (sqt ? kChainSq : 0), k, r, 0, dur[1] + (sqt ? dur[2] * 0.5f : 0.f));
      t.dep(D[k]);
      if (k > 0 && live(r / 4, k - 1))
        t.dep(u_of(k - 1, r));
      else if (k > 0)
        t.ty |= kChainFirst;  // (the slice's first live panel: nothing updated it before)
      if (sqt) {
        const int lu = last_upd[(size_t)(k + 1) * nbt + (k + 1)];
        if (lu >= 0) t.dep(lu);
        for (int q = 4 * (k + 1); q < r; ++q) t.dep(s_of(k, q));
      }
      S[(size_t)k * nr + r] = add(t);
      if (sqt) {
        uq_of[r].push_back(S[(size_t)k * nr + r]);
        U[(size_t)k * nr + r] = S[(size_t)k * nr + r];
      }
    }
    for (int r = 4 * (k + 1); r <= rlast; ++r) {
      if (!live(r / 4, k)) continue;
      if (sq && k + 1 < nblk && r < 4 * (k + 2)) continue;  // (done by the slice's SQ task)
      const int lu = last_upd[(size_t)(r / 4) * nbt + (k + 1)];
      const int first = (lu < 0 && k > 0) ? kChainFirst : 0;
      if (uq && k + 1 < nblk && r < 4 * (k + 2)) {
        const int rl = r - 4 * (k + 1);
        for (int q = 0; q <= rl; ++q) {  // lower quarters of the diagonal block's slice r
          Task t = mk(CH_U32 | ((q + 1) << kChainGShift) | first, k, r, k + 1, dur[2] * 0.5f);
          t.dep(s_of(k, r));
          if (q != rl) t.dep(s_of(k, 4 * (k + 1) + q));
          if (lu >= 0) t.dep(lu);
          uq_of[r].push_back(add(t));
        }
        U[(size_t)k * nr + r] = uq_of[r].back();  // (not read: D(k + 1) waits for every quarter)
        continue;
      }
      if (kn.u128 && r >= 4 * (k + 2)) {
        // chain_u128: below the next diagonal block, the four slices of a block row take ONE 128 x 128 tile update
        // over panel k (a BLK task: the same k-steps, half the CU time of four slice updates); it publishes every
        // slice's counter, so each slice's next panel solve waits for the block row instead of its own slice
        if (r % 4 == 0 || r == 4 * (k + 2)) {
          blk(k, 1, r / 4, k + 1);
          const int bt = last_upd[(size_t)(r / 4) * nbt + (k + 1)];
          for (int s2 = r; s2 <= std::min(4 * (r / 4) + 3, rlast); ++s2) U[(size_t)k * nr + s2] = bt;
        }
        continue;
      }
      Task t = mk(CH_U32 | first, k, r, k + 1, dur[2]);
      t.dep(s_of(k, r));
      for (int s = 4 * (k + 1); s <= std::min(4 * (k + 1) + 3, rlast); ++s)
        if (s != r) t.dep(s_of(k, s));
      if (lu >= 0) t.dep(lu);
      U[(size_t)k * nr + r] = add(t);
    }
    for (int jj = k + 2; jj <= yb; ++jj) {
      // identity-augmented lists: the corner's columns (jj >= nblk) are read by no later task -- only the
      // read-out and the gradient use -K^-1 -- so their tiles take deeper groups (chain_group_corner)
      // (the corner's last updates wait for the last panel solves and form the factorisation's tail: the last
      // tail_c panels keep depth G)
      const bool corner = eye && jj >= nblk;
      const int qlim = corner ? std::max(0, nblk - tail_c) : 0;
      int q0, q1;
      if (corner && k < qlim) {
        q0 = k / Gc * Gc;
        q1 = std::min(q0 + Gc, qlim);
      } else {
        q0 = qlim + (k - qlim) / G * G;
        q1 = std::min(q0 + G, nblk);
      }
      const bool grouped = q1 - q0 > 1 && jj >= q1 + LA;
      if (grouped && k != q1 - 1) continue;  // the group's one task comes with its last panel
      // the columns too near the diagonal for the group (chain_group_near > 1): sub-groups of Gn panels of the
      // group, under the same rule (a column at least LA past the sub-group's last panel), else panel by panel
      const int p0 = q0 + (k - q0) / Gn * Gn, p1 = std::min(p0 + Gn, q1);
      const bool sub = !grouped && p1 - p0 > 1 && jj >= p1 + kn.near_la;
      if (sub && k != p1 - 1) continue;
      for (int i = jj; i <= yb; ++i) {
        if (grouped)
          blk(q0, q1 - q0, i, jj);
        else if (sub)
          blk(p0, p1 - p0, i, jj);
        else
          blk(k, 1, i, jj);
      }
    }
  }
  // independent members (a small batch): one copy of the graph per member, tagged in the type word's bits
  // 8.. (task fields: ty | (g - 1) << 2 | member << 8), scheduled together so that every member's diagonal
  // chain runs beside the others' tile updates
  if (nmem > 1) {
    const int n1 = (int)T.size();
    T.reserve((size_t)n1 * nmem);
    for (int m = 1; m < nmem; ++m)
      for (int t = 0; t < n1; ++t) {
        Task c = T[t];
        c.ty |= m << kChainMemberShift;
        for (int e = 0; e < c.nd; ++e) c.deps[e] += m * n1;
        T.push_back(c);
      }
  }
  if (overflow) return {};
  const int n = (int)T.size();
  // successors in CSR form, each task's in the order its dependants were built
  std::vector<int> indeg(n, 0), soff(n + 1, 0);
  for (int t = 0; t < n; ++t)
    for (int e = 0; e < T[t].nd; ++e) ++soff[T[t].deps[e] + 1];
  for (int t = 0; t < n; ++t) soff[t + 1] += soff[t];
  std::vector<int> succ(soff[n]), fill(soff.begin(), soff.end() - 1);
  for (int t = 0; t < n; ++t)
    for (int e = 0; e < T[t].nd; ++e) {
      succ[fill[T[t].deps[e]]++] = t;
      ++indeg[t];
    }
  std::vector<float> bl(n, 0.f);
  for (int t = n - 1; t >= 0; --t) {  // the construction order is topological
    float m = 0.f;
    for (int e = soff[t]; e < soff[t + 1]; ++e) m = std::max(m, bl[succ[e]]);
    bl[t] = T[t].dur + m;
  }
  auto cmp = [&](int a, int b) { return bl[a] != bl[b] ? bl[a] < bl[b] : a > b; };
  std::priority_queue<int, std::vector<int>, decltype(cmp)> ready(cmp);
  std::priority_queue<std::pair<float, int>, std::vector<std::pair<float, int>>, std::greater<std::pair<float, int>>> ev;
  for (int t = 0; t < n; ++t)
    if (indeg[t] == 0) ready.push(t);
  std::vector<int32_t> out;
  out.reserve((size_t)n * 4);
  int free = std::max(1, grid);
  float now = 0.f;
  while ((int)out.size() < 4 * n) {
    while (free > 0 && !ready.empty()) {
      const int t = ready.top();
      ready.pop();
      out.insert(out.end(), {T[t].ty, T[t].k, T[t].r, T[t].j});
      ev.push({now + T[t].dur, t});
      --free;
    }
    if (ev.empty()) break;  // (cannot happen for a well-formed graph)
    const auto e = ev.top();
    ev.pop();
    now = e.first;
    ++free;
    for (int x = soff[e.second]; x < soff[e.second + 1]; ++x)
      if (--indeg[succ[x]] == 0) ready.push(succ[x]);
  }
  return out;
}

}  // namespace gpk
