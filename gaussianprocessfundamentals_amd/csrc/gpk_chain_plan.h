// Task order of chain_kernel (gpk_potrf.hip) for one shape: the task graph (D / S / U32 / BLK, see there)
// list-scheduled on `grid` workers with estimated durations, highest bottom level (longest path to the
// end) first; the order in which the simulation starts the tasks is a topological order, which the
// kernel needs (every task waits only for tasks claimed before it), and puts the diagonal chain ahead
// of the trailing tiles whenever both are ready.  Plain C++17, no HIP header; the task word: gpk_const.h.
#pragma once

#include <stdint.h>

#include <tuple>
#include <vector>

#include "gpk_tune.h"

namespace gpk {

// Every tuning input of chain_order, resolved once per call from the knobs (and part of the plan cache key, so a
// cached device plan and gpk_chain_plan_ex always agree)
struct ChainKnobs {
  int group, uq, group_corner, corner_tail, group_la, group_near, u128, near_la, s128;
  // (a new field goes into this list too: it is the plan cache key's ordering)
  auto tie() const { return std::tie(group, uq, group_corner, corner_tail, group_la, group_near, u128, near_la, s128); }
};
static_assert(sizeof(ChainKnobs) == 9 * sizeof(int), "a new ChainKnobs field also goes into ChainKnobs::tie");
ChainKnobs chain_knobs(const Tune& tn, int64_t n_pad, bool eye, bool f32 = false, int grid = 0);

// Key of a cached device plan: everything chain_order and chain_split_lists read
struct ChainPlanKey {
  int dev;
  int64_t n_pad, y_row;
  int grid, nmem, eye, xcd;
  ChainKnobs kn;
  auto tie() const { return std::tuple_cat(std::tie(dev, n_pad, y_row, grid, nmem, eye, xcd), kn.tie()); }
  bool operator<(const ChainPlanKey& o) const { return tie() < o.tie(); }
};

std::vector<int32_t> chain_order(int64_t n_pad, int64_t y_row, int grid, int nmem, const ChainKnobs& kn,
                                 bool eye = false);
int32_t chain_split_lists(std::vector<int32_t>& ord);

}  // namespace gpk
