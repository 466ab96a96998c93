// The schedule of the launch path (gpk_potrf_aug and its _ex / _ragged forms, gpk_abi.hip potrf_impl): every launch
// and every event edge of one factorisation as a flat list of steps, a pure function of the shape, the flags and the
// knobs.  potrf_impl walks the list and issues it; gpk_launch_plan (gpk.h) returns it for inspection;
// tests/test_launch_plan.py replays it on the CPU.  Plain C++17, no HIP header.
#pragma once

#include <stdint.h>

#include <vector>

#include "gpk_tune.h"

namespace gpk {

constexpr int kFuseCtr = 256;  // ticket counters of the fused panel solve per stream: members per launch

// LaunchStep::kind.  PREP: the right operand of a folded panel solve (in-group mode 4, gpk_launch_plan.cpp), per member
// Wop = [ -L_kk^-1 B | L_kk^-1 ], B = W[128 kblk .. + 127, j0 .. j0 + kdepth - 1], into the panel stream's scratch
enum { LP_DIAG = 0, LP_TRSM = 1, LP_UPDATE = 2, LP_RECORD = 3, LP_WAIT = 4, LP_PREP = 5 };
// LaunchStep::stream -- logical: with the look-ahead off every step is on the caller's stream; which queue the panel
// stream is (gpk_tune "panel_stream") is the issuer's business
enum { LP_CALLER = 0, LP_PANEL = 1, LP_BULK = 2 };
enum { LP_EV_FORK = 0, LP_EV_PANEL = 1, LP_EV_BULK = 2, LP_EV_JOIN_P = 3, LP_EV_JOIN_B = 4, LP_NUM_EVENTS = 5 };
// LaunchStep::role of an UPDATE: in-group (thin: one block column or, right-looking, the group's remaining columns;
// half: the two-level schedule's second half) or the group's trailing update (look-ahead + bulk, or whole)
enum { LP_ROLE_NONE = 0, LP_ROLE_THIN = 1, LP_ROLE_HALF = 2, LP_ROLE_LOOKAHEAD = 3, LP_ROLE_BULK = 4, LP_ROLE_GROUP = 5 };

// One step: GPK_LAUNCH_STEP_WORDS (gpk.h) 8-byte words, in this order -- the record gpk_launch_plan writes.
struct LaunchStep {
  int64_t kind, stream;
  int64_t event;  // RECORD / WAIT: LP_EV_*; else -1
  int64_t role;   // UPDATE: LP_ROLE_*; else 0
  int64_t cls;    // timing class (gpk_timing_read): 1 diag, 2 trsm, 3 update; events -1
  // DIAG: block kblk (j0 = 128 kblk); trsm_tiles > 0: the panel solve of the 64-row tiles from row0 runs inside the
  // launch (no TRSM step follows), with the zero band [zlo, zhi)
  int64_t kblk, trsm_tiles;
  // TRSM with kdepth > 128 (folded, in-group mode 4): block column j0 / 128 is updated with the kdepth - 128 columns
  // left of it and solved in one launch -- X = [A | C] Wop^T over the columns [j0 + 128 - kdepth, j0 + 128), Wop the
  // preceding PREP step's; flops: the solve's and the folded update's
  // PREP: kblk, the B columns [j0, j0 + kdepth), row0 = 128 kblk
  // TRSM / UPDATE: panel columns [j0, j0 + kdepth), trailing region from row0; launch tile edge (128 / 64); nt tiles
  // of that edge from row0 and the update's tile-column range [c_lo, c_hi), both in the enumeration that leaves out
  // the bzn tiles from bz0 (the tiles wholly inside the zero band [zlo, zhi) of identity rows); tile order `band`;
  // rows >= row_end are zero in every panel (0: not used); kbuild: C is evaluated, not loaded (gpk_nlml)
  int64_t j0, row0, kdepth, tile, nt, c_lo, c_hi, zlo, zhi, bz0, bzn, band, row_end, kbuild;
  double flops, bytes;  // algorithmic work of the launch, as accumulated by gpk_timing_read
};
constexpr int kLaunchStepWords = 23;
static_assert(sizeof(LaunchStep) == kLaunchStepWords * 8, "LaunchStep is the record of gpk_launch_plan (gpk.h)");

// The layout scalars the schedule depends on (gpk_layout)
struct LaunchShape {
  bool f32;
  int64_t batch, m, n_pad, y_row, p;
  bool ragged = false;   // per-member sizes (gpk_potrf_aug_ragged): no folded panel solves
  bool no_fold = false;  // the panel stream has no operand scratch (as for `counters`): no folded panel solves
};

// Bytes of the operand scratch a plan with folded panel solves needs (0: it has none): batch x 128 x 128 ceil(G / 2),
// the deepest operand of the group size whatever the shape
int64_t launch_fold_bytes(const LaunchShape& sh, bool eye, const Tune& tn, const std::vector<LaunchStep>& steps);

// Whether the panel chain and the bulk updates run on side streams (look-ahead): the issuer needs the answer before
// the plan, to create the streams and to find the panel stream's fuse counters
bool launch_lookahead(const Tune& tn, int64_t p);

// Panels of the first group: the block columns a fused K build (gpk_nlml) must find assembled -- the first step with
// kbuild set comes after exactly this many DIAG steps
int64_t launch_first_group(const Tune& tn, bool eye, int64_t n_pad);

// counters: the panel stream has ticket counters (else no panel solve is fused); kbuild: the first group's trailing
// update carries the fused K build.  Clears and fills `out` (reserve it once and reuse it: no other allocation).
void launch_plan(const LaunchShape& sh, bool eye, bool counters, bool kbuild, const Tune& tn,
                 std::vector<LaunchStep>& out);

}  // namespace gpk
