// Constants shared by the kernels and the host-only units (no HIP header: plain C++17).
#pragma once

namespace gpk {

constexpr int NB = 128;     // panel width == update tile edge == diagonal block edge
constexpr int ATILE = 64;   // assemble tile edge

// Type word of a task of the persistent factorisation, written by chain_order (gpk_chain_plan.cpp), decoded by
// chain_kernel (gpk_potrf.hip) and documented with gpk_chain_plan_ex (gpk.h):
// ty (bits 0..1) | (g - 1) << 2 (BLK over g panels; UQ: quarter + 1; S: the slices of a chain_s128 task; bits 2..5) |
// kChainFirst | kChainSq | member << 8.
enum { CH_D = 0, CH_S = 1, CH_U32 = 2, CH_BLK = 3 };
constexpr int kChainTypeMask = 3;
constexpr int kChainGShift = 2, kChainGMask = 15;
// bit 6: the (slice, block column) cells the task updates have no earlier update -- its counter wait is for 0, not
// for the task's first panel; identity-augmented lists only
constexpr int kChainFirstBit = 6, kChainFirst = 1 << kChainFirstBit;
// bit 7 on an S task (chain_uq 2): SQ -- the panel solve of a slice of the next diagonal block followed by the
// slice's lower quarters of that block's update (chain_sq); it publishes sdone after the solve, qdone = 1 at the end
constexpr int kChainSqBit = 7, kChainSq = 1 << kChainSqBit;
constexpr int kChainMemberShift = 8;

}  // namespace gpk
