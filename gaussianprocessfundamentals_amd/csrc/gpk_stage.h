// Staging of a tile edge's points in LDS and the row / column classes of the augmented layout: what the K build
// (gpk_assemble.hip) and the gradient kernels (gpk_grad.hip) both need.
#pragma once

#include "gpk_internal.h"
#include "gpk_kernels.h"

namespace gpk {
namespace {

enum { CLS_TRAIN = 0, CLS_PAD = 1, CLS_TEST = 2, CLS_Y = 3, CLS_ZERO = 4 };

// row / column class of index g for a member with n training and m test points
__device__ __forceinline__ int classify(const AsmArgs& a, int64_t g, int64_t n, int64_t m) {
  if (g < n) return CLS_TRAIN;
  if (g < a.n_pad) return CLS_PAD;
  if (g < a.n_pad + m) return CLS_TEST;
  if (g == a.y_row) return CLS_Y;
  return CLS_ZERO;
}

// training / test points of member b (ragged batches: its own counts)
__device__ __forceinline__ int64_t member_n(const AsmArgs& a, int b) { return a.nb ? a.nb[b] : a.n; }
__device__ __forceinline__ int64_t member_m(const AsmArgs& a, int b) { return a.mb ? a.mb[b] : a.m; }

// Stage 64 points (raw + per-ARD-node rescaled copies) of one tile edge into LDS.  sc_slot > 0: also
// sin(pi f) and cos(pi f) of u = x / p (f = u - rint(u)) for the periodic node sc_node(kd) into slots
// sc_slot and sc_slot + 1, clearing *sc_flag if any |u| exceeds SC_MAX_U.  w_slot > 0 (the K build of a program with
// change-point window leaves, dim 1): the k-th window leaf's w(x) of every point into slot w_slot + k -- once per
// point and tile edge, so the leaf costs one multiply per element -- and bit q of *cp_nz set if window node q is
// nonzero at any of the 64 points (padding points stage x = 0, whose w counts too: the skip only gets rarer).
__device__ __forceinline__ void stage_points(const gpk_kdesc& kd, const AsmArgs& a, const double* hyp,
                                             double* dst, int64_t g0, int b, bool rows, int slot_stride,
                                             int sc_slot = 0, double sc_iper = 0.0, int* sc_flag = nullptr,
                                             int w_slot = 0, unsigned long long* cp_nz = nullptr) {
  const int tid = threadIdx.x;
  unsigned long long nz = 0ull;
  for (int e = tid; e < ATILE * a.d; e += 256) {
    const int pt = e / a.d, k = e - pt * a.d;
    const int64_t g = g0 + pt;
    double v = 0.0;
    if (a.plain) {
      const int64_t lim = rows ? a.n : a.m;
      const double* src = rows ? a.X : a.Xs;
      if (g < lim) v = src[g * a.d + k];
    } else {
      const int c = classify(a, g, member_n(a, b), member_m(a, b));
      if (c == CLS_TRAIN) v = a.X[(int64_t)b * a.x_bs + g * a.d + k];
      else if (c == CLS_TEST && a.E == nullptr && !a.eye) v = a.Xs[(int64_t)b * a.xs_bs + (g - a.n_pad) * a.d + k];
    }
    dst[pt * a.dp + k] = v;
    if (sc_slot > 0) {
      const double u = v * sc_iper;
      if (!(fabs(u) <= SC_MAX_U)) atomicAnd(sc_flag, 0);
      double sv, cv;
      sincospi(u - rint(u), &sv, &cv);
      dst[sc_slot * slot_stride + pt * a.dp + k] = sv;
      dst[(sc_slot + 1) * slot_stride + pt * a.dp + k] = cv;
    }
    // ARD copies: u = x / ls (the reference kernel with l = 1 on rescaled inputs)
    for (int q = 0; q < kd.n_nodes; ++q) {
      const gpk_node nd = kd.nodes[q];
      if (nd.op != GPK_OP_ADD && nd.op != GPK_OP_MUL && (nd.flags & GPK_NODE_ARD))
        dst[(nd.ard_slot + 1) * slot_stride + pt * a.dp + k] = v / hyp[nd.hyp_offset + k];
    }
    if (w_slot > 0) {
      int kw = 0;
      for (int q = 0; q < kd.n_nodes; ++q) {
        const gpk_node nd = kd.nodes[q];
        if (nd.op != GPK_OP_CPW) continue;
        const double w = cp_window(nd.flags, hyp + nd.hyp_offset, v);
        dst[(w_slot + kw) * slot_stride + pt * a.dp + k] = w;
        if (w != 0.0) nz |= 1ull << q;
        ++kw;
      }
    }
  }
  if (w_slot > 0 && nz != 0ull) atomicOr(cp_nz, nz);
}

}  // namespace
}  // namespace gpk
