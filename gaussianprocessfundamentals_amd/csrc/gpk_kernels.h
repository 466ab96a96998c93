// Device evaluation of the kernel program (shared by the K build in gpk_assemble.hip, the gradient
// kernels in gpk_grad.hip and the fused first trailing update in gpk_potrf.hip).  Reference formulas:
// see gpk_assemble.hip.
// Multiply-adds are contracted within a source expression only (fp contract(on)): with hipcc's
// default (fast) the fusions across statements depend on the inlining context, so the K build's
// interior / edge loops and the fused build would round a few elements differently.
#pragma once

#include <math.h>

#include "gpk_internal.h"

namespace gpk {
namespace {

constexpr double SQRT3 = 1.7320508075688772;
constexpr double SQRT5 = 2.23606797749979;
constexpr double PI = 3.141592653589793;

// ------------------------------------------------------------------ change-point window leaf (GPK_OP_CPW)
// ChangePointOperator's masks (KernelBasics/Operators.py:379-408) on 1-D inputs.  ONE function with one operation
// order computes a point's window everywhere (the K build stages it once per point and tile edge, the gradient
// kernels call it per element), so every path multiplies the same two doubles.
//   INDICATOR         [x < cp]                              d / d cp: 0 (tf.less passes no gradient)
//   SIGMOID           0.5 (1 + tanh((cp - x) / 0.0025))     d / d cp: 200 sech^2((cp - x) / 0.0025)
//   APPROX_INDICATOR  1 / (1 + exp(-100 (x - cp)))          d / d cp: -100 s (1 - s)        (rises with x, as upstream)
// The hard mask is exactly 0.0 / 1.0; the SIGMOID one is exactly 0.0 / 1.0 wherever tanh has rounded to -1 / +1
// (|cp - x| >~ 0.048): such points make a window exactly +0.0, which the tile-level child skip relies on.
constexpr double CP_SIGMOID_WIDTH = 0.0025;
constexpr double CP_APPROX_SLOPE = 100.0;

__device__ __forceinline__ double cp_ind(int fl, double x, double cp) {
#pragma clang fp contract(on)
  if (fl & GPK_NODE_CP_SIGMOID) return 0.5 * (1.0 + tanh((cp - x) / CP_SIGMOID_WIDTH));
  if (fl & GPK_NODE_CP_APPROX) return 1.0 / (1.0 + exp(-CP_APPROX_SLOPE * (x - cp)));
  return x < cp ? 1.0 : 0.0;
}

// d ind / d cp (= -d ind / d x)
__device__ __forceinline__ double cp_ind_dcp(int fl, double x, double cp) {
#pragma clang fp contract(on)
  if (fl & GPK_NODE_CP_SIGMOID) {
    const double ch = cosh((cp - x) / CP_SIGMOID_WIDTH);  // (overflows to inf far from cp: the derivative is 0 there)
    return (0.5 / CP_SIGMOID_WIDTH) / (ch * ch);
  }
  if (fl & GPK_NODE_CP_APPROX) {
    const double sv = 1.0 / (1.0 + exp(-CP_APPROX_SLOPE * (x - cp)));
    return -CP_APPROX_SLOPE * (sv * (1.0 - sv));
  }
  return 0.0;
}

__host__ __device__ inline int cp_bounds(int fl) {
  return ((fl & GPK_NODE_CP_LO) ? 1 : 0) + ((fl & GPK_NODE_CP_HI) ? 1 : 0);
}

// Hyperparameters a leaf owns from hyp_offset on: its shape entries -- a window leaf's bounds; the d entries of an
// ARD node (l_k) or a linear node (c_k); [l, p] of PER and [l, a] of RQ; else the one l -- then sg if it is scaled.
// The one statement of the rule: valid_kdesc bounds the offsets with it, the gradient kernels write these slots.
__host__ __device__ inline int node_shape_params(const gpk_node& nd, int d) {
  if (nd.op == GPK_OP_CPW) return cp_bounds(nd.flags);
  if ((nd.flags & GPK_NODE_ARD) || nd.op == GPK_OP_LIN) return d;
  return (nd.op == GPK_OP_PER || nd.op == GPK_OP_RQ) ? 2 : 1;
}
__host__ __device__ inline int node_params(const gpk_node& nd, int d) {
  return node_shape_params(nd, d) + ((nd.flags & GPK_NODE_SCALED) ? 1 : 0);
}

// w(x) = (1 - ind(x; h[0])) [CP_LO] * ind(x; h[lo ? 1 : 0]) [CP_HI]: the reference's previous-complement times this
// change point's indicator (:414-417, :431-436)
__device__ __forceinline__ double cp_window(int fl, const double* h, double x) {
#pragma clang fp contract(on)
  const bool lo = (fl & GPK_NODE_CP_LO) != 0, hi = (fl & GPK_NODE_CP_HI) != 0;
  const double wl = lo ? 1.0 - cp_ind(fl, x, h[0]) : 1.0;
  return hi ? (lo ? wl * cp_ind(fl, x, h[1]) : cp_ind(fl, x, h[0])) : wl;
}

// d w(x) / d (h[0], h[1]) into dw[0 .. bounds); d w / d x is minus their sum
__device__ __forceinline__ void cp_window_dcp(int fl, const double* h, double x, double (&dw)[2]) {
#pragma clang fp contract(on)
  const bool lo = (fl & GPK_NODE_CP_LO) != 0, hi = (fl & GPK_NODE_CP_HI) != 0;
  dw[0] = dw[1] = 0.0;
  if (lo && hi) {
    dw[0] = -cp_ind_dcp(fl, x, h[0]) * cp_ind(fl, x, h[1]);
    dw[1] = (1.0 - cp_ind(fl, x, h[0])) * cp_ind_dcp(fl, x, h[1]);
  } else if (lo) {
    dw[0] = -cp_ind_dcp(fl, x, h[0]);
  } else if (hi) {
    dw[0] = cp_ind_dcp(fl, x, h[0]);
  }
}

// whether a window leaf BEFORE node qn reads hyperparameter slot s (adjacent windows share a bound): the gradient
// reductions then add node qn's partial sum to the slot instead of assigning it
__host__ __device__ inline bool cp_slot_written(const gpk_kdesc& kd, int qn, int s) {
  for (int q = 0; q < qn; ++q) {
    const gpk_node nd = kd.nodes[q];
    if (nd.op == GPK_OP_CPW && s >= nd.hyp_offset && s < nd.hyp_offset + cp_bounds(nd.flags)) return true;
  }
  return false;
}

// number of window leaves of a program
__host__ __device__ inline int cp_windows(const gpk_kdesc& kd) {
  int nw = 0;
  for (int q = 0; q < kd.n_nodes; ++q) nw += kd.nodes[q].op == GPK_OP_CPW ? 1 : 0;
  return nw;
}

// A window leaf directly left of its sibling under a MUL (postfix W <sibling subtree> MUL, what ChangePointOperator
// emits): the index of that MUL, 0 if the op that consumes the window is not a MUL.  Where the window is zero the
// evaluator pushes +0.0 and continues after that index.
__host__ __device__ inline int cp_skip_to(const gpk_kdesc& kd, int q) {
  int depth = 1;  // stack entries from the window's upwards
  for (int j = q + 1; j < kd.n_nodes; ++j) {
    const int op = kd.nodes[j].op;
    if (op == GPK_OP_ADD || op == GPK_OP_MUL) {
      // the first op that reaches down to the window's entry consumes it (as the left operand iff depth 2 -> 1)
      if (--depth <= 1) return (depth == 1 && op == GPK_OP_MUL) ? j : 0;
    } else {
      ++depth;
    }
  }
  return 0;
}

// ------------------------------------------------------------------ rational quadratic leaf (GPK_OP_RQ)
// k = (1 + u)^(-a) = exp(-a log1p(u)), u = s / (2 a l^2), s the squared Euclidean distance (SE's direct sum).  ONE
// pair of functions with one operation order computes it everywhere (base_values for the gradient kernels,
// fast_value_at_c for every K-build path), so every path writes the same bits: iu = 1 / (2 a l^2) once per
// thread, then one multiply, one log1p, one multiply and one exp per element.  a is used as given: a <= 0 gives
// IEEE NaN / inf (gpk.h).  Rounding: u carries <= 3 eps relative, so the exponent a log1p(u) carries
// <= ~4 eps a log1p(u) absolute, which is the relative error of k.
__device__ __forceinline__ double rq_iu(double l, double a) {
#pragma clang fp contract(on)
  return 1.0 / ((2.0 * a) * (l * l));
}
__device__ __forceinline__ double rq_value(double s, double iu, double a) {
#pragma clang fp contract(on)
  const double u = s * iu;
  return exp(-a * log1p(u));
}

// g(u) = u / (1 + u) - log1p(u) = d log k / d a, u >= 0.  The two terms cancel: g = -u^2 / 2 + O(u^3), and the
// direct form's relative error is ~ 2 eps / u.  With w = u / (1 + u), log1p(u) = -log(1 - w), so
// g = -sum_{k >= 2} w^k / k: below RQ_G_SERIES_U the series to w^10 (truncation <= (2 / 11) w^9 relative, 1e-17 at
// the threshold), above it the direct form (2 eps / u <= 3e-14 there).  Measured against mpmath: DESIGN 16.
constexpr double RQ_G_SERIES_U = 0.015625;  // 2^-6
__device__ __forceinline__ double rq_g(double u) {
#pragma clang fp contract(on)
  const double w = u / (1.0 + u);
  if (u < RQ_G_SERIES_U) {
    double p = 1.0 / 10.0;
    p = fma(p, w, 1.0 / 9.0);
    p = fma(p, w, 1.0 / 8.0);
    p = fma(p, w, 1.0 / 7.0);
    p = fma(p, w, 1.0 / 6.0);
    p = fma(p, w, 1.0 / 5.0);
    p = fma(p, w, 1.0 / 4.0);
    p = fma(p, w, 1.0 / 3.0);
    p = fma(p, w, 0.5);
    return -(w * w) * p;
  }
  return w - log1p(u);
}

// number of rational quadratic leaves of a program: one or more selects the instantiations that carry the leaf's
// code (template parameter RQL of the evaluators below; launch_assemble in gpk_assemble.hip, launch_grad and launch_vjp
// in gpk_grad.hip).  log1p on top of exp costs registers -- 127 -> 171 VGPRs in the single-node K build, four waves
// per SIMD down to two -- so the kernels every other program runs compile none of it and are, instruction for
// instruction, what they were before the leaf existed.  Every evaluation of a program goes through one of those three
// launches (or the fused first trailing update, single SE / MAT32 / MAT52 nodes only), so an instantiation without the
// code never sees an RQ node.
__host__ __device__ inline int rq_leaves(const gpk_kdesc& kd) {
  int nr = 0;
  for (int q = 0; q < kd.n_nodes; ++q) nr += kd.nodes[q].op == GPK_OP_RQ ? 1 : 0;
  return nr;
}

// Values of one base node for R row points a[i] against one column point b.  The R evaluations
// are independent, so the compiler interleaves their long f64 chains (exp / sin / sqrt / div).
template <int R, bool RQL = false>
__device__ __forceinline__ void base_values(const gpk_node& nd, const double* __restrict__ hyp,
                                            const double* const (&a)[R], const double* b, int d, double (&r)[R]) {
#pragma clang fp contract(on)  // fuse within an expression only: every caller rounds alike
  const int fl = nd.flags;
  const bool ard = (fl & GPK_NODE_ARD) != 0;
  const double* h = hyp + nd.hyp_offset;
  int sg_at;
  if (nd.op == GPK_OP_SE) {
    double s[R];
    if (fl & GPK_NODE_SE_EXPANDED) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        double na = 0.0, nb = 0.0, ab = 0.0;
        for (int k = 0; k < d; ++k) {
          na += a[i][k] * a[i][k];
          nb += b[k] * b[k];
          ab += a[i][k] * b[k];
        }
        const double dist = sqrt((na - 2.0 * ab) + nb);  // NaN on a negative argument, as the reference
        s[i] = dist * dist;
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) s[i] = 0.0;
      for (int k = 0; k < d; ++k) {
        const double bk = b[k];
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const double t = a[i][k] - bk;
          s[i] += t * t;
        }
      }
    }
    const double l = ard ? 1.0 : h[0];
    const double l2 = l * l;
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = exp(-0.5 * (s[i] / l2));
    sg_at = ard ? d : 1;
  } else if (nd.op == GPK_OP_PER) {
    const double l = h[0], per = h[1];
    double sn[R];
    if (fl & GPK_NODE_STANDARD) {  // product of 1-D periodic kernels
#pragma unroll
      for (int i = 0; i < R; ++i) sn[i] = 0.0;
      for (int k = 0; k < d; ++k) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const double t = sin(PI * (fabs(a[i][k] - b[k]) / per));
          sn[i] += t * t;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        double dist = 0.0;
        for (int k = 0; k < d; ++k) dist += fabs(a[i][k] - b[k]);
        const double t = sin(PI * (dist / per));
        sn[i] = t * t;
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = exp((-2.0 * sn[i]) / (l * l));
    sg_at = 2;
  } else if (nd.op == GPK_OP_LIN) {  // sum_k (a_k - c_k)(b_k - c_k), c = h[0..d): the raw points, no ARD slot
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = 0.0;
    for (int k = 0; k < d; ++k) {
      const double ck = h[k];
      const double tb = b[k] - ck;
#pragma unroll
      for (int i = 0; i < R; ++i) r[i] += (a[i][k] - ck) * tb;
    }
    sg_at = d;
  } else if (RQL && nd.op == GPK_OP_RQ) {  // (1 + s / (2 a l^2))^(-a): SE's direct sum of squares, then rq_value
    double s[R];
#pragma unroll
    for (int i = 0; i < R; ++i) s[i] = 0.0;
    for (int k = 0; k < d; ++k) {
      const double bk = b[k];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double t = a[i][k] - bk;
        s[i] += t * t;
      }
    }
    const double av = h[1];
    const double iu = rq_iu(h[0], av);
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = rq_value(s[i], iu, av);
    sg_at = 2;
  } else if (nd.op == GPK_OP_CPW) {  // w(a) w(b): the direct form (the K build multiplies the staged w's: same bits)
    const double wb = cp_window(fl, h, b[0]);
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = cp_window(fl, h, a[i][0]) * wb;
    return;  // (no sg)
  } else {  // MAT32 / MAT52
    double dist[R];
#pragma unroll
    for (int i = 0; i < R; ++i) dist[i] = 0.0;
    if (fl & GPK_NODE_STANDARD) {  // Euclidean distance
      for (int k = 0; k < d; ++k) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          const double t = a[i][k] - b[k];
          dist[i] += t * t;
        }
      }
#pragma unroll
      for (int i = 0; i < R; ++i) dist[i] = sqrt(dist[i]);
    } else {
      for (int k = 0; k < d; ++k) {
#pragma unroll
        for (int i = 0; i < R; ++i) dist[i] += fabs(a[i][k] - b[k]);
      }
    }
    const double l = ard ? 1.0 : fabs(h[0]);
    if (nd.op == GPK_OP_MAT52) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double frac = (SQRT5 * dist[i]) / l;
        const double third = (5.0 * (dist[i] * dist[i])) / (3.0 * (l * l));
        r[i] = ((1.0 + frac) + third) * exp(-frac);
      }
    } else {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const double frac = (SQRT3 * dist[i]) / l;
        r[i] = (1.0 + frac) * exp(-frac);
      }
    }
    sg_at = ard ? d : 1;
  }
  if (fl & GPK_NODE_SCALED) {
    const double sg = h[sg_at];
#pragma unroll
    for (int i = 0; i < R; ++i) r[i] = sg * r[i];
  }
}

template <bool RQL = false>
__device__ __forceinline__ double base_value(const gpk_node& nd, const double* __restrict__ hyp,
                                             const double* a, const double* b, int d) {
  const double* aa[1] = {a};
  double r[1];
  base_values<1, RQL>(nd, hyp, aa, b, d, r);
  return r[0];
}

// Register stack of the postfix program.  The stack pointer is wave-uniform, so the switch
// lowers to scalar branches and nothing is indexed dynamically (no scratch).
struct Stack {
  double s0, s1, s2, s3, s4, s5, s6, s7;
  __device__ __forceinline__ double get(int i) const {
    switch (i) {
      case 0: return s0; case 1: return s1; case 2: return s2; case 3: return s3;
      case 4: return s4; case 5: return s5; case 6: return s6; default: return s7;
    }
  }
  __device__ __forceinline__ void set(int i, double v) {
    switch (i) {
      case 0: s0 = v; break; case 1: s1 = v; break; case 2: s2 = v; break; case 3: s3 = v; break;
      case 4: s4 = v; break; case 5: s5 = v; break; case 6: s6 = v; break; default: s7 = v; break;
    }
  }
};

// Single-base-node trees (the common case, e.g. every SURVEY config but C5): the node's constants
// are computed once per thread into registers and every division by a hyperparameter becomes a
// multiplication by its reciprocal (|error| <= ~1e-14 relative in K).  Multi-node trees go through
// eval_tree_fast with the same reciprocals and periodic nodes through sin2_pi, so the K build no
// longer keeps the reference's literal operation order anywhere.  The gradient kernel re-evaluates K
// with base_values (divisions, library sin): for trees its K differs from the factorised one by
// ~1e-14 relative, far inside the gradient tests' tolerances.
struct FastNode {
  int op, flags, d, off;
  double il, il2, i3l2, iper, sg;
  const double* c;  // linear node: its d offsets (the node's hyperparameters where the caller staged them)
  // periodic node through the staged sin / cos of its points (sc_node): sin(pi u), cos(pi u) per point and
  // dimension at offsets sc_sin / sc_cos from the point (tiles whose points all have |u| = |x / p| <= 4)
  int sc, sc_sin, sc_cos;
  // window leaf (GPK_OP_CPW): `off` is the point slot that holds its staged w; skip_to > 0: the MUL that closes
  // (window, sibling) -- on a tile where the window is zero the evaluator continues after it (cp_skip_to)
  int skip_to;
};
static_assert(sizeof(FastNode) == 80, "the K build's LDS request counts GPK_MAX_NODES of these");

// The periodic node whose sin^2(pi (x_k - y_k) / p) terms the K build takes from per-point sin / cos
// (sin(a - b) = sin a cos b - cos a sin b; separable per dimension: the standard form, or D = 1 where the
// reference's L1 form is the same): the first such node of the program, -1 if none.
__host__ __device__ inline int sc_node(const gpk_kdesc& kd) {
  for (int q = 0; q < kd.n_nodes; ++q)
    if (kd.nodes[q].op == GPK_OP_PER && ((kd.nodes[q].flags & GPK_NODE_STANDARD) || kd.dim == 1)) return q;
  return -1;
}
constexpr double SC_MAX_U = 4.0;  // |x / p| bound of a tile for the sin / cos form (phase error <= 8 pi eps)

__device__ __forceinline__ int fast_off(const gpk_kdesc& kd, int slot_stride) {
  return (kd.nodes[0].flags & GPK_NODE_ARD) ? (kd.nodes[0].ard_slot + 1) * slot_stride : 0;
}

// (RQL: as the evaluators' -- the instantiations never launched on a program with a rational quadratic leaf carry none
// of its code, here its two constants)
template <bool RQL = false>
__device__ __forceinline__ FastNode make_fast_node(const gpk_node& nd, const double* hyp, int d) {
  FastNode f;
  f.op = nd.op;
  f.flags = nd.flags;
  f.d = d;
  f.off = 0;
  const double* h = hyp + nd.hyp_offset;
  const bool ard = (nd.flags & GPK_NODE_ARD) != 0;
  double l = 1.0;
  int sg_at = 1;
  f.c = nullptr;
  if (nd.op == GPK_OP_PER) {
    l = h[0];
    f.iper = 1.0 / h[1];
    sg_at = 2;
  } else if (nd.op == GPK_OP_LIN) {  // no length scale: hyp [c_0..c_{d-1}, (sg)]
    f.c = h;
    f.iper = 0.0;
    sg_at = d;
  } else if (RQL && nd.op == GPK_OP_RQ) {  // hyp [l, a, (sg)]: a in iper (free for every node but PER), il2 set below
    l = h[0];
    f.iper = h[1];
    sg_at = 2;
  } else {  // (a window leaf, GPK_OP_CPW, lands here too: it uses none of these constants)
    l = ard ? 1.0 : (nd.op == GPK_OP_SE ? h[0] : fabs(h[0]));
    f.iper = 0.0;
    sg_at = ard ? d : 1;
  }
  f.il = 1.0 / l;
  // (a rational quadratic node keeps 1 / (2 a l^2) here: u = s * il2, rq_value)
  f.il2 = (RQL && nd.op == GPK_OP_RQ) ? rq_iu(l, f.iper) : 1.0 / (l * l);
  f.i3l2 = 1.0 / (3.0 * (l * l));
  f.sg = (nd.flags & GPK_NODE_SCALED) ? h[sg_at] : 1.0;
  f.sc = 0;
  f.sc_sin = f.sc_cos = 0;
  f.skip_to = 0;
  return f;
}

// sin^2 over the dimensions from per-point sin(pi u) / cos(pi u) (u = x / p, reduced by the nearest integer
// before the sincospi: the sign (-1)^n cancels in the square): sin(pi (u_a - u_b)) = s_a c_b - c_a s_b.
// Same contraction everywhere it is used (interior, generic and plain paths write the same bits).  Against the
// reference's sin(pi |x_a - x_b| / p) the phase error is eps (|u_a| + |u_b|) pi <= 8 pi eps on a tile that
// qualifies (SC_MAX_U): 3 VALU operations per dimension instead of the reduced Taylor series' ~25.
template <typename SA, typename CA, typename SB, typename CB>
__device__ __forceinline__ double per_sc_value(const FastNode& f, SA sa, CA ca, SB sb, CB cb) {
#pragma clang fp contract(on)  // fuse within an expression only: every caller rounds alike
  double sn = 0.0;
  for (int k = 0; k < f.d; ++k) {
    // sin(pi (a - b) / p) = sa cb - ca sb, the two products rounded separately (no FMA between them): swapping
    // the points swaps them exactly, so t(b, a) = -t(a, b) and K stays exactly symmetric (a contracted
    // fma(sa, cb, -ca sb) left 1-ulp asymmetries, found by tests/test_gpu_properties.py)
    const double p1 = sa(k) * cb(k);
    const double p2 = ca(k) * sb(k);
    const double t = p1 - p2;
    sn += t * t;
  }
  return f.sg * exp((-2.0 * sn) * f.il2);
}

// sin^2(pi t), t >= 0 (the periodic kernel's sin^2(pi d / p) with t = d / p).  sin^2 has period 1 in
// t, so t is reduced to its fraction (exact in floating point), folded onto [0, 1/2] by
// sin(pi g) = sin(pi (1 - g)) (1 - g exact there), and sin(pi g) is its Taylor series to x^19 on
// [0, pi/2] (truncation <= 2.6e-16): about a third of the library sin's work, with no quadrant
// branches.  The phase error of t itself, |t| ulp, is the reference formula's as well.
__device__ __forceinline__ double sin2_pi(double t) {
#pragma clang fp contract(on)  // fuse within an expression only: every caller rounds alike
  const double f = t - floor(t);
  const double g = fmin(f, 1.0 - f);
  const double x = PI * g;
  const double x2 = x * x;
  double p = -1.0 / 121645100408832000.0;     // -1/19!
  p = fma(p, x2, 1.0 / 355687428096000.0);    //  1/17!
  p = fma(p, x2, -1.0 / 1307674368000.0);     // -1/15!
  p = fma(p, x2, 1.0 / 6227020800.0);         //  1/13!
  p = fma(p, x2, -1.0 / 39916800.0);          // -1/11!
  p = fma(p, x2, 1.0 / 362880.0);             //  1/9!
  p = fma(p, x2, -1.0 / 5040.0);              // -1/7!
  p = fma(p, x2, 1.0 / 120.0);                //  1/5!
  p = fma(p, x2, -1.0 / 6.0);                 // -1/3!
  const double sv = fma(x * x2, p, x);
  return sv * sv;
}

// fast_value over coordinate accessors: a(k), b(k) return coordinate k of the two points, c(k) offset k of a
// linear node (read by that node only: callers that hold the offsets in registers pass them here)
template <bool RQL = false, typename PA, typename PB, typename PC>
__device__ __forceinline__ double fast_value_at_c(const FastNode& f, PA a, PB b, PC c) {
#pragma clang fp contract(on)  // fuse within an expression only: every caller rounds alike
  const int d = f.d;
  double r;
  if (f.op == GPK_OP_SE) {
    double s = 0.0;
    if (f.flags & GPK_NODE_SE_EXPANDED) {
      double na = 0.0, nb = 0.0, ab = 0.0;
      for (int k = 0; k < d; ++k) {
        na += a(k) * a(k);
        nb += b(k) * b(k);
        ab += a(k) * b(k);
      }
      const double dist = sqrt((na - 2.0 * ab) + nb);
      s = dist * dist;
    } else {
      for (int k = 0; k < d; ++k) {
        const double t = a(k) - b(k);
        s += t * t;
      }
    }
    r = exp(-0.5 * (s * f.il2));
  } else if (f.op == GPK_OP_PER) {
    double sn = 0.0;
    if (f.flags & GPK_NODE_STANDARD) {
      for (int k = 0; k < d; ++k) sn += sin2_pi(fabs(a(k) - b(k)) * f.iper);
    } else {
      double dist = 0.0;
      for (int k = 0; k < d; ++k) dist += fabs(a(k) - b(k));
      sn = sin2_pi(dist * f.iper);
    }
    r = exp((-2.0 * sn) * f.il2);
  } else if (f.op == GPK_OP_LIN) {
    // the first non-stationary leaf: both points shifted by c, the products accumulated in k order (one fma
    // per term: |error| <= (d + 2) eps / 2 sum_k |a_k - c_k| |b_k - c_k|).  Where the caller holds b and
    // c in registers, (b_k - c_k) is invariant over the lane's rows: hoisting it is left to the compiler
    r = 0.0;
    for (int k = 0; k < d; ++k) r += (a(k) - c(k)) * (b(k) - c(k));
  } else if (RQL && f.op == GPK_OP_RQ) {
    // SE's direct sum of squares, then the shared rq_value (il2 = 1 / (2 a l^2), iper = a: make_fast_node)
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      const double t = a(k) - b(k);
      s += t * t;
    }
    r = rq_value(s, f.il2, f.iper);
  } else {
    double dist = 0.0;
    if (f.flags & GPK_NODE_STANDARD) {
      for (int k = 0; k < d; ++k) {
        const double t = a(k) - b(k);
        dist += t * t;
      }
      dist = sqrt(dist);
    } else {
      for (int k = 0; k < d; ++k) dist += fabs(a(k) - b(k));
    }
    if (f.op == GPK_OP_MAT52) {
      const double frac = (SQRT5 * dist) * f.il;
      r = ((1.0 + frac) + (5.0 * (dist * dist)) * f.i3l2) * exp(-frac);
    } else {
      const double frac = (SQRT3 * dist) * f.il;
      r = (1.0 + frac) * exp(-frac);
    }
  }
  return f.sg * r;
}

template <bool RQL = false, typename PA, typename PB>
__device__ __forceinline__ double fast_value_at(const FastNode& f, PA a, PB b) {
  const double* cc = f.c;
  return fast_value_at_c<RQL>(f, a, b, [cc](int k) { return cc[k]; });
}

template <bool RQL = false>
__device__ __forceinline__ double fast_value(const FastNode& f, const double* a, const double* b, bool sc_on = false) {
  if (sc_on && f.sc && f.op == GPK_OP_PER) {
    const int so = f.sc_sin, co = f.sc_cos;
    return per_sc_value(f, [a, so](int k) { return a[so + k]; }, [a, co](int k) { return a[co + k]; },
                        [b, so](int k) { return b[so + k]; }, [b, co](int k) { return b[co + k]; });
  }
  return fast_value_at<RQL>(f, [a](int k) { return a[k]; }, [b](int k) { return b[k]; });
}

// The postfix program with every base node's constants precomputed (fns[q] = make_fast_node of
// node q, fns[q].off its ARD slot offset): the tree form of the single-node fast path -- no division
// by a hyperparameter per element, the periodic nodes through sin2_pi.  WIN (the instantiation for programs with
// change-point window leaves; the others carry none of this code): a window leaf's value is the product of its two
// staged w's (the point slot fns[q].off) -- one multiply per element; cp_zero: bit q set -- window leaf q is exactly
// zero on this tile (workgroup-uniform): +0.0 stands for (window, sibling, MUL) where the node has a skip_to.
// RQL: the instantiation for programs with rational quadratic leaves (rq_leaves).
template <bool WIN = false, bool RQL = false>
__device__ __forceinline__ double eval_tree_fast(const gpk_kdesc& kd, const FastNode* fns, const double* pa,
                                                 const double* pb, bool sc_on = false, unsigned cp_zero = 0u) {
  Stack st;
  st.s0 = 0.0;
  int sp = 0;
  for (int q = 0; q < kd.n_nodes; ++q) {
    const int op = kd.nodes[q].op;
    if (op == GPK_OP_ADD || op == GPK_OP_MUL) {
      const double top = st.get(sp - 1);
      const double below = st.get(sp - 2);
      st.set(sp - 2, op == GPK_OP_ADD ? below + top : below * top);
      sp -= 1;
    } else if (WIN && op == GPK_OP_CPW) {
      const int off = fns[q].off;
      // (read as a scalar, so the program counter stays wave-uniform)
      const int skip_to = __builtin_amdgcn_readfirstlane(fns[q].skip_to);
      if (((cp_zero >> q) & 1u) && skip_to > 0) {
        st.set(sp, 0.0);
        q = skip_to;  // (the loop's increment steps past the MUL)
      } else {
        st.set(sp, pa[off] * pb[off]);
      }
      sp += 1;
    } else {
      const FastNode f = fns[q];
      st.set(sp, fast_value<RQL>(f, pa + f.off, pb + f.off, sc_on));
      sp += 1;
    }
  }
  return st.s0;
}

}  // namespace
}  // namespace gpk
