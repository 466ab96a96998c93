// Reverse mode of the kernel program: the LML gradient (gpk_nlml_grad: grad_kernel), the adjoints of a rectangular
// kernel matrix (gpk_kernel_vjp: vjp_kernel) and the gradient of the held-out mean squared error (gpk_mse_backward:
// mse_tile_kernel), and the forward planes d K / d theta_p written as matrices (gpk_kernel_jacobian: jacobian_kernel, at
// the end, element-major: it reduces nothing and shares none of the three loops below).  All walk 64 x 64 tiles staged as the K build stages them (gpk_stage.h) and re-evaluate the
// program per element with the reference's literal formulas (base_values, gpk_kernels.h).  launch_grad_cot runs
// grad_kernel over a cotangent buffer instead of W's corner (the leave-one-out gradient, gpk_loo.hip): a host launcher,
// launch_grad_tiles with five fields swapped.  The host side of the tile passes is said once (stage_args,
// tile_lds_bytes, launch_tiles_then_reduce, at the end of this file).
// Two things are written more than once here on purpose, in the same words, and a change to one belongs in the others
// (profiles/grad_split_codegen.txt, profiles/grad_split_ab.txt):
// - the three kernels' loops over the program's leaves (adjoint product over adj_mask, base_partials, the leaf's
//   node_params slots, the four-wave reduction into red, the window leaf's add to a shared bound): as one function
//   template the body takes vjp_kernel<true>, which sits at exactly 256 VGPRs, to one wave per SIMD (mse_tile_kernel's
//   copy is the third, under the same rule: it leaves the other two kernels' code as it was);
// - the distance and Matern prologues of base_partials and base_input_partials: as shared helpers they compute the
//   same bits but kernel_vjp measured 1 to 2 % slower than with this text.
#include <string.h>

#include "gpk_internal.h"
#include "gpk_kernels.h"
#include "gpk_stage.h"

namespace gpk {
namespace {

// ================================================================================ LML gradient
// d(-LML)/d theta_p = 1/2 sum_ij (K^-1 - alpha alpha^T)_ij dK_ij/d theta_p: the reverse-mode
// derivative TensorFlow's GradientTape takes through LogLikelihood.get_metric for
// VariationalSgdFitter (gpbasics/Optimizer/Fitter.py:104-158).  K^-1 and alpha come out of ONE
// factorisation of the augmented matrix with identity extra rows: its corner holds -K^-1 (lower
// triangle) and its y row -alpha^T.  Every workgroup takes one 64 x 64 lower tile of the n x n
// training block, re-evaluates the kernel tree there (values of every node, so the adjoint of a
// base node is the product of the node values its ancestors multiply it by -- a host-built mask)
// and reduces the weighted partial derivatives of each base node's hyperparameters; partial sums
// per tile go to a workspace reduced in a fixed order by grad_reduce_kernel (deterministic).

// values of every node of the postfix program (node q's value = its subtree's value) into the
// thread's LDS column v[q * 256]
template <bool RQL>
__device__ __forceinline__ void eval_nodes(const gpk_kdesc& kd, const double* hyp, const double* pa,
                                           const double* pb, int slot_stride, int d, double* v) {
  Stack st;
  st.s0 = 0.0;
  int sp = 0;
#pragma unroll 1
  for (int q = 0; q < kd.n_nodes; ++q) {
    const gpk_node nd = kd.nodes[q];
    if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) {
      const double top = st.get(sp - 1);
      const double below = st.get(sp - 2);
      st.set(sp - 2, nd.op == GPK_OP_ADD ? below + top : below * top);
      sp -= 1;
    } else {
      const int off = (nd.flags & GPK_NODE_ARD) ? (nd.ard_slot + 1) * slot_stride : 0;
      st.set(sp, base_value<RQL>(nd, hyp, pa + off, pb + off, d));
      sp += 1;
    }
    v[q * 256] = st.get(sp - 1);
  }
}

constexpr int GNP = GPK_MAX_DIM + 1;  // hyperparameters of one base node, at most (ARD l + sg)

// acc[k] += coef * d k_node / d h[k] for the node's hyperparameters h (reference formulas, see the citations at
// the top of gpk_assemble.hip; |l| of the Matern kernels differentiates to sign(l)).  RQL: the instantiation for
// programs with rational quadratic leaves (rq_leaves): the others carry none of that leaf's code.
template <bool RQL>
__device__ __forceinline__ void base_partials(const gpk_node& nd, const double* __restrict__ hyp,
                                              const double* a, const double* b, int d, double coef,
                                              double (&acc)[GNP]) {
  const int fl = nd.flags;
  const bool ard = (fl & GPK_NODE_ARD) != 0;
  const bool scaled = (fl & GPK_NODE_SCALED) != 0;
  const double* h = hyp + nd.hyp_offset;
  if (nd.op == GPK_OP_SE) {
    double s = 0.0;
    if (fl & GPK_NODE_SE_EXPANDED) {
      double na = 0.0, nb = 0.0, ab = 0.0;
      for (int k = 0; k < d; ++k) {
        na += a[k] * a[k];
        nb += b[k] * b[k];
        ab += a[k] * b[k];
      }
      const double dist = sqrt((na - 2.0 * ab) + nb);
      s = dist * dist;
    } else {
      for (int k = 0; k < d; ++k) {
        const double t = a[k] - b[k];
        s += t * t;
      }
    }
    const int sg_at = ard ? d : 1;
    const double sg = scaled ? h[sg_at] : 1.0;
    if (ard) {
      const double r = exp(-0.5 * s);
#pragma unroll
      for (int k = 0; k < GPK_MAX_DIM; ++k)
        if (k < d) {
          const double t = a[k] - b[k];  // (x_k - y_k) / l_k
          acc[k] += coef * sg * r * (t * t) / h[k];
        }
      if (scaled) acc[GPK_MAX_DIM] += coef * r;
    } else {
      const double l = h[0];
      const double r = exp(-0.5 * (s / (l * l)));
      acc[0] += coef * sg * r * s / (l * l * l);
      if (scaled) acc[1] += coef * r;
    }
    return;
  }
  if (nd.op == GPK_OP_LIN) {
    // k = sg sum_k (a_k - c_k)(b_k - c_k): d k / d c_k = -sg ((a_k - c_k) + (b_k - c_k)), d k / d sg the sum; the
    // slots as an ARD node's (c in acc[0..d), sg in acc[GPK_MAX_DIM])
    const double sg = scaled ? h[d] : 1.0;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < d) {
        const double ta = a[k] - h[k], tb = b[k] - h[k];
        s += ta * tb;
        acc[k] -= coef * sg * (ta + tb);
      }
    if (scaled) acc[GPK_MAX_DIM] += coef * s;
    return;
  }
  if (RQL && nd.op == GPK_OP_RQ) {
    // k = sg q^(-a), q = 1 + u, u = s / (2 a l^2): d k / d l = k s / (l^3 q), d k / d a = k g(u) with
    // g = u / q - log1p(u) (rq_g: a series where the two terms cancel), d k / d sg the unscaled value
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      const double t = a[k] - b[k];
      s += t * t;
    }
    const double l = h[0], av = h[1];
    const double sg = scaled ? h[2] : 1.0;
    const double iu = rq_iu(l, av);
    const double u = s * iu;
    const double r = rq_value(s, iu, av);
    acc[0] += coef * sg * r * s / ((l * l * l) * (1.0 + u));
    acc[1] += coef * sg * r * rq_g(u);
    if (scaled) acc[2] += coef * r;
    return;
  }
  if (nd.op == GPK_OP_CPW) {
    // k = w(a) w(b): d k / d cp = w'(a) w(b) + w(a) w'(b) for each bound the leaf has (acc[0], acc[1]); the hard
    // mask has no derivative (cp_ind_dcp)
    const double wa = cp_window(fl, h, a[0]), wb = cp_window(fl, h, b[0]);
    double da[2], db[2];
    cp_window_dcp(fl, h, a[0], da);
    cp_window_dcp(fl, h, b[0], db);
    acc[0] += coef * (da[0] * wb + wa * db[0]);
    acc[1] += coef * (da[1] * wb + wa * db[1]);
    return;
  }
  if (nd.op == GPK_OP_PER) {
    const double l = h[0], per = h[1];
    double sn, tw;  // sum sin^2(theta), sum theta sin(2 theta)
    if (fl & GPK_NODE_STANDARD) {
      sn = 0.0;
      tw = 0.0;
      for (int k = 0; k < d; ++k) {
        const double th = PI * (fabs(a[k] - b[k]) / per);
        const double t = sin(th);
        sn += t * t;
        tw += th * sin(2.0 * th);
      }
    } else {
      double dist = 0.0;
      for (int k = 0; k < d; ++k) dist += fabs(a[k] - b[k]);
      const double th = PI * (dist / per);
      const double t = sin(th);
      sn = t * t;
      tw = th * sin(2.0 * th);
    }
    const double r = exp((-2.0 * sn) / (l * l));
    const double sg = scaled ? h[2] : 1.0;
    acc[0] += coef * sg * r * 4.0 * sn / (l * l * l);
    acc[1] += coef * sg * r * 2.0 * tw / (l * l * per);
    if (scaled) acc[2] += coef * r;
    return;
  }
  // MAT32 / MAT52
  const bool std_form = (fl & GPK_NODE_STANDARD) != 0;
  double dist = 0.0;
  if (std_form) {
    for (int k = 0; k < d; ++k) {
      const double t = a[k] - b[k];
      dist += t * t;
    }
    dist = sqrt(dist);
  } else {
    for (int k = 0; k < d; ++k) dist += fabs(a[k] - b[k]);
  }
  const double c = (nd.op == GPK_OP_MAT52) ? SQRT5 : SQRT3;
  const int sg_at = ard ? d : 1;
  const double sg = scaled ? h[sg_at] : 1.0;
  const double l = ard ? 1.0 : h[0];
  const double f = (c * dist) / fabs(l);
  const double e = exp(-f);
  double r, drdf;  // value and d value / d f
  if (nd.op == GPK_OP_MAT52) {
    r = ((1.0 + f) + f * f / 3.0) * e;
    drdf = -(f / 3.0) * (1.0 + f) * e;
  } else {
    r = (1.0 + f) * e;
    drdf = -f * e;
  }
  if (ard) {
    // f = c dist(u, v), u = x / l: d dist / d l_k = -|u_k - v_k| / l_k (L1) or
    // -(u_k - v_k)^2 / (l_k dist) (Euclidean)
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < d) {
        const double t = a[k] - b[k];
        double dd;
        if (std_form) dd = dist > 0.0 ? -(t * t) / (h[k] * dist) : 0.0;
        else dd = -fabs(t) / h[k];
        acc[k] += coef * sg * drdf * c * dd;
      }
    if (scaled) acc[GPK_MAX_DIM] += coef * r;
  } else {
    acc[0] += coef * sg * drdf * (-f / l);  // d f / d l = -f / l  (f uses |l|)
    if (scaled) acc[1] += coef * r;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// training points of member b: the batch's one n, or (RAG) the member's own.  Spelled as a read of g.n at every use in
// the uniform instantiations, as before the ragged ones existed: a local copy of it changed their code.
template <bool RAG>
__device__ __forceinline__ int64_t grad_member_n(const GradArgs& g, int b) {
  if constexpr (RAG) return g.nb[b];
  else return g.n;
}

// RAG: the ragged instantiation (gpk_grad_ragged) -- member b's own n_b = g.nb[b] bounds the alpha staging, qval and
// (through a.nb, member_n) the points staged; a tile wholly at or beyond n_b writes its n_hyp + 1 partial sums as
// plain zeros and evaluates nothing (the workspace is not cleared and grad_reduce_kernel sums every tile of the layout,
// a window leaf's shared bound included: no read-modify-write of an unwritten slot).  The tile index t does not depend
// on n, so a member's nonzero partials sit where they do when it is factored alone.
template <typename T, bool RQL, bool RAG = false>
__global__ __launch_bounds__(256) void grad_kernel(gpk_kdesc kd, AsmArgs a, GradArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int slot_stride = ATILE * a.dp;
  double* hyp_s = smem;                                  // GPK_MAX_HYP
  double* al_r = hyp_s + GPK_MAX_HYP;                    // alpha of the tile rows / columns
  double* al_c = al_r + ATILE;
  double* red = al_c + ATILE;                            // [4 waves][GNP + 1]
  double* prow = red + 4 * (GNP + 1);
  double* pcol = prow + (1 + kd.n_ard) * slot_stride;
  double* vals = pcol + (1 + kd.n_ard) * slot_stride;   // [n_nodes][256] node values (MUL trees)

  const int b = blockIdx.y;
  const int64_t t = blockIdx.x;
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  const int64_t ti = r, tj = t - r * (r + 1) / 2;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int np1 = kd.n_hyp + 1;
  double* part = g.part + ((int64_t)b * gridDim.x + t) * np1;

  if constexpr (RAG) {
    if (ti * ATILE >= grad_member_n<RAG>(g, b)) {  // (tj <= ti: a lower tile whose rows are padding has no element below n_b; workgroup-uniform)
      for (int e = tid; e < np1; e += 256) part[e] = 0.0;
      return;
    }
  }
  const double* hyp_g = g.hyp + (int64_t)b * g.hyp_stride;
  for (int e = tid; e < kd.n_hyp; e += 256) hyp_s[e] = hyp_g[e];
  const T* W = reinterpret_cast<const T*>(g.W) + (int64_t)b * g.w_bs;
  const int64_t gi0 = ti * ATILE, gj0 = tj * ATILE;
  if (tid < 2 * ATILE) {
    const int64_t gg = (tid < ATILE ? gi0 : gj0) + (tid & (ATILE - 1));
    // y row of the corner: -alpha^T
    const double v = gg < grad_member_n<RAG>(g, b) ? -(double)W[g.y_row * g.ld + g.n_pad + gg] : 0.0;
    (tid < ATILE ? al_r : al_c)[tid & (ATILE - 1)] = v;
  }
  __syncthreads();
  stage_points(kd, a, hyp_s, prow, gi0, b, true, slot_stride);
  stage_points(kd, a, hyp_s, pcol, gj0, b, false, slot_stride);
  __syncthreads();

  const int c = lane;
  const int64_t gj = gj0 + c;
  // weighted (K^-1 - alpha alpha^T)_ij of this thread's 16 elements: weight 2 off the diagonal
  // (the strictly lower triangle stands for both halves), 1 on it; the corner holds -K^-1
  auto qval = [&](int rr) -> double {
    const int64_t gi = gi0 + rr;
    if (gi >= grad_member_n<RAG>(g, b) || gj > gi) return 0.0;
    const double qq = -(double)W[(g.n_pad + gi) * g.ld + g.n_pad + gj] - al_r[rr] * al_c[c];
    return gi == gj ? qq : 2.0 * qq;
  };
  double noise_acc = 0.0;  // d K / d noise = I: the diagonal of the weighted matrix
  if (ti == tj && (c & 3) == wave) noise_acc = qval(c);

  for (int qn = 0; qn < kd.n_nodes; ++qn) {
    const gpk_node nd = kd.nodes[qn];
    if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) continue;
    const uint32_t mask = g.adj_mask[qn];
    const int off = (nd.flags & GPK_NODE_ARD) ? (nd.ard_slot + 1) * slot_stride : 0;
    double acc[GNP];
#pragma unroll
    for (int k = 0; k < GNP; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int k = 0; k < ATILE / 4; ++k) {
      const int rr = wave + 4 * k;
      const double qk = qval(rr);
      if (qk == 0.0) continue;
      double adj = 1.0;
      if (mask != 0u) {
        eval_nodes<RQL>(kd, hyp_s, prow + rr * a.dp, pcol + c * a.dp, slot_stride, a.d, vals + tid);
#pragma unroll 1
        for (int q = 0; q < kd.n_nodes; ++q)
          if (mask & (1u << q)) adj *= vals[q * 256 + tid];
      }
      base_partials<RQL>(nd, hyp_s, prow + off + rr * a.dp, pcol + off + c * a.dp, a.d, qk * adj, acc);
    }
    // hyperparameter slots of this node (node_params): ARD l_0..l_{d-1} then sg (stored at acc[GPK_MAX_DIM])
    const bool ard = (nd.flags & GPK_NODE_ARD) != 0;
    const bool vec = ard || nd.op == GPK_OP_LIN;  // d vector entries (ARD l, LIN c), then sg
    const bool win = nd.op == GPK_OP_CPW;         // its one or two bounds, no sg
    const bool scaled = (nd.flags & GPK_NODE_SCALED) != 0;
    const bool sg_moved = vec && scaled;
    const int np = node_params(nd, a.d);
#pragma unroll
    for (int k = 0; k < GNP; ++k) {
      if (k < np) {
        const double sres = wave_sum((sg_moved && k == a.d) ? acc[GPK_MAX_DIM] : acc[k]);
        if (lane == 0) red[wave * (GNP + 1) + k] = sres;
      }
    }
    __syncthreads();
    if (win) {
      // adjacent window leaves share a bound's slot (cp_i: upper bound of window i, lower bound of window i + 1): the
      // later leaf adds to what the earlier one wrote.  Thread s owns slot s for every window leaf, so the sum is
      // that thread's own read-modify-write in program order (deterministic)
      const int k = tid - nd.hyp_offset;
      if (k >= 0 && k < np) {
        const double sres = red[k] + red[(GNP + 1) + k] + red[2 * (GNP + 1) + k] + red[3 * (GNP + 1) + k];
        part[tid] = cp_slot_written(kd, qn, tid) ? part[tid] + sres : sres;
      }
    } else if (tid < np) {
      part[nd.hyp_offset + tid] = red[tid] + red[(GNP + 1) + tid] + red[2 * (GNP + 1) + tid] +
                                  red[3 * (GNP + 1) + tid];
    }
    __syncthreads();
  }
  const double ns = wave_sum(noise_acc);
  if (lane == 0) red[wave * (GNP + 1) + GNP] = ns;
  __syncthreads();
  if (tid == 0)
    part[kd.n_hyp] = red[GNP] + red[(GNP + 1) + GNP] + red[2 * (GNP + 1) + GNP] + red[3 * (GNP + 1) + GNP];
}

// grad[b][p] = 1/2 sum over tiles (fixed order); NaN where the factorisation failed
__global__ __launch_bounds__(256) void grad_reduce_kernel(GradArgs g, int64_t ntri, int np1) {
  __shared__ double red[256];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const double* part = g.part + (int64_t)b * ntri * np1 + p;
  double s = 0.0;
  for (int64_t t = tid; t < ntri; t += 256) s += part[t * np1];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) g.grad[(int64_t)b * np1 + p] = g.info[b] != 0 ? NAN : 0.5 * red[0];
}

// ===================================================================== kernel-matrix reverse mode
// gpk_kernel_vjp: for a weight matrix G [n, m] (the adjoint of K(X, Z) = kernel(X, Z), as TensorFlow's
// tape would hand it back from the ops downstream of get_tf_tensor), the hyperparameter adjoints
// sum_ij G_ij dK_ij / d theta_p and the adjoints of the SECOND argument's points, sum_i G_ij dK_ij / d z_jk
// (the inducing inputs of the Nystroem metrics, Optimizer/Fitter.py:76-87,128-130).  A symmetric K(Z, Z)
// is handled by the caller with G + G^T (k(a, b) = k(b, a)).  Derivatives are the analytic ones of the
// reference formulas; at coincident points the distance terms differentiate to 0 (tf.abs' sign(0)
// = 0 for the L1 kernels; for SE the reference's sqrt-then-square, Auxiliary/Distances.py:5-7, would
// give TensorFlow's 0 * inf = NaN there -- the analytic limit 0 is returned instead).

// acc_z[k] += coef * d k_node(a, b) / d b_k in the node's own coordinates (ARD nodes: scaled points)
template <bool RQL>
__device__ __forceinline__ void base_input_partials(const gpk_node& nd, const double* __restrict__ hyp,
                                                    const double* a, const double* b, int d, double coef,
                                                    double (&acc)[GPK_MAX_DIM]) {
  const int fl = nd.flags;
  const bool ard = (fl & GPK_NODE_ARD) != 0;
  const bool scaled = (fl & GPK_NODE_SCALED) != 0;
  const double* h = hyp + nd.hyp_offset;
  if (nd.op == GPK_OP_LIN) {  // d k / d b_k = sg (a_k - c_k)
    const double sg = scaled ? h[d] : 1.0;
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < d) acc[k] += coef * sg * (a[k] - h[k]);
    return;
  }
  if (nd.op == GPK_OP_CPW) {  // d (w(a) w(b)) / d b = w(a) w'(b), w'(x) = -(d w / d cp_lo + d w / d cp_hi); dimension 0
    double db[2];
    cp_window_dcp(fl, h, b[0], db);
    acc[0] -= coef * cp_window(fl, h, a[0]) * (db[0] + db[1]);
    return;
  }
  const double v = base_value<RQL>(nd, hyp, a, b, d);  // includes sg
  if (nd.op == GPK_OP_SE) {
    const double l = ard ? 1.0 : h[0];
    const double c = coef * v / (l * l);
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < d) acc[k] += c * (a[k] - b[k]);
    return;
  }
  if (RQL && nd.op == GPK_OP_RQ) {  // d k / d b_k = k (a_k - b_k) / (l^2 q), q = 1 + s / (2 a l^2): 0 at coincident points
    const double l = h[0];
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      const double t = a[k] - b[k];
      s += t * t;
    }
    const double c = coef * v / ((l * l) * (1.0 + s * rq_iu(l, h[1])));
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < d) acc[k] += c * (a[k] - b[k]);
    return;
  }
  if (nd.op == GPK_OP_PER) {
    const double l = h[0], per = h[1];
    const double c = coef * v * (-2.0 / (l * l)) * (PI / per);  // d k / d sn * d theta / d |t|
    if (fl & GPK_NODE_STANDARD) {
#pragma unroll
      for (int k = 0; k < GPK_MAX_DIM; ++k)
        if (k < d) {
          const double t = a[k] - b[k];
          const double th = PI * (fabs(t) / per);
          const double sgn = t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);
          acc[k] += c * sin(2.0 * th) * (-sgn);
        }
    } else {
      double dist = 0.0;
      for (int k = 0; k < d; ++k) dist += fabs(a[k] - b[k]);
      const double s2 = sin(2.0 * PI * (dist / per));
#pragma unroll
      for (int k = 0; k < GPK_MAX_DIM; ++k)
        if (k < d) {
          const double t = a[k] - b[k];
          const double sgn = t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0);
          acc[k] += c * s2 * (-sgn);
        }
    }
    return;
  }
  // MAT32 / MAT52: k = sg r(f), f = c dist / |l|
  const bool std_form = (fl & GPK_NODE_STANDARD) != 0;
  double dist = 0.0;
  if (std_form) {
    for (int k = 0; k < d; ++k) {
      const double t = a[k] - b[k];
      dist += t * t;
    }
    dist = sqrt(dist);
  } else {
    for (int k = 0; k < d; ++k) dist += fabs(a[k] - b[k]);
  }
  const double cc = (nd.op == GPK_OP_MAT52) ? SQRT5 : SQRT3;
  const double sg = scaled ? h[ard ? d : 1] : 1.0;
  const double l = ard ? 1.0 : fabs(h[0]);
  const double f = (cc * dist) / l;
  const double e = exp(-f);
  const double drdf = (nd.op == GPK_OP_MAT52) ? -(f / 3.0) * (1.0 + f) * e : -f * e;
  const double c = coef * sg * drdf * (cc / l);  // times d dist / d b_k
#pragma unroll
  for (int k = 0; k < GPK_MAX_DIM; ++k)
    if (k < d) {
      const double t = a[k] - b[k];
      double dd;
      if (std_form) dd = dist > 0.0 ? -t / dist : 0.0;
      else dd = -(t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0));
      acc[k] += c * dd;
    }
}

// one 64 x 64 tile of K(X, Z) per workgroup (row tile ti = blockIdx.y, column tile tj = blockIdx.x);
// lane = column, wave w = rows w, w + 4, ...; per-tile partial sums to the workspace, reduced in a
// fixed order by vjp_reduce_kernel (deterministic)
template <bool RQL>
__global__ __launch_bounds__(256) void vjp_kernel(gpk_kdesc kd, AsmArgs a, VjpArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int slot_stride = ATILE * a.dp;
  double* hyp_s = smem;                                  // GPK_MAX_HYP
  double* red = hyp_s + GPK_MAX_HYP;                     // [4 waves][GNP]
  double* zred = red + 4 * GNP;                          // [4 waves][64][d]
  double* prow = zred + 4 * ATILE * a.d;
  double* pcol = prow + (1 + kd.n_ard) * slot_stride;
  double* vals = pcol + (1 + kd.n_ard) * slot_stride;    // [n_nodes][256] node values (MUL trees)

  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < kd.n_hyp; e += 256) hyp_s[e] = g.hyp[e];
  __syncthreads();
  const int64_t gi0 = ti * ATILE, gj0 = tj * ATILE;
  stage_points(kd, a, hyp_s, prow, gi0, 0, true, slot_stride);
  stage_points(kd, a, hyp_s, pcol, gj0, 0, false, slot_stride);
  __syncthreads();
  const int c = lane;
  const int64_t gj = gj0 + c;
  double* part = g.part_h + (ti * (int64_t)gridDim.x + tj) * kd.n_hyp;
  double gz[GPK_MAX_DIM];
#pragma unroll
  for (int k = 0; k < GPK_MAX_DIM; ++k) gz[k] = 0.0;
  for (int qn = 0; qn < kd.n_nodes; ++qn) {
    const gpk_node nd = kd.nodes[qn];
    if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) continue;
    const uint32_t mask = g.adj_mask[qn];
    const bool ard = (nd.flags & GPK_NODE_ARD) != 0;
    const int off = ard ? (nd.ard_slot + 1) * slot_stride : 0;
    double acc[GNP], az[GPK_MAX_DIM];
#pragma unroll
    for (int k = 0; k < GNP; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k) az[k] = 0.0;
#pragma unroll 1
    for (int k = 0; k < ATILE / 4; ++k) {
      const int rr = wave + 4 * k;
      const int64_t gi = gi0 + rr;
      if (gi >= a.n || gj >= a.m) continue;
      const double qk = g.G ? g.G[gi * g.ldg + gj] : g.gu[gi] * g.gv[gj];
      if (qk == 0.0) continue;
      double adj = 1.0;
      if (mask != 0u) {
        eval_nodes<RQL>(kd, hyp_s, prow + rr * a.dp, pcol + c * a.dp, slot_stride, a.d, vals + tid);
#pragma unroll 1
        for (int q = 0; q < kd.n_nodes; ++q)
          if (mask & (1u << q)) adj *= vals[q * 256 + tid];
      }
      base_partials<RQL>(nd, hyp_s, prow + off + rr * a.dp, pcol + off + c * a.dp, a.d, qk * adj, acc);
      if (g.want_z) base_input_partials<RQL>(nd, hyp_s, prow + off + rr * a.dp, pcol + off + c * a.dp, a.d, qk * adj, az);
    }
    // raw coordinates: an ARD node sees z_k / l_k
#pragma unroll
    for (int k = 0; k < GPK_MAX_DIM; ++k)
      if (k < a.d) gz[k] += ard ? az[k] / hyp_s[nd.hyp_offset + k] : az[k];
    const bool vec = ard || nd.op == GPK_OP_LIN;  // d vector entries (ARD l, LIN c), then sg
    const bool win = nd.op == GPK_OP_CPW;         // its one or two bounds, no sg
    const bool scaled = (nd.flags & GPK_NODE_SCALED) != 0;
    const bool sg_moved = vec && scaled;
    const int np = node_params(nd, a.d);
#pragma unroll
    for (int k = 0; k < GNP; ++k) {
      if (k < np) {
        const double sres = wave_sum((sg_moved && k == a.d) ? acc[GPK_MAX_DIM] : acc[k]);
        if (lane == 0) red[wave * GNP + k] = sres;
      }
    }
    __syncthreads();
    if (win) {
      // a bound shared with an earlier window leaf: add (thread s owns slot s, as in grad_kernel)
      const int k = tid - nd.hyp_offset;
      if (k >= 0 && k < np) {
        const double sres = red[k] + red[GNP + k] + red[2 * GNP + k] + red[3 * GNP + k];
        part[tid] = cp_slot_written(kd, qn, tid) ? part[tid] + sres : sres;
      }
    } else if (tid < np) {
      part[nd.hyp_offset + tid] = red[tid] + red[GNP + tid] + red[2 * GNP + tid] + red[3 * GNP + tid];
    }
    __syncthreads();
  }
  if (!g.want_z) return;
  for (int k = 0; k < a.d; ++k) zred[(wave * ATILE + c) * a.d + k] = gz[k];
  __syncthreads();
  for (int e = tid; e < ATILE * a.d; e += 256) {
    const int cc = e / a.d, k = e - cc * a.d;
    if (gj0 + cc < a.m)
      g.part_z[(ti * a.m + gj0 + cc) * a.d + k] = zred[(0 * ATILE + cc) * a.d + k] + zred[(1 * ATILE + cc) * a.d + k] +
                                                   zred[(2 * ATILE + cc) * a.d + k] + zred[(3 * ATILE + cc) * a.d + k];
  }
}

// out[p] = scale * sum_t part[t * stride + p] over t < nt (fixed order); one workgroup per p
__global__ __launch_bounds__(256) void vjp_reduce_kernel(const double* part, int64_t nt, int64_t stride, double scale,
                                                         double* out) {
  __shared__ double red[256];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int64_t t = tid; t < nt; t += 256) s += part[t * stride + p];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) out[p] = scale * red[0];
}

// ================================================================================ MSE gradient
// f = (1 / m) r^T r, r = mu - y_test, mu = V z, of a factored augmented matrix with m test rows (V = K_s^T L^-T in the
// test rows, z = L^-1 y in the y row, -mu in the corner's y row).  With alpha = L^-T z and q = L^-T (V^T r):
//   d f / d theta = (2 / m) [ sum_it alpha_i r_t d k(x_i, x*_t) / d theta - sum_ij q_i alpha_j d k(x_i, x_j) / d theta ],
//   d f / d noise = -(2 / m) q^T alpha
// -- both weights rank one, K^-1 never formed.  mse_residual_kernel computes r, f and the two right-hand
// sides; the batched backward solve gives q and alpha; mse_tile_kernel sums the weighted partials per tile;
// mse_reduce_kernel adds the tiles in a fixed order.

// r_b, sum r^2 and the right-hand sides c = V^T r, z of member b: workgroup x takes 256 columns j, re-reads r in chunks
// of 256 test rows (LDS) and accumulates c_j down the test rows in row order; workgroup 0 also writes r and the value
template <bool RAG>
__global__ __launch_bounds__(256) void mse_residual_kernel(MseArgs g) {
  __shared__ double rs[256];
  __shared__ double red[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + tid;
  int64_t nn = g.n, mm = g.m;
  if constexpr (RAG) {
    nn = g.nb[b];
    mm = g.mb[b];
  }
  const double* W = g.W + (int64_t)b * g.w_bs;
  const double* ys = g.ys + (int64_t)b * g.ys_bs;
  double cj = 0.0, sq = 0.0;
  for (int64_t t0 = 0; t0 < g.m; t0 += 256) {  // (the layout's m: workgroup-uniform trip count)
    const int64_t tt = t0 + tid;
    const double r = tt < mm ? -W[g.y_row * g.ld + g.n_pad + tt] - ys[tt] : 0.0;  // the corner's y row holds -mu
    rs[tid] = r;
    sq += r * r;
    if (blockIdx.x == 0 && tt < g.m) g.res[(int64_t)b * g.m + tt] = r;
    __syncthreads();
    const int kn = (int)((mm - t0) < 256 ? (mm - t0) : 256);
    if (j < nn)
      for (int k = 0; k < kn; ++k) cj = fma(W[(g.n_pad + t0 + k) * g.ld + j], rs[k], cj);
    __syncthreads();
  }
  if (j < g.n_pad) {
    double* rhs = g.rhs + (int64_t)b * 2 * g.n_pad;
    rhs[j] = j < nn ? cj : 0.0;
    rhs[g.n_pad + j] = j < nn ? W[g.y_row * g.ld + j] : 0.0;
  }
  if (blockIdx.x != 0) return;
  red[tid] = sq;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    g.out[b * 4 + 0] = g.info[b] != 0 ? INFINITY : red[0] / (double)mm;
    g.out[b * 4 + 1] = red[0];
    g.out[b * 4 + 2] = (double)mm;
    g.out[b * 4 + 3] = (double)nn;
  }
}

// One 64 x 64 tile per workgroup: tiles t < ntr (ntr + 1) / 2 are the lower TRAIN x TRAIN tiles (weight
// -(q_i alpha_j + q_j alpha_i) strictly below the diagonal, -q_i alpha_i on it -- whose sum is also the noise partial
// -- 0 above), the nte * ntr tiles after them TEST x TRAIN (weight r_t alpha_j; rows = test points).  The q, alpha and r
// slices of the tile's edges are staged in LDS once; no matrix is read.  RAG: member b's own n_b / m_b bound the
// staging, and a tile wholly in padding writes plain zeros for its n_hyp + 1 partials and evaluates nothing (as
// grad_kernel<.., RAG>).  The leaf loop is grad_kernel's, in the same words (see the top of this file).
template <bool RQL, bool RAG>
__global__ __launch_bounds__(256) void mse_tile_kernel(gpk_kdesc kd, AsmArgs a, MseArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int slot_stride = ATILE * a.dp;
  double* hyp_s = smem;                                  // GPK_MAX_HYP
  double* q_r = hyp_s + GPK_MAX_HYP;                     // q (TEST rows: r) of the tile rows
  double* al_r = q_r + ATILE;                            // alpha of the tile rows (TEST rows: unused)
  double* q_c = al_r + ATILE;                            // q, alpha of the tile columns
  double* al_c = q_c + ATILE;
  double* red = al_c + ATILE;                            // [4 waves][GNP + 1]
  double* prow = red + 4 * (GNP + 1);
  double* pcol = prow + (1 + kd.n_ard) * slot_stride;
  double* vals = pcol + (1 + kd.n_ard) * slot_stride;   // [n_nodes][256] node values (MUL trees)

  const int b = blockIdx.y;
  const int64_t t = blockIdx.x;
  const int64_t ntri = g.ntr * (g.ntr + 1) / 2;
  const bool test = t >= ntri;
  int64_t ti, tj;
  if (test) {
    ti = (t - ntri) / g.ntr;
    tj = (t - ntri) - ti * g.ntr;
  } else {
    int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    ti = r;
    tj = t - r * (r + 1) / 2;
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int np1 = kd.n_hyp + 1;
  double* part = g.part + ((int64_t)b * gridDim.x + t) * np1;
  int64_t nn = g.n, mm = g.m;
  if constexpr (RAG) {
    nn = g.nb[b];
    mm = g.mb[b];
    // (workgroup-uniform) rows or columns wholly past the member's points: every weight is zero
    if (test ? (ti * ATILE >= mm || tj * ATILE >= nn) : (ti * ATILE >= nn)) {
      for (int e = tid; e < np1; e += 256) part[e] = 0.0;
      return;
    }
  }
  const double* hyp_g = g.hyp + (int64_t)b * g.hyp_stride;
  for (int e = tid; e < kd.n_hyp; e += 256) hyp_s[e] = hyp_g[e];
  const int64_t gi0 = test ? g.n_pad + ti * ATILE : ti * ATILE, gj0 = tj * ATILE;
  if (tid < 2 * ATILE) {
    const int e = tid & (ATILE - 1);
    const double* rhs = g.rhs + (int64_t)b * 2 * g.n_pad;
    if (tid < ATILE && test) {
      const int64_t tt = ti * ATILE + e;
      q_r[e] = tt < mm ? g.res[(int64_t)b * g.m + tt] : 0.0;
      al_r[e] = 0.0;
    } else {
      const int64_t gg = (tid < ATILE ? gi0 : gj0) + e;
      const bool in = gg < nn;
      (tid < ATILE ? q_r : q_c)[e] = in ? rhs[gg] : 0.0;
      (tid < ATILE ? al_r : al_c)[e] = in ? rhs[g.n_pad + gg] : 0.0;
    }
  }
  __syncthreads();
  stage_points(kd, a, hyp_s, prow, gi0, b, true, slot_stride);
  stage_points(kd, a, hyp_s, pcol, gj0, b, false, slot_stride);
  __syncthreads();

  const int c = lane;
  const int64_t gj = gj0 + c;
  // weight of this thread's element in tile row rr (the strictly lower triangle stands for both halves)
  auto qval = [&](int rr) -> double {
    if (test) return q_r[rr] * al_c[c];
    const int64_t gi = gi0 + rr;
    if (gi >= nn || gj > gi) return 0.0;
    const double qq = q_r[rr] * al_c[c];
    return gi == gj ? -qq : -(qq + q_c[c] * al_r[rr]);
  };
  double noise_acc = 0.0;  // d K / d noise = I: the diagonal of the weighted matrix
  if (!test && ti == tj && (c & 3) == wave) noise_acc = qval(c);

  for (int qn = 0; qn < kd.n_nodes; ++qn) {
    const gpk_node nd = kd.nodes[qn];
    if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) continue;
    const uint32_t mask = g.adj_mask[qn];
    const int off = (nd.flags & GPK_NODE_ARD) ? (nd.ard_slot + 1) * slot_stride : 0;
    double acc[GNP];
#pragma unroll
    for (int k = 0; k < GNP; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int k = 0; k < ATILE / 4; ++k) {
      const int rr = wave + 4 * k;
      const double qk = qval(rr);
      if (qk == 0.0) continue;
      double adj = 1.0;
      if (mask != 0u) {
        eval_nodes<RQL>(kd, hyp_s, prow + rr * a.dp, pcol + c * a.dp, slot_stride, a.d, vals + tid);
#pragma unroll 1
        for (int q = 0; q < kd.n_nodes; ++q)
          if (mask & (1u << q)) adj *= vals[q * 256 + tid];
      }
      base_partials<RQL>(nd, hyp_s, prow + off + rr * a.dp, pcol + off + c * a.dp, a.d, qk * adj, acc);
    }
    // hyperparameter slots of this node (node_params): ARD l_0..l_{d-1} then sg (stored at acc[GPK_MAX_DIM])
    const bool ard = (nd.flags & GPK_NODE_ARD) != 0;
    const bool vec = ard || nd.op == GPK_OP_LIN;  // d vector entries (ARD l, LIN c), then sg
    const bool win = nd.op == GPK_OP_CPW;         // its one or two bounds, no sg
    const bool scaled = (nd.flags & GPK_NODE_SCALED) != 0;
    const bool sg_moved = vec && scaled;
    const int np = node_params(nd, a.d);
#pragma unroll
    for (int k = 0; k < GNP; ++k) {
      if (k < np) {
        const double sres = wave_sum((sg_moved && k == a.d) ? acc[GPK_MAX_DIM] : acc[k]);
        if (lane == 0) red[wave * (GNP + 1) + k] = sres;
      }
    }
    __syncthreads();
    if (win) {
      // adjacent window leaves share a bound's slot (cp_i: upper bound of window i, lower bound of window i + 1): the
      // later leaf adds to what the earlier one wrote.  Thread s owns slot s for every window leaf, so the sum is
      // that thread's own read-modify-write in program order (deterministic)
      const int k = tid - nd.hyp_offset;
      if (k >= 0 && k < np) {
        const double sres = red[k] + red[(GNP + 1) + k] + red[2 * (GNP + 1) + k] + red[3 * (GNP + 1) + k];
        part[tid] = cp_slot_written(kd, qn, tid) ? part[tid] + sres : sres;
      }
    } else if (tid < np) {
      part[nd.hyp_offset + tid] = red[tid] + red[(GNP + 1) + tid] + red[2 * (GNP + 1) + tid] +
                                  red[3 * (GNP + 1) + tid];
    }
    __syncthreads();
  }
  const double ns = wave_sum(noise_acc);
  if (lane == 0) red[wave * (GNP + 1) + GNP] = ns;
  __syncthreads();
  if (tid == 0)
    part[kd.n_hyp] = red[GNP] + red[(GNP + 1) + GNP] + red[2 * (GNP + 1) + GNP] + red[3 * (GNP + 1) + GNP];
}

// grad[b][p] = (2 / m_b) sum over tiles (fixed order); NaN where the factorisation failed
__global__ __launch_bounds__(256) void mse_reduce_kernel(MseArgs g, int64_t ntile, int np1) {
  __shared__ double red[256];
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const double* part = g.part + (int64_t)b * ntile * np1 + p;
  double s = 0.0;
  for (int64_t t = tid; t < ntile; t += 256) s += part[t * np1];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double mm = (double)(g.mb ? g.mb[b] : g.m);
    g.grad[(int64_t)b * np1 + p] = g.info[b] != 0 ? NAN : (2.0 / mm) * red[0];
  }
}

// ================================================================================ derivative matrices
// gpk_kernel_jacobian: the planes J[b][p][i][j] = d k(x_i, z_j) / d theta_p of K(X, Z), written instead of reduced.  One
// 64 x 64 tile per workgroup (column tile blockIdx.x, row tile blockIdx.y, member blockIdx.z), staged as vjp_kernel
// stages its tiles (rectangular, plain); lane = column, wave w = rows w, w + 4, ..., so a wave stores 64 consecutive
// doubles of one row of a plane.  Per element the node values are evaluated once (programs with products), then every
// leaf's base_partials runs with coef = its adjoint product over adj_mask and a zeroed acc, and the leaf's node_params
// slots are stored to their planes (acc[GPK_MAX_DIM]: a moved sg, as in grad_kernel).  A bound shared by two adjacent
// window leaves receives both contributions: the thread that owns the element adds the later leaf's to what it stored
// for the earlier one (its own read-modify-write in program order: deterministic).  Every element of every plane of a
// valid program is written, structural zeros included.  a0.uplo: tiles above the diagonal are skipped (gpk_fisher builds
// the lower tiles of the symmetric X-against-X planes and mirrors them).  No reduction, no atomics.
template <bool RQL>
__global__ __launch_bounds__(256) void jacobian_kernel(gpk_kdesc kd, AsmArgs a0, JacArgs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int64_t ti = blockIdx.y, tj = blockIdx.x;
  if (a0.uplo && tj > ti) return;  // (workgroup-uniform)
  const int b = blockIdx.z;
  AsmArgs a = a0;
  a.X = a0.X + (int64_t)b * a0.x_bs;
  a.Xs = a0.Xs + (int64_t)b * a0.xs_bs;
  const int slot_stride = ATILE * a.dp;
  double* hyp_s = smem;                                  // GPK_MAX_HYP
  double* prow = hyp_s + GPK_MAX_HYP;
  double* pcol = prow + (1 + kd.n_ard) * slot_stride;
  double* vals = pcol + (1 + kd.n_ard) * slot_stride;    // [n_nodes][256] node values (MUL trees)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const double* hyp_g = g.hyp + (int64_t)b * g.hyp_stride;
  for (int e = tid; e < kd.n_hyp; e += 256) hyp_s[e] = hyp_g[e];
  __syncthreads();
  const int64_t gi0 = ti * ATILE, gj0 = tj * ATILE;
  stage_points(kd, a, hyp_s, prow, gi0, 0, true, slot_stride);
  stage_points(kd, a, hyp_s, pcol, gj0, 0, false, slot_stride);
  __syncthreads();
  const int c = lane;
  const int64_t gj = gj0 + c;
  if (gj >= a.m) return;  // (no barrier below)
  double* J = g.J + (int64_t)b * g.j_bs;
#pragma unroll 1
  for (int k = 0; k < ATILE / 4; ++k) {
    const int rr = wave + 4 * k;
    const int64_t gi = gi0 + rr;
    if (gi >= a.n) break;
    if (g.has_mul) eval_nodes<RQL>(kd, hyp_s, prow + rr * a.dp, pcol + c * a.dp, slot_stride, a.d, vals + tid);
    double* Je = J + gi * g.ldj + gj;
#pragma unroll 1
    for (int qn = 0; qn < kd.n_nodes; ++qn) {
      const gpk_node nd = kd.nodes[qn];
      if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) continue;
      const uint32_t mask = g.adj_mask[qn];
      const int off = (nd.flags & GPK_NODE_ARD) ? (nd.ard_slot + 1) * slot_stride : 0;
      double adj = 1.0;
      if (mask != 0u) {
#pragma unroll 1
        for (int q = 0; q < kd.n_nodes; ++q)
          if (mask & (1u << q)) adj *= vals[q * 256 + tid];
      }
      double acc[GNP];
#pragma unroll
      for (int s = 0; s < GNP; ++s) acc[s] = 0.0;
      base_partials<RQL>(nd, hyp_s, prow + off + rr * a.dp, pcol + off + c * a.dp, a.d, adj, acc);
      // hyperparameter slots of this node (node_params): ARD l_0..l_{d-1} then sg (stored at acc[GPK_MAX_DIM])
      const bool vec = (nd.flags & GPK_NODE_ARD) != 0 || nd.op == GPK_OP_LIN;
      const bool win = nd.op == GPK_OP_CPW;
      const bool sg_moved = vec && (nd.flags & GPK_NODE_SCALED) != 0;
      const int np = node_params(nd, a.d);
#pragma unroll
      for (int s = 0; s < GNP; ++s) {
        if (s < np) {
          const double v = (sg_moved && s == a.d) ? acc[GPK_MAX_DIM] : acc[s];
          double* dst = Je + (int64_t)(nd.hyp_offset + s) * g.plane_stride;
          // a bound shared with an earlier window leaf: add to what this thread stored for it
          *dst = (win && cp_slot_written(kd, qn, nd.hyp_offset + s)) ? *dst + v : v;
        }
      }
    }
  }
}

}  // namespace

int64_t mse_tiles(int64_t n, int64_t m) {
  const int64_t ntr = (n + ATILE - 1) / ATILE, nte = (m + ATILE - 1) / ATILE;
  return ntr * (ntr + 1) / 2 + nte * ntr;
}

hipError_t launch_mse_residual(const MseArgs& g, int32_t batch, hipStream_t s) {
  dim3 grid((unsigned)((g.n_pad + 255) / 256), (unsigned)batch);
  if (g.nb != nullptr)
    hipLaunchKernelGGL(mse_residual_kernel<true>, grid, dim3(256), 0, s, g);
  else
    hipLaunchKernelGGL(mse_residual_kernel<false>, grid, dim3(256), 0, s, g);
  return hipGetLastError();
}

// ---- host side of the two tile passes (grad_kernel, mse_tile_kernel): one statement of what they share
// the AsmArgs the staging helpers (stage_points) read the points through, an augmented layout: the fields GradArgs and
// MseArgs both carry, m extra rows, and -- ragged (nb / mb NULL: uniform) -- the members' own counts, which bound
// the points stage_points reads (member_n / member_m)
template <class G>
static AsmArgs stage_args(const G& g, int64_t m, const int64_t* mb) {
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = g.hyp;
  a.hyp_stride = g.hyp_stride;
  a.X = g.X;
  a.x_bs = g.x_bs;
  a.n = g.n;
  a.m = m;
  a.n_pad = g.n_pad;
  a.y_row = g.y_row;
  a.d = g.d;
  a.dp = g.dp;
  a.nb = g.nb;
  a.mb = mb;
  return a;
}

// dynamic LDS of a tile pass: the hyperparameters, row_vectors 64-vectors of weights (grad_kernel 2, mse_tile_kernel
// 4), the reduction scratch, the two edges' staged points and -- programs with products -- every node's values
static size_t tile_lds_bytes(const gpk_kdesc& kd, const uint32_t* adj_mask, int32_t dp, int row_vectors) {
  bool has_mul = false;
  for (int q = 0; q < kd.n_nodes; ++q) has_mul |= adj_mask[q] != 0u;
  return sizeof(double) * (GPK_MAX_HYP + (size_t)row_vectors * ATILE + 4 * (GNP + 1) +
                           2 * (size_t)(1 + kd.n_ard) * ATILE * dp + (has_mul ? (size_t)kd.n_nodes * 256 : 0));
}

// the tile kernel over ntile x batch workgroups, then its reduction of the per-tile partial sums (fixed order)
template <class Tile, class Reduce, class G>
static hipError_t launch_tiles_then_reduce(Tile tile, Reduce reduce, const gpk_kdesc& kd, const AsmArgs& a, const G& g,
                                           int64_t ntile, size_t lds, int32_t batch, hipStream_t s) {
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(tile), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tile, dim3((unsigned)ntile, (unsigned)batch, 1), dim3(256), lds, s, kd, a, g);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(reduce, dim3((unsigned)(kd.n_hyp + 1), (unsigned)batch), dim3(256), 0, s, g, ntile,
                     kd.n_hyp + 1);
  return hipGetLastError();
}

hipError_t launch_mse_tiles(const gpk_kdesc& kd, const MseArgs& g, int32_t batch, hipStream_t s) {
  AsmArgs a = stage_args(g, g.m, g.mb);  // (test rows from Xs)
  a.Xs = g.Xs;
  a.xs_bs = g.xs_bs;
  // (a program with a rational quadratic leaf: the instantiation that carries the leaf's code, rq_leaves)
  const bool rq = rq_leaves(kd) > 0;
  const auto tile = g.nb != nullptr ? (rq ? mse_tile_kernel<true, true> : mse_tile_kernel<false, true>)
                                    : (rq ? mse_tile_kernel<true, false> : mse_tile_kernel<false, false>);
  return launch_tiles_then_reduce(tile, mse_reduce_kernel, kd, a, g, g.ntr * (g.ntr + 1) / 2 + g.nte * g.ntr,
                                  tile_lds_bytes(kd, g.adj_mask, g.dp, 4), batch, s);
}

size_t vjp_workspace_elems(const gpk_kdesc& kd, int64_t n, int64_t m, int32_t d, bool want_z) {
  const int64_t tr = (n + ATILE - 1) / ATILE, tc = (m + ATILE - 1) / ATILE;
  return (size_t)(tr * tc * kd.n_hyp) + (want_z ? (size_t)(tr * m * d) : 0);
}

hipError_t launch_vjp(const gpk_kdesc& kd, const VjpArgs& g0, const double* X, int64_t n, const double* Z, int64_t m,
                      int32_t d, double* grad_hyp, double* grad_z, hipStream_t s) {
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = g0.hyp;
  a.X = X;
  a.Xs = Z;
  a.n = n;
  a.m = m;
  a.d = d;
  a.dp = padded_dim(d);
  a.plain = 1;
  VjpArgs g = g0;
  g.want_z = grad_z != nullptr ? 1 : 0;
  const int64_t tr = (n + ATILE - 1) / ATILE, tc = (m + ATILE - 1) / ATILE;
  g.part_z = g.part_h + tr * tc * kd.n_hyp;
  bool has_mul = false;
  for (int q = 0; q < kd.n_nodes; ++q) has_mul |= g.adj_mask[q] != 0u;
  const size_t lds = sizeof(double) * (GPK_MAX_HYP + 4 * GNP + 4 * (size_t)ATILE * d +
                                       2 * (size_t)(1 + kd.n_ard) * ATILE * a.dp +
                                       (has_mul ? (size_t)kd.n_nodes * 256 : 0));
  // (a program with a rational quadratic leaf: the instantiation that carries the leaf's code, rq_leaves)
  const auto vjp = rq_leaves(kd) > 0 ? vjp_kernel<true> : vjp_kernel<false>;
  {
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(vjp), lds);  // (d = 16, two ARD nodes: 118 KB)
    if (e != hipSuccess) return e;
  }
  if (kd.n_hyp > 0) {
    hipLaunchKernelGGL(vjp, dim3((unsigned)tc, (unsigned)tr), dim3(256), lds, s, kd, a, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vjp_reduce_kernel, dim3((unsigned)kd.n_hyp), dim3(256), 0, s, g.part_h, tr * tc,
                       (int64_t)kd.n_hyp, 1.0, grad_hyp);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  } else if (g.want_z) {
    hipLaunchKernelGGL(vjp, dim3((unsigned)tc, (unsigned)tr), dim3(256), lds, s, kd, a, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (g.want_z) {
    hipLaunchKernelGGL(vjp_reduce_kernel, dim3((unsigned)(m * d)), dim3(256), 0, s, g.part_z, tr, m * (int64_t)d, 1.0,
                       grad_z);
    return hipGetLastError();
  }
  return hipSuccess;
}

// grad_kernel over the points of ``pts`` (its n, n_pad, y_row: the real layout; m_b = n_b) with the weights g addresses
static hipError_t launch_grad_tiles(const gpk_kdesc& kd, const GradArgs& pts, const GradArgs& g, int dtype,
                                    int32_t batch, hipStream_t s) {
  AsmArgs a = stage_args(pts, pts.n, pts.nb);
  a.eye = 1;
  // (a program with a rational quadratic leaf: the instantiation that carries the leaf's code, rq_leaves)
  const bool rq = rq_leaves(kd) > 0;
  const auto grad =
      g.nb != nullptr
          ? (dtype == GPK_F64 ? (rq ? grad_kernel<double, true, true> : grad_kernel<double, false, true>)
                              : (rq ? grad_kernel<float, true, true> : grad_kernel<float, false, true>))
          : (dtype == GPK_F64 ? (rq ? grad_kernel<double, true> : grad_kernel<double, false>)
                              : (rq ? grad_kernel<float, true> : grad_kernel<float, false>));
  return launch_tiles_then_reduce(grad, grad_reduce_kernel, kd, a, g, g.ntile * (g.ntile + 1) / 2,
                                  tile_lds_bytes(kd, g.adj_mask, g.dp, 2), batch, s);
}

hipError_t launch_grad(const gpk_kdesc& kd, const GradArgs& g, int dtype, int32_t batch, hipStream_t s) {
  return launch_grad_tiles(kd, g, g, dtype, batch, s);
}

// launch_grad with the weights read from a cotangent buffer (gpk_loo_backward): the AsmArgs that stage_points reads
// carry g0's real layout, the GradArgs fields that address the corner and its y row (g.W, g.ld, g.w_bs, g.n_pad,
// g.y_row: grad_kernel uses them for nothing else) carry the buffer's.  The kernels are launch_grad's f64 ones.
hipError_t launch_grad_cot(const gpk_kdesc& kd, const GradArgs& g0, const double* C, int64_t c_ld, int64_t c_bs,
                           int64_t c_yrow, int32_t batch, hipStream_t s) {
  GradArgs g = g0;
  g.W = C;
  g.ld = c_ld;
  g.w_bs = c_bs;
  g.n_pad = 0;
  g.y_row = c_yrow;
  return launch_grad_tiles(kd, g0, g, GPK_F64, batch, s);
}

hipError_t launch_jacobian(const gpk_kdesc& kd, const JacArgs& g0, const double* X, int64_t x_bs, int64_t n,
                           const double* Z, int64_t z_bs, int64_t m, int32_t d, int32_t lower_tiles, int32_t batch,
                           hipStream_t s) {
  if (kd.n_hyp == 0 || batch == 0) return hipSuccess;
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.X = X;
  a.x_bs = x_bs;
  a.Xs = Z;
  a.xs_bs = z_bs;
  a.n = n;
  a.m = m;
  a.d = d;
  a.dp = padded_dim(d);
  a.plain = 1;
  a.uplo = lower_tiles;
  JacArgs g = g0;
  g.has_mul = 0;
  for (int q = 0; q < kd.n_nodes; ++q) g.has_mul |= g.adj_mask[q] != 0u ? 1 : 0;
  const int64_t tr = (n + ATILE - 1) / ATILE, tc = (m + ATILE - 1) / ATILE;
  const size_t lds = sizeof(double) * (GPK_MAX_HYP + 2 * (size_t)(1 + kd.n_ard) * ATILE * a.dp +
                                       (g.has_mul ? (size_t)kd.n_nodes * 256 : 0));
  // (a program with a rational quadratic leaf: the instantiation that carries the leaf's code, rq_leaves)
  const auto jac = rq_leaves(kd) > 0 ? jacobian_kernel<true> : jacobian_kernel<false>;
  hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(jac), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jac, dim3((unsigned)tc, (unsigned)tr, (unsigned)batch), dim3(256), lds, s, kd, a, g);
  return hipGetLastError();
}

}  // namespace gpk
