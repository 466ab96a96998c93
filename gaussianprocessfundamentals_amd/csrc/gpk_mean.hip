// Mean-function programs (include/gpk.h, "mean-function programs"): the value / detrending kernel and the
// reverse-mode kernels of gpk_mean_eval and gpk_mean_vjp, gfx950.
//
// One thread per point, GPK_MEAN_POINTS_PER_WG points per workgroup.  The workgroup stages the program, the
// member's hyperparameters and its points in LDS once (coalesced loads; a point's row stride is odd, so the 32
// lanes of a ds_read_b64 half land on 32 different bank pairs).  The evaluation stack and the node values live in
// registers: the program counter and the stack pointer are wave-uniform, so the switch-indexed register files
// below lower to scalar branches (no scratch).
//
// Contraction is off for the whole file: m is the same bits in the value kernel, the detrending form (y - m must
// not fuse with a MUL node's product) and the reverse mode's forward pass; the sums that are meant to be fused say
// fma().
#pragma clang fp contract(off)

#include "gpk_internal.h"

namespace gpk {

namespace {

constexpr int MPW = GPK_MEAN_POINTS_PER_WG;
constexpr int MWAVES = MPW / 64;
static_assert(MPW % 64 == 0 && MPW >= GPK_MAX_HYP && MPW >= GPK_MAX_NODES, "staging loops assume it");

struct Reg8 {
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

struct Reg16 {
  Reg8 lo, hi;
  __device__ __forceinline__ double get(int i) const { return i < 8 ? lo.get(i) : hi.get(i - 8); }
  __device__ __forceinline__ void set(int i, double v) {
    if (i < 8) lo.set(i, v); else hi.set(i - 8, v);
  }
};

// what a workgroup stages besides its points
struct MeanLds {
  double hyp[GPK_MAX_HYP];
  double red[MWAVES][GPK_MAX_HYP];  // reverse mode: per-wave partial sums
  int32_t op[GPK_MAX_NODES];
  int32_t off[GPK_MAX_NODES];
  int32_t lhs[GPK_MAX_NODES];
  int32_t rhs[GPK_MAX_NODES];
};

__device__ __forceinline__ bool is_binary(int op) { return op == GPK_MOP_ADD || op == GPK_MOP_MUL; }

// s = sum_k (a_k x_k - b_k), k ascending
__device__ __forceinline__ double affine_sum(const double* h, const double* x, int d) {
  double s = 0.0;
  for (int k = 0; k < d; ++k) s += fma(h[k], x[k], -h[d + k]);
  return s;
}

__device__ __forceinline__ double leaf_value(int op, const double* h, const double* x, int d) {
  switch (op) {
    case GPK_MOP_C:
      return h[0];
    case GPK_MOP_LIN: {
      double s = 0.0;
      for (int k = 0; k < d; ++k) s = fma(h[k], x[k], s);
      return s;
    }
    case GPK_MOP_EXP:
      return pow(h[2 * d], affine_sum(h, x, d));
    default:  // GPK_MOP_LOGIT
      return h[2 * d] / (1.0 + exp(affine_sum(h, x, d)));
  }
}

// forward pass of the postfix program; REC: vals receives the value every node pushed
template <bool REC>
__device__ __forceinline__ double forward(const MeanLds& L, int n_nodes, int d, const double* x, Reg16& vals) {
  Reg8 st;
  int sp = 0;
  for (int q = 0; q < n_nodes; ++q) {
    const int op = L.op[q];
    double v;
    if (is_binary(op)) {
      const double top = st.get(sp - 1);
      const double below = st.get(sp - 2);
      v = op == GPK_MOP_ADD ? below + top : below * top;
      sp -= 2;
    } else {
      v = leaf_value(op, L.hyp + L.off[q], x, d);
    }
    st.set(sp, v);
    sp += 1;
    if (REC) vals.set(q, v);
  }
  return st.get(0);
}

// program, hyperparameters and the workgroup's points -> LDS (rows past cnt: zeros)
__device__ __forceinline__ void stage(const MeanArgs& a, MeanLds& L, double* xs, int64_t b, int64_t i0, int cnt) {
  const int tid = threadIdx.x;
  const int d = a.d, dp = a.d | 1;
  if (tid < a.n_nodes) {
    L.op[tid] = a.op[tid];
    L.off[tid] = a.off[tid];
    L.lhs[tid] = a.lhs[tid];
    L.rhs[tid] = a.rhs[tid];
  }
  if (tid < a.n_hyp) L.hyp[tid] = a.hyp[b * a.hyp_stride + tid];
  const double* xb = a.X + b * a.x_bs + i0 * d;
  for (int idx = tid; idx < MPW * d; idx += MPW) {
    const int row = idx / d, k = idx - row * d;
    xs[row * dp + k] = row < cnt ? xb[idx] : 0.0;
  }
  __syncthreads();
}

__global__ __launch_bounds__(MPW) void mean_eval_kernel(MeanArgs a) {
  __shared__ MeanLds L;
  extern __shared__ double xs[];
  const int64_t b = blockIdx.x / a.nblk;
  const int64_t i0 = (blockIdx.x - b * a.nblk) * MPW;
  const int cnt = (int)(a.n - i0 < MPW ? a.n - i0 : MPW);
  stage(a, L, xs, b, i0, cnt);
  const int tid = threadIdx.x;
  if (tid >= cnt) return;
  Reg16 unused;
  const double m = forward<false>(L, a.n_nodes, a.d, xs + tid * (a.d | 1), unused);
  const int64_t i = i0 + tid;
  a.out[b * a.out_bs + i] = a.y ? a.y[b * a.y_bs + i] - m : m;
}

// sum over the wave in a fixed tree, the result in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(MPW) void mean_vjp_kernel(MeanArgs a) {
  __shared__ MeanLds L;
  extern __shared__ double xs[];
  const int64_t b = blockIdx.x / a.nblk;
  const int64_t blk = blockIdx.x - b * a.nblk;
  const int64_t i0 = blk * MPW;
  const int cnt = (int)(a.n - i0 < MPW ? a.n - i0 : MPW);
  stage(a, L, xs, b, i0, cnt);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool live = tid < cnt;
  const int d = a.d;
  const double* x = xs + tid * (d | 1);
  Reg16 vals, adj;
  forward<true>(L, a.n_nodes, d, x, vals);
  // node adjoints, seeded with the point's weight; one leaf's partials at a time
  adj.set(a.n_nodes - 1, live ? a.g[b * a.g_bs + i0 + tid] : 0.0);
  for (int q = a.n_nodes - 1; q >= 0; --q) {
    const int op = L.op[q];
    const double aq = adj.get(q);
    if (is_binary(op)) {
      const int l = L.lhs[q], r = L.rhs[q];
      if (op == GPK_MOP_ADD) {
        adj.set(l, aq);
        adj.set(r, aq);
      } else {
        const double vl = vals.get(l), vr = vals.get(r);
        adj.set(l, aq * vr);
        adj.set(r, aq * vl);
      }
      continue;
    }
    const double* h = L.hyp + L.off[q];
    double* red = L.red[wave] + L.off[q];
    if (op == GPK_MOP_C) {
      const double t = wave_sum(live ? aq : 0.0);
      if (lane == 0) red[0] = t;
    } else if (op == GPK_MOP_LIN) {
      for (int k = 0; k < d; ++k) {
        const double t = wave_sum(live ? aq * x[k] : 0.0);
        if (lane == 0) red[k] = t;
      }
    } else {
      const double m = vals.get(q);
      const double s = affine_sum(h, x, d);
      double da, dlast;  // d/da_k = da x_k, d/db_k = -da
      if (op == GPK_MOP_EXP) {
        da = m * log(h[2 * d]);
        dlast = s * pow(h[2 * d], s - 1.0);
      } else {
        da = -(m * (1.0 / (1.0 + exp(-s))));
        dlast = 1.0 / (1.0 + exp(s));
      }
      for (int k = 0; k < d; ++k) {
        const double t = wave_sum(live ? aq * (da * x[k]) : 0.0);
        if (lane == 0) red[k] = t;
      }
      const double tb = wave_sum(live ? aq * -da : 0.0);
      if (lane == 0)
        for (int k = 0; k < d; ++k) red[d + k] = tb;
      const double tl = wave_sum(live ? aq * dlast : 0.0);
      if (lane == 0) red[2 * d] = tl;
    }
  }
  __syncthreads();
  if (tid < a.n_hyp) {
    double t = L.red[0][tid];
#pragma unroll
    for (int w = 1; w < MWAVES; ++w) t += L.red[w][tid];
    a.part[((int64_t)blockIdx.x) * a.n_hyp + tid] = t;
  }
}

// grad[b][p] = the workgroups' partial sums in workgroup order
__global__ __launch_bounds__(GPK_MAX_HYP) void mean_vjp_sum_kernel(const double* part, int64_t nblk, int n_hyp,
                                                                    double* grad) {
  const int p = threadIdx.x;
  if (p >= n_hyp) return;
  const double* pb = part + (int64_t)blockIdx.x * nblk * n_hyp + p;
  double t = 0.0;
  for (int64_t k = 0; k < nblk; ++k) t += pb[k * n_hyp];
  grad[(int64_t)blockIdx.x * n_hyp + p] = t;
}

}  // namespace

int mean_leaf_hyp(int32_t op, int32_t dim) {
  switch (op) {
    case GPK_MOP_C: return 1;
    case GPK_MOP_LIN: return dim;
    case GPK_MOP_EXP: case GPK_MOP_LOGIT: return 2 * dim + 1;
    default: return -1;
  }
}

const char* mean_desc_error(const gpk_mdesc* md) {
  if (!md) return "mean descriptor (NULL)";
  if (md->dim < 1 || md->dim > GPK_MAX_DIM) return "mean descriptor: dim must be in [1, 16]";
  if (md->n_nodes < 1 || md->n_nodes > GPK_MAX_NODES) return "mean descriptor: n_nodes must be in [1, 16]";
  if (md->n_hyp < 0 || md->n_hyp > GPK_MAX_HYP) return "mean descriptor: n_hyp must be in [0, 64]";
  if (md->reserved != 0) return "mean descriptor: the reserved field must be 0";
  int sp = 0, used = 0;
  for (int q = 0; q < md->n_nodes; ++q) {
    const gpk_node& nd = md->nodes[q];
    if (nd.flags != 0) return "mean descriptor: node flags must be 0";
    if (nd.ard_slot != -1) return "mean descriptor: node ard_slot must be -1";
    if (nd.op == GPK_MOP_ADD || nd.op == GPK_MOP_MUL) {
      if (sp < 2) return "mean descriptor: stack underflow (a binary op needs two operands)";
      sp -= 1;
      continue;
    }
    const int cnt = mean_leaf_hyp(nd.op, md->dim);
    if (cnt < 0) return "mean descriptor: unknown op";
    if (nd.hyp_offset != used) return "mean descriptor: leaf hyperparameters must be consecutive (DFS order)";
    used += cnt;
    if (used > md->n_hyp) return "mean descriptor: the leaves read more than n_hyp hyperparameters";
    sp += 1;
  }
  if (sp != 1) return "mean descriptor: operands left on the stack";
  if (used != md->n_hyp) return "mean descriptor: n_hyp is not the leaves' hyperparameter count";
  return nullptr;
}

int64_t mean_blocks(int64_t n) { return (n + MPW - 1) / MPW; }

static void fill_program(const gpk_mdesc& md, MeanArgs& a) {
  a.n_nodes = md.n_nodes;
  a.n_hyp = md.n_hyp;
  a.d = md.dim;
  int st[GPK_MAX_NODES], sp = 0;
  for (int q = 0; q < md.n_nodes; ++q) {
    a.op[q] = md.nodes[q].op;
    a.off[q] = md.nodes[q].hyp_offset;
    a.lhs[q] = a.rhs[q] = 0;
    if (md.nodes[q].op == GPK_MOP_ADD || md.nodes[q].op == GPK_MOP_MUL) {
      a.rhs[q] = st[sp - 1];
      a.lhs[q] = st[sp - 2];
      sp -= 2;
    }
    st[sp++] = q;
  }
}

static size_t points_lds(int d) { return (size_t)MPW * (size_t)(d | 1) * sizeof(double); }

// (md valid, n >= 1, batch >= 1, mean_blocks(n) * batch < 2^31: checked by the callers in gpk_abi.hip)
hipError_t launch_mean_eval(const gpk_mdesc& md, MeanArgs a, int32_t batch, hipStream_t s) {
  fill_program(md, a);
  a.nblk = mean_blocks(a.n);
  hipLaunchKernelGGL(mean_eval_kernel, dim3((unsigned)(a.nblk * batch)), dim3(MPW), points_lds(a.d), s, a);
  return hipGetLastError();
}

hipError_t launch_mean_vjp(const gpk_mdesc& md, MeanArgs a, int32_t batch, double* grad, hipStream_t s) {
  fill_program(md, a);
  a.nblk = mean_blocks(a.n);
  hipLaunchKernelGGL(mean_vjp_kernel, dim3((unsigned)(a.nblk * batch)), dim3(MPW), points_lds(a.d), s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mean_vjp_sum_kernel, dim3((unsigned)batch), dim3(GPK_MAX_HYP), 0, s, a.part, a.nblk, a.n_hyp, grad);
  return hipGetLastError();
}

}  // namespace gpk
