// Posterior mean and latent variance at new points from a factored identity-augmented W (gpk_predict).
// The factorisation left R = L^-T in the extra rows (R[t][i] = (L^-1)[i][t], non-zero only for i >= t) and -alpha in
// the corner's y row.  With Ks' = k(Xs, X) [m, n], test point major:
//   mu[c]  = sum_t Ks'[c][t] alpha[t]
//   var[c] = k(xs_c, xs_c) - sum_i V'[c][i]^2,   V'[c][i] = sum_{t <= i} Ks'[c][t] R[t][i]   (V' = (L^-1 Ks)^T)
// V' is a dense-times-upper-triangular product: column block i needs the row blocks t <= i only, nothing is sequential
// (a forward substitution against L would serialise the n_pad / 128 column blocks), and only its row norms are needed.
// The test points go through the workspace in chunks of `rows`:
//   a. Ks' of the chunk [rows, n_pad] by the K build's plain launch (launch_assemble: the values of gpk_kernel_matrix
//      bit for bit), padding columns zeroed;
//   b. k(xs_c, xs_c) per test point by predict_kdiag_kernel: the point staged like a K-build tile edge (stage_points)
//      and the program evaluated by eval_tree_fast against itself -- a linear leaf gives sum (x - c)^2, a change-point
//      tree sum_i w_i(x)^2 k_i(x, x);
//   c. predict_norm_kernel: f64 MFMA 16x16x4 tiles (64 test rows x 64 training columns) of V', staged through LDS like
//      dgemm_kernel (gpk_approx.hip), the K loop over t < min(j0 + 64, n) only; the tile is never stored: it is squared
//      and each test row summed over the tile's columns -- one partial per (test row, column tile);
//   d. predict_reduce_kernel: var[c] = kdiag[c] - sum over the column tiles in index order;
//   mu by the library's gemv (gemv_kernel, one wave per test row) with alpha = -1 on the y row's -alpha.
// Of R exactly the elements i >= t, t < n, i < n are read (what _IdentityReadout.l_inv reads): the identity-row tiles
// left of the diagonal are skipped by the factorisation and hold whatever was there; rows and columns n .. n_pad - 1
// are never read.  No atomics.  Per accumulator element the k-steps come in the same order whatever row of a tile the
// test point sits in, and per row the partials are summed in the same order, so the bits of mu[c] and var[c] do not
// depend on the chunking.  fp64 only; W is only read.
#include <math.h>
#include <string.h>

#include "gpk_internal.h"
#include "gpk_kernels.h"
#include "gpk_stage.h"

namespace gpk {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------ k(xs_c, xs_c)
// One workgroup per 64 test points.  LDS (dynamic): the hyperparameters, the points' slots of one tile edge (raw, one
// per ARD node, the periodic node's sin / cos, one per window leaf -- stage_points), the nodes' constants.
__global__ __launch_bounds__(256) void predict_kdiag_kernel(gpk_kdesc kd, AsmArgs a, double* kdiag) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sc_flag;
  __shared__ unsigned long long cp_nz;
  const int slot_stride = ATILE * a.dp;
  const int scq = sc_node(kd);
  const int sc_slot = 1 + kd.n_ard;
  const int nw = cp_windows(kd);
  const int w_slot = sc_slot + (scq >= 0 ? 2 : 0);
  const int nslot = w_slot + nw;
  double* hyp_s = smem;               // GPK_MAX_HYP
  double* pts = smem + GPK_MAX_HYP;   // nslot * slot_stride
  FastNode* fns = reinterpret_cast<FastNode*>(pts + nslot * slot_stride);
  const int tid = threadIdx.x;
  for (int e = tid; e < kd.n_hyp; e += 256) hyp_s[e] = a.hyp[e];
  if (tid == 0) {
    sc_flag = 1;
    cp_nz = 0ull;
  }
  __syncthreads();
  if (tid < kd.n_nodes) {
    const gpk_node nd = kd.nodes[tid];
    if (nd.op != GPK_OP_ADD && nd.op != GPK_OP_MUL) {
      FastNode f = make_fast_node<true>(nd, hyp_s, a.d);
      f.off = (nd.flags & GPK_NODE_ARD) ? (nd.ard_slot + 1) * slot_stride : 0;
      if (nd.op == GPK_OP_CPW) {
        int kw = 0;  // its rank among the window leaves: the slot stage_points fills for it
        for (int q = 0; q < tid; ++q) kw += kd.nodes[q].op == GPK_OP_CPW ? 1 : 0;
        f.off = (w_slot + kw) * slot_stride;
      }
      if (tid == scq) {
        f.sc = 1;
        f.sc_sin = sc_slot * slot_stride;
        f.sc_cos = (sc_slot + 1) * slot_stride;
      }
      fns[tid] = f;
    }
  }
  const int64_t g0 = (int64_t)blockIdx.x * ATILE;
  const double sc_iper = scq >= 0 ? 1.0 / hyp_s[kd.nodes[scq].hyp_offset + 1] : 0.0;
  stage_points(kd, a, hyp_s, pts, g0, 0, true, slot_stride, scq >= 0 ? sc_slot : 0, sc_iper, &sc_flag,
               nw > 0 ? w_slot : 0, &cp_nz);
  __syncthreads();
  // (at distance zero the periodic leaf's two forms give the same bits: both exponents are exactly -0)
  const bool sc_on = scq >= 0 && sc_flag != 0;
  if (tid < ATILE) {  // wave 0: the program's stack pointer stays wave-uniform
    const int64_t g = g0 + tid;
    const double* p = pts + tid * a.dp;
    const double v = eval_tree_fast<true, true>(kd, fns, p, p, sc_on, 0u);
    if (g < a.n) kdiag[g] = v;
  }
}

// ------------------------------------------------------------------------------------------ row norms of V'
// dgemm_kernel's geometry (gpk_approx.hip): 64 x 64 tiles, 256 threads = 2 x 2 waves of 32 x 32 (2 x 2 MFMA blocks),
// K staged 16 at a time as [row][k] with row stride 18, the MFMA k-step s of lane group q takes k = 4 q + s for both
// operands, two LDS stages with the next chunk's global loads issued before the current chunk's MFMAs.
constexpr int PT = 64, PKC = 16, PLD = PKC + 2;

struct NormArgs {
  const double* A;   // Ks' [mc][lda], columns n .. lda - 1 zero
  int64_t lda;
  const double* R;   // the extra rows of W: R[t][i] at R + t ldr + i
  int64_t ldr;
  int64_t mc, n;
  double* part;      // [column tile][part_ld]
  int64_t part_ld;
};

struct NormStage {
  double a[4], b[4];
};

__device__ __forceinline__ void norm_fetch(const NormArgs& g, int64_t i0, int64_t j0, int64_t k0, int tid,
                                           NormStage& st) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;  // 1024 elements of each operand chunk
    const int ii = e / PKC, kk = e % PKC;
    const int64_t gi = i0 + ii, gk = k0 + kk;
    st.a[u] = (gi < g.mc && gk < g.n) ? g.A[gi * g.lda + gk] : 0.0;
    const int kb = e / PT, jj = e % PT;
    const int64_t gt = k0 + kb, gj = j0 + jj;
    // the upper triangle of R inside the training block: everything else is unwritten, padding or another row class
    st.b[u] = (gt < g.n && gj < g.n && gj >= gt) ? g.R[gt * g.ldr + gj] : 0.0;
  }
}

__device__ __forceinline__ void norm_store(int tid, const NormStage& st, double* As, double* Bs) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    As[(e / PKC) * PLD + e % PKC] = st.a[u];
    Bs[(e % PT) * PLD + e / PT] = st.b[u];
  }
}

__global__ __launch_bounds__(256) void predict_norm_kernel(NormArgs g) {
  __shared__ __attribute__((aligned(16))) double As[2][PT * PLD];
  __shared__ __attribute__((aligned(16))) double Bs[2][PT * PLD];
  __shared__ double red[2][PT];
  // (the deepest column tiles first: tile jt sums over (jt + 1) * 64 rows of R)
  const int64_t jt = (int64_t)gridDim.x - 1 - blockIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * PT, j0 = jt * PT;
  const int64_t kend = j0 + PT < g.n ? j0 + PT : g.n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, q = lane >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  NormStage st;
  norm_fetch(g, i0, j0, 0, tid, st);
  norm_store(tid, st, As[0], Bs[0]);
  __syncthreads();
  const int nk = (int)((kend + PKC - 1) / PKC);
  for (int c = 0; c < nk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nk) norm_fetch(g, i0, j0, (int64_t)(c + 1) * PKC, tid, st);
    d2 fa[2][2], fb[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const d2* src = reinterpret_cast<const d2*>(&As[cur][(wr * 32 + mi * 16 + lr) * PLD + 4 * q]);
      fa[mi][0] = src[0];
      fa[mi][1] = src[1];
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const d2* src = reinterpret_cast<const d2*>(&Bs[cur][(wc * 32 + ni * 16 + lr) * PLD + 4 * q]);
      fb[ni][0] = src[0];
      fb[ni][1] = src[1];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mi][s >> 1][s & 1], fb[ni][s >> 1][s & 1],
                                                             acc[mi][ni], 0, 0, 0);
    if (c + 1 < nk) norm_store(tid, st, As[cur ^ 1], Bs[cur ^ 1]);
    __syncthreads();
  }
  // Epilogue: the squares of a test row over the tile's 64 columns, in one order for every row -- the lane's two
  // column blocks, a butterfly over the 16 lanes of the row's lane group (every lane ends with the same sum), then the
  // two wave columns.  Accumulator register r of lane (q, lr) holds row q + 4 r, column lr of its 16 x 16 block.
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double p = acc[mi][0][r] * acc[mi][0][r];
      p = fma(acc[mi][1][r], acc[mi][1][r], p);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
      if (lr == 0) red[wc][wr * 32 + mi * 16 + q + 4 * r] = p;
    }
  __syncthreads();
  if (tid < PT) {
    const int64_t gi = i0 + tid;
    if (gi < g.mc) g.part[jt * g.part_ld + gi] = red[0][tid] + red[1][tid];
  }
}

// var[c] = kdiag[c] - sum over the column tiles, in index order
__global__ __launch_bounds__(256) void predict_reduce_kernel(const double* part, int64_t part_ld, int64_t ntc,
                                                             const double* kdiag, int64_t mc, double* var) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= mc) return;
  double s = 0.0;
  for (int64_t j = 0; j < ntc; ++j) s += part[j * part_ld + c];
  var[c] = kdiag[c] - s;
}

}  // namespace

int64_t predict_max_rows() { return (int64_t)65535 * PT; }  // (the norm kernel's grid.y)

size_t predict_workspace_elems(int64_t n, int64_t n_pad, int64_t rows) {
  const int64_t ntc = (n + PT - 1) / PT;
  return (size_t)rows * (size_t)(n_pad + 1 + ntc);
}

hipError_t launch_predict(const gpk_kdesc& kd, const PredictArgs& g, hipStream_t s) {
  const int64_t n = g.n, n_pad = g.n_pad;
  const int64_t ntc = (n + PT - 1) / PT;
  double* Ks = g.work;
  double* kdiag = Ks + g.rows * n_pad;
  double* part = kdiag + g.rows;
  const double* R = g.W + n_pad * g.ld;
  const double* neg_alpha = g.W + g.y_row * g.ld + n_pad;
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = g.hyp;
  a.d = g.d;
  a.dp = padded_dim(g.d);
  a.plain = 1;
  size_t kd_lds = 0;
  if (g.var) {
    const int nslot = 1 + kd.n_ard + (sc_node(kd) >= 0 ? 2 : 0) + cp_windows(kd);
    kd_lds = sizeof(double) * (GPK_MAX_HYP + (size_t)nslot * ATILE * a.dp) + sizeof(FastNode) * GPK_MAX_NODES;
    hipError_t e = ensure_dyn_lds(reinterpret_cast<const void*>(predict_kdiag_kernel), kd_lds);
    if (e != hipSuccess) return e;
  }
  for (int64_t c0 = 0; c0 < g.m; c0 += g.rows) {
    const int64_t mc = g.m - c0 < g.rows ? g.m - c0 : g.rows;
    const double* Xc = g.Xs + c0 * g.d;
    hipError_t e;
    if (n_pad > n) {
      e = hipMemset2DAsync(Ks + n, (size_t)n_pad * sizeof(double), 0, (size_t)(n_pad - n) * sizeof(double),
                           (size_t)mc, s);
      if (e != hipSuccess) return e;
    }
    // Ks' = k(Xs chunk, X): what gpk_kernel_matrix(Xs, X) launches
    a.X = Xc;
    a.n = mc;
    a.Xs = g.X;
    a.m = n;
    a.W = Ks;
    a.ld = n_pad;
    e = launch_assemble(kd, a, GPK_F64, 1, s);
    if (e != hipSuccess) return e;
    if (g.mu) {
      e = launch_gemv(Ks, mc, n, n_pad, neg_alpha, g.mu + c0, -1.0, 0.0, s);
      if (e != hipSuccess) return e;
    }
    if (!g.var) continue;
    AsmArgs ad = a;  // the chunk's points alone (rows of a plain build)
    ad.Xs = Xc;
    ad.m = mc;
    ad.W = nullptr;
    hipLaunchKernelGGL(predict_kdiag_kernel, dim3((unsigned)((mc + ATILE - 1) / ATILE)), dim3(256), kd_lds, s, kd, ad,
                       kdiag);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const NormArgs na{Ks, n_pad, R, g.ld, mc, n, part, g.rows};
    hipLaunchKernelGGL(predict_norm_kernel, dim3((unsigned)ntc, (unsigned)((mc + PT - 1) / PT)), dim3(256), 0, s, na);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(predict_reduce_kernel, dim3((unsigned)((mc + 255) / 256)), dim3(256), 0, s, part, g.rows, ntc,
                       kdiag, mc, g.var + c0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace gpk
