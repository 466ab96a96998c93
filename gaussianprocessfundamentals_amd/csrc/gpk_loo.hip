// Leave-one-out cross-validation from the identity-augmented factorisation (gpk_loo_backward).
// The factored W holds -K^-1 in its corner (lower triangle) and -alpha^T in the corner's y row.  With
// d_i = (K^-1)_ii the LOO prediction of point i is mu_i = y_i - alpha_i / d_i with variance 1 / d_i (Rasmussen &
// Williams 5.4.2), and any objective f = sum_i phi(alpha_i, d_i) has the cotangent
//   d f / d K = G = -1/2 (alpha u^T + u alpha^T) - K^-1 diag(phi_d) K^-1,   u = K^-1 phi_alpha.
// Three kernels: the per-point read-out (loo_point_kernel, with loo_out_kernel adding its slabs), the symmetric
// matrix-vector product u (loo_symv_kernel) and the lower 64 x 64 tiles of P = K^-1 diag(phi_d) K^-1 on the f64
// matrix cores (loo_cot_kernel), whose epilogue writes C = -2 G in the layout grad_kernel reads its corner in: the
// tile pass over the kernel program is then gpk_grad.hip's, unchanged (launch_grad_cot).  fp64 only; every sum has a
// fixed order and W is only read.
#include <math.h>

#include "gpk_internal.h"

namespace gpk {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr double HALF_LOG_2PI = 0.91893853320467274178;
constexpr int LOO_SLAB = 256;  // points per workgroup of loo_point_kernel

__device__ __forceinline__ int64_t loo_member_n(const LooArgs& g, int b) { return g.nb ? g.nb[b] : g.n; }

// the corner of member b: element (i, j), j <= i, holds -(K^-1)_ij
__device__ __forceinline__ const double* loo_corner(const LooArgs& g, int b) {
  return g.W + (int64_t)b * g.w_bs + g.n_pad * g.ld + g.n_pad;
}

// Per point: mu, 1 / d, phi_alpha, phi_d, alpha (zeros past the member's n_b, up to n_pad) and the slab's partial sums
// of f, (alpha / d)^2 and log(1 / d), reduced in a fixed tree.  Also clears the cotangent buffer's last row.
__global__ __launch_bounds__(256) void loo_point_kernel(LooArgs g) {
  __shared__ double red[3][LOO_SLAB];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * LOO_SLAB + tid;
  const int64_t nn = loo_member_n(g, b);
  const double* W = g.W + (int64_t)b * g.w_bs;
  double f = 0.0, sq = 0.0, lv = 0.0, pa = 0.0, pd = 0.0, al = 0.0, mu = 0.0, var = 0.0;
  if (i < nn) {
    const double d = -W[(g.n_pad + i) * g.ld + g.n_pad + i];
    al = -W[g.y_row * g.ld + g.n_pad + i];
    const double r = al / d;  // y_i - mu_i
    mu = g.y[(int64_t)b * g.y_bs + i] - r;
    var = 1.0 / d;
    sq = r * r;
    lv = -log(d);
    if (g.loss == GPK_LOO_LPD) {
      f = HALF_LOG_2PI + 0.5 * lv + 0.5 * (al * r);
      pa = r;
      pd = -0.5 / d - 0.5 * sq;
    } else {
      const double inv_n = 1.0 / (double)nn;
      f = sq * inv_n;
      pa = 2.0 * r * inv_n / d;
      pd = -2.0 * sq * inv_n / d;
    }
  }
  if (i < g.n_pad) {
    double* pts = g.pts + (int64_t)b * 4 * g.n_pad;
    pts[i] = pa;
    pts[g.n_pad + i] = pd;
    pts[2 * g.n_pad + i] = al;
    if (g.cot) g.cot[(int64_t)b * (g.n_pad + 1) * g.n_pad + g.n_pad * g.n_pad + i] = 0.0;
  }
  if (i < g.n) {
    const bool bad = g.info[b] != 0;
    if (g.mu) g.mu[(int64_t)b * g.n + i] = bad ? NAN : mu;
    if (g.var) g.var[(int64_t)b * g.n + i] = bad ? NAN : var;
  }
  red[0][tid] = f;
  red[1][tid] = sq;
  red[2][tid] = lv;
  __syncthreads();
  for (int w = LOO_SLAB / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
      red[2][tid] += red[2][tid + w];
    }
    __syncthreads();
  }
  if (tid < 3) g.slab[((int64_t)b * gridDim.x + blockIdx.x) * 3 + tid] = red[tid][0];
}

// out[b] = {f, sum (alpha_i / d_i)^2, sum log sigma_i^2, n_b}: the slabs in order; +inf where the factorisation failed
__global__ __launch_bounds__(64) void loo_out_kernel(LooArgs g, int nslab) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid >= 3) return;
  const double* sl = g.slab + (int64_t)b * nslab * 3 + tid;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s += sl[k * 3];
  if (tid == 0 && g.info[b] != 0) s = INFINITY;
  g.out[b * 4 + tid] = s;
  if (tid == 0) g.out[b * 4 + 3] = (double)loo_member_n(g, b);
}

__device__ __forceinline__ double loo_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// u = K^-1 phi_alpha for the 64 rows of one block.  Only the lower triangle of the corner is stored: row i is its row
// part (j <= i: wave w takes rows w, w + 4, ..., lanes stride along the row) plus its column part (j > i, read down
// column i: lane = column, wave w takes rows i0 + w, i0 + w + 4, ...).  The order of every sum depends on the
// member's n_b alone.  Blocks past n_b write zeros (u is defined up to n_pad).
__global__ __launch_bounds__(256) void loo_symv_kernel(LooArgs g) {
  __shared__ double rowsum[ATILE];
  __shared__ double colsum[4][ATILE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * ATILE;
  const int64_t nn = loo_member_n(g, b);
  double* pts = g.pts + (int64_t)b * 4 * g.n_pad;
  double* u = pts + 3 * g.n_pad;
  if (i0 >= nn) {  // (workgroup-uniform)
    if (tid < ATILE) u[i0 + tid] = 0.0;
    return;
  }
  const double* Wc = loo_corner(g, b);
  const double* pa = pts;
#pragma unroll 1
  for (int k = 0; k < ATILE / 4; ++k) {
    const int rr = wave + 4 * k;
    const int64_t gi = i0 + rr;
    double s = 0.0;
    if (gi < nn)  // (wave-uniform)
      for (int64_t j = lane; j <= gi; j += 64) s = fma(Wc[gi * g.ld + j], pa[j], s);
    s = loo_wave_sum(s);
    if (lane == 0) rowsum[rr] = s;
  }
  {
    const int64_t gi = i0 + lane;
    double s = 0.0;
    for (int64_t j = i0 + wave; j < nn; j += 4)
      if (j > gi) s = fma(Wc[j * g.ld + gi], pa[j], s);
    colsum[wave][lane] = s;
  }
  __syncthreads();
  if (tid < ATILE) {
    const double s = rowsum[tid] + ((colsum[0][tid] + colsum[1][tid]) + (colsum[2][tid] + colsum[3][tid]));
    u[i0 + tid] = i0 + tid < nn ? -s : 0.0;  // the corner holds -K^-1
  }
}

// ----------------------------------------------------------------------------------------- cotangent
// One lower 64 x 64 tile (ti, tj) of P = S diag(phi_d) S, S = K^-1 (the two signs of the stored -S cancel), per
// workgroup: 2 x 2 waves of 32 x 32, each 2 x 2 blocks of v_mfma_f64_16x16x4_f64, K staged 16 at a time in LDS as
// [row][k] with row stride 18 doubles -- dgemm_kernel's fragment handling (gpk_approx.hip).  Both operands are rows
// of the symmetric S: element (a, k) is stored at (a, k) when k <= a and at (k, a) otherwise.  A chunk wholly left of
// the tile rows' diagonal is read along rows; any other chunk is read with the transposed map (consecutive threads
// take consecutive rows a of one k, i.e. consecutive addresses of the stored row k), so that the part above the
// diagonal is transposed while it is staged.  Rows, columns and k at or past n_b are zero by an explicit test, never
// by what the factorisation left there.  phi_d multiplies the A operand while staging.  The K loop runs over
// ceil(n_b / 64) tiles in order: the same inputs give the same bits, in a ragged batch as alone.
constexpr int CT = 64, CKC = 16, CLD = CKC + 2;

__device__ __forceinline__ double loo_sym_at(const double* Wc, int64_t ld, int64_t a, int64_t k, int64_t nn) {
  if (a >= nn || k >= nn) return 0.0;
  return a >= k ? Wc[a * ld + k] : Wc[k * ld + a];
}

// (e -> tile row, chunk column) of the staging element e of a chunk at k0 for tile rows from r0
__device__ __forceinline__ void loo_map(int e, int64_t r0, int64_t k0, int& ii, int& kk) {
  if (k0 + CKC - 1 > r0) {
    kk = e / CT;
    ii = e % CT;
  } else {
    ii = e / CKC;
    kk = e % CKC;
  }
}

struct LooStage {
  double a[4], b[4];
};

__device__ __forceinline__ void loo_fetch(const double* Wc, int64_t ld, const double* pd, int64_t i0, int64_t j0,
                                          int64_t k0, int64_t nn, int tid, LooStage& st) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    int ii, kk;
    loo_map(e, i0, k0, ii, kk);
    const int64_t gk = k0 + kk;
    st.a[u] = loo_sym_at(Wc, ld, i0 + ii, gk, nn) * (gk < nn ? pd[gk] : 0.0);
    loo_map(e, j0, k0, ii, kk);
    st.b[u] = loo_sym_at(Wc, ld, j0 + ii, k0 + kk, nn);
  }
}

__device__ __forceinline__ void loo_store(int64_t i0, int64_t j0, int64_t k0, int tid, const LooStage& st, double* As,
                                          double* Bs) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    int ii, kk;
    loo_map(e, i0, k0, ii, kk);
    As[ii * CLD + kk] = st.a[u];
    loo_map(e, j0, k0, ii, kk);
    Bs[ii * CLD + kk] = st.b[u];
  }
}

__global__ __launch_bounds__(256) void loo_cot_kernel(LooArgs g) {
  __shared__ __attribute__((aligned(16))) double As[2][CT * CLD];
  __shared__ __attribute__((aligned(16))) double Bs[2][CT * CLD];
  const int b = blockIdx.y;
  const int64_t t = blockIdx.x;
  int64_t rt = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (rt * (rt + 1) / 2 > t) --rt;
  while ((rt + 1) * (rt + 2) / 2 <= t) ++rt;
  const int64_t ti = rt, tj = t - rt * (rt + 1) / 2;
  const int64_t i0 = ti * CT, j0 = tj * CT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, q = lane >> 4;
  const int64_t nn = loo_member_n(g, b);
  const int64_t ldc = g.n_pad;
  double* C = g.cot + (int64_t)b * (g.n_pad + 1) * g.n_pad;
  if (i0 >= nn) {  // (workgroup-uniform; tj <= ti) a tile wholly at or past n_b: zeros
    for (int e = tid; e < CT * CT; e += 256) C[(i0 + e / CT) * ldc + j0 + e % CT] = 0.0;
    return;
  }
  const double* Wc = loo_corner(g, b);
  const double* pts = g.pts + (int64_t)b * 4 * g.n_pad;
  const double* pd = pts + g.n_pad;
  const double* al = pts + 2 * g.n_pad;
  const double* uu = pts + 3 * g.n_pad;

  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  LooStage st;
  loo_fetch(Wc, g.ld, pd, i0, j0, 0, nn, tid, st);
  loo_store(i0, j0, 0, tid, st, As[0], Bs[0]);
  __syncthreads();
  const int nk = (int)((nn + CT - 1) / CT) * (CT / CKC);
  for (int c = 0; c < nk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nk) loo_fetch(Wc, g.ld, pd, i0, j0, (int64_t)(c + 1) * CKC, nn, tid, st);
    d2 fa[2][2], fb[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const d2* src = reinterpret_cast<const d2*>(&As[cur][(wr * 32 + mi * 16 + lr) * CLD + 4 * q]);
      fa[mi][0] = src[0];
      fa[mi][1] = src[1];
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const d2* src = reinterpret_cast<const d2*>(&Bs[cur][(wc * 32 + ni * 16 + lr) * CLD + 4 * q]);
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
    if (c + 1 < nk) loo_store(i0, j0, (int64_t)(c + 1) * CKC, tid, st, As[cur ^ 1], Bs[cur ^ 1]);
    __syncthreads();
  }
  // C_ij = -2 G_ij = 2 P_ij + alpha_i u_j + u_i alpha_j for j <= i < n_b, zero elsewhere in the tile
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int64_t gj = j0 + wc * 32 + ni * 16 + lr;
      const double al_j = al[gj], u_j = uu[gj];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = i0 + wr * 32 + mi * 16 + q + 4 * r;  // f64 C/D row = (lane >> 4) + 4 reg
        double v = 0.0;
        if (gi < nn && gj <= gi) v = 2.0 * acc[mi][ni][r] + (al[gi] * u_j + uu[gi] * al_j);
        C[gi * ldc + gj] = v;
      }
    }
}

}  // namespace

int64_t loo_slabs(int64_t n_pad) { return (n_pad + LOO_SLAB - 1) / LOO_SLAB; }

hipError_t launch_loo_points(const LooArgs& g, int32_t batch, hipStream_t s) {
  const int nslab = (int)loo_slabs(g.n_pad);
  hipLaunchKernelGGL(loo_point_kernel, dim3((unsigned)nslab, (unsigned)batch), dim3(256), 0, s, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(loo_out_kernel, dim3((unsigned)batch), dim3(64), 0, s, g, nslab);
  return hipGetLastError();
}

hipError_t launch_loo_symv(const LooArgs& g, int32_t batch, hipStream_t s) {
  hipLaunchKernelGGL(loo_symv_kernel, dim3((unsigned)(g.n_pad / ATILE), (unsigned)batch), dim3(256), 0, s, g);
  return hipGetLastError();
}

hipError_t launch_loo_cot(const LooArgs& g, int32_t batch, hipStream_t s) {
  const int64_t nt = (g.n + ATILE - 1) / ATILE;
  hipLaunchKernelGGL(loo_cot_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)batch), dim3(256), 0, s, g);
  return hipGetLastError();
}

}  // namespace gpk
