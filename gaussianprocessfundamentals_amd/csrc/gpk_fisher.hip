// Fisher information of the kernel hyperparameters and the noise from the identity-augmented factorisation
// (gpk_fisher):  F_pq = 1/2 tr(K^-1 d_pK  K^-1 d_qK),  d_noise K = I.
// The factored W holds -K^-1 in its corner (lower triangle).  The direct route, one member at a time through one
// workspace:
//   1. Q = K^-1 dense and symmetric: the corner's lower triangle, negated and mirrored (fisher_expand_kernel);
//   2. D_p = d_pK for X against X: the lower tiles by jacobian_kernel (gpk_grad.hip), mirrored by the same
//      fisher_expand_kernel in place, so the planes are symmetric bit for bit;
//   3. T_p = Q D_p on the f64 matrix cores: one batched launch of dgemm_kernel (gpk_approx.hip, what gpk_dgemm runs)
//      over the P planes with the A operand shared; T_noise = Q needs no product;
//   4. F_pq = 1/2 sum_ab T_p[a, b] T_q[b, a] for the (P + 1)(P + 2) / 2 pairs p <= q: fisher_contract_kernel takes one
//      64 x 64 tile (ta, tb) of T_p against the tile (tb, ta) of T_q, which it brings through LDS with a padded row
//      stride and reads transposed; one partial per tile and pair, summed in a fixed order by fisher_reduce_kernel,
//      which writes F_pq and F_qp from the one value and NaN for the whole matrix where info != 0.
// 2 P n^3 flops in the products; (2 P + 1) n^2 + (P + 1)(P + 2) / 2 ceil(n / 64)^2 doubles of workspace.  No atomics:
// two calls give the same bits.  fp64 only; W is only read.
#include <math.h>
#include <string.h>

#include "gpk_internal.h"

namespace gpk {
namespace {

constexpr int FT = 64, FLD = FT + 1;  // tile edge, LDS row stride (odd: a transposed read walks distinct banks)

__device__ __forceinline__ double fisher_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lower tile t -> (ti, tj), tj <= ti
__device__ __forceinline__ void fisher_lower_tile(int64_t t, int64_t& ti, int64_t& tj) {
  int64_t r = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (r * (r + 1) / 2 > t) --r;
  while ((r + 1) * (r + 2) / 2 <= t) ++r;
  ti = r;
  tj = t - r * (r + 1) / 2;
}

// dst plane z (n x n, row stride ldd) = the symmetric matrix whose lower triangle is scale * src plane z (row stride
// lds): one lower tile per workgroup, elements j <= i < n.  write_lower: also store the lower elements (src != dst);
// else only the strictly upper ones are written (src == dst: the plane is completed in place -- every read of the tile
// precedes the barrier, every write follows it, and no other workgroup touches either tile).
__global__ __launch_bounds__(256) void fisher_expand_kernel(const double* src, int64_t lds, int64_t src_ps, double* dst,
                                                            int64_t ldd, int64_t dst_ps, int64_t n, double scale,
                                                            int write_lower) {
  __shared__ double tile[FT * FLD];
  int64_t ti, tj;
  fisher_lower_tile(blockIdx.x, ti, tj);
  const int64_t i0 = ti * FT, j0 = tj * FT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* S = src + (int64_t)blockIdx.y * src_ps;
  double* D = dst + (int64_t)blockIdx.y * dst_ps;
#pragma unroll 1
  for (int k = 0; k < FT / 4; ++k) {
    const int r = wave + 4 * k;
    const int64_t gi = i0 + r, gj = j0 + lane;
    double v = 0.0;
    if (gi < n && gj <= gi) {
      v = scale * S[gi * lds + gj];
      if (write_lower) D[gi * ldd + gj] = v;
    }
    tile[r * FLD + lane] = v;
  }
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < FT / 4; ++k) {
    const int r = wave + 4 * k;
    const int64_t row = j0 + r, col = i0 + lane;  // element (row, col) = source element (col, row)
    if (col < n && row < col) D[row * ldd + col] = tile[lane * FLD + r];
  }
}

// plane p of the contraction: T_p for p < P, Q (= T_noise) for p == P
__device__ __forceinline__ const double* fisher_plane(const double* T, const double* Q, int64_t nn, int P, int p) {
  return p < P ? T + (int64_t)p * nn : Q;
}

// part[pair][tile] = sum over the tile (ta, tb) of T_p[a, b] T_q[b, a]; pair = blockIdx.y enumerates p <= q row by row
__global__ __launch_bounds__(256) void fisher_contract_kernel(const double* T, const double* Q, int64_t n, int P,
                                                              int64_t nt, double* part) {
  __shared__ double tq[FT * FLD];
  __shared__ double red[4];
  int p = 0, q = (int)blockIdx.y;
  while (q >= P + 1 - p) {  // row p holds the pairs (p, p) .. (p, P)
    q -= P + 1 - p;
    ++p;
  }
  q += p;
  const int64_t t = blockIdx.x;
  const int64_t ta = t / nt, tb = t - ta * nt;
  const int64_t a0 = ta * FT, b0 = tb * FT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* Tp = fisher_plane(T, Q, n * n, P, p);
  const double* Tq = fisher_plane(T, Q, n * n, P, q);
#pragma unroll 1
  for (int k = 0; k < FT / 4; ++k) {
    const int r = wave + 4 * k;
    const int64_t gb = b0 + r, ga = a0 + lane;
    tq[r * FLD + lane] = (gb < n && ga < n) ? Tq[gb * n + ga] : 0.0;
  }
  __syncthreads();
  double s = 0.0;
#pragma unroll 1
  for (int k = 0; k < FT / 4; ++k) {
    const int r = wave + 4 * k;
    const int64_t ga = a0 + r, gb = b0 + lane;
    const double v = (ga < n && gb < n) ? Tp[ga * n + gb] : 0.0;
    s = fma(v, tq[lane * FLD + r], s);
  }
  s = fisher_wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) part[(int64_t)blockIdx.y * (nt * nt) + t] = (red[0] + red[1]) + (red[2] + red[3]);
}

// F[p][q] = F[q][p] = 1/2 sum over the tiles (fixed order); NaN where the factorisation failed
__global__ __launch_bounds__(256) void fisher_reduce_kernel(const double* part, int64_t ntile, int P, const int32_t* info,
                                                            double* F) {
  __shared__ double red[256];
  int p = 0, q = (int)blockIdx.x;
  while (q >= P + 1 - p) {
    q -= P + 1 - p;
    ++p;
  }
  q += p;
  const int tid = threadIdx.x;
  const double* pp = part + (int64_t)blockIdx.x * ntile;
  double s = 0.0;
  for (int64_t t = tid; t < ntile; t += 256) s += pp[t];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = *info != 0 ? NAN : 0.5 * red[0];
    F[p * (P + 1) + q] = v;
    F[q * (P + 1) + p] = v;
  }
}

}  // namespace

size_t fisher_workspace_elems(int n_hyp, int64_t n) {
  const int64_t nt = (n + FT - 1) / FT;
  const size_t pairs = (size_t)(n_hyp + 1) * (size_t)(n_hyp + 2) / 2;
  return (size_t)(2 * n_hyp + 1) * (size_t)n * (size_t)n + pairs * (size_t)(nt * nt);
}

hipError_t launch_fisher(const gpk_kdesc& kd, const FisherArgs& g, int32_t batch, hipStream_t s) {
  const int P = kd.n_hyp;
  const int64_t n = g.n, nn = n * n;
  const int64_t nt = (n + FT - 1) / FT, ntri = nt * (nt + 1) / 2;
  const int pairs = (P + 1) * (P + 2) / 2;
  double* Q = g.work;
  double* D = Q + nn;
  double* T = D + (int64_t)P * nn;
  double* part = T + (int64_t)P * nn;
  for (int32_t b = 0; b < batch; ++b) {  // (members follow each other on the stream through the one workspace)
    const double* corner = g.W + (int64_t)b * g.w_bs + g.n_pad * g.ld + g.n_pad;
    hipLaunchKernelGGL(fisher_expand_kernel, dim3((unsigned)ntri, 1), dim3(256), 0, s, corner, g.ld, (int64_t)0, Q, n,
                       (int64_t)0, n, -1.0, 1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (P > 0) {
      JacArgs j;
      memset(&j, 0, sizeof(j));
      j.hyp = g.hyp + (int64_t)b * g.hyp_stride;
      j.J = D;
      j.ldj = n;
      j.plane_stride = nn;
      memcpy(j.adj_mask, g.adj_mask, sizeof(j.adj_mask));
      const double* Xb = g.X + (int64_t)b * g.x_bs;
      e = launch_jacobian(kd, j, Xb, 0, n, Xb, 0, n, g.d, 1, 1, s);
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(fisher_expand_kernel, dim3((unsigned)ntri, (unsigned)P), dim3(256), 0, s, D, n, nn, D, n, nn,
                         n, 1.0, 0);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
      const DgemmArgs ga{0, 0, n, n, n, Q, n, 0, D, n, nn, T, n, nn, 1.0, 0.0};
      e = launch_dgemm(ga, P, s);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fisher_contract_kernel, dim3((unsigned)(nt * nt), (unsigned)pairs), dim3(256), 0, s, T, Q, n, P,
                       nt, part);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fisher_reduce_kernel, dim3((unsigned)pairs), dim3(256), 0, s, part, nt * nt, P, g.info + b,
                       g.fisher + (int64_t)b * (P + 1) * (P + 1));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace gpk
