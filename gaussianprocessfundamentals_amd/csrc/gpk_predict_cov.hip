// Joint posterior covariance at new points from a factored identity-augmented W (gpk_predict_vt, gpk_predict_cov;
// DESIGN 28).  The factorisation left R = L^-T in the extra rows (R[t][i] = (L^-1)[i][t], non-zero only for i >= t).
// With Ks' = k(Xs, X) [m, n], test point major:
//   V'[c][i]  = sum_{t <= i, t < n} Ks'[c][t] R[t][i]                  (V' = (L^-1 Ks)^T, stored for i < n)
//   C[a][b]   = k(xa_a, xb_b) - sum_{i < n} Va[a][i] Vb[b][i]          (Sigma = K_ss - V' V'^T)
// predict_vt_kernel is predict_norm_kernel (gpk_predict.hip) with another epilogue: the same 64 x 64 tiles, the same
// staging, the same masked fetch of R (exactly i >= t, t < n, i < n; everything else 0.0 in the fetch), the same K loop
// over t < min(j0 + 64, n) -- and the tile is stored instead of squared and summed.  Ks' per chunk of test rows comes
// from the K build's plain launch, as in launch_predict.
// predict_cov_kernel: the K build of (Xa, Xb) has written k into C; the kernel sums s = Va Vb^T over k = 0 .. n - 1 in
// ascending chunks of 16 on the f64 matrix cores, accumulators starting at zero, and writes k - s in the epilogue
// -- one form for every tile.  Symmetric mode (Xa = Xb, Va = Vb): the blocks are the tiles on or below the diagonal,
// each computed element (a, b), a >= b, goes to (a, b) directly and to (b, a) through an LDS transpose (so the mirror
// tile's stores are row-contiguous too); only k of the lower triangle is read, the strictly upper part of the K build's
// output is overwritten, and C is symmetric bit for bit.  No atomics; per element the k-steps come in one order
// whatever tile, row of a tile or chunk of points it sits in.  fp64 only; W, Va and Vb are only read.
#include <math.h>
#include <string.h>

#include "gpk_internal.h"

namespace gpk {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// predict_norm_kernel's geometry: 64 x 64 tiles, 256 threads = 2 x 2 waves of 32 x 32 (2 x 2 MFMA blocks), K staged 16
// at a time as [row][k] with row stride 18, the MFMA k-step s of lane group q takes k = 4 q + s for both operands, two
// LDS stages with the next chunk's global loads issued before the current chunk's MFMAs.
constexpr int CT = 64, CKC = 16, CLD = CKC + 2;
constexpr int CTS = CT + 1;  // row stride of the transposed tile (symmetric epilogue)

struct CovStage {
  double a[4], b[4];
};

__device__ __forceinline__ void cov_stage_store_a(int tid, const double (&v)[4], double* S) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    S[(e / CKC) * CLD + e % CKC] = v[u];
  }
}

// one chunk's 2 x 2 blocks x 4 k-steps from the staged operands (both [row][k])
__device__ __forceinline__ void cov_mfma_chunk(const double* As, const double* Bs, int wr, int wc, int lr, int q,
                                               d4 (&acc)[2][2]) {
  d2 fa[2][2], fb[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const d2* src = reinterpret_cast<const d2*>(&As[(wr * 32 + mi * 16 + lr) * CLD + 4 * q]);
    fa[mi][0] = src[0];
    fa[mi][1] = src[1];
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const d2* src = reinterpret_cast<const d2*>(&Bs[(wc * 32 + ni * 16 + lr) * CLD + 4 * q]);
    fb[ni][0] = src[0];
    fb[ni][1] = src[1];
  }
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mi][s >> 1][s & 1], fb[ni][s >> 1][s & 1], acc[mi][ni],
                                                           0, 0, 0);
}

// ------------------------------------------------------------------------------------------------- V' = Ks' R
struct VtArgs {
  const double* A;   // Ks' [mc][lda], columns n .. lda - 1 zero
  int64_t lda;
  const double* R;   // the extra rows of W: R[t][i] at R + t ldr + i
  int64_t ldr;
  int64_t mc, n;
  double* V;         // the chunk's rows of V': V[c][i] at V + c ldv + i, i < n
  int64_t ldv;
};

__device__ __forceinline__ void vt_fetch(const VtArgs& g, int64_t i0, int64_t j0, int64_t k0, int tid, CovStage& st) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;  // 1024 elements of each operand chunk
    const int ii = e / CKC, kk = e % CKC;
    const int64_t gi = i0 + ii, gk = k0 + kk;
    st.a[u] = (gi < g.mc && gk < g.n) ? g.A[gi * g.lda + gk] : 0.0;
    const int kb = e / CT, jj = e % CT;
    const int64_t gt = k0 + kb, gj = j0 + jj;
    // the upper triangle of R inside the training block: everything else is unwritten, padding or another row class
    st.b[u] = (gt < g.n && gj < g.n && gj >= gt) ? g.R[gt * g.ldr + gj] : 0.0;
  }
}

__device__ __forceinline__ void vt_store(int tid, const CovStage& st, double* As, double* Bs) {
  cov_stage_store_a(tid, st.a, As);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    Bs[(e % CT) * CLD + e / CT] = st.b[u];
  }
}

__global__ __launch_bounds__(256) void predict_vt_kernel(VtArgs g) {
  __shared__ __attribute__((aligned(16))) double As[2][CT * CLD];
  __shared__ __attribute__((aligned(16))) double Bs[2][CT * CLD];
  // (the deepest column tiles first: tile jt sums over (jt + 1) * 64 rows of R)
  const int64_t jt = (int64_t)gridDim.x - 1 - blockIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * CT, j0 = jt * CT;
  const int64_t kend = j0 + CT < g.n ? j0 + CT : g.n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, q = lane >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  CovStage st;
  vt_fetch(g, i0, j0, 0, tid, st);
  vt_store(tid, st, As[0], Bs[0]);
  __syncthreads();
  const int nk = (int)((kend + CKC - 1) / CKC);
  for (int c = 0; c < nk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nk) vt_fetch(g, i0, j0, (int64_t)(c + 1) * CKC, tid, st);
    cov_mfma_chunk(As[cur], Bs[cur], wr, wc, lr, q, acc);
    if (c + 1 < nk) vt_store(tid, st, As[cur ^ 1], Bs[cur ^ 1]);
    __syncthreads();
  }
  // Epilogue: the tile as it is.  Accumulator register r of lane (q, lr) holds row q + 4 r, column lr of its block.
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = i0 + wr * 32 + mi * 16 + q + 4 * r;
        const int64_t gj = j0 + wc * 32 + ni * 16 + lr;
        if (gi < g.mc && gj < g.n) g.V[gi * g.ldv + gj] = acc[mi][ni][r];
      }
}

// ------------------------------------------------------------------------------------- C = k - Va Vb^T
struct CovArgs {
  const double* Va;  // [ma][lda], columns >= n never read
  int64_t lda;
  const double* Vb;  // [mb][ldb]
  int64_t ldb;
  int64_t ma, mb, n;
  double* C;         // [ma][ldc]: k(xa_a, xb_b) on entry
  int64_t ldc;
};

__device__ __forceinline__ void cov_fetch(const CovArgs& g, int64_t i0, int64_t j0, int64_t k0, int tid, CovStage& st) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid * 4 + u;
    const int ii = e / CKC, kk = e % CKC;
    const int64_t gk = k0 + kk;
    st.a[u] = (i0 + ii < g.ma && gk < g.n) ? g.Va[(i0 + ii) * g.lda + gk] : 0.0;
    st.b[u] = (j0 + ii < g.mb && gk < g.n) ? g.Vb[(j0 + ii) * g.ldb + gk] : 0.0;
  }
}

template <bool SYM>
__global__ __launch_bounds__(256) void predict_cov_kernel(CovArgs g) {
  // two stages of both operands; the symmetric epilogue reuses the space for the transposed tile
  __shared__ __attribute__((aligned(16))) double smem[4 * CT * CLD];
  static_assert(CT * CTS <= 4 * CT * CLD, "the transposed tile fits the staging space");
  double* const As0 = smem;
  double* const Bs0 = smem + 2 * CT * CLD;
  int64_t ti, tj;
  if (SYM) {
    // block t of the row-major lower triangle: t = ti (ti + 1) / 2 + tj, tj <= ti
    const int64_t t = blockIdx.x;
    ti = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    tj = t - ti * (ti + 1) / 2;
  } else {
    ti = blockIdx.y;
    tj = blockIdx.x;
  }
  const int64_t i0 = ti * CT, j0 = tj * CT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w >> 1, wc = w & 1;
  const int lr = lane & 15, q = lane >> 4;
  d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = d4{0.0, 0.0, 0.0, 0.0};

  CovStage st;
  cov_fetch(g, i0, j0, 0, tid, st);
  cov_stage_store_a(tid, st.a, As0);
  cov_stage_store_a(tid, st.b, Bs0);
  __syncthreads();
  const int nk = (int)((g.n + CKC - 1) / CKC);
  for (int c = 0; c < nk; ++c) {
    const int cur = c & 1;
    if (c + 1 < nk) cov_fetch(g, i0, j0, (int64_t)(c + 1) * CKC, tid, st);
    cov_mfma_chunk(As0 + cur * CT * CLD, Bs0 + cur * CT * CLD, wr, wc, lr, q, acc);
    if (c + 1 < nk) {
      cov_stage_store_a(tid, st.a, As0 + (cur ^ 1) * CT * CLD);
      cov_stage_store_a(tid, st.b, Bs0 + (cur ^ 1) * CT * CLD);
    }
    __syncthreads();
  }
  // Epilogue: k - s.  Accumulator register r of lane (q, lr) holds row q + 4 r, column lr of its block.
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wr * 32 + mi * 16 + q + 4 * r, lj = wc * 32 + ni * 16 + lr;
        const int64_t gi = i0 + li, gj = j0 + lj;
        const bool on = gi < g.ma && gj < g.mb && (!SYM || gi >= gj);
        double v = 0.0;
        if (on) {
          v = g.C[gi * g.ldc + gj] - acc[mi][ni][r];
          g.C[gi * g.ldc + gj] = v;
        }
        if (SYM) smem[lj * CTS + li] = v;  // (the loop's last barrier is behind every read of the stages)
      }
  if (SYM) {
    // the mirror: element (gj, gi) of C for gi > gj, rows of the transposed tile, 64 consecutive columns per wave
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < CT / 4; ++rr) {
      const int lj = w * (CT / 4) + rr, li = lane;
      const int64_t gi = i0 + li, gj = j0 + lj;
      if (gi < g.ma && gj < g.mb && gi > gj) g.C[gj * g.ldc + gi] = smem[lj * CTS + li];
    }
  }
}

}  // namespace

size_t predict_vt_workspace_elems(int64_t n_pad, int64_t rows) { return (size_t)rows * (size_t)n_pad; }

hipError_t launch_predict_vt(const gpk_kdesc& kd, const PredictVtArgs& g, hipStream_t s) {
  const int64_t n = g.n, n_pad = g.n_pad;
  const int64_t ntc = (n + CT - 1) / CT;
  double* Ks = g.work;
  const double* R = g.W + n_pad * g.ld;
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = g.hyp;
  a.d = g.d;
  a.dp = padded_dim(g.d);
  a.plain = 1;
  for (int64_t c0 = 0; c0 < g.m; c0 += g.rows) {
    const int64_t mc = g.m - c0 < g.rows ? g.m - c0 : g.rows;
    // Ks' = k(Xs chunk, X): what gpk_kernel_matrix(Xs, X) launches (the padding columns are never read here: the
    // fetch masks t < n)
    a.X = g.Xs + c0 * g.d;
    a.n = mc;
    a.Xs = g.X;
    a.m = n;
    a.W = Ks;
    a.ld = n_pad;
    hipError_t e = launch_assemble(kd, a, GPK_F64, 1, s);
    if (e != hipSuccess) return e;
    const VtArgs va{Ks, n_pad, R, g.ld, mc, n, g.V + c0 * g.ldv, g.ldv};
    hipLaunchKernelGGL(predict_vt_kernel, dim3((unsigned)ntc, (unsigned)((mc + CT - 1) / CT)), dim3(256), 0, s, va);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_predict_cov(const gpk_kdesc& kd, const PredictCovArgs& g, hipStream_t s) {
  // k(Xa, Xb) into C: what gpk_kernel_matrix(Xa, Xb) launches
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = g.hyp;
  a.X = g.Xa;
  a.Xs = g.Xb;
  a.W = g.C;
  a.ld = g.ldc;
  a.n = g.ma;
  a.m = g.mb;
  a.d = g.d;
  a.dp = padded_dim(g.d);
  a.plain = 1;
  hipError_t e = launch_assemble(kd, a, GPK_F64, 1, s);
  if (e != hipSuccess) return e;
  const int64_t nta = (g.ma + CT - 1) / CT, ntb = (g.mb + CT - 1) / CT;
  const CovArgs ca{g.Va, g.lda, g.Vb, g.ldb, g.ma, g.mb, g.n, g.C, g.ldc};
  if (g.symmetric)
    hipLaunchKernelGGL(predict_cov_kernel<true>, dim3((unsigned)(nta * (nta + 1) / 2)), dim3(256), 0, s, ca);
  else
    hipLaunchKernelGGL(predict_cov_kernel<false>, dim3((unsigned)ntb, (unsigned)nta), dim3(256), 0, s, ca);
  return hipGetLastError();
}

}  // namespace gpk
