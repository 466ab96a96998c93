// The f64 trailing update's diagonal tiles as lower-triangle work (gpk_tune "upd_tri").
//
// gemm_kernel<double, UPDATE, 128, 128> (gpk_potrf.hip) spends one full workgroup on each diagonal tile (j, j) of an
// update, 64 blocks of 16 x 16 of which only the 36 on or below the diagonal are ever read, and one on each tile of
// the y row's tile row, which has one live 16-row block: 8 useful blocks of 64, at a whole tile's staging and chunk
// barriers.  Here ONE workgroup per (member, block column j) does both: C -= P P^T on the 36 blocks I >= J of tile
// (j, j), P = the panel rows of block column j, and on the 8 blocks of the y block against the same P.  A and B of a
// diagonal tile are the same 128 rows, staged once per chunk, the y block's 16 rows behind them: 144 rows of 128 B
// per stage, two stages (36 KiB; two workgroups per CU).
//
// The 44 blocks are dealt over the 8 waves by gpk_tri_map.h (11 per SIMD, at most 6 per wave); every wave's blocks
// are a compile-time list, one instantiation of tri_wave per wave and tile kind.
//
// Bits: the staging (128-B rows, the same swizzle, global_load_lds), the fragment pieces a lane feeds to each MFMA
// k-step and the order of the k-steps onto C loaded first are TileCore's (gpk_potrf.hip), and a diagonal 16 x 16
// block is computed whole, so every element written is bit for bit what gemm_kernel writes.  The 28 blocks strictly
// above the diagonal are not written: no kernel reads them (the diagonal-block kernels load the lower 16-tiles only).
#include "gpk_internal.h"
#include "gpk_tile_dev.h"
#include "gpk_tri_map.h"

namespace gpk {
namespace {

constexpr int TRI_T = 128;                            // tile edge
constexpr int TRI_GBK = ROWB / (int)sizeof(double);   // K depth per stage (16)
constexpr int TRI_ROWS = TRI_T + 16;                  // staged rows per chunk: P's 128, then the y block's 16
constexpr int TRI_STAGE = TRI_ROWS * ROWB;            // bytes per stage

// full tile (all 8 row blocks live); the same plus the y blocks; the tile that holds row_end (the y row's own
// diagonal tile): row blocks < ilim only, a run-time bound
enum { TRI_FULL = 0, TRI_FULL_Y = 1, TRI_PART = 2 };

typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef decltype(__builtin_amdgcn_raw_buffer_load_b64(__amdgpu_buffer_rsrc_t(), 0, 0, 0)) raw64_t;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tri_rsrc(const double* p, int bytes) {
  const uint64_t u = reinterpret_cast<uint64_t>(p);
  const uint64_t uu = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(u >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(uu), 0, bytes, 0x00020000);
}

// Wave W's share of one tile.  Pg: row 0 of P (block column j's rows, panel column j0); Yg: the y block's first row
// there; C / Cy: element (0, 0) of tile (j, j) and of the y block's tile; ld in elements; NK chunks of 16.
template <int W, int KIND>
__device__ __forceinline__ void tri_wave(char* smem, const double* Pg, const double* Yg, double* C, double* Cy,
                                         int64_t ld, int NK, int ilim) {
  constexpr bool WITH_Y = KIND == TRI_FULL_Y;
  constexpr int NBLK = kTriDeal[W].n;
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, lr = lane & 15;
  const auto bi = [](int b) { return kTriDeal[W].blk[b].i; };
  const auto bj = [](int b) { return kTriDeal[W].blk[b].j; };
  // whether block b of the wave's list is computed: the y blocks with the fold only, a tile block when its rows
  // lie above row_end (wave-uniform)
  const auto live = [&](int b) { return bi(b) == kTriY ? WITH_Y : (KIND != TRI_PART || bi(b) < ilim); };

  // this wave's DMA instructions: groups 2 W and 2 W + 1 of P's 16, and waves 4 and 5 (five blocks each) one of the
  // y block's two.  Lane l of group g writes LDS bytes g 1024 + 16 l: row 8 g + (l >> 3), piece l & 7, which holds
  // logical piece swz(row, l & 7) of that row
  constexpr int NG = (WITH_Y && (W == 4 || W == 5)) ? 3 : 2;
  const double* src[NG];
#pragma unroll
  for (int i = 0; i < NG; ++i) {
    const int g = i < 2 ? 2 * W + i : 16 + (W - 4);
    const int r = g * 8 + (lane >> 3);
    src[i] = (i < 2 ? Pg + (int64_t)r * ld : Yg + (int64_t)(r - TRI_T) * ld) + swz(r, lane & 7) * 2;
  }
  const auto dma = [&](int stage, int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int g = i < 2 ? 2 * W + i : 16 + (W - 4);
      glds16(src[i] + (int64_t)kc * TRI_GBK, smem + stage * TRI_STAGE + g * 1024);
    }
  };

  // C through buffer descriptors (TileCore::csoff's form): one per-lane offset, the block and register in soffset
  const int ldb_s = wave_uniform((int)(ld * (int64_t)sizeof(double)));
  const __amdgpu_buffer_rsrc_t crs = tri_rsrc(C, TRI_T * ldb_s);
  const __amdgpu_buffer_rsrc_t yrs = tri_rsrc(WITH_Y ? Cy : C, 16 * ldb_s);
  const int cvo = (int)(((int64_t)Mfma<double>::row(lane, 0) * ld + (lane & 15)) * (int64_t)sizeof(double));
  const auto soff = [&](int b, int r) {
    return ((bi(b) == kTriY ? 0 : bi(b) * 16) + r * 4) * ldb_s + bj(b) * 16 * (int)sizeof(double);
  };

  d4 acc[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b)
    if (live(b)) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[b][r] = __builtin_bit_cast(
            double, __builtin_amdgcn_raw_buffer_load_b64(bi(b) == kTriY ? yrs : crs, cvo, soff(b, r), 0));
    }
  dma(0, 0);

  // a lane's place in a staged row block: row lr, pieces q (k-steps 0, 1) and q + 4 (k-steps 2, 3)
  const int roff = lr * ROWB;
  const int p0 = swz(lr, q) * 16, p1 = swz(lr, q + 4) * 16;
#define GPK_TRI_KSTEPS(S0, S1)                                                                      \
  _Pragma("unroll") for (int s = (S0); s < (S1); ++s)                                               \
  _Pragma("unroll") for (int b = 0; b < NBLK; ++b)                                                  \
    if (live(b)) acc[b] = Mfma<double>::op_neg(f[bi(b)][s / 2][s % 2], f[bj(b)][s / 2][s % 2], acc[b]);
#pragma nounroll
  for (int kc = 0; kc < NK; ++kc) {
    const int st = kc & 1;
    // one barrier per chunk, at the top: it retires the chunk's DMA (vmcnt(0), explicit as in TileCore::chunk) and
    // frees the other stage, read during chunk kc - 1
    __builtin_amdgcn_s_waitcnt(0x0F70);  // gfx9 encoding: vmcnt(0), expcnt(7), lgkmcnt(15)
    __syncthreads();
    const char* sb = smem + st * TRI_STAGE + roff;
    dbl2 f[kTriEdge + 1][2];  // by row block; only the wave's own are read (the rest never exist)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r <= kTriEdge; ++r)
        if (tri_wave_reads(W, r, WITH_Y)) f[r][h] = *reinterpret_cast<const dbl2*>(sb + r * 16 * ROWB + (h ? p1 : p0));
    __builtin_amdgcn_sched_barrier(0);  // (every read goes out ahead of the first MFMA, which waits for its own two)
    GPK_TRI_KSTEPS(0, 2)
    // the next chunk's DMA behind the first half of the MFMAs (TileCore::chunk, GMID: the compiler's wait for an
    // LDS DMA in flight then falls on fragment reads long completed)
    __builtin_amdgcn_sched_barrier(0);
    if (kc + 1 < NK) dma(st ^ 1, kc + 1);
    __builtin_amdgcn_sched_barrier(0);
    GPK_TRI_KSTEPS(2, 4)
  }
#undef GPK_TRI_KSTEPS

#pragma unroll
  for (int b = 0; b < NBLK; ++b)
    if (live(b)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = acc[b][r];  // (a value: bit_cast of the vector element itself reads element 0)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(raw64_t, v), bi(b) == kTriY ? yrs : crs, cvo,
                                              soff(b, r), 0);
      }
    }
}

// grid (c_hi - c_lo, batch): workgroup x is block column c_lo + x of member y.  FOLD: the launch also carries the y
// block (a.tri = 2; the last tile row, nt - 1, has exactly one live 16-row block)
template <bool FOLD>
__global__ __launch_bounds__(512, 4) void update_tri_kernel(GemmArgs a) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * TRI_STAGE];
  const int b = blockIdx.y;
  const int64_t tj = a.c_lo + blockIdx.x;
  double* W = reinterpret_cast<double*>(a.W) + (int64_t)b * a.w_bs;
  const int64_t R = a.row0 + tj * TRI_T;               // first row and column of tile (tj, tj)
  const int64_t Ry = a.row0 + (int64_t)(a.nt - 1) * TRI_T;  // first row of the last tile row
  // live 16-row blocks of the tile: rows >= row_end are zero in every panel
  const int64_t lv = (a.row_end - R + 15) / 16;
  const int ilim = wave_uniform((int)(lv < kTriEdge ? lv : kTriEdge));
  const double* Pg = W + R * a.ld + a.j0;
  const double* Yg = W + Ry * a.ld + a.j0;
  double* C = W + R * a.ld + R;
  double* Cy = W + Ry * a.ld + R;
  const int NK = a.kdepth / TRI_GBK;
  const int wid = wave_uniform(threadIdx.x >> 6);
  // every wave passes the same NK barriers whatever its list (as gemm_kernel's row-block forms do side by side)
#define GPK_TRI_WAVE(Wv)                                                                             \
  case Wv:                                                                                           \
    if (ilim < kTriEdge)                                                                             \
      tri_wave<Wv, TRI_PART>(smem, Pg, Yg, C, Cy, a.ld, NK, ilim);                                   \
    else                                                                                             \
      tri_wave<Wv, FOLD ? TRI_FULL_Y : TRI_FULL>(smem, Pg, Yg, C, Cy, a.ld, NK, ilim);               \
    break;
  switch (wid) {
    GPK_TRI_WAVE(0) GPK_TRI_WAVE(1) GPK_TRI_WAVE(2) GPK_TRI_WAVE(3)
    GPK_TRI_WAVE(4) GPK_TRI_WAVE(5) GPK_TRI_WAVE(6) GPK_TRI_WAVE(7)
  }
#undef GPK_TRI_WAVE
}

}  // namespace

hipError_t launch_update_tri(const GemmArgs& a, int32_t batch, hipStream_t s) {
  if (a.c_hi <= a.c_lo) return hipSuccess;
  if (a.row_end <= 0 || a.nb != nullptr || a.kbuild || a.bzn != 0 || a.zhi > a.zlo) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.c_hi - a.c_lo), batch);
  if (a.tri == 2)
    hipLaunchKernelGGL(update_tri_kernel<true>, grid, dim3(512), 0, s, a);
  else
    hipLaunchKernelGGL(update_tri_kernel<false>, grid, dim3(512), 0, s, a);
  return hipGetLastError();
}

}  // namespace gpk
