// Device helpers of the MFMA tile kernels (gpk_potrf.hip's shared tile core, gpk_update_tri.hip's triangle tiles): the
// MFMA wrappers with their C/D maps, the LDS image of a staged K chunk and the global -> LDS DMA.  Included by both
// translation units (anonymous namespace: one copy each).
#pragma once
#include "gpk_internal.h"

namespace gpk {
namespace {

template <typename T>
struct Mfma;
template <>
struct Mfma<double> {
  typedef d4 acc_t;
  static __device__ __forceinline__ acc_t op(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // c - a b: on the f64 MFMA the blgp field is the neg modifier (neg:[1,0,0] negates A)
  static __device__ __forceinline__ acc_t op_neg(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 1);
  }
  // v_mfma_f64_16x16x4_f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <>
struct Mfma<float> {
  typedef f4 acc_t;
  static __device__ __forceinline__ acc_t op(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ acc_t op_neg(float a, float b, acc_t c) { return op(-a, b, c); }
  // f32 16x16 C/D map: col = lane & 15, row = 4 * (lane >> 4) + reg
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

typedef __attribute__((address_space(3))) void lds_void;

constexpr int ROWB = 128;  // bytes of one row of a staged K chunk (8 pieces of 16 B)

// LDS image of a staged K chunk: one 128-B row per operand row, 16-B piece c of row r stored at
// piece c ^ ((r >> 1) & 7).  The 16 rows a quarter-wave ds_read_b128 touches then fill all 16
// slots of a 256-B bank row (conflict-free), while every global_load_lds wave-instruction still
// writes its 1 KiB lane-linearly (8 rows): the swizzle is applied to the per-lane SOURCE address.
__device__ __forceinline__ int swz(int r, int c) { return c ^ ((r >> 1) & 7); }

// 16 B per lane global -> LDS (wave-uniform LDS base + 16 lane).  The gfx950 builtins sit in
// __device__ helpers so that the host pass still emits the kernels' launch stubs.
__device__ __forceinline__ void glds16(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (lds_void*)lds_base, 16, 0, 0);
}
template <int AUX>  // cache-policy bits (16: sc1)
__device__ __forceinline__ void glds16a(const void* src, void* lds_base) {
  __builtin_amdgcn_global_load_lds(src, (lds_void*)lds_base, 16, 0, AUX);
}
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// LDS byte address of a pointer into shared memory (what M0 holds for an LDS DMA)
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(unsigned long)(lds_void*)const_cast<void*>(p);
}

}  // namespace
}  // namespace gpk
