// Multi-start L-BFGS step (include/gpk.h, "multi-start L-BFGS fitter step"): gpk_fit_init, gpk_fit_step and
// gpk_fit_current, gfx950.
//
// One wave64 per member, FIT_WAVES members per workgroup, no LDS and no communication between the waves: a
// member's arithmetic is the same instructions on the same operands whatever batch it runs in.  Lane j holds
// parameters j and j + 64 of every vector (the second only at n_par = 65, in lane 0); lanes past n_par hold zeros,
// so the reductions need no masks.  Every inner product is one fused multiply-add per lane and a five-stage
// xor-shuffle butterfly: both partners of a stage add the same two values, so all 64 lanes end with the same bits
// and the scalar decisions taken from them (pass / fail, converged, push the pair) are wave-uniform without a
// broadcast.  The ring of (s, y) pairs stays in the member's state in device memory (at most 2 x 16 x 65 doubles,
// read twice by the two-loop recursion, L2-resident between the launches); alpha lives in registers (the loops
// over the history are unrolled to GPK_FIT_MAX_HISTORY with wave-uniform guards).  Header fields are read by every
// lane (one broadcast load each) and written by lane 0 with plain vector stores.
//
// Contraction is off: the sums that are meant to be fused say fma(), so the trial point is exactly
// clamp(fma(t, d, x)).
#pragma clang fp contract(off)

#include "gpk_internal.h"

namespace gpk {

namespace {

constexpr int FIT_WAVES = 4;
constexpr int HDR = GPK_FIT_HEADER;
constexpr int MAXH = GPK_FIT_MAX_HISTORY;
enum { H_PHASE = 0, H_STATUS, H_ITERS, H_NBACK, H_CNT, H_HEAD, H_F, H_T, H_FPREV, H_SD, H_EVALS, H_STRIDE, H_M,
       H_NPAR };
enum { PH_INIT = 0, PH_SEARCH = 1 };

struct V2 {
  double a, b;
};

__device__ __forceinline__ V2 ld(const double* p, int lane, int P) {
  V2 v;
  v.a = lane < P ? p[lane] : 0.0;
  v.b = lane + 64 < P ? p[lane + 64] : 0.0;
  return v;
}

__device__ __forceinline__ void st(double* p, int lane, int P, V2 v) {
  if (lane < P) p[lane] = v.a;
  if (lane + 64 < P) p[lane + 64] = v.b;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ double dot(V2 u, V2 v) { return wave_sum(fma(u.b, v.b, u.a * v.a)); }

__device__ __forceinline__ V2 axpy(double s, V2 u, V2 v) {  // s u + v
  V2 r;
  r.a = fma(s, u.a, v.a);
  r.b = fma(s, u.b, v.b);
  return r;
}

__device__ __forceinline__ V2 clamp(V2 v, V2 lo, V2 hi) {
  V2 r;
  r.a = fmin(fmax(v.a, lo.a), hi.a);
  r.b = fmin(fmax(v.b, lo.b), hi.b);
  return r;
}

// 1.0 on the free set, 0.0 elsewhere (lanes past n_par hold lo = hi = 0: never free)
__device__ __forceinline__ double free1(double x, double g, double lo, double hi) {
  return (lo < hi && !(x == lo && g > 0.0) && !(x == hi && g < 0.0)) ? 1.0 : 0.0;
}

__device__ __forceinline__ V2 free_mask(V2 x, V2 g, V2 lo, V2 hi) {
  V2 r;
  r.a = free1(x.a, g.a, lo.a, hi.a);
  r.b = free1(x.b, g.b, lo.b, hi.b);
  return r;
}

__device__ __forceinline__ V2 mul(V2 u, V2 v) {
  V2 r;
  r.a = u.a * v.a;
  r.b = u.b * v.b;
  return r;
}

// steepest descent on the free set and its first step length
__device__ __forceinline__ V2 descent(V2 g, V2 mask, double& t) {
  V2 d;
  d.a = mask.a != 0.0 ? -g.a : 0.0;
  d.b = mask.b != 0.0 ? -g.b : 0.0;
  t = fmin(1.0, 1.0 / sqrt(dot(d, d)));
  return d;
}

// the newest pair, still in registers in the step that pushed it (nothing a step writes is read back from memory
// in the same launch)
struct Pair {
  V2 s, y;
  double rho;
  bool live;
};

// r = H q by the two-loop recursion over the cnt newest pairs (newest in slot head - 1; `nw`, when live, is that pair)
__device__ __forceinline__ V2 two_loop(V2 q, const Pair& nw, const double* pS, const double* pY, const double* prho,
                                       int m, int cnt, int head, int P, int lane) {
  if (cnt == 0) return q;
  double al[MAXH];
  auto pair = [&](int k, V2& s, V2& y, double& rho) {
    int i = head - 1 - k;
    if (i < 0) i += m;
    if (k == 0 && nw.live) {
      s = nw.s;
      y = nw.y;
      rho = nw.rho;
    } else {
      s = ld(pS + (int64_t)i * P, lane, P);
      y = ld(pY + (int64_t)i * P, lane, P);
      rho = prho[i];
    }
  };
#pragma unroll
  for (int k = 0; k < MAXH; ++k) {
    al[k] = 0.0;
    if (k < cnt) {
      V2 s, y;
      double rho;
      pair(k, s, y, rho);
      al[k] = rho * dot(s, q);
      q = axpy(-al[k], y, q);
    }
  }
  {
    V2 s, y;
    double rho;
    pair(0, s, y, rho);
    const double gamma = dot(s, y) / dot(y, y);
    q.a *= gamma;
    q.b *= gamma;
  }
#pragma unroll
  for (int k = MAXH - 1; k >= 0; --k) {
    if (k < cnt) {
      V2 s, y;
      double rho;
      pair(k, s, y, rho);
      const double beta = rho * dot(y, q);
      q = axpy(al[k] - beta, s, q);
    }
  }
  return q;
}

__host__ __device__ inline int64_t state_doubles(int n_par, int m) {
  return (int64_t)HDR + 5 * (int64_t)n_par + (int64_t)m + 2 * (int64_t)m * (int64_t)n_par;
}

__global__ __launch_bounds__(FIT_WAVES * 64) void fit_init_kernel(FitArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * FIT_WAVES + (threadIdx.x >> 6);
  if (b >= a.batch) return;
  const int P = a.n_par;
  double* sp = a.state + (int64_t)b * a.state_stride;
  const double* x0 = a.g + (int64_t)b * a.g_stride;
  // every double of the member is written once: the header, x = clamp(x0), the bounds, zeros elsewhere
  for (int64_t i = lane; i < a.state_stride; i += 64) {
    double v = 0.0;
    if (i < HDR) {
      v = i == H_STRIDE ? (double)a.state_stride : i == H_M ? (double)a.m : i == H_NPAR ? (double)P : 0.0;
    } else if (i < HDR + 5 * (int64_t)P) {
      const int seg = (int)((i - HDR) / P), k = (int)((i - HDR) - (int64_t)seg * P);
      if (seg == 0) v = fmin(fmax(x0[k], a.lo[k]), a.hi[k]);
      if (seg == 3) v = a.lo[k];
      if (seg == 4) v = a.hi[k];
    }
    sp[i] = v;
  }
  st(a.xt + (int64_t)b * a.xt_stride, lane, P, clamp(ld(x0, lane, P), ld(a.lo, lane, P), ld(a.hi, lane, P)));
}

__global__ __launch_bounds__(FIT_WAVES * 64) void fit_step_kernel(FitArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * FIT_WAVES + (threadIdx.x >> 6);
  if (b >= a.batch) return;
  const int P = a.n_par;
  // (member 0's header holds the stride and the history length gpk_fit_init sized the buffer with)
  const int64_t stride = (int64_t)a.state[H_STRIDE];
  const int m = (int)a.state[H_M];
  if ((int)a.state[H_NPAR] != P || m < 1 || m > MAXH || stride != state_doubles(P, m)) {
    if (lane == 0) a.status[b] = -1;
    return;
  }
  double* sp = a.state + (int64_t)b * stride;
  int status = (int)sp[H_STATUS];
  if (status != GPK_FIT_RUNNING) {  // frozen: x_trial and the state stay
    if (lane == 0) a.status[b] = status;
    return;
  }
  double* px = sp + HDR;
  double* pg = px + P;
  double* pd = pg + P;
  double* prho = pd + 3 * P;
  double* pS = prho + m;
  double* pY = pS + (int64_t)m * P;
  double* pxt = a.xt + (int64_t)b * a.xt_stride;

  const int phase = (int)sp[H_PHASE];
  int iters = (int)sp[H_ITERS], nback = (int)sp[H_NBACK], cnt = (int)sp[H_CNT], head = (int)sp[H_HEAD];
  int sd = (int)sp[H_SD];
  const int evals = (int)sp[H_EVALS] + 1;
  double f = sp[H_F], t = sp[H_T], fprev = sp[H_FPREV];
  V2 x = ld(px, lane, P), g = ld(pg, lane, P), d = ld(pd, lane, P);
  const V2 lo = ld(pd + P, lane, P), hi = ld(pd + 2 * P, lane, P);
  V2 xt = ld(pxt, lane, P);
  const V2 gt = ld(a.g + (int64_t)b * a.g_stride, lane, P);
  const double ft = a.f[(int64_t)b * a.f_stride];
  const int info = a.info ? a.info[b] : 0;
  const bool bad = info != 0 || !isfinite(ft) || __ballot(!isfinite(gt.a) || !isfinite(gt.b)) != 0;

  bool accepted = false, new_dir = false;
  if (phase == PH_INIT) {
    if (bad) {
      status = GPK_FIT_BAD_START;
    } else {
      x = xt;
      f = fprev = ft;
      g = gt;
      accepted = true;
      d = descent(g, free_mask(x, g, lo, hi), t);
      sd = 1;
      nback = 0;
      new_dir = true;
    }
  } else {
    V2 s;
    s.a = xt.a - x.a;
    s.b = xt.b - x.b;
    const double gts = dot(g, s);
    const bool pass = !bad && gts <= 0.0 && ft <= fma(a.c1, gts, f);
    if (pass) {
      V2 y;
      y.a = gt.a - g.a;
      y.b = gt.b - g.b;
      const double sy = dot(s, y), ss = dot(s, s), yy = dot(y, y);
      Pair nw;
      nw.s = s;
      nw.y = y;
      nw.rho = 1.0 / sy;
      nw.live = sy > 2.2e-16 * (sqrt(ss) * sqrt(yy));
      if (nw.live) {
        st(pS + (int64_t)head * P, lane, P, s);
        st(pY + (int64_t)head * P, lane, P, y);
        if (lane == 0) prho[head] = nw.rho;
        head = head + 1 == m ? 0 : head + 1;
        cnt = cnt < m ? cnt + 1 : m;
      } else {
        // an accepted step without usable curvature (s^T y <= 0 where f is concave along s, or no displacement): the
        // pairs held describe another region -- kept, they would scale every later step by a stale gamma and the
        // search would crawl -- so the history is cleared and the next direction is steepest descent
        cnt = 0;
        head = 0;
      }
      fprev = f;
      x = xt;
      f = ft;
      g = gt;
      accepted = true;
      iters += 1;
      const V2 mask = free_mask(x, g, lo, hi);
      const double pgn = wave_max(fmax(fabs(g.a) * mask.a, fabs(g.b) * mask.b));
      if (pgn <= a.gtol) {
        status = GPK_FIT_CONVERGED_G;
      } else if (fprev - f <= a.ftol * fmax(1.0, fmax(fabs(f), fabs(fprev)))) {
        status = GPK_FIT_CONVERGED_F;
      } else if (iters >= a.max_iter) {
        status = GPK_FIT_MAX_ITER;
      } else {
        const V2 r = two_loop(mul(g, mask), nw, pS, pY, prho, m, cnt, head, P, lane);
        d.a = -(r.a * mask.a);
        d.b = -(r.b * mask.b);
        const double dg = dot(d, g);
        t = 1.0;
        sd = cnt == 0 ? 1 : 0;
        if (!(dg < 0.0)) {
          cnt = 0;
          head = 0;
          sd = 1;
        }
        if (sd) d = descent(g, mask, t);
        nback = 0;
        new_dir = true;
      }
    } else {
      nback += 1;
      if (nback > a.max_backtracks) {
        if (sd) {
          status = GPK_FIT_STALLED;
        } else {
          cnt = 0;
          head = 0;
          d = descent(g, free_mask(x, g, lo, hi), t);
          sd = 1;
          nback = 0;
          new_dir = true;
        }
      } else {
        t *= 0.5;
      }
    }
  }

  xt = status == GPK_FIT_RUNNING ? clamp(axpy(t, d, x), lo, hi) : x;
  st(pxt, lane, P, xt);
  if (accepted) {
    st(px, lane, P, x);
    st(pg, lane, P, g);
  }
  if (new_dir) st(pd, lane, P, d);
  if (lane == 0) {
    sp[H_PHASE] = (double)PH_SEARCH;
    sp[H_STATUS] = (double)status;
    sp[H_ITERS] = (double)iters;
    sp[H_NBACK] = (double)nback;
    sp[H_CNT] = (double)cnt;
    sp[H_HEAD] = (double)head;
    sp[H_F] = f;
    sp[H_T] = t;
    sp[H_FPREV] = fprev;
    sp[H_SD] = (double)sd;
    sp[H_EVALS] = (double)evals;
    a.status[b] = status;
  }
}

__global__ __launch_bounds__(FIT_WAVES * 64) void fit_current_kernel(int P, int batch, const double* state, double* x,
                                                                    int64_t x_stride, double* f, double* g,
                                                                    int64_t g_stride, int32_t* iters) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * FIT_WAVES + (threadIdx.x >> 6);
  if (b >= batch) return;
  if ((int)state[H_NPAR] != P) {  // not this call's state: every output says so (NaN, iterations -1)
    V2 nan2;
    nan2.a = nan2.b = __builtin_nan("");
    if (x) st(x + (int64_t)b * x_stride, lane, P, nan2);
    if (g) st(g + (int64_t)b * g_stride, lane, P, nan2);
    if (lane == 0) {
      if (f) f[b] = nan2.a;
      if (iters) iters[b] = -1;
    }
    return;
  }
  const double* sp = state + (int64_t)b * (int64_t)state[H_STRIDE];
  if (x) st(x + (int64_t)b * x_stride, lane, P, ld(sp + HDR, lane, P));
  if (g) st(g + (int64_t)b * g_stride, lane, P, ld(sp + HDR + P, lane, P));
  if (lane == 0) {
    if (f) f[b] = sp[H_F];
    if (iters) iters[b] = (int32_t)sp[H_ITERS];
  }
}

unsigned fit_grid(int batch) { return (unsigned)((batch + FIT_WAVES - 1) / FIT_WAVES); }

}  // namespace

int64_t fit_state_doubles(int n_par, int m) { return state_doubles(n_par, m); }

hipError_t launch_fit_init(const FitArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fit_init_kernel, dim3(fit_grid(a.batch)), dim3(FIT_WAVES * 64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_fit_step(const FitArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fit_step_kernel, dim3(fit_grid(a.batch)), dim3(FIT_WAVES * 64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_fit_current(int n_par, int batch, const double* state, double* x, int64_t x_stride, double* f,
                              double* g, int64_t g_stride, int32_t* iters, hipStream_t s) {
  hipLaunchKernelGGL(fit_current_kernel, dim3(fit_grid(batch)), dim3(FIT_WAVES * 64), 0, s, n_par, batch, state, x,
                     x_stride, f, g, g_stride, iters);
  return hipGetLastError();
}

}  // namespace gpk
