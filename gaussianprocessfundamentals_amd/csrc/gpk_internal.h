// Internal declarations shared by the libgpk translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "gpk.h"
#include "gpk_const.h"

namespace gpk {

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize, which is a per-device
// attribute of the kernel: raised (never lowered -- one kernel may be launched with several sizes) to the
// largest size requested so far on the device, before the launch that needs it.
inline hipError_t ensure_dyn_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> done;
  if (bytes <= 65536) return hipSuccess;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = done[{dev, fn}];
  if (have >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) have = bytes;
  return e;
}

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ----------------------------------------------------------------------------------- launch args
// LDS row stride of a staged point (AsmArgs::dp and its kin): odd when d is even, so that rows do not share a bank
inline int32_t padded_dim(int64_t d) { return (int32_t)((d % 2 == 0) ? d + 1 : d); }

struct AsmArgs {
  const double* hyp;
  int64_t hyp_stride;
  const double* noise;
  int64_t noise_stride;
  const double* X;
  int64_t x_bs;
  const double* Xs;
  int64_t xs_bs;
  const double* E;   // explicit extra rows (NULL: kernel rows of Xs)
  int64_t e_bs;
  const double* y;
  int64_t y_bs;
  void* W;
  int64_t ld;
  int64_t w_bs;
  int64_t n, m, n_pad, y_row, p;
  int32_t d;
  int32_t dp;        // LDS row stride of a point (odd when d is even: no bank conflicts)
  int32_t plain;     // 0 = augmented layout, 1 = plain rectangular kernel matrix
  int32_t uplo;      // plain mode: 1 = write j <= i only
  int64_t ntile;     // augmented: 64-tiles per dimension
  double diag_add;   // plain mode
  int32_t eye;       // augmented: the m extra rows are the identity (E = I, m == n), zero corner
  int64_t tcol_hi;   // augmented: > 0 builds only the tiles of 64-tile columns [0, tcol_hi) (all rows below)
  int32_t generic;   // 1: interior tiles too through the generic per-element loop (bitwise A/B of the fast one)
  // ragged batches (NULL: every member uses n / m): member b uses its first nb[b] training points
  // (rows nb[b] .. n_pad-1 become identity rows) and its first mb[b] test points (zero rows after)
  const int64_t* nb;
  const int64_t* mb;
  // dense mode (gpk_assemble_dense): the training block is read from A (lower triangle, mirrored)
  // instead of evaluated from the kernel program
  const double* A;
  int64_t a_ld;
  int64_t a_bs;
  // set by launch_assemble only (callers leave them): the two-leaf SE + periodic MFMA path's per-point features
  // (pair_feat_kernel: rows of feat_fs doubles [u_1..u_D | C_1..C_D | S_1..S_D | |u|^2 | 0], member stride feat_bs)
  // and per 64-point block (max |u|^2, sin / cos form allowed) in faux; NULL: features staged per tile
  const double* feat;
  const double* faux;
  int64_t feat_bs;
  int32_t feat_fs;
  // set by launch_assemble only: tiles the MFMA fast kernel left (count, then (member, ti, tj) triples); the
  // general instantiation then loops over this list instead of the grid
  const int32_t* tlist;
  // set by launch_assemble only: gpk_tune("cp_skip") -- a change-point window leaf that is exactly zero on a whole
  // tile edge skips its MUL sibling on that tile
  int32_t cp_skip;
};

struct GemmArgs {
  void* W;
  int64_t ld;
  int64_t w_bs;
  const void* Binv;  // trsm: inverted diagonal block of this step (folded: prep_kernel's operand, see below)
  int64_t inv_bs;
  int64_t j0;        // first column of the panel
  int64_t row0;      // first row (and column) of the trailing region
  int32_t nt;        // 128-tiles of the trailing region
  int32_t c_lo, c_hi;  // tile-column range handled by this launch (update)
  int32_t kdepth;      // panel width summed over (multiple of 16): 128, or 256 for the deferred update
  // rows [zlo, zhi) are structurally zero in the panel columns [j0, j0 + kdepth) (identity extra
  // rows: row n_pad + t of E L^-T is zero left of column t); tiles inside the range are skipped
  int64_t zlo, zhi;
  // tiles [bz0, bz0 + bzn) (launch-tile units from row0) lie inside [zlo, zhi): the grid enumerates the
  // remaining tiles only -- tile index t >= bz0 stands for t + bzn (rows and, for the update, columns)
  int32_t bz0, bzn;
  // ragged batches (NULL: uniform): member b's training rows nb[b] .. n_pad-1 are identity rows and
  // its test rows n_pad + mb[b] .. y_row-1 zero rows; tiles of rows that are zero in the panel are skipped
  const int64_t* nb;
  const int64_t* mb;
  int64_t n_pad, y_row, p;
  // fused K build (first trailing update of an m = 0, single-base-node factorisation): the tile's C is
  // evaluated -- k(x_i, x_j) + noise [i == j], identity padding, y row -- instead of loaded; the K
  // build then wrote only the panel columns of the first group
  int32_t band;    // update tile order: 0 row-major lower triangle, B > 0 bands of B tile rows
  // the update split by tile class (gpk_tune "upd_tri").  gemm_kernel: 1 = the strictly lower tiles only.
  // update_tri_kernel (launch_update_tri, the diagonal tiles of [c_lo, c_hi)): 2 = also the one live 16-row block
  // of the last tile row (nt - 1, the y row's), which the caller then left out of gemm_kernel's nt
  int32_t tri;
  int64_t row_end; // rows >= row_end are zero in every panel (0: unknown); MFMAs on them are skipped
  int32_t kbuild;
  int32_t d;
  int64_t n;
  gpk_node node;
  const double* hyp;
  int64_t hyp_stride;
  const double* noise;
  int64_t noise_stride;
  const double* X;
  int64_t x_bs;
  const double* y;
  int64_t y_bs;
};
// (The folded panel solve -- f64 trsm with kdepth > 128, the planner's in-group mode 4 -- takes no field of its own, so
// that every other kernel's argument block stays what it was: X = [A | C] Wop^T over K = kdepth, the left operand's
// columns [j0 + 128 - kdepth, j0 + 128) of W (the last 128 are the block column itself), the right operand
// prep_kernel's: row n of member b at Binv + b inv_bs + n kdepth; stored in place at j0.)

// prep_kernel (f64): per member Wop = [ -L_kk^-1 B | L_kk^-1 ] (128 x (kdepth + 128), row stride ld_op), B = W[128 kblk
// .. + 127, j0 .. j0 + kdepth - 1], L_kk^-1 from Winv with exact zeros above the diagonal
struct PrepArgs {
  const void* W;
  int64_t ld, w_bs;
  const void* Winv;
  int64_t inv_bs;
  int64_t kblk, j0;
  int32_t kdepth;
  void* Wop;
  int64_t ld_op, op_bs;
};

struct DiagArgs {
  void* W;
  int64_t ld;
  int64_t w_bs;
  void* Winv;
  int64_t inv_bs;
  int64_t j0;
  int64_t kblk;
  int32_t* info;
  int32_t dbg;  // timing-only ablations (GPK_DIAG_DEBUG): 1 no inverse, 2 no potf2, 4 no tile ops,
                // 8 no stores, 16 no step loop, 32 no final block row (diag2)
  int32_t version;  // 2: look-ahead schedule (default), 1: the phase-serial kernel (A/B measurements)
  // Fused panel solve (f64, diag2 only; 0: the diagonal block alone): trsm_tiles + 1 workgroups per
  // member each factor the block like the plain kernel.  After loading the block every workgroup draws
  // a ticket from ctr[b] (zero on entry): the last one to load writes L, L^-1 and info and resets the
  // counter -- so no workgroup can still be reading the block when L overwrites it (workgroups of one
  // launch may start far apart when other streams hold the CUs) -- and ticket t < trsm_tiles solves
  // the 64 rows row0 + 64 t .. +63 of member b against its L^-1 in LDS; the gemm<TRSM> launch of that
  // panel is then skipped.  Rows that are zero in the panel are skipped as in gemm<TRSM> (zlo / zhi,
  // nb / mb).  ctr: per-stream device counters (launches on one stream never overlap).
  int32_t trsm_tiles;
  int64_t row0, p, n_pad, y_row, zlo, zhi;
  const int64_t* nb;
  const int64_t* mb;
  int32_t* ctr;
  uint64_t* prof;  // (GPK_DIAG_PROF builds) per step and wave: s_memtime stamps of the phases, else NULL
  int32_t* half_flag;     // (persistent factorisation) set once block rows 0 .. half_step - 1 of L_kk^-1 are stored
  int32_t half_step;      //   (P phase after which they are; half_flag NULL: no early flag)
  int32_t defer_l_store;  // 1: L_kk stays in LDS only (the persistent factorisation stores it after publishing:
                          // no task of the launch reads it)
  int32_t no_inv_zeros;  // 1: leave the tiles of Winv above the diagonal tiles unwritten (the persistent
                         // factorisation's panel solves never read them; the launch path's TRSM does)
};

// rows of L_kk^-1 behind the diagonal task's early flag (multiples of 16; D publishes after its step rows / 16), for
// chains of more than / at most 32 diagonal blocks
#ifndef GPK_CHAIN_SHALF_ROWS
#define GPK_CHAIN_SHALF_ROWS 96
#endif
#ifndef GPK_CHAIN_SHALF_ROWS_SMALL
#define GPK_CHAIN_SHALF_ROWS_SMALL 112
#endif

// persistent factorisation (gpk_potrf.hip chain_kernel<T>): one member (or a small batch), tasks in host-computed order
struct ChainArgs {
  void* W;               // f64 or f32 (chain_kernel<double> / <float>), like Winv
  int64_t ld;
  void* Winv;
  int32_t* info;
  const int32_t* tasks;  // [ntasks + ntasks_b][4]: type (0 D, 1 S, 2 U32, 3 BLK), panel, slice / block row, block column
  int32_t ntasks;        // tasks of list A (all of them unless xcd_b >= 0)
  int32_t ntasks_b;      // chain_xcd: list B (the diagonal chain's D / S / UQ tasks), claimed first by the workgroups
  int32_t xcd_b;         //   running on XCD xcd_b (up to b_seats of them; -1: one list), then by everyone
  int32_t b_seats;
  int32_t* ctl;          // [0] claim counter (list A), [1] timeout flag, [2] list B's claim counter, [3] B seats
  int32_t* dflag;        // [nblk]: D(k) done
  int32_t* sdone;        // [nblk][nsl]: S(k, r) done
  int32_t* ucnt;         // [nsl][nbc]: panels applied to slice r of block column j
  int32_t* qdone;        // [nblk][nsl]: quarter updates (UQ) of panel k done on slice r of diagonal block k + 1
  int32_t* hflag;        // [nblk]: rows 0 .. 16 half_step - 1 of L_kk^-1 stored (D(k) before its end: the diagonal
                         // chain's S(k, .) start their first column blocks)
  int32_t half_step;     //   (D's step after which it sets hflag)
  int32_t uq;            // D(k) waits for the UQ tasks of panel k - 1 (else for ucnt)
  int32_t nsl, nbc;      // live 32-row slices (the last one holds the y row), live block columns
  int32_t nmem;          // members (task word bits 8..): W + m w_bs, Winv + m inv_bs, info + m, counters + m ctl_stride
  int64_t w_bs, inv_bs, ctl_stride;
  int64_t row_end;       // y_row + 1: rows below are zero
  int64_t timeout;       // per wait, in s_memrealtime ticks (100 MHz)
  int32_t* trace;        // debugging (GPK_CHAIN_TRACE=1, else NULL): host-visible [grid][32] progress words
  int32_t dbg;           // debugging (GPK_CHAIN_DBG): 4 = one diagonal task alone (chain_d_only_kernel)
  int32_t force_abort;   // testing (gpk_tune "chain_force_timeout"): the first wait reports a timeout
  uint64_t* dprof;       // (GPK_DIAG_PROF builds) the D tasks' phase stamps, else NULL
  uint64_t* times;       // profiling (GPK_CHAIN_TIMES=1, else NULL): per task [claimed, inputs ready, wave 0's body done, published, S / U32: loads returned, MFMAs retired] (100 MHz)
};

struct FinArgs {
  const void* W;
  int64_t ld;
  int64_t w_bs;
  int64_t n, m, n_pad, y_row;
  const int32_t* info;
  double* out;
  double* mu;
  double* var;
  const int64_t* nb;  // ragged batches: training points of member b (NULL: n)
};

struct GradArgs {
  const void* W;       // factored augmented matrix with identity extra rows (m == n)
  int64_t ld;
  int64_t w_bs;
  int64_t n, n_pad, y_row;
  const double* hyp;
  int64_t hyp_stride;
  const double* X;
  int64_t x_bs;
  int32_t d;
  int32_t dp;
  int64_t ntile;       // 64-tiles per edge of the n x n training block
  double* part;        // [batch][ntile (ntile + 1) / 2][n_hyp + 1] per-tile partial sums
  double* grad;        // [batch][n_hyp + 1]
  const int32_t* info;
  uint32_t adj_mask[GPK_MAX_NODES];  // per node: nodes whose values multiply its adjoint
  const int64_t* nb;   // ragged batches (gpk_grad_ragged): training points of member b (NULL: n); last, so that the
                       // uniform instantiations read every other field where they did
};

// gpk_mse_backward (gpk_grad.hip): gradient of the held-out mean squared error from a factored augmented matrix with
// m test rows.  rhs holds, per member, the two right-hand sides of the backward solves and then their solutions:
// slot 0 c = V^T r -> q = L^-T c, slot 1 z -> alpha = L^-T z (entries at and past the member's n_b zero).
struct MseArgs {
  const double* W;     // factored augmented matrix (fp64), test rows n_pad .. n_pad + m - 1
  int64_t ld;
  int64_t w_bs;
  int64_t n, m, n_pad, y_row;
  const double* hyp;
  int64_t hyp_stride;
  const double* X;
  int64_t x_bs;
  const double* Xs;
  int64_t xs_bs;
  const double* ys;    // test targets
  int64_t ys_bs;
  int32_t d;
  int32_t dp;
  int64_t ntr, nte;    // 64-tiles of the training / test points: ntr (ntr + 1) / 2 lower TRAIN x TRAIN tiles, then
                       // nte * ntr TEST x TRAIN tiles (test tile major)
  double* rhs;         // [batch][2][n_pad]
  double* res;         // [batch][m] residual r = mu - ys (0 past the member's m_b)
  double* part;        // [batch][tiles][n_hyp + 1] per-tile partial sums
  double* out;         // [batch][4]: mse, sum r^2, m_b, n_b
  double* grad;        // [batch][n_hyp + 1]
  const int32_t* info;
  uint32_t adj_mask[GPK_MAX_NODES];
  const int64_t* nb;   // ragged batches: training / test points of member b (NULL: n / m)
  const int64_t* mb;
};

// gpk_loo_backward (gpk_loo.hip): leave-one-out read-out and cotangent of a factored identity-augmented W (fp64)
struct LooArgs {
  const double* W;     // corner -K^-1 (lower triangle), the corner's y row -alpha^T
  int64_t ld;
  int64_t w_bs;
  int64_t n, n_pad, y_row;
  const double* y;     // the assembled targets
  int64_t y_bs;
  int32_t loss;        // GPK_LOO_LPD / GPK_LOO_MSE
  double* pts;         // [batch][4][n_pad]: phi_alpha, phi_d, alpha, u (zeros at and past the member's n_b)
  double* slab;        // [batch][loo_slabs(n_pad)][3] partial sums of f, (alpha / d)^2, log(1 / d)
  double* cot;         // [batch][n_pad + 1][n_pad] cotangent C = -2 G (lower triangle), last row zeros; NULL: value only
  double* out;         // [batch][4]: f, sum (alpha / d)^2, sum log sigma^2, n_b
  double* mu;          // [batch][n] (may be NULL)
  double* var;
  const int32_t* info;
  const int64_t* nb;   // ragged batches: training points of member b (NULL: n)
};

// gpk_kernel_vjp (gpk_grad.hip): adjoints of K(X, Z) = kernel(X, Z) for a weight matrix G [n, ldg]
struct VjpArgs {
  const double* hyp;   // [n_hyp] device
  const double* G;     // dense weights, or (G == NULL) the rank-1 weights gu[i] gv[j]
  int64_t ldg;
  const double* gu;
  const double* gv;
  double* part_h;      // [row tiles * column tiles][n_hyp] per-tile partial sums
  double* part_z;      // [row tiles][m][d] (set by launch_vjp)
  int32_t want_z;
  uint32_t adj_mask[GPK_MAX_NODES];
};

// gpk_kernel_jacobian (gpk_grad.hip): the planes d K(X, Z) / d theta_p, J[b][p][i][j] at J + b j_bs + p plane_stride + i ldj + j
struct JacArgs {
  const double* hyp;   // [batch][hyp_stride] device
  int64_t hyp_stride;
  double* J;
  int64_t ldj, plane_stride, j_bs;
  int32_t has_mul;     // set by launch_jacobian: some leaf has a MUL ancestor (node values are needed)
  uint32_t adj_mask[GPK_MAX_NODES];
};

// gpk_fisher (gpk_fisher.hip): Fisher information of the hyperparameters and the noise from a factored
// identity-augmented W (fp64), one member at a time through one workspace
struct FisherArgs {
  const double* W;     // corner -K^-1 (lower triangle)
  int64_t ld;
  int64_t w_bs;
  int64_t n, n_pad;
  int32_t d;
  const double* hyp;
  int64_t hyp_stride;
  const double* X;
  int64_t x_bs;
  const int32_t* info;
  double* fisher;      // [batch][n_hyp + 1][n_hyp + 1]
  double* work;        // Q [n][n], D [n_hyp][n][n], T [n_hyp][n][n], part [pairs][tiles]
  uint32_t adj_mask[GPK_MAX_NODES];
};

// gpk_predict (gpk_predict.hip): posterior mean and latent variance at new points from one member of a factored
// identity-augmented W (fp64), `rows` test points per pass through the workspace
struct PredictArgs {
  const double* W;     // the member's W: extra rows L^-T (upper triangle), the corner's y row -alpha^T
  int64_t ld;
  int64_t n, n_pad, y_row;
  int32_t d;
  const double* hyp;   // the member's hyperparameters
  const double* X;     // the member's training points
  const double* Xs;    // [m][d]
  int64_t m;
  double* mu;          // [m] or NULL
  double* var;         // [m] or NULL
  double* work;        // Ks' [rows][n_pad], kdiag [rows], part [ceil(n / 64)][rows]
  int64_t rows;
};

// gpk_predict_vt (gpk_predict_cov.hip): the rows V' = k(Xs, X) L^-T of new points from one member of a factored
// identity-augmented W (fp64), `rows` test points per pass through the workspace
struct PredictVtArgs {
  const double* W;     // the member's W: extra rows L^-T (upper triangle)
  int64_t ld;
  int64_t n, n_pad;
  int32_t d;
  const double* hyp;   // the member's hyperparameters
  const double* X;     // the member's training points
  const double* Xs;    // [m][d]
  int64_t m;
  double* V;           // [m][ldv], columns < n written
  int64_t ldv;
  double* work;        // Ks' [rows][n_pad]
  int64_t rows;
};

// gpk_predict_cov (gpk_predict_cov.hip): C = k(Xa, Xb) - Va Vb^T over the first n columns
struct PredictCovArgs {
  const double* hyp;
  int32_t d;
  const double* Xa;    // [ma][d]
  int64_t ma;
  const double* Va;    // [ma][lda]
  int64_t lda;
  const double* Xb;    // [mb][d]
  int64_t mb;
  const double* Vb;    // [mb][ldb]
  int64_t ldb;
  int64_t n;
  double* C;           // [ma][ldc]
  int64_t ldc;
  int32_t symmetric;   // Xa = Xb, Va = Vb: lower tiles computed, mirrored
};

struct TrsvArgs {
  const void* W;
  int64_t ld;
  int64_t w_bs;
  const void* Winv;
  int64_t inv_bs;
  double* x;
  int64_t x_bs;
  int64_t kblk;
  int64_t n_pad;
  int32_t trans;
  int64_t n_valid;  // rows / columns of W that exist (n_pad for an augmented matrix; n for a caller's L)
};

// ----------------------------------------------------------------------------------- launchers
bool tune_asm_feat();  // gpk_tune("asm_feat") in effect on this thread
bool tune_asm_f32_fast();  // gpk_tune("asm_f32_fast") in effect on this thread
int tune_asm_f32_chunk();  // gpk_tune("asm_f32_chunk"), clamped to 1 .. 64
bool tune_cp_skip();       // gpk_tune("cp_skip") in effect on this thread
hipError_t launch_assemble(const gpk_kdesc& kd, const AsmArgs& a, int dtype, int32_t batch,
                           hipStream_t s);
hipError_t launch_diag(const DiagArgs& a, int dtype, int32_t batch, hipStream_t s);
hipError_t launch_gemm(const GemmArgs& a, int dtype, int mode, int tile, int32_t batch, hipStream_t s);
hipError_t launch_prep(const PrepArgs& a, int32_t batch, hipStream_t s);
// f64 update, 128-tiles: the lower 16 x 16 blocks of the diagonal tiles of [c_lo, c_hi) (gpk_update_tri.hip)
hipError_t launch_update_tri(const GemmArgs& a, int32_t batch, hipStream_t s);
hipError_t launch_finalize(const FinArgs& a, int dtype, int32_t batch, hipStream_t s);
hipError_t launch_chain(const ChainArgs& a, int dtype, int grid, hipStream_t s);
hipError_t chain_timeouts_read(int64_t* out);  // timed-out persistent launches on this device (synchronous)
hipError_t launch_grad(const gpk_kdesc& kd, const GradArgs& g, int dtype, int32_t batch, hipStream_t s);
// grad_kernel / grad_reduce_kernel over a cotangent buffer C [batch][c_rows][c_ld] instead of W's corner: the points are
// staged through g's real layout, the weight -C_ij - a_i a_j is read with the corner at (0, 0) and the "y row" a at row
// c_yrow of C (gpk_loo_backward: a row of zeros).  fp64.
hipError_t launch_grad_cot(const gpk_kdesc& kd, const GradArgs& g, const double* C, int64_t c_ld, int64_t c_bs,
                           int64_t c_yrow, int32_t batch, hipStream_t s);
int64_t loo_slabs(int64_t n_pad);  // workgroups per member of the LOO read-out
hipError_t launch_loo_points(const LooArgs& g, int32_t batch, hipStream_t s);
hipError_t launch_loo_symv(const LooArgs& g, int32_t batch, hipStream_t s);
hipError_t launch_loo_cot(const LooArgs& g, int32_t batch, hipStream_t s);
int64_t mse_tiles(int64_t n, int64_t m);  // tiles of the MSE gradient's tile pass
hipError_t launch_mse_residual(const MseArgs& g, int32_t batch, hipStream_t s);
hipError_t launch_mse_tiles(const gpk_kdesc& kd, const MseArgs& g, int32_t batch, hipStream_t s);
size_t vjp_workspace_elems(const gpk_kdesc& kd, int64_t n, int64_t m, int32_t d, bool want_z);
hipError_t launch_vjp(const gpk_kdesc& kd, const VjpArgs& g, const double* X, int64_t n, const double* Z, int64_t m,
                      int32_t d, double* grad_hyp, double* grad_z, hipStream_t s);
// the planes d K(X, Z) / d theta_p of ``batch`` members (Z member stride z_bs; lower_tiles: only tiles tj <= ti)
hipError_t launch_jacobian(const gpk_kdesc& kd, const JacArgs& g, const double* X, int64_t x_bs, int64_t n,
                           const double* Z, int64_t z_bs, int64_t m, int32_t d, int32_t lower_tiles, int32_t batch,
                           hipStream_t s);
size_t fisher_workspace_elems(int n_hyp, int64_t n);
hipError_t launch_fisher(const gpk_kdesc& kd, const FisherArgs& g, int32_t batch, hipStream_t s);
int64_t predict_max_rows();  // test points per pass at most (a grid dimension)
size_t predict_workspace_elems(int64_t n, int64_t n_pad, int64_t rows);
hipError_t launch_predict(const gpk_kdesc& kd, const PredictArgs& g, hipStream_t s);
size_t predict_vt_workspace_elems(int64_t n_pad, int64_t rows);
hipError_t launch_predict_vt(const gpk_kdesc& kd, const PredictVtArgs& g, hipStream_t s);
hipError_t launch_predict_cov(const gpk_kdesc& kd, const PredictCovArgs& g, hipStream_t s);
hipError_t launch_trsv_diag(const TrsvArgs& a, int dtype, int32_t batch, hipStream_t s);
hipError_t launch_trsv_update(const TrsvArgs& a, int dtype, int32_t batch, hipStream_t s);
hipError_t launch_gemv(const double* A, int64_t n, int64_t m, int64_t lda, const double* x, double* y,
                       double alpha, double beta, hipStream_t s);

// approximation paths (gpk_approx.hip)
struct DgemmArgs {
  int32_t ta, tb;
  int64_t M, N, K;
  const double* A;
  int64_t lda, a_bs;
  const double* B;
  int64_t ldb, b_bs;
  double* C;
  int64_t ldc, c_bs;
  double alpha, beta;
};

struct JacobiArgs {
  const double* Ain;
  double* Aout;
  const double* Vin;
  double* Vout;
  int32_t m, mm;
  int32_t* flag;
  double tol_abs;  // pairs with |a_pq| <= tol_abs are not rotated (besides the relative criterion)
};

hipError_t launch_dgemm(const DgemmArgs& g, int32_t batch, hipStream_t s);
hipError_t launch_jacobi_init(const double* A, int64_t lda, int64_t a_bs, int m, double* A0, double* V0,
                              int32_t batch, hipStream_t s);
hipError_t launch_jacobi_round(const JacobiArgs& a, int r, int32_t batch, hipStream_t s);
hipError_t launch_diag_absmax(const double* A0, int m, int32_t batch, double* out, hipStream_t s);
hipError_t launch_jacobi_out(const double* Af, const double* Vf, int m, double* V, double* lam, int32_t batch,
                             hipStream_t s);
hipError_t launch_pinv_factor(const double* V, const double* lam, int m, double rcond, int mode, double* mu,
                              double* U, int32_t* rank, int32_t batch, hipStream_t s);
// tridiagonal eigensolver (gpk_eig.hip)
hipError_t launch_eig_tridiag(double* W, int m, double* d, double* e, double* tau, double* PV, double* vg,
                              double* yg, int split_m, hipStream_t s);
struct DcLevel {  // divide-and-conquer scratch, every array [m] (pair arrays [m / 2 + 1])
  double *lam, *dK, *zK, *rc, *rs, *root_t, *zhat, *rho;
  double* gscr;  // [5 m]: the deflation's sort arrays of merged blocks too large for LDS
  int32_t *idx, *ord, *rp, *rn, *root_o, *kcnt, *rcnt, *flip;
};
hipError_t launch_eig_dc(const double* d, const double* e, int m, const DcLevel& L, double* Q, double* Qg, double* U,
                         hipStream_t s);
hipError_t launch_eig_transpose(const double* A, int m, double* B, hipStream_t s);
hipError_t launch_eig_identity(double* Z, int m, hipStream_t s);
hipError_t launch_eig_build_y(const double* W, int m, int k0, int nb, double* Y, hipStream_t s);
hipError_t launch_eig_larft(const double* G, const double* tau, int k0, int nb, double* S, hipStream_t s);
bool eig_bt_fused(int m);
hipError_t launch_eig_backtransform(const double* W, const double* tau, int m, double* Sall, double* V,
                                    hipStream_t s);
hipError_t launch_sym_copy(const double* A, int64_t lda, int m, double* W, hipStream_t s);
hipError_t launch_pinv_bwd_scale(const double* lam, const double* mu, int m, double* T, int32_t batch, hipStream_t s);
hipError_t launch_ski_weights(const double* X, int64_t n, const double* Z, int64_t m, int d, double* Wm,
                              double* work, hipStream_t s);
hipError_t launch_copy_lower(const double* src, int64_t lds, double* dst, int64_t ldd, int64_t n, hipStream_t s);
// caller-matrix entries of the §8(b) sketch (gpk_flat.hip)
hipError_t launch_pack_lower(int dtype, const void* A, int64_t lda, int64_t n, int64_t n_pad, int64_t p, void* W,
                             hipStream_t s);
hipError_t launch_unpack_lower(int dtype, const void* W, int64_t ld, int64_t n, void* A, int64_t lda, hipStream_t s);
hipError_t launch_trtri_blocks(const double* L, int64_t ldl, int64_t n, double* Winv, hipStream_t s);
hipError_t launch_posterior_var(const double* V, int64_t n, int64_t m, const double* kdiag, double* var,
                                hipStream_t s);
hipError_t launch_distance(int mode, const double* A, int64_t n, int64_t a_bs, const double* B, int64_t m,
                           int64_t b_bs, int d, int32_t batch, double* out, int64_t ldo, int64_t o_bs, hipStream_t s);
hipError_t launch_add_diag(double* A, int64_t n, int64_t lda, int64_t a_bs, double value, int32_t batch,
                           hipStream_t s);

// mean-function programs (gpk_mean.hip)
struct MeanArgs {
  const double* hyp;
  int64_t hyp_stride;
  const double* X;
  int64_t x_bs;
  int64_t n;
  const double* y;  // eval: NULL = the mean itself, else the targets to detrend
  int64_t y_bs;
  double* out;      // eval
  int64_t out_bs;
  const double* g;  // vjp: per-point weights
  int64_t g_bs;
  double* part;     // vjp: [batch][nblk][n_hyp] per-workgroup partial sums
  // set by the launchers
  int64_t nblk;     // workgroups per member
  int32_t n_nodes, n_hyp, d;
  int32_t op[GPK_MAX_NODES];
  int32_t off[GPK_MAX_NODES];
  int32_t lhs[GPK_MAX_NODES];  // binary nodes: the nodes whose values they pop (below, top)
  int32_t rhs[GPK_MAX_NODES];
};
const char* mean_desc_error(const gpk_mdesc* md);  // NULL for a valid program, else what is wrong with it
int mean_leaf_hyp(int32_t op, int32_t dim);         // hyperparameters of a leaf op, -1 for anything else
int64_t mean_blocks(int64_t n);                     // workgroups per member
hipError_t launch_mean_eval(const gpk_mdesc& md, MeanArgs a, int32_t batch, hipStream_t s);
hipError_t launch_mean_vjp(const gpk_mdesc& md, MeanArgs a, int32_t batch, double* grad, hipStream_t s);

// multi-start L-BFGS step (gpk_fit.hip); the state layout is the one include/gpk.h documents
struct FitArgs {
  int32_t n_par, batch;
  int32_t m, max_iter, max_backtracks;  // (init: m is written into the state; step reads it back from there)
  double c1, gtol, ftol;
  const double* f;     // step: f_t of member b at f[b * f_stride]
  int64_t f_stride;
  const double* g;     // step: g_t; init: x0
  int64_t g_stride;
  const int32_t* info; // step (may be NULL)
  const double* lo;    // init
  const double* hi;    // init
  double* state;
  int64_t state_stride;  // init: doubles per member
  double* xt;
  int64_t xt_stride;
  int32_t* status;     // step
};
int64_t fit_state_doubles(int n_par, int m);  // per member
hipError_t launch_fit_init(const FitArgs& a, hipStream_t s);
hipError_t launch_fit_step(const FitArgs& a, hipStream_t s);
hipError_t launch_fit_current(int n_par, int batch, const double* state, double* x, int64_t x_stride, double* f,
                              double* g, int64_t g_stride, int32_t* iters, hipStream_t s);

enum { GEMM_UPDATE = 0, GEMM_TRSM = 1 };

}  // namespace gpk
