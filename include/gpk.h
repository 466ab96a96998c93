/*
 * gpk.h -- C ABI of libgpk.so, the MI355X (gfx950) exact-GP likelihood engine.
 *
 * This is the drop-in boundary underneath the Python mirror of gpbasics' plugin API.
 * The reference has no native layer: every entry point below replaces a TensorFlow call
 * site on the reference's hot path (citations are relative to
 * Bernsai/GaussianProcessFundamentals main/gpbasics/):
 *
 *   gpk_kernel_matrix  <- Kernel.get_tf_tensor                 KernelBasics/Kernel.py:51-52
 *                         (SE :277-294, PER :440-457, MAT32 :702-720, MAT52 :859-880 of
 *                          KernelBasics/BaseKernels.py; ADD/MUL KernelBasics/Operators.py:207-225,
 *                          :306-326; distances Auxiliary/Distances.py:4-12)
 *   gpk_assemble       <- HolisticCovarianceMatrix.get_K / get_K_noised / get_K_s / get_K_ss
 *                                                               Statistics/CovarianceMatrix.py:187-225, :277-286
 *   gpk_potrf_aug      <- tf.linalg.cholesky + both tf.linalg.triangular_solve of get_L_K /
 *                         get_L_alpha                           Statistics/CovarianceMatrix.py:247-265
 *   gpk_finalize       <- LogLikelihood.get_metric (-LML)       Metrics/LogLikelihood.py:30-65,
 *                         Metrics/Metrics.py:138-139, :152-154;
 *                         posterior mu / var                    Statistics/Auxiliary.py:57-93
 *   gpk_trsv           <- the backward triangular_solve of get_L_alpha
 *                                                               Statistics/CovarianceMatrix.py:260-262
 *   gpk_nlml           <- LogLikelihood.get_metric, composed of the three calls above
 *
 * Conventions
 *  - Every device buffer is allocated and owned by the caller (PyTorch-ROCm); the library
 *    never allocates or frees caller memory and never synchronises the stream.
 *  - Points are row-major fp64: X[batch][n][d] with a caller-given batch stride (0 =
 *    shared by every batch member), y[batch][n], hyperparameters hyp[batch][n_hyp] fp64.
 *  - Return value: 0 on success, -i for an invalid i-th argument, > 0 for a HIP error
 *    code.  A matrix that is not positive definite is NOT an error of the call: it is
 *    reported through info_dev[b] (LAPACK convention: 1-based index of the first
 *    non-positive pivot, 0 when the factorisation succeeded).  info_dev[b] = -1 is an
 *    infrastructure failure of the persistent factorisation (a bounded wait timed out, gpk_tune
 *    "chain"), never "not positive definite": that member's results are undefined and the call must
 *    be repeated with gpk_tune("chain", 0) (or gpk_tune_thread).  Every entry that factors a single
 *    f64 member, or a batch of at most "chain_max_batch" members, can report it -- gpk_nlml,
 *    gpk_potrf_aug(_ex), gpk_nlml_batched, gpk_potrf_lower included.
 *  - gpk_last_error() returns a thread-local description of the last failure.
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream).
 *
 * Augmented layout: the engine factors one matrix per batch member
 *
 *      W = [ K + noise*I    .      .  ]   rows 0 .. n_pad-1   (padding rows: identity)
 *          [ Ks^T          Kss     .  ]   rows n_pad .. n_pad+m-1
 *          [ y^T            0      0  ]   row  y_row = n_pad+m
 *
 * over its first n_pad columns only.  Afterwards the first n_pad columns hold L, the test
 * rows hold V^T = Ks^T L^-T, the y row holds z^T = (L^-1 y)^T and the trailing corner holds
 * the Schur complement  [[Kss - V^T V, .], [-mu^T, -z^T z]]: posterior covariance,
 * posterior mean and the data-fit term of the LML fall out of one factorisation.
 */
#ifndef GPK_H
#define GPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPK_ABI_VERSION 7

/* arithmetic types of the factorisation */
enum { GPK_F64 = 0, GPK_F32 = 1 };

/* kernel-tree op codes: values follow KernelManifestation (KernelBasics/Kernel.py:23-37) */
enum {
  GPK_OP_LIN = 102, /* sum_k (x_k - c_k)(y_k - c_k) (KernelBasics/BaseKernels.py:114-134): hyp [c_0..c_{dim-1}, (sg)];
                       flags GPK_NODE_SCALED or 0 only (no ARD, expanded or standard form), ard_slot -1 */
  GPK_OP_RQ = 103,  /* rational quadratic, sg (1 + u)^(-a) with u = s / (2 a l^2), s = sum_k (x_k - y_k)^2 (the standard
                       definition; the reference names RQ = 103 and defines no formula): hyp [l, a, (sg)], the slot layout
                       of GPK_OP_PER.  flags GPK_NODE_SCALED or 0 only (no ARD, expanded or standard form), ard_slot -1.
                       `a` is used as given (no fabs): a <= 0 gives IEEE NaN / inf in K, which the factorisation reports
                       through `info` like any matrix that is not positive definite */
  GPK_OP_PER = 104,
  GPK_OP_SE = 105,
  GPK_OP_MAT32 = 107,
  GPK_OP_MAT52 = 108,
  GPK_OP_ADD = 201, /* binary: pops two, pushes sum (left fold of an n-ary ADD) */
  GPK_OP_MUL = 202, /* binary: pops two, pushes product                         */
  GPK_OP_CPW = 203  /* leaf: the change-point window w(x) w(y) of ChangePointOperator (KernelBasics/Operators.py:
                       410-476; the value of KernelManifestation.CP), dim 1 only:
                         w(x) = (1 - ind(x; h[0]))  [GPK_NODE_CP_LO]  *  ind(x; h[lo ? 1 : 0])  [GPK_NODE_CP_HI]
                       ind: [x < cp], or 0.5 (1 + tanh((cp - x) / 0.0025)) with GPK_NODE_CP_SIGMOID, or
                       1 / (1 + exp(-100 (x - cp))) with GPK_NODE_CP_APPROX.  hyp_offset: the first bound it reads (its
                       one or two bounds are consecutive; adjacent windows of one operator share a slot, and the
                       gradient entries of a shared slot are summed).  A change-point tree is
                       W_0 K_0 MUL  W_1 K_1 MUL ADD ...: a window directly left of its sibling under a MUL lets the K
                       build skip the sibling on tiles where the window is exactly zero (gpk_tune "cp_skip").
                       flags: at least one of CP_LO / CP_HI, at most one of CP_SIGMOID / CP_APPROX, none of
                       SCALED / ARD / SE_EXPANDED / STANDARD; ard_slot -1 */
};

/* per-node flags of a base-kernel node */
enum {
  GPK_NODE_SCALED = 1,     /* p_scaled_base_kernel: signal variance sg multiplies the kernel */
  GPK_NODE_ARD = 2,        /* build extension: one length scale per input dimension          */
  GPK_NODE_SE_EXPANDED = 4, /* SE distance by the reference's expanded norm (Distances.py:5-7) */
  GPK_NODE_STANDARD = 8,    /* MAT: Euclidean distance; PER: sum_d sin^2 per dimension (build
                               option; equal to the reference's L1 forms when d == 1)          */
  /* GPK_OP_CPW nodes only */
  GPK_NODE_CP_LO = 16,      /* the factor 1 - ind(.; h[0]) is present                          */
  GPK_NODE_CP_HI = 32,      /* the factor ind(.; h[lo ? 1 : 0]) is present                     */
  GPK_NODE_CP_SIGMOID = 64, /* mask form SIGMOID          (neither form bit: INDICATOR)        */
  GPK_NODE_CP_APPROX = 128  /* mask form APPROX_INDICATOR                                      */
};

#define GPK_MAX_NODES 16
#define GPK_MAX_DIM 16
#define GPK_MAX_ARD 2
#define GPK_MAX_HYP 64

/* one postfix-program node */
typedef struct {
  int32_t op;         /* GPK_OP_*                                               */
  int32_t hyp_offset; /* first hyperparameter of a base node inside hyp[b][:]   */
  int32_t ard_slot;   /* 0..GPK_MAX_ARD-1 for GPK_NODE_ARD nodes, else -1       */
  int32_t flags;      /* GPK_NODE_*                                             */
} gpk_node;

/* kernel tree flattened to postfix (children left to right, binary ADD/MUL after each
 * child beyond the first), hyperparameters in the reference's DFS order */
typedef struct {
  int32_t n_nodes;
  int32_t n_hyp;
  int32_t dim;
  int32_t n_ard;
  gpk_node nodes[GPK_MAX_NODES];
} gpk_kdesc;

/* sizes of the augmented factorisation of one problem shape */
typedef struct {
  int32_t dtype;          /* GPK_F64 / GPK_F32                                   */
  int32_t batch;          /* independent problems factored by every launch       */
  int64_t n;              /* training points                                     */
  int64_t m;              /* test points carried through the factorisation       */
  int64_t d;              /* input dimensions                                    */
  int64_t nb;             /* panel width (columns per factorisation step)        */
  int64_t n_pad;          /* factored columns: n rounded up to nb                */
  int64_t y_row;          /* row holding y (= n_pad + m)                         */
  int64_t p;              /* rows and columns of W (multiple of nb)              */
  int64_t ld;             /* leading dimension of W in elements                  */
  int64_t w_batch_stride; /* elements between consecutive batch members of W     */
  int64_t inv_batch_stride; /* elements between batch members of Winv            */
  size_t w_bytes;         /* bytes of W for the whole batch                      */
  size_t inv_bytes;       /* bytes of Winv (inverted diagonal blocks), whole batch */
} gpk_layout;

int gpk_abi_version(void);
const char* gpk_last_error(void);
/* 1 for every kernel-program op (GPK_OP_*) this library evaluates, else 0 (host only).  Ops are added without a new
 * ABI number (programs that do not use them mean what they meant): a binding asks here before emitting a new one. */
int gpk_op_supported(int32_t op);

/* fill *out for the given shape (no device work) */
int gpk_plan(int dtype, int32_t batch, int64_t n, int64_t m, int64_t d, gpk_layout* out);

/* Build W (see layout above) for every batch member.  hyp_dev[b*hyp_stride ...],
 * noise_dev[b*noise_stride]; X/Xs/E/y batch strides in elements (0 = shared).
 * The m extra rows are either kernel rows k(Xs_t, X_j) with the Kss corner (E == NULL), or the
 * explicit dense rows E[b][t][j] (t < m, j < n) with a zero corner (Xs ignored): E = I gives
 * L^-T in the extra rows and -K^-1 in the corner.  Xs and E may both be NULL when m == 0. */
int gpk_assemble(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                 int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                 const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride,
                 const double* E, int64_t e_bstride, const double* y, int64_t y_bstride,
                 void* W, void* stream);

/* Blocked right-looking Cholesky of the first n_pad columns of every W, all rows.
 * Winv receives the inverted nb x nb diagonal blocks (needed by gpk_trsv).
 * info_dev[batch] must be zeroed by the caller before the call. */
int gpk_potrf_aug(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, void* stream);

/* gpk_potrf_aug with flags: GPK_AUG_EXTRA_IDENTITY declares that the m (= n) extra rows were
 * assembled as the identity (gpk_assemble_inverse); row n_pad + t of E L^-T is then zero left of
 * column t, so every panel-solve and trailing-update tile made of such zero rows is skipped and the
 * factorisation costs n^3 flops instead of 7 n^3 / 3 (potrf + trtri + lauum, the work of
 * tf.linalg.inv(L) and L^-T L^-1 in get_L_inv_K / get_K_inv, Statistics/CovarianceMatrix.py:267-275). */
#define GPK_AUG_EXTRA_IDENTITY 1
int gpk_potrf_aug_ex(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, int32_t flags,
                     void* stream);
/* gpk_assemble with E = I (layout planned with m = n) without materialising E: after
 * gpk_potrf_aug_ex(.., GPK_AUG_EXTRA_IDENTITY, ..) the extra rows hold L^-T (upper triangle),
 * the corner -K^-1 (lower triangle) and the corner's y row -alpha^T. */
int gpk_assemble_inverse(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                         int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                         const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                         void* W, void* stream);
/* Read the results out of a factored W.  out_dev[b*4 + {0,1,2,3}] =
 * {nlml, fit = y^T alpha, logdet = 2 sum log L_ii, n}; nlml = +inf where info != 0.
 * mu_dev[b*m + t] = posterior mean (may be NULL), var_dev[b*m + t] = posterior variance
 * diagonal (may be NULL). */
int gpk_finalize(const gpk_layout* lay, const void* W, const int32_t* info_dev,
                 double* out_dev, double* mu_dev, double* var_dev, void* stream);

/* assemble + potrf_aug + finalize with m = 0 */
int gpk_nlml(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
             int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
             const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
             void* W, void* Winv, int32_t* info_dev, double* out_dev, void* stream);

/* -LML and its gradient for every batch member (layout planned with m = n):
 *   gpk_assemble_inverse + gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY) + gpk_finalize, then
 *   grad_dev[b*(n_hyp+1) + p] = d(-LML)/d hyp[p] (p < n_hyp, DFS order of the kernel tree) and
 *   grad_dev[b*(n_hyp+1) + n_hyp] = d(-LML)/d noise, from
 *   1/2 sum_ij ((K^-1)_ij - alpha_i alpha_j) dK_ij/d theta  -- the derivative the reference takes by
 *   tf.GradientTape through LogLikelihood.get_metric (Optimizer/Fitter.py:104-158).
 * grad_dev may be NULL (then only -LML and the inverse, e.g. for get_K_inv); NaN where info != 0.
 * work: device scratch of gpk_grad_workspace_bytes(kd, lay) bytes (0 for a kernel program that is not valid for
 * the layout's dimension -- gpk_nlml_grad refuses it). */
size_t gpk_grad_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay);
int gpk_nlml_grad(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                  const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                  const double* y, int64_t y_bstride, void* W, void* Winv, int32_t* info_dev,
                  double* out_dev, double* grad_dev, void* work, size_t work_bytes, void* stream);
/* Ragged batches: independent problems of different sizes factored by the same launches.
 * Replaces the per-segment loops of SegmentedCovarianceMatrix.get_K_noised_blocks / get_L_K_blocks /
 * get_L_alpha_blocks (Statistics/CovarianceMatrix.py:346-357, :445-456, :469-484) and the per-block
 * LogLikelihood of BlockwiseLogLikelihood.get_metric (Metrics/LogLikelihood.py:68-104), which the
 * reference runs one TensorFlow Cholesky after another.
 * The layout is planned for the largest member (n = max n_b, m = max m_b); member b uses the first
 * n_dev[b] points of X[b] / y[b] and the first m_dev[b] points of Xs[b] (device int64 arrays,
 * 1 <= n_dev[b] <= n, 0 <= m_dev[b] <= m).  Its rows n_dev[b] .. n_pad-1 are assembled as identity
 * rows (contributing log 1 = 0 to the log-determinant and 0 to the data fit) and its test rows past
 * m_dev[b] as zero rows; the factorisation skips every tile made of such rows.  m_dev may be NULL
 * when the layout has m = 0.  Results are those of each member factored on its own:
 * out_dev[b*4 + 3] = n_dev[b] and the -LML uses n_dev[b] in its normalising constant.
 * The flop counts of gpk_timing_read for ragged launches are those of the padded problem. */
int gpk_assemble_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                        int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                        const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride,
                        const double* y, int64_t y_bstride, const int64_t* n_dev, const int64_t* m_dev,
                        void* W, void* stream);
int gpk_potrf_aug_ragged(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev,
                         const int64_t* n_dev, const int64_t* m_dev, void* stream);
int gpk_finalize_ragged(const gpk_layout* lay, const void* W, const int32_t* info_dev, const int64_t* n_dev,
                        double* out_dev, double* mu_dev, double* var_dev, void* stream);
/* gpk_assemble_ragged + gpk_potrf_aug_ragged + gpk_finalize_ragged with m = 0 */
int gpk_nlml_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                    const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                    const double* y, int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv,
                    int32_t* info_dev, double* out_dev, void* stream);

/* Ragged identity-augmented batches: -LML, K^-1, alpha and the gradient of members of different sizes from one set
 * of launches (entries added without a new ABI number, found by symbol like gpk_op_supported).  The layout is
 * planned with m = n = max n_b.  Member b uses its first n_dev[b] points; its training rows n_dev[b] .. n_pad-1
 * are identity padding as in gpk_assemble_ragged, its extra rows t < n_dev[b] are e_t and its extra rows
 * t >= n_dev[b] zero rows (m_b = n_b), which the factorisation skips like unused test rows.  After the
 * factorisation member b's corner holds -K_b^-1 in its first n_b rows and columns and its y row -alpha_b^T.
 *
 * gpk_assemble_inverse_ragged: gpk_assemble_inverse per member -- the K build of the per-segment inverses of
 *   SegmentedCovarianceMatrix.get_K_inv_blocks / get_L_inv_K_blocks (Statistics/CovarianceMatrix.py:520-556).
 *   Errors: -11 n_dev NULL, -2 layout planned with m != n, -1 invalid layout or kernel program.
 * gpk_potrf_aug_ragged_ex: gpk_potrf_aug_ragged with flags (GPK_AUG_EXTRA_IDENTITY: m_dev[b] = n_dev[b]); always
 *   the launch path (the persistent launch takes no ragged members).  Errors: -6 n_dev NULL, -7 m_dev NULL with
 *   m > 0, -5 unknown flags, -1 invalid layout or identity rows with m != n.
 * gpk_grad_ragged: the gradient pass alone on a factored identity-augmented W, for members that share one kernel
 *   program: grad_dev[b*(n_hyp+1) + p] as gpk_nlml_grad writes it (NaN where info_dev[b] != 0) -- the derivative the
 *   reference's tape takes through blockwise_LL and through the mean of the folds' metrics (Optimizer/Fitter.py:97-102,
 *   :124-158; Metrics/LogLikelihood.py:68-104).  work: gpk_grad_workspace_bytes(kd, lay) bytes (the layout holds the
 *   largest member).  Errors: -7 n_dev NULL, -2 layout invalid or planned with m != n, -1 invalid kernel program,
 *   -11 work NULL or too small; -3, -5, -8, -9, -10 the other NULL pointers.
 * gpk_nlml_grad_ragged: memset of info + the three calls above + gpk_finalize_ragged, the ragged twin of
 *   gpk_nlml_grad; grad_dev == NULL gives value and inverse only.  Errors: -11 n_dev NULL, -2 layout invalid or
 *   planned with m != n, -1 invalid kernel program, -14 info_dev, -15 out_dev, -17 work NULL or too small. */
int gpk_assemble_inverse_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                                int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                                const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                                const int64_t* n_dev, void* W, void* stream);
int gpk_potrf_aug_ragged_ex(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, int32_t flags,
                            const int64_t* n_dev, const int64_t* m_dev, void* stream);
int gpk_grad_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                    const double* X, int64_t x_bstride, const int64_t* n_dev, const void* W,
                    const int32_t* info_dev, double* grad_dev, void* work, size_t work_bytes, void* stream);
int gpk_nlml_grad_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                         const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                         const double* y, int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv,
                         int32_t* info_dev, double* out_dev, double* grad_dev, void* work, size_t work_bytes,
                         void* stream);

/* Held-out mean squared error and its gradient for every batch member (fp64; entries added without a new ABI number,
 * found by symbol like gpk_op_supported): the objective of MeanSquaredError.get_metric (Metrics/MeanSquaredError.py:
 * 26-42) and of CrossValidation's default metric, differentiated as the reference's tape would.  The layout is
 * planned with m >= 1 test points; W is factored as gpk_assemble + gpk_potrf_aug leave it (test rows V = K_s^T L^-T,
 * y row z = L^-1 y, -mu in the corner's y row).  With r = mu - ys, alpha = L^-T z and q = L^-T (V^T r):
 *   mse = r^T r / m,
 *   d mse / d hyp[p] = (2/m) [ sum_it alpha_i r_t dk(x_i, xs_t)/d hyp[p] - sum_ij q_i alpha_j dk(x_i, x_j)/d hyp[p] ],
 *   d mse / d noise  = -(2/m) q^T alpha
 * -- two rank-one weights: no inverse and no n x n cotangent is formed, and the factorisation is the n^3/3 one.
 *
 * gpk_mse_grad_workspace_bytes: bytes of `work` for both entries (host only); 0 for a kernel program that is not
 *   valid for the layout's dimension, or a layout with m < 1.
 * gpk_mse_backward: the pass alone on an already factored W: one kernel for r, sum r^2 and the right-hand sides
 *   V^T r and z, the batched backward solve (as gpk_trsv, trans = 1) on both, one tile pass over the lower
 *   TRAIN x TRAIN and the TEST x TRAIN 64-tiles that re-evaluates the kernel program, and a fixed-order reduction (no
 *   floating-point atomics: the same inputs give the same bits).  ys[b*ys_bstride + t]: test targets.
 *   out_dev[b*4 + {0,1,2,3}] = {mse, sum r^2, m_b, n_b}; grad_dev[b*(n_hyp+1) + p] laid out as gpk_nlml_grad's, the
 *   noise last.  Where info_dev[b] != 0 the mse is +inf and the gradient NaN -- including info = -1, which a
 *   persistent factorisation sets on the members a timed-out wait left unfinished (gpk_tune "chain_timeout_ms"), as
 *   in gpk_nlml_grad; the other members are unaffected.
 *   Ragged batches: n_dev and m_dev both given (device int64 arrays, 1 <= n_dev[b] <= n, 1 <= m_dev[b] <= m: the
 *   device reads them blindly, the caller checks them) for a W factored by the _ragged entries, or both NULL.  What
 *   lies in X / Xs / ys past a member's own counts is never read.
 *   Errors: -1 invalid kernel program, -2 layout invalid or planned with m < 1, -30 layout planned with GPK_F32,
 *   -3 hyp_dev, -5 X, -7 Xs, -9 ys, -11 only one of n_dev / m_dev, -13 W, -14 Winv, -15 info_dev, -16 out_dev,
 *   -17 grad_dev, -18 work NULL or too small.
 * gpk_mse_grad: memset of info + gpk_assemble + gpk_potrf_aug (their _ragged twins when n_dev / m_dev are given) +
 *   gpk_mse_backward, whose first kernel is the read-out (gpk_finalize is not run: out_dev is the four values above).
 *   Errors: -1, -2, -30 as above, -3 hyp_dev, -5 noise_dev, -7 X, -9 Xs, -11 y, -13 ys, -15 only one of n_dev / m_dev,
 *   -17 W, -18 Winv, -19 info_dev, -20 out_dev, -21 grad_dev, -22 work NULL or too small. */
size_t gpk_mse_grad_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay);
int gpk_mse_backward(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                     const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride, const double* ys,
                     int64_t ys_bstride, const int64_t* n_dev, const int64_t* m_dev, const void* W, const void* Winv,
                     const int32_t* info_dev, double* out_dev, double* grad_dev, void* work, size_t work_bytes,
                     void* stream);
int gpk_mse_grad(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                 const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride, const double* Xs,
                 int64_t xs_bstride, const double* y, int64_t y_bstride, const double* ys, int64_t ys_bstride,
                 const int64_t* n_dev, const int64_t* m_dev, void* W, void* Winv, int32_t* info_dev, double* out_dev,
                 double* grad_dev, void* work, size_t work_bytes, void* stream);

/* Leave-one-out cross-validation for every batch member (fp64; entries added without a new ABI number, found by symbol
 * like gpk_op_supported): Rasmussen & Williams 5.4.2.  The layout is planned with m = n and W factored as
 * gpk_assemble_inverse + gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY) leave it (corner -K^-1, the corner's y row -alpha^T).
 * With d_i = (K^-1)_ii the prediction of point i from the other n - 1 points is
 *   mu_i = y_i - alpha_i / d_i,  sigma_i^2 = 1 / d_i   (d_i > 0 wherever info == 0),
 * so all n refits are an O(n) read-out.  loss selects f = sum_i phi(alpha_i, d_i):
 *   GPK_LOO_LPD  minus the LOO log predictive density (minus R&W eq. 5.13, summed like -LML):
 *                phi = 1/2 log 2 pi - 1/2 log d + alpha^2 / (2 d)
 *   GPK_LOO_MSE  the LOO mean squared error: phi = (alpha / d)^2 / n
 * and the gradient follows from d alpha = -K^-1 dK alpha, d d_i = -(K^-1 dK K^-1)_ii:
 *   d f / d K = G = -1/2 (alpha u^T + u alpha^T) - K^-1 diag(phi_d) K^-1,  u = K^-1 phi_alpha,
 *   d f / d hyp[p] = sum_ij G_ij dK_ij / d hyp[p],  d f / d noise = tr G
 * -- one n^3 product on the f64 matrix cores (lower tiles only) for the whole cotangent, then the tile pass of
 * gpk_nlml_grad over it.  Fixed-order sums, no floating-point atomics: the same inputs give the same bits.  W is only
 * read.
 *
 * gpk_loo_workspace_bytes: bytes of `work` for both entries (host only); 0 for an invalid kernel program, a layout
 *   planned with m != n or with GPK_F32.
 * gpk_loo_backward: the pass alone on a W factored by gpk_nlml_grad (or gpk_nlml_grad_ragged) with any grad_dev.
 *   y[b*y_bstride + i]: the targets that were assembled (detrended ones when a mean function was subtracted); mu is in
 *   those units.  out_dev[b*4 + {0,1,2,3}] = {f, sum_i (alpha_i / d_i)^2, sum_i log sigma_i^2, n_b};
 *   mu_dev[b*n + i], var_dev[b*n + i]: the LOO predictions (either may be NULL; zeros past a ragged member's n_b);
 *   grad_dev[b*(n_hyp+1) + p] laid out as gpk_nlml_grad's, the noise last.  grad_dev == NULL: value and predictions
 *   only (the read-out kernels alone).  Where info_dev[b] != 0 f is +inf, the gradient and the predictions NaN --
 *   including info = -1 of a timed-out persistent factorisation; the other members are unaffected.
 *   Ragged batches: n_dev (device int64, 1 <= n_dev[b] <= n, read blindly) for a W factored by the _ragged entries,
 *   or NULL.  What lies in X / y past a member's own count is never read, nor is any element of the corner there.
 *   Errors: -1 unknown loss, -2 invalid kernel program, -3 layout invalid or planned with m != n, -30 layout planned
 *   with GPK_F32, -4 hyp_dev, -6 X, -8 y, -11 W, -12 info_dev, -13 out_dev, -17 work NULL or too small.
 * gpk_loo_grad: memset of info + gpk_assemble_inverse + gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY) (their _ragged twins
 *   when n_dev is given) + gpk_loo_backward (gpk_finalize is not run: out_dev is the four values above).
 *   Errors: -1, -2, -3, -30 as above, -4 hyp_dev, -6 noise_dev, -8 X, -10 y, -13 W, -14 Winv, -15 info_dev,
 *   -16 out_dev, -20 work NULL or too small.
 * Every argument check precedes any device work.  gpk_timing_read classes of the pass: 4 the read-out, 5 u, 3 the
 * cotangent product (with its n^3 flops per member), 6 the tile pass. */
enum { GPK_LOO_LPD = 0, GPK_LOO_MSE = 1 };
size_t gpk_loo_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay);
int gpk_loo_backward(int32_t loss, const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                     int64_t hyp_stride, const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                     const int64_t* n_dev, const void* W, const int32_t* info_dev, double* out_dev, double* mu_dev,
                     double* var_dev, double* grad_dev, void* work, size_t work_bytes, void* stream);
int gpk_loo_grad(int32_t loss, const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                 const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride, const double* y,
                 int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv, int32_t* info_dev, double* out_dev,
                 double* mu_dev, double* var_dev, double* grad_dev, void* work, size_t work_bytes, void* stream);

/* Plain kernel matrix K[i*ldk + j] = k(X_i, Y_j) (+ diag_add where i == j) for i < n, j < m.
 * uplo: 0 = full, 1 = lower triangle only.  dtype selects the stored element type. */
int gpk_kernel_matrix(const gpk_kdesc* kd, const double* hyp_dev, int dtype, int uplo,
                      const double* X, int64_t n, const double* Y, int64_t m, int32_t d,
                      double diag_add, void* K, int64_t ldk, void* stream);

/* Triangular solve with the factor held in W (first n_pad columns):
 *   trans = 0: x <- L^-1 x      trans = 1: x <- L^-T x
 * x is fp64 of length n_pad per batch member (batch stride n_pad; entries >= n must be 0). */
int gpk_trsv(const gpk_layout* lay, int trans, const void* W, const void* Winv, double* x,
             void* stream);

/* y <- alpha A x + beta y for a row-major fp64 matrix A [n, m] (leading dimension lda >= m).
 * The matrix-vector products of the non-Cholesky numerical handlings of the metrics:
 * A p_k of linear_cg (Auxiliary/LinearConjugateGradients.py:44-45) and inv(K) y of
 * get_alpha_strict_inverse (Metrics/Metrics.py:132-133).  Timed under class 5. */
int gpk_gemv(const double* A, int64_t n, int64_t m, int64_t lda, const double* x, double* y, double alpha,
             double beta, void* stream);

/* ------------------------------------------------------ workspace-style entries
 * The flat signatures of the survey's boundary sketch: one caller scratch buffer of
 * gpk_workspace_bytes(op, dtype, n, m, batch) bytes replaces the layout and W / Winv (the sketch's
 * gpk_trsv_lower / gpk_posterior take that buffer as two extra arguments).  The single-problem gpk_nlml of
 * the sketch is gpk_nlml_batched with batch = 1.  GPK_WS_POTRF: fp64 or fp32; GPK_WS_TRSV, GPK_WS_POSTERIOR
 * (m = test points): fp64.  0 for an unsupported combination. */
enum { GPK_WS_NLML = 0, GPK_WS_POTRF = 1, GPK_WS_TRSV = 2, GPK_WS_POSTERIOR = 3 };
size_t gpk_workspace_bytes(int op, int dtype, int64_t n, int64_t m, int32_t batch);

/* x <- L^-1 x (trans 0) or L^-T x (trans 1) for a caller's lower-triangular fp64 L [n, ldl] (row-major, the
 * upper triangle not read) and a device vector x [n]: the triangular_solve of get_L_alpha
 * (Statistics/CovarianceMatrix.py:256-265) on an arbitrary factor.  The 128 x 128 diagonal blocks of L are
 * inverted once into the workspace (forward substitution), then the blocked solve of gpk_trsv runs on L itself. */
int gpk_trsv_lower(int dtype, int trans, const double* L, int64_t n, int64_t ldl, double* x, void* work,
                   size_t work_bytes, void* stream);

/* Posterior of a GP from a caller's factor L [n, ldl] of K + noise I and alpha = (K + noise I)^-1 y
 * (Statistics/Auxiliary.py:57-103, GaussianProcess.predict): mu [m] = K_s^T alpha (may be NULL) and, if var is not
 * NULL, var_mode 0: var [m] = diag(K_ss - V^T V), var_mode 1: var [m, ldv] = K_ss - V^T V, with K_s = k(X, Xs),
 * V = L^-1 K_s (blocked, MFMA GEMMs against the inverted diagonal blocks).  var_mode 0 takes k(x*, x*) from the
 * first test point (every kernel of a descriptor is stationary).  fp64.  (The augmented factorisation's test rows
 * -- gpk_assemble with Xs + gpk_potrf_aug + gpk_finalize -- give the same without a separate pass over L.) */
int gpk_posterior(const gpk_kdesc* kd, const double* hyp_dev, int dtype, const double* L, int64_t ldl,
                  const double* alpha, const double* X, int64_t n, const double* Xs, int64_t m, int32_t d,
                  int32_t var_mode, double* mu, double* var, int64_t ldv, void* work, size_t work_bytes,
                  void* stream);

/* -LML of `batch` hyperparameter / noise candidates on shared X [n, d], y [n] (device):
 * hyp_dev [batch][kd->n_hyp], noise_dev [batch], nlml_dev [batch] (+inf where info_dev[b] != 0; info_dev[b] = -1:
 * the persistent launch timed out, see Conventions -- repeat the call with gpk_tune("chain", 0)).
 * LogLikelihood.get_metric for each candidate (Metrics/LogLikelihood.py:30-65). */
int gpk_nlml_batched(const gpk_kdesc* kd, int32_t batch, const double* hyp_dev, const double* noise_dev, int dtype,
                     const double* X, const double* y, int64_t n, int32_t d, void* work, size_t work_bytes,
                     double* nlml_dev, int32_t* info_dev, void* stream);

/* In-place lower Cholesky of a row-major fp64 (double*) or fp32 (float*, dtype GPK_F32: factored on the f32
 * MFMA path) A [n, lda] (upper triangle untouched, LAPACK potrf semantics) through the blocked MFMA
 * factorisation: tf.linalg.cholesky of get_L_K
 * (Statistics/CovarianceMatrix.py:247-254).  *info_dev: 0 or the first non-positive pivot
 * (1-based), or -1 when the persistent launch timed out (A undefined; see Conventions); *logdet_dev (may be
 * NULL) = 2 sum log diag L (Metrics/Metrics.py:152-154). */
int gpk_potrf_lower(int dtype, void* A, int64_t n, int64_t lda, void* work, size_t work_bytes, int32_t* info_dev,
                    double* logdet_dev, void* stream);

/* ---------------------------------------------------------------- approximation paths (§8f.4)
 * Building blocks of the Nyström / SKC / SKI matrices of the reference
 * (Statistics/Nystroem_K.py, Metrics/SkcLogLikelihood.py, Metrics/StructuredKernelInterpolation.py);
 * the resulting dense matrices are factored through gpk_assemble_dense + gpk_potrf_aug. */

/* Training block of the augmented matrix from a caller matrix A [n, lda] (fp64; the lower
 * triangle is read and mirrored) + noise[b] on its diagonal, instead of a kernel evaluation
 * (the metrics' get_covariance_matrix for an approximate K, Metrics/Metrics.py:113-126).  Extra
 * rows: E [m, n] (corner 0: it becomes -E A^-1 E^T) or, with eye != 0 and a layout planned with
 * m = n, the identity (corner -A^-1 after gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY)). */
int gpk_assemble_dense(const gpk_layout* lay, const double* A, int64_t lda, int64_t a_bstride,
                       const double* noise_dev, int64_t noise_stride, const double* E, int64_t e_bstride,
                       int32_t eye, const double* y, int64_t y_bstride, void* W, void* stream);

/* C <- alpha op(A) op(B) + beta C, row-major fp64, op(A) [M, K], op(B) [K, N], batched by
 * strides (f64 MFMA 16x16x4, 64 x 64 tiles): the tf.matmul / tf.tensordot products of
 * Nystroem_K.py:62, :81-88, :98-104 and StructuredKernelInterpolation.py:25. */
int gpk_dgemm(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, double alpha,
              const double* A, int64_t lda, int64_t a_bstride, const double* B, int64_t ldb, int64_t b_bstride,
              double beta, double* C, int64_t ldc, int64_t c_bstride, int32_t batch, void* stream);

/* Symmetric eigendecomposition A = V diag(lam) V^T (V [m, m] row-major, eigenvectors in its
 * columns) by two-sided cyclic Jacobi (round-robin pairs, one launch per round), batched.  The
 * spectral half of tf.linalg.pinv (Nystroem_K.py:53).  Synchronises the stream once per sweep;
 * *sweeps_out = sweeps run (the last one without rotations).  work: gpk_syevj_workspace_bytes. */
size_t gpk_syevj_workspace_bytes(int64_t m, int32_t batch);
int gpk_syevj(int64_t m, int32_t batch, const double* A, int64_t lda, int64_t a_bstride, double* V, double* lam,
              void* work, size_t work_bytes, int32_t max_sweeps, int32_t* sweeps_out, void* stream);

/* Symmetric eigendecomposition, tridiagonal route (the default of the metrics): Householder
 * tridiagonalisation, divide and conquer on the tridiagonal matrix (deflation, Gu-Eisenstat eigenvectors,
 * MFMA GEMM merges), compact-WY back-transformation on the f64 MFMA GEMM.  Same outputs as gpk_syevj
 * (V [m, m] row-major, eigenvectors in its columns; lam in no particular order); A's lower triangle is read.
 * m <= 46340 (merged blocks above 4096 rows sort in the workspace instead of LDS, and above 16384 rows their
 * gather stages each row in the workspace too).  Asynchronous on the stream.
 * work: gpk_syevd_workspace_bytes(m) (reused across the batch). */
size_t gpk_syevd_workspace_bytes(int64_t m);
int gpk_syevd(int64_t m, int32_t batch, const double* A, int64_t lda, int64_t a_bstride, double* V, double* lam,
              void* work, size_t work_bytes, void* stream);

/* U = V diag(mu) with mu_i = 1 / lam_i (mode 0; pinv = U V^T), 1 / sqrt(lam_i) (mode 1;
 * pinv = U U^T) or 1 / sqrt(|lam_i|) (mode 2; pinv = U diag(sign lam) U^T, for an indefinite matrix) for
 * |lam_i| > rcond max|lam| and 0 otherwise -- tf.linalg.pinv's cutoff (rcond < 0: its default 10 m eps).
 * rank_dev[b] = kept eigenvalues, -1 if mode 1 keeps a negative one. */
int gpk_pinv_factor(int64_t m, int32_t batch, const double* V, const double* lam, double rcond, int32_t mode,
                    double* mu, double* U, int32_t* rank_dev, void* stream);

/* Reverse mode of pinv for symmetric matrices (tf.linalg.pinv, Nystroem_K.py:53, as TensorFlow's tape
 * differentiates it): with lam, V the eigendecomposition (gpk_syevd or gpk_syevj) and mu the mode-0 factors of
 * gpk_pinv_factor, and T = V^T Pbar V for the adjoint Pbar of pinv(A), replaces T (in place, [batch, m, m])
 * by F o (T + T^T)/2 with F_ij = (mu_i - mu_j) / (lam_i - lam_j) (-mu_i mu_j for two kept values, 0 for two
 * dropped ones); the adjoint of A is then V T V^T. */
int gpk_pinv_backward_scale(int64_t m, int32_t batch, const double* lam, const double* mu, double* T, void* stream);

/* SKI interpolation weights W [n, m] (row-major) of training points X [n, d] on inducing points
 * Z [m, d]: get_weight_matrix (StructuredKernelInterpolation.py:31-49), expanded-norm euclidean
 * distances, nearest (all ties) 1 - d1 / (d1 + d2), second nearest d1 / (d1 + d2).
 * work: 2 n + 1 doubles. */
int gpk_ski_weights(const double* X, int64_t n, const double* Z, int64_t m, int32_t d, double* Wm, double* work,
                    void* stream);

/* Pairwise distance matrices out[b] [n, m] (row stride ldo) of A[b] [n, d] and B[b] [m, d] (row-major),
 * replacing gpbasics/Auxiliary/Distances.py: mode 0 euclidian_distance (:4-7, the expanded norm
 * sqrt(|a|^2 - 2 a.b + |b|^2), unclamped: NaN where rounding makes it negative), 1 manhattan_distance
 * (:10-12), 2 the direct euclidean sqrt(sum (a - b)^2).  Batch strides 0 broadcast one operand. */
int gpk_distance_matrix(int mode, const double* A, int64_t n, int64_t a_bstride, const double* B, int64_t m,
                        int64_t b_bstride, int32_t d, int32_t batch, double* out, int64_t ldo, int64_t o_bstride,
                        void* stream);

/* Reverse mode of the kernel matrix K = kernel(X, Z) (X [n, d], Z [m, d], hyp_dev [kd->n_hyp], all
 * device fp64) for a weight matrix G [n, ldg] -- or, with G = NULL, the rank-1 weights G_ij = gu[i] gv[j]
 * (gu [n], gv [m]) -- (the adjoint of K, e.g. what tf.GradientTape hands back
 * to get_tf_tensor, Optimizer/Fitter.py:124-132 / :155-156, through the Nystroem metrics'
 * K_nm and K_mm, Statistics/Nystroem_K.py:36-47):
 *   grad_hyp[p]     = sum_ij G_ij dK_ij / d hyp_p        (device [n_hyp]; may be NULL if n_hyp == 0)
 *   grad_z[j*d + k] = sum_i  G_ij dK_ij / d Z_jk         (device [m, d]; NULL: not computed)
 * For a symmetric K(Z, Z) pass X = Z and G + G^T: grad_z is then the full derivative and grad_hyp
 * twice the hyperparameter adjoint.  Derivatives of the distance terms at coincident points are 0
 * (tf.abs' sign(0); TensorFlow would give NaN through the SE kernel's sqrt-then-square there).
 * work: gpk_kernel_vjp_workspace_bytes(kd, n, m, d, grad_z != NULL).  Deterministic (fixed-order
 * reductions). */
size_t gpk_kernel_vjp_workspace_bytes(const gpk_kdesc* kd, int64_t n, int64_t m, int32_t d, int32_t want_z);
int gpk_kernel_vjp(const gpk_kdesc* kd, const double* hyp_dev, const double* X, int64_t n, const double* Z, int64_t m,
                   int32_t d, const double* G, int64_t ldg, const double* gu, const double* gv, double* grad_hyp,
                   double* grad_z, void* work, size_t work_bytes, void* stream);

/* The derivative matrices of K = kernel(X, Z), written as planes (added without a new ABI number; look the symbols up
 * like gpk_op_supported):
 *   J[b*j_bstride + p*plane_stride + i*ldj + j] = d k(X_b,i, Z_b,j) / d hyp_b[p]   for p < n_hyp, i < n, j < m.
 * X [batch][n, d] (member stride x_bstride), Z [batch][m, d] (z_bstride), hyp_dev [batch][n_hyp] (hyp_stride), all
 * device fp64; a stride of 0 shares the operand between the members.  The derivatives are the analytic ones of the
 * formulas the library evaluates, those gpk_kernel_vjp and gpk_nlml_grad sum: sign(l) for the Matern kernels' |l|, 0
 * for the distance terms at coincident points, 0 for the hard change-point mask.  A change point shared by two windows
 * holds the sum of both windows' terms.  Every element of every plane is written, structural zeros included, so J need
 * not be cleared; nothing outside i < n, j < m is touched.  No reduction and no atomics: the same inputs give the same
 * bits, and a member of a batch the bits of a single call.
 * gpk_kernel_jacobian_workspace_bytes: bytes of `work` (host only); 0 -- the planes are written directly, and `work`
 *   may be NULL.
 * Errors: -1 invalid kernel program (or kd->dim != d), -2 hyp_dev, -3 hyp_stride, -4 batch (1 .. 65535), -5 X, -6 n,
 *   -7 x_bstride, -8 Z, -9 m, -10 z_bstride, -11 d, -12 J, -13 ldj < m, -14 plane_stride < (n-1) ldj + m,
 *   -15 j_bstride smaller than one member's planes.  n_hyp == 0 returns 0 and writes nothing. */
size_t gpk_kernel_jacobian_workspace_bytes(const gpk_kdesc* kd, int64_t n, int64_t m, int32_t d);
int gpk_kernel_jacobian(const gpk_kdesc* kd, const double* hyp_dev, int64_t hyp_stride, int32_t batch, const double* X,
                        int64_t n, int64_t x_bstride, const double* Z, int64_t m, int64_t z_bstride, int32_t d,
                        double* J, int64_t ldj, int64_t plane_stride, int64_t j_bstride, void* work, size_t work_bytes,
                        void* stream);

/* Fisher information of the hyperparameters and the noise (added without a new ABI number; fp64 only):
 *   F_pq = 1/2 tr(K^-1 d_pK  K^-1 d_qK),  p, q <= n_hyp,  d_{n_hyp} K = d K / d noise = I,
 * the expected Hessian of -LML, for every member of a layout planned with m = n whose W is factored as gpk_nlml_grad
 * (or gpk_assemble_inverse + gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY)) leaves it: the corner holds -K^-1.  W is only
 * read.  hyp_dev, X: the operands of that factorisation.  fisher_dev[b*(n_hyp+1)^2 + p*(n_hyp+1) + q], hyperparameters
 * in the program's order, the noise last; F_pq and F_qp are the same bits; the whole matrix of member b is NaN where
 * info_dev[b] != 0.  Per member: K^-1 mirrored into a dense matrix, the planes d_pK (lower tiles of
 * gpk_kernel_jacobian's kernel, mirrored: symmetric bit for bit), T_p = K^-1 d_pK on the f64 matrix cores (gpk_dgemm's
 * kernel, 2 n_hyp n^3 flops), then 1/2 sum_ab T_p[a,b] T_q[b,a] per pair with fixed-order sums -- no atomics, the same
 * inputs give the same bits.  Members are processed one after the other through the one workspace:
 * gpk_fisher_workspace_bytes = 8 ((2 n_hyp + 1) n^2 + (n_hyp+1)(n_hyp+2)/2 ceil(n/64)^2) bytes, whatever the batch
 *   (host only); 0 for an invalid kernel program, a layout planned with m != n or with GPK_F32.
 * Errors: -1 invalid kernel program, -2 layout invalid, planned with m != n or with GPK_F32, -3 hyp_dev, -5 X, -7 W,
 *   -8 info_dev, -9 fisher_dev, -11 work NULL or too small.  gpk_timing_read class 5 (gpk_dgemm's). */
size_t gpk_fisher_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay);
int gpk_fisher(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride, const double* X,
               int64_t x_bstride, const void* W, const int32_t* info_dev, double* fisher_dev, void* work,
               size_t work_bytes, void* stream);

/* Posterior mean and latent variance at new points from a kept factorisation (added without a new ABI number; fp64
 * only): for member `member` of a layout planned with m = n whose W is factored as gpk_nlml_grad (or
 * gpk_assemble_inverse + gpk_potrf_aug_ex(GPK_AUG_EXTRA_IDENTITY)) leaves it -- L^-T in the extra rows, -alpha^T in the
 * corner's y row -- and test points Xs [m, d]:
 *   mu[c]  = sum_t k(xs_c, x_t) alpha_t                                     (S/Auxiliary.py:57-66)
 *   var[c] = k(xs_c, xs_c) - sum_i (sum_{t <= i} k(xs_c, x_t) L^-1[i][t])^2   (the diagonal of S/Auxiliary.py:68-93)
 * var is the latent variance: no noise is added.  k(xs_c, xs_c) is evaluated per test point (programs with a linear
 * or a change-point window leaf are not stationary).  hyp_dev and X are the MEMBER's hyperparameters and training
 * points (the caller adds member * stride); W is the batch's base pointer and is only read.  Either of mu / var may be
 * NULL, not both.  The test points pass through `work` in chunks: as many per pass as work_bytes holds (all m, or a
 * multiple of 64).  Per pass: k(Xs, X) of the chunk by gpk_kernel_matrix's launch (the same bits), mu by gpk_gemv's
 * kernel, the row norms of the dense-times-triangular product on the f64 matrix cores (n^2 flops per test point; of
 * the extra rows only the upper triangle of the training block is read), partial sums per 64 columns added in index
 * order.  No atomics: the same inputs give the same bits, whatever the chunking.  info is not read: the caller checks
 * it (the outputs of a failed factorisation are meaningless).
 * gpk_predict_workspace_bytes = 8 rows (n_pad + 1 + ceil(n / 64)): the bytes one pass over `rows` test points needs,
 *   1 <= rows <= 65535 * 64 (host only); 0 for an invalid kernel program, a layout planned with m != n or with GPK_F32.
 * Errors: -1 invalid kernel program, -2 layout invalid, planned with m != n or with GPK_F32, -3 hyp_dev, -4 X, -5 W,
 *   -6 member outside 0 .. batch - 1, -7 Xs, -8 m <= 0, -9 mu and var both NULL, -11 work NULL or smaller than
 *   gpk_predict_workspace_bytes(kd, lay, min(m, 64)).  gpk_timing_read class 5 (gpk_dgemm's). */
size_t gpk_predict_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay, int64_t rows);
int gpk_predict(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, const double* X, const void* W,
                int32_t member, const double* Xs, int64_t m, double* mu, double* var, void* work, size_t work_bytes,
                void* stream);

/* The joint posterior covariance at new points from a kept factorisation (added without a new ABI number; fp64 only):
 * the m x m matrix of S/Auxiliary.py:83-93 (get_posterior_var), the input of the draws of S/GaussianProcess.py:97-110
 * (get_n_posterior_functions), without factoring again.  Two steps on the W that gpk_predict reads:
 *   gpk_predict_vt:   Vt[c][i] = sum_{t <= i} k(xs_c, x_t) L^-1[i][t], i < n        (V' = (L^-1 K_s)^T, [m, n])
 *   gpk_predict_cov:  C[a][b]  = k(xa_a, xb_b) - sum_{i < n} Va[a][i] Vb[b][i]       (Sigma = K_ss - V' V'^T, latent)
 * gpk_predict_vt takes gpk_predict's arguments (hyp_dev and X the MEMBER's, W the batch's base pointer, only read) and
 * passes the points through `work` in the same chunks; k(Xs, X) of a chunk is gpk_kernel_matrix's launch, the product
 * runs on the f64 matrix cores in the 64 x 64 tiles of gpk_predict, and of the extra rows only the upper triangle of
 * the training block is read.  It writes columns 0 .. n - 1 of each of the m rows of Vt (row stride ldv) and touches
 * nothing else.  The same bits for any chunking and for any order of the points.
 * gpk_predict_vt_workspace_bytes = 8 rows n_pad: the bytes one pass over `rows` test points needs; 0 under the
 *   conditions of gpk_predict_workspace_bytes.
 * Errors of gpk_predict_vt: -1 .. -8 as gpk_predict, -9 Vt NULL, -10 ldv < n, -11 work NULL or smaller than
 *   gpk_predict_vt_workspace_bytes(kd, lay, min(m, 64)).
 * gpk_predict_cov takes two sets of points with their rows of V' (Va [ma, lda], Vb [mb, ldb], columns >= n never
 * read) and writes every element of C [ma, mb] (row stride ldc): k(Xa, Xb) by gpk_kernel_matrix's launch (the same
 * bits), then per 64 x 64 tile the product summed over i in ascending order on the f64 matrix cores and subtracted
 * from k in the epilogue.  symmetric = 1 (Xa = Xb, Va = Vb, ma = mb, lda = ldb -- the same pointers): only the tiles
 * on or below the diagonal are computed and each element (a, b), a >= b, is written to (a, b) and to (b, a), so C is
 * symmetric bit for bit (half the product's work).  No atomics; an element's bits do not depend on the tile or the
 * block of points it sits in.  ma, mb <= 65535 * 64 (symmetric: 5792 * 64).
 * Errors of gpk_predict_cov: -i for the i-th argument -- -1 invalid kernel program (or not of dimension d), -2 d
 *   outside 1 .. GPK_MAX_DIM, -3 hyp_dev, -4 Xa, -5 ma, -6 Va, -7 lda < n, -8 Xb (symmetric: != Xa), -9 mb (symmetric:
 *   != ma), -10 Vb (symmetric: != Va), -11 ldb < n (symmetric: != lda), -12 n <= 0, -13 C, -14 ldc < mb, -15 symmetric
 *   not 0 or 1.
 * Every argument error returns before any device work.  gpk_timing_read class 5 (gpk_dgemm's) for both. */
size_t gpk_predict_vt_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay, int64_t rows);
int gpk_predict_vt(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, const double* X, const void* W,
                   int32_t member, const double* Xs, int64_t m, double* Vt, int64_t ldv, void* work, size_t work_bytes,
                   void* stream);
int gpk_predict_cov(const gpk_kdesc* kd, int32_t d, const double* hyp_dev, const double* Xa, int64_t ma,
                    const double* Va, int64_t lda, const double* Xb, int64_t mb, const double* Vb, int64_t ldb,
                    int64_t n, double* C, int64_t ldc, int32_t symmetric, void* stream);

/* A[b] += value * I (the "+ tf.eye(n) * noise" of Nystroem_K.py:68-69 and
 * StructuredKernelInterpolation.py:27). */
int gpk_add_diagonal(double* A, int64_t n, int64_t lda, int64_t a_bstride, int32_t batch, double value,
                     void* stream);

/* ------------------------------------------------------------------------ mean-function programs
 * The mean functions of the reference (MeanFunctionBasics/BaseMeanFunctions.py:37-193) and its mean-function
 * operators (MeanFunctionBasics/Operators.py:117-184) as one postfix program over the points, in value
 * (gpk_mean_eval: m(X), or the detrended targets y - m(X) of DataInput.get_detrended_y_*) and in reverse mode
 * (gpk_mean_vjp: what the reference's tape gives the fitter for the mean hyperparameters).
 * Op codes follow MeanFunctionManifestation (MeanFunctionBasics/MeanFunction.py:20-28); with d = dim and
 * s = sum_k (a_k x_k - b_k), accumulated k = 0 .. d-1 by fused multiply-adds: */
enum {
  GPK_MOP_C = 101,     /* c                              hyp [c]                               */
  GPK_MOP_LIN = 102,   /* sum_k a_k x_k                  hyp [a_0..a_{d-1}]                    */
  GPK_MOP_EXP = 103,   /* base ^ s  (pow)                hyp [a_0..a_{d-1}, b_0..b_{d-1}, base] */
  GPK_MOP_LOGIT = 104, /* c / (1 + exp(s))               hyp [a_0..a_{d-1}, b_0..b_{d-1}, c]    */
  GPK_MOP_ADD = 201,   /* binary: pops two, pushes the sum (left fold of an n-ary operator)   */
  GPK_MOP_MUL = 202    /* binary: pops two, pushes the product                                */
};                     /* (MeanFunctionManifestation.CP = 203 has no class upstream: not an op) */
/* Numerics.  Every value is used as given (no fabs): base <= 0 with a non-integer exponent gives IEEE NaN, as
 * tf.pow does.  The partial derivatives the reverse mode uses:
 *   EXP    d/da_k = m ln(base) x_k,  d/db_k = -m ln(base),  d/dbase = s base^(s-1)
 *   LOGIT  d/da_k = -m sg(s) x_k,    d/db_k = m sg(s),      d/dc = 1 / (1 + exp(s)),   sg(s) = 1 / (1 + exp(-s))
 * LOGIT's are evaluated in exactly this form -- two exponentials of opposite sign, each only ever in a denominator
 * next to 1 -- so value and partials stay finite for every finite s (the quotient form -c e^s / (1 + e^s)^2 is
 * inf / inf beyond s = 355): at s = 800 the value and every partial are 0, at s = -800 the value is c, d/dc is 1 and
 * the others 0.
 * The mean program: postfix like gpk_kdesc (children left to right, the binary op after each child beyond the
 * first); hyperparameters flattened in the reference's DFS order, so leaf offsets are consecutive from 0 and add up
 * to n_hyp.  In every node ard_slot is -1 and flags 0.  dim in [1, GPK_MAX_DIM], n_hyp <= GPK_MAX_HYP. */
typedef struct {
  int32_t n_nodes;
  int32_t n_hyp;
  int32_t dim;
  int32_t reserved; /* 0 */
  gpk_node nodes[GPK_MAX_NODES];
} gpk_mdesc;

/* 1 for every mean-program op (GPK_MOP_*) this library evaluates, else 0 (host only): the gpk_op_supported of the
 * mean programs -- a binding asks here (and finds the symbol missing in a library built before it existed). */
int gpk_mean_op_supported(int32_t op);

/* out[b*out_bstride + i] = m(X[b][i]; hyp[b])  (y == NULL), or  y[b*y_bstride + i] - m(X[b][i]; hyp[b])  -- the
 * detrended targets, one IEEE subtraction of the same m -- for i < n, b < batch.  X[b] = X + b*x_bstride is
 * [n, dim] row-major; hyp[b] = hyp_dev + b*hyp_stride; a stride of 0 shares hyp, X or y between the members.
 * Asynchronous on the stream.  -1: the program is not valid (stack discipline, per-op hyperparameter counts
 * against dim and n_hyp, an unknown op, non-zero flags, dim out of range); -5 / -7: n < 1 / batch < 1. */
int gpk_mean_eval(const gpk_mdesc* md, const double* hyp_dev, int64_t hyp_stride, const double* X, int64_t n,
                  int64_t x_bstride, int32_t batch, const double* y, int64_t y_bstride, double* out,
                  int64_t out_bstride, void* stream);

/* Reverse mode: grad_hyp[b*n_hyp + p] = sum_i g[b*g_bstride + i] dm(X[b][i]; hyp[b]) / dhyp_p  (device
 * [batch, n_hyp]).  g is contiguous within a member, so it may point into an identity-augmented factored W at
 * element y_row*ld + n_pad with g_bstride = w_batch_stride -- the -alpha row gpk_nlml_grad leaves there -- and the
 * result is then d(-LML)/d(mean hyperparameters), without a copy.  Deterministic: each workgroup of
 * GPK_MEAN_POINTS_PER_WG points writes its partial sums (a fixed shuffle tree, then the waves in order) to the
 * workspace and one ordered pass adds them up; no floating-point atomics, so two calls on the same inputs give the
 * same bits.  work: gpk_mean_vjp_workspace_bytes(md, n, batch) bytes (host only; 0 for a program that is not valid
 * or n < 1 or batch < 1 -- gpk_mean_vjp refuses those).  Errors as gpk_mean_eval. */
#define GPK_MEAN_POINTS_PER_WG 256
size_t gpk_mean_vjp_workspace_bytes(const gpk_mdesc* md, int64_t n, int32_t batch);
int gpk_mean_vjp(const gpk_mdesc* md, const double* hyp_dev, int64_t hyp_stride, const double* X, int64_t n,
                 int64_t x_bstride, int32_t batch, const double* g, int64_t g_bstride, double* grad_hyp, void* work,
                 size_t work_bytes, void* stream);

/* ------------------------------------------------------------------- multi-start L-BFGS fitter step
 * The optimiser the batched value + gradient evaluation (gpk_nlml_grad) exists to serve -- the role of the
 * reference's Optimizer/Fitter.py, as `batch` restarts that advance in lockstep: each iteration is one batched
 * evaluation of (f, g) at x_trial followed by ONE launch of gpk_fit_step, which runs every member's
 * bound-projected L-BFGS update, Armijo backtracking decision and convergence test on the device and writes the
 * next x_trial.  One wave64 per member (four members per 256-thread workgroup, no communication between waves);
 * lane j owns parameters j and j + 64; every inner product is a fixed-order shuffle tree (no floating-point
 * atomics: two runs give the same bits, and a member's trajectory does not depend on the batch it runs in).
 *
 * Per member, one call consumes (f_t, g_t, info_t) of the current x_trial:
 *   INIT    accept the trial as (x, f, g); d = -g on the free set; t = min(1, 1 / |d|_2); a failed trial ends the
 *           member with GPK_FIT_BAD_START.
 *   SEARCH  the trial fails if info_t != 0, f_t is not finite or any g_t is not finite.  It passes if
 *           f_t <= f + c1 g^T (x_trial - x) with the actual (projected) displacement and g^T (x_trial - x) <= 0 (so an
 *           accepted f never increases).  Pass: s = x_trial - x, y = g_t - g, pushed into the ring iff
 *           s^T y > 2.2e-16 |s| |y| -- otherwise the ring is cleared (the pairs held describe the curvature of another
 *           region; the next direction is then steepest descent); accept, count one iteration; GPK_FIT_CONVERGED_G if the projected-gradient
 *           inf-norm <= gtol, else GPK_FIT_CONVERGED_F if f_prev - f <= ftol max(1, |f|, |f_prev|), else
 *           GPK_FIT_MAX_ITER at max_iter iterations; otherwise a new direction.  Fail: t <- t / 2; after
 *           max_backtracks halvings the history is cleared and the search restarts from steepest descent -- or, if
 *           the failing direction was steepest descent already, the member ends with GPK_FIT_STALLED.
 *   direction  free set F = {j : lo_j < hi_j, not (x_j = lo_j and g_j > 0), not (x_j = hi_j and g_j < 0)}; the
 *           two-loop recursion on g masked to F with gamma = s^T y / y^T y of the newest pair, masked to F again;
 *           if d^T g >= 0 the history is cleared and d = -g on F.  t = 1 for a quasi-Newton direction,
 *           min(1, 1 / |d|_2) for steepest descent.
 *   trial   x_trial = min(max(fma(t, d, x), lo), hi): the clamp is exact.
 * A member whose status is not GPK_FIT_RUNNING is frozen: x_trial stays at its accepted x and its state is not
 * written again.
 * The four entries were added without a new ABI number (nothing that existed changed meaning): a binding looks the
 * symbols up and finds them missing in a library built before them.
 *
 * State: member b's doubles start at state_dev + b * S, S = gpk_fit_state_bytes / (8 batch) =
 * GPK_FIT_HEADER + 5 n_par + m + 2 m n_par:
 *   [GPK_FIT_HEADER] header (integers stored as doubles): 0 phase (0 INIT, 1 SEARCH), 1 status, 2 iterations,
 *     3 backtracks of the running search, 4 pairs held, 5 ring slot the next pair goes to, 6 f, 7 t, 8 f_prev,
 *     9 1 if d is steepest descent, 10 evaluations consumed, 11 S, 12 m, 13 n_par, 14 .. 15 zero
 *   x [n_par], g [n_par], d [n_par], lo [n_par], hi [n_par], rho [m], S [m][n_par], Y [m][n_par]. */
enum {
  GPK_FIT_RUNNING = 0,
  GPK_FIT_CONVERGED_G = 1,
  GPK_FIT_CONVERGED_F = 2,
  GPK_FIT_MAX_ITER = 3,
  GPK_FIT_STALLED = 4,
  GPK_FIT_BAD_START = 5
};
#define GPK_FIT_HEADER 16
#define GPK_FIT_MAX_PAR (GPK_MAX_HYP + 1)
#define GPK_FIT_MAX_HISTORY 16

/* NULL where an entry takes one: m 8, max_iter 200, max_backtracks 20, c1 1e-4, gtol 1e-5, ftol 1e-9 */
typedef struct gpk_fit_opts {
  int32_t m;              /* pairs kept, 1 .. GPK_FIT_MAX_HISTORY */
  int32_t max_iter;       /* accepted steps, >= 1 */
  int32_t max_backtracks; /* halvings of one search, >= 0 */
  int32_t reserved;       /* 0 */
  double c1;              /* Armijo constant, in (0, 1) */
  double gtol;            /* >= 0 */
  double ftol;            /* >= 0 */
} gpk_fit_opts;

/* bytes of the state buffer (host only); 0, with a sentence in gpk_last_error, for n_par outside
 * 1 .. GPK_FIT_MAX_PAR, m outside 1 .. GPK_FIT_MAX_HISTORY, batch < 1 or any other invalid option */
size_t gpk_fit_state_bytes(int n_par, int batch, const gpk_fit_opts* opts);

/* x0 [batch] rows of n_par (row stride x0_stride >= n_par) clamped into [lo, hi] (device [n_par] each, shared by the
 * members, +-inf allowed, lo <= hi expected) -> the state's x and x_trial (row stride xt_stride >= n_par). */
int gpk_fit_init(int n_par, int batch, const gpk_fit_opts* opts, const double* x0_dev, int64_t x0_stride,
                 const double* lo_dev, const double* hi_dev, double* state_dev, double* x_trial_dev,
                 int64_t xt_stride, void* stream);

/* One step of every member: f_dev[b * f_stride], g_dev[b * g_stride + j] and info_dev[b] (may be NULL: 0) are the
 * evaluation at x_trial -- strided so that they may point into a factorisation's read-out ([batch][4], -LML first)
 * and its gradient buffer without a copy.  status_dev [batch] receives every member's status.  The history length
 * is the one gpk_fit_init wrote into the state (opts->m is only validated); a state whose n_par is not the call's
 * gets status -1 and is left alone. */
int gpk_fit_step(int n_par, int batch, const gpk_fit_opts* opts, const double* f_dev, int64_t f_stride,
                 const double* g_dev, int64_t g_stride, const int32_t* info_dev, double* state_dev,
                 double* x_trial_dev, int64_t xt_stride, int32_t* status_dev, void* stream);

/* The accepted point of every member: x_dev (row stride x_stride), f_dev [batch], g_dev (row stride g_stride),
 * iters_dev [batch]; each may be NULL.  A state whose n_par is not the call's is not read: every output given is
 * filled with NaN and iters_dev with -1 (the gpk_fit_step status -1 of this call). */
int gpk_fit_current(int n_par, int batch, const double* state_dev, double* x_dev, int64_t x_stride, double* f_dev,
                    double* g_dev, int64_t g_stride, int32_t* iters_dev, void* stream);

/* Per-kernel-class timing with HIP events recorded on the launch stream.
 * class: 0 assemble, 1 diag, 2 trsm, 3 update, 4 finalize, 5 trsv, 6 grad.
 * With folded columns (gpk_tune "ingroup" 4) the classes of a factorisation shift: a folded panel solve carries its
 * column's in-group update in class 2 (those flops leave class 3), and class 1 also holds the launches that form the
 * folded solves' operands with their 128 * 129 * 128 d flops per member and column -- work the algorithm does not
 * have, so class 1's flops (and the classes' total) exceed the closed form of the factorisation by exactly that, and a
 * class 1 rate is no longer that of the diagonal-block kernel alone. */
#define GPK_NUM_CLASSES 7
int gpk_timing_enable(int on);
/* synchronises the recorded events; returns totals since the last reset */
int gpk_timing_read(double* ms_by_class, int64_t* launches_by_class, double* flops_by_class,
                    double* bytes_by_class);
int gpk_timing_reset(void);

/* Scheduling knobs of the factorisation (no reference counterpart: tf.linalg.cholesky exposes
 * none).  Keys: "lookahead" (1: panel chain on a high-priority stream overlapping the bulk
 * trailing update, 0: one stream, 2: auto -- on from "la_min_blocks" (64) 128-blocks of the augmented
 * matrix, the default), "panel_stream" (the look-ahead's chain: 0 high-priority side stream, 1 the
 * caller's, 2 a normal-priority side stream), "fuse_trsm" (f64 panel solve inside the diagonal-block
 * launch while batch x (64-row tiles + 1) <= "fuse_trsm_max": 1 with the look-ahead off, 2 always,
 * 0 never; bitwise identical results; callers that overlap factorisations on several streams set
 * 0), "reserve_cus" (CUs masked off the bulk-update stream; read
 * when that stream is first created), "group" (panels per trailing update, K = 128 group), "group_first"
 * (panels of the first group), "fuse_kbuild" (K build inside the first trailing update),
 * "upd_band" (trailing-update tile order), "skip_zero_rows" (skip the MFMAs of the zero rows below
 * the y row), "upd_t128_min", "trsm_t128_min" (128-tile thresholds), "diag_version" (2: look-ahead
 * diagonal-block kernel, 1: the phase-serial one; bitwise identical results), "ingroup" (in-group
 * updates: 0 auto, 1 left-looking, 2 right-looking, 3 two-level left-looking, 4 two-level with folded columns -- a
 * column with earlier panels in its half is updated and solved by ONE panel-solve launch against the operand
 * [-L^-1 B | L^-1]; uniform f64 batches without identity rows, where the panel solve is a launch of its own and the
 * panel stream can hold the operand scratch -- not hipStreamPerThread and not a stream being captured, the condition
 * of the fused panel solve's counters; everywhere else 4 runs 3, so a captured call and the same call made eagerly
 * agree to summation order (about 1e-14 relative on -LML), not bit for bit, unless "ingroup" is set to 1-3; results
 * agree with 1-3 to summation order, not bitwise) with "rl_max_tiles"
 * (auto picks right-looking while batch x block rows stays below it, the folded two-level form otherwise),
 * "band_skip" (1: with identity extra rows, the grid leaves out the tiles of the structurally zero
 * band instead of launching them to exit at once), "group_eye" (panels per trailing update of the
 * identity-augmented factorisations, gpk_potrf_aug_ex / gpk_nlml_grad; "group" for the others),
 * "asm_generic" (1: the K build's interior tiles through the generic per-element loop as well; the
 * same bits, slower -- for A/B checks), "trd_split_m" (gpk_syevd: above this m, at most 1024, the
 * tridiagonalisation's A22 v runs over the chip, three launches per column, instead of one workgroup per
 * panel; default 1024), "chain" (every f64, batch-1, non-ragged factorisation with at most
 * "chain_max_p" (12416) rows -- identity-augmented ones (gpk_potrf_aug_ex, gpk_nlml_grad) while "chain_eye" (1) and
 * at most "chain_max_p_eye" (16640) rows -- that is not being captured runs as ONE persistent launch -- "chain_grid"
 * workgroups (0: one per CU), every wait bounded by "chain_timeout_ms": 1, the default, auto: unless a
 * factorisation this library enqueued on another stream of the device is still in flight (each
 * persistent launch claims every CU); 2 always; 0 never), with "chain_group" panels per deferred tile update
 * (0, the default: 4 below 80 diagonal blocks, 8 from there), "chain_uq" (1: the next diagonal block's update by each panel as 32-column quarter tasks; 0: one task
 * per 32-row slice; 2: slice r's panel solve and the next diagonal block's quarter updates as one task) and, for
 * batches, "chain_max_batch" members (8) while batch x p <= "chain_batch_max_rows" (17500).  Several persistent
 * launches may run side by side on different streams, each with "chain_grid" workgroups (a CU share): no launch
 * waits for another's workgroups (bench.py's C2 schedule: 8 in flight, 64 workgroups each on 256 CUs).
 * With "chain" 1 (auto) factorisations of fewer than "chain_min_p" (768) rows -- identity-augmented ones:
 * "chain_min_p_eye" (3072) -- keep the launch path (a handful of panels: its few launches are faster).
 * Identity-augmented plans take "chain_group_eye" (8) panels per deferred tile update (0: chain_group's
 * rule) and defer the corner's tile updates (-K^-1, read by no later task) in groups of
 * "chain_group_corner" (16) panels, except the last "chain_corner_tail" (8) panels, which keep "chain_group"; a
 * deferred (grouped) update covers only block columns at least "chain_group_la" (2) columns past the group's last
 * panel.  Every knob the planner reads is part of its plan cache key.
 * "asm_f32_fast" (1: the f32 K build of a single SE / MAT32 / MAT52 node writes its interior tiles with f64
 * distances and the f32 hardware sqrt / exp -- a few f32 ulps from the f64 build; 0: every tile through the
 * general f64 evaluation, A/B; "asm_f32_chunk" (4) consecutive lower tiles per workgroup).
 * "cp_skip" (1: on a tile where a change-point window leaf is exactly 0.0 for all 64 row points or all 64 column
 * points, the K build does not evaluate the window's MUL sibling and pushes +0.0 -- equal under == to the unskipped
 * value for finite sibling values; 0: every node on every tile, A/B).
 * "chain_xcd" (0; 1: the persistent launch's diagonal-chain tasks -- D, the next diagonal block's panel solves and
 * quarter updates -- as a second task list claimed first by up to "chain_xcd_seats" (16) workgroups of XCD 0, the
 * rest by everyone else, each workgroup falling back to the other list once its own is exhausted; measured no
 * faster).
 * "chain_f32" (1: f32 factorisations without identity rows take the persistent launch under the same rules --
 * chain_kernel<float>: f32 MFMA panel solves and tile updates, the diagonal blocks as the launch path's; bitwise
 * the f32 launch path's results; one slice-update task per slice whatever "chain_uq"; 0: the launch path).
 * Planner knobs of the persistent launch (all part of the plan cache key, all bitwise the launch path's results):
 * "chain_group_near" (2: the tile updates of the columns too near the diagonal for the deferred group go in
 * sub-groups of this many panels, for columns at least "chain_near_la" (1) past the sub-group's last panel; 1: one
 * panel at a time), "chain_u128" (2 auto, 1, 0: below the next diagonal block the next panel's column is updated by
 * one 128 x 128 tile task per block row instead of four 32-row slice tasks; auto: except below 48 diagonal blocks on
 * a grid of more than 2 workgroups per block), "chain_s128" (2 auto, 1, 0: the panel solves below the next diagonal
 * block as one task per block row; auto: on grids of at most 2 workgroups per diagonal block -- the CU-share launches
 * side by side -- and identity-augmented plans of at least 64 diagonal blocks).
 * "asm_feat" (1: the K build of a two-leaf SE + periodic tree at D = 4 or 8 computes the per-point features in a
 * pre-pass and runs its interior tiles on the f64 MFMA fast-tile kernel; 0: every tile stages its points itself
 * -- the same bits, slower; A/B).
 * "diag_debug" (0; timing-only ablation flags of the diagonal-block kernel, never set in production; GPK_DIAG_DEBUG).
 * "syevj_abs_tol_e3" (0; gpk_syevj: absolute rotation threshold in units of 1e-3 eps max|a_ii|).
 * A persistent launch whose wait timed out
 * sets info = -1 -- an infrastructure failure, not a non-positive pivot: the factorisation is
 * incomplete and W undefined; re-assemble and re-run it with "chain" 0 (the Python layer does,
 * engine.AugmentedFactorization).  "chain_force_timeout" (testing) makes the next `value` persistent
 * launches report a timeout at their first wait.
 * Stores the value and returns the previous one through *old (may be NULL); 0 or -1 (unknown
 * key).  Defaults come from the environment (GPK_LOOKAHEAD, GPK_RESERVE_CUS, ...). */
int gpk_tune(const char* key, int64_t value, int64_t* old);
/* One more gpk_tune key, the entry point's own like "chain_force_timeout" (process-wide only: gpk_tune_thread does not
 * take it; default 1, environment GPK_UPD_TRI): "upd_tri" -- uniform f64 128-tile group / half trailing updates run
 * their diagonal tiles and the y row's live 16-row block as lower-triangle work in a kernel of their own (1: after the
 * strictly lower tiles, 2: before them, 0: one kernel over all tiles; bitwise identical results on and below the
 * diagonal, the blocks above the diagonal of diagonal tiles are not written). */

/* Per-host-thread override of a gpk_tune knob (no reference counterpart): set = 1 pins `value` for
 * the calls of the calling thread only, set = 0 removes the thread's override (the global knob applies
 * again).  *old_value / *old_set (may be NULL) return the override in effect before the call (old_set
 * 0: none, *old_value is then the global value).  0 or -1 (unknown key). */
int gpk_tune_thread(const char* key, int64_t value, int32_t set, int64_t* old_value, int32_t* old_set);

/* Counters of the persistent factorisation: out[0] persistent launches enqueued (all threads),
 * out[1] factorisations that took the launch path because another stream was busy (chain = 1),
 * out[2] 1 if the calling thread's last factorisation was a persistent launch (its info must then be
 * checked for -1, see gpk_tune "chain"), out[3] forced timeouts still pending, out[4] (n >= 5 only: a
 * synchronous device read) persistent launches on the current device whose waits timed out so far (each
 * such launch aborted and set info = -1 on its unfinished members; forced timeouts included).
 * Writes min(n, 5). */
int gpk_chain_stats(int64_t* out, int32_t n);

/* The task list of the persistent single-member factorisation (gpk_tune "chain"; no reference
 * counterpart): the order in which the workgroups of its one launch claim the tasks, for an augmented
 * matrix with n_pad training rows, the y row at y_row and `grid` workgroups.  Four int32 per task:
 * type (0: factor diagonal block k; 1: solve 32-row slice r below block k; 2: slice r of block column
 * j = k + 1 -= panel k; 3: 128 x 128 tile (r, j) -= panel k), k, r, j.  Host only (no device call):
 * tasks_out may be NULL to query *ntasks; cap = its capacity in tasks. */
int gpk_chain_plan(int64_t n_pad, int64_t y_row, int32_t grid, int32_t* tasks_out, int64_t cap, int64_t* ntasks);
/* gpk_chain_plan with flags: GPK_AUG_EXTRA_IDENTITY plans the identity-augmented factorisation (gpk_potrf_aug_ex,
 * gpk_nlml_grad; y_row = n_pad + n): tasks that would only move the structurally zero parts of E L^-T are left
 * out, and a task word with bit 6 set updates cells no earlier task updated (its counter wait is for 0).  The
 * type word: type (bits 0..1) | (g - 1) << 2 (bits 2..5; type 3: an update over the g panels k .. k + g - 1;
 * type 2 with g > 1: the 32 x 32 quarter g - 2 of slice r in diagonal block j) | bit 6 | bit 7 (an SQ task of
 * "chain_uq" 2: the slice's panel solve, then the next diagonal block's quarter updates) | member << 8.
 * GPK_CHAIN_PLAN_F32: the plan of an f32 factorisation (chain_kernel<float>: one slice-update task per slice, the
 * f32 deferred-update depth). */
#define GPK_CHAIN_PLAN_F32 256
int gpk_chain_plan_ex(int64_t n_pad, int64_t y_row, int32_t grid, int32_t flags, int32_t* tasks_out, int64_t cap,
                      int64_t* ntasks);

/* The schedule of the launch path (no reference counterpart -- it replaces nothing in gpbasics; introspection only):
 * the launches and event edges gpk_potrf_aug / _ex / _ragged enqueue, in order, for this layout when the persistent
 * launch does not apply (gpk_tune "chain"), under the knobs in effect for the calling thread.  flags: those of
 * gpk_potrf_aug_ex.  counters: nonzero if the panel stream has the fused panel solve's ticket counters (every
 * ordinary stream; not hipStreamPerThread or a stream being captured; without them the stream has no operand scratch
 * either, so the plan then has no folded panel solve).  The plan is that of a uniform batch: gpk_potrf_aug_ragged runs
 * the same steps except that it never folds ("ingroup" 4 there is 3).  kbuild: nonzero for gpk_nlml's factorisation
 * with the K build fused into the first trailing update.  One step is GPK_LAUNCH_STEP_WORDS 8-byte words, 21 int64
 * and two doubles:
 *   0 kind (0 diagonal block, 1 panel solve, 2 trailing update, 3 event record, 4 wait for event, 5 the operand of a
 *     folded panel solve ("ingroup" 4): kblk, the columns [j0, j0 + kdepth) of block row kblk; the panel solve that
 *     follows it then has kdepth > 128 and also applies the kdepth - 128 columns left of its block column)
 *   1 stream (0 the caller's, 1 panel, 2 bulk; with the look-ahead off every step is on 0)
 *   2 event (record / wait: 0 fork, 1 panel, 2 bulk, 3 join_p, 4 join_b; else -1)
 *   3 role of an update (1 thin, 2 half, 3 look-ahead, 4 bulk, 5 a group's whole trailing update; else 0)
 *   4 timing class (gpk_timing_read; events -1)     5 kblk (diagonal block)
 *   6 trsm_tiles (diagonal block: 64-row tiles of the panel solve fused into the launch; then no step of kind 1)
 *   7 j0   8 row0   9 kdepth   10 tile edge   11 nt   12 c_lo   13 c_hi   14 zlo   15 zhi   16 bz0   17 bzn
 *   18 band   19 row_end   20 kbuild (the launch arguments of the same names)
 *   21 flops, 22 bytes (doubles: the algorithmic work gpk_timing_read accumulates for the launch).
 * Host only (no device call): steps_out may be NULL to query *nsteps; cap = its capacity in steps.  *first_group
 * (may be NULL): the panels of the first group -- the diagonal-block steps before the first step with kbuild set. */
#define GPK_LAUNCH_STEP_WORDS 23
int gpk_launch_plan(const gpk_layout* lay, int32_t flags, int32_t counters, int32_t kbuild, void* steps_out,
                    int64_t cap, int64_t* nsteps, int64_t* first_group);

#ifdef __cplusplus
}
#endif
#endif /* GPK_H */
