// The tuning knobs of libgpk (gpk_tune / gpk_tune_thread, gpk.h): one table, from which struct Tune, its
// environment-initialised process-wide instance and the name lookup are generated.  Plain C++17, no HIP header.
#pragma once

#include <stdint.h>

// Launch-shape thresholds (environment overrides for tuning runs).  One row per knob: K(field, default), with the
// record of why the default is what it is.  The gpk_tune key is the field's name and the environment variable is
// "GPK_" + the key in upper case; a row whose names differ states them: KN(field, default, key, environment name).
// The order of the rows does not matter.
#define GPK_KNOBS(K, KN)                                                                                               \
  K(upd_t128_min, 512)     /* 128 x 128 update tiles when at least this many (else 64 x 64) */                         \
  K(trsm_t128_min, 256)    /* 128-row panel-solve tiles when at least this many (else 64) */                           \
  KN(diag_dbg, 0, "diag_debug", "GPK_DIAG_DEBUG")                                                                      \
                           /* timing-only ablation flags of the diagonal kernel (never set in production) */           \
  K(lookahead, 2)          /* 1: panel chain on a high-priority side stream, 0: one stream, 2: auto (default:          \
                              on for large matrices, launch_lookahead) */                                              \
  K(la_min_blocks, 64)     /* auto look-ahead: on from this many 128-blocks of the augmented matrix */                 \
  K(fuse_trsm, 1)          /* f64: panel solve fused into the diagonal-block launch (1: look-ahead off only,           \
                              2: always; one workgroup per */                                                          \
  K(fuse_trsm_max, 256)    /*   64-row tile, each factoring the block) while batch x tiles <= fuse_trsm_max */         \
  K(reserve_cus, 32)       /* CUs kept free of the bulk trailing update for the panel chain (32: single N = 8192       \
                              6.46 -> 6.26 ms, -LML + gradient N = 4096 3.29 -> 3.04 ms, batches of 2 / 8 / 32         \
                              without pipelining +1.9 / +0.6 / +0.4 % against 8) */                                    \
  K(group, 8)              /* panels per trailing update (K = 128 group) */                                            \
  K(group_first, 8)        /* panels of the first group (a short first chain lets the bulk start early) */             \
  K(fuse_kbuild, 1)        /* gpk_nlml: K build fused into the first trailing update (single-node kernels) */          \
  K(upd_band, 0)           /* trailing-update tile order: 0 row-major, B > 0 bands of B tile rows */                   \
  K(skip_zero_rows, 1)     /* skip the MFMAs of the all-zero 16-row blocks below the y row */                          \
  K(syevj_abs_tol_e3, 0)   /* Jacobi: absolute rotation threshold in units of 1e-3 eps max|a_ii| */                    \
  K(diag_version, 2)       /* diagonal-block kernel: 2 look-ahead schedule, 1 phase-serial */                          \
  K(ingroup, 0)            /* in-group updates: 1 left-looking, 2 right-looking, 3 two-level, 4 two-level with the     \
                              columns' updates folded into their panel solves (uniform f64 plain batches; else 3),     \
                              0 auto (by batch: 2 or 4) */                                                             \
  K(rl_max_tiles, 256)     /* auto: right-looking while batch x (block rows) stays below this */                       \
  K(band_skip, 1)          /* identity extra rows: leave the zero band's tiles out of the grid */                      \
  K(group_eye, 4)          /* panels per trailing update of identity-augmented factorisations */                       \
  K(asm_generic, 0)        /* K build: interior tiles through the generic loop too (A/B; bitwise equal) */             \
  K(panel_stream, 0)       /* look-ahead panel chain: 0 high-priority side stream, 1 caller's stream,                  \
                              2 normal-priority side stream */                                                         \
  K(trd_split_m, 1024)     /* gpk_syevd: above this m the tridiagonalisation's A22 v runs over the chip (three         \
                              launches per column) instead of inside one workgroup per panel */                        \
  K(chain, 1)              /* single f64 factorisations as ONE persistent launch (chain_kernel): 1 auto (default: on   \
                              unless a factorisation enqueued on another stream of the device is still in flight --    \
                              each persistent launch claims every CU, so overlapped factorisations keep the launch     \
                              path: C2 at 4 in flight 1315 vs 779 evals/s), 2 always, 0 off */                         \
  K(chain_max_p, 12416)    /*   ... while the augmented matrix has at most this many rows */                           \
  K(chain_grid, 0)         /*   workgroups of that launch (0: one per CU) */                                           \
  K(chain_timeout_ms, 1000)  /* bound of every wait inside it (then info = -1) */                                      \
  K(chain_group, 0)        /*   panels per deferred tile update (1: every tile update one panel deep; 0: auto,         \
                                chain_group_for) */                                                                    \
  K(chain_max_batch, 8)    /* batches of up to this many members run as one persistent launch too ... */               \
  K(chain_batch_max_rows, 17500)  /* ... while batch x (rows of the augmented matrix) stays within this                \
                                     (batch x span, persistent vs launch path: N = 2048 x 8 1.15 vs 1.38 ms,           \
                                     4096 x 2 1.87 vs 2.53, 4096 x 4 2.83 vs 3.51; 4096 x 8 5.32 vs 5.07,              \
                                     2048 x 16 2.02 vs 1.94 -- profiles/r04_chain_batch.jsonl) */                      \
  K(chain_uq, 1)           /*   the next diagonal block's update split by 32-column quarter (0: one task per slice) */ \
  K(chain_eye, 1)          /*   identity-augmented factorisations (the gradient / explicit inverse) too (1: auto as    \
                                above, 0: never) */                                                                    \
  K(chain_max_p_eye, 16640)  /* ... while their augmented matrix has at most this many rows */                         \
  K(asm_feat, 1)           /* K build, two-leaf SE + periodic trees on MFMA: per-point features in a pre-pass          \
                              (pair_feat_kernel; 0: staged per tile, A/B -- bitwise equal) */                          \
  K(chain_min_p, 768)      /* chain = 1 (auto): the launch path below this many rows (a handful of panels: the         \
                              launch path's few launches win -- get_metric N = 128 / 256 / 384 0.119 / 0.165 / 0.216   \
                              vs 0.145 / 0.187 / 0.224 ms, equal at 512, the persistent launch ahead from 768,         \
                              profiles/r05ak_api_small_n_chain_vs_launch.jsonl) */                                     \
  K(chain_min_p_eye, 3072)   /* ... and for identity-augmented factorisations (value + gradient): N = 1024 / 1280      \
                                0.554 / 0.657 ms on the launch path vs 0.590 / 0.683, N = 1536 0.809 vs 0.786          \
                                (profiles/r05al_api_crossover.jsonl) */                                                \
  K(chain_group_corner, 16)  /* identity-augmented plans: panels per deferred update of the corner's tiles (-K^-1,     \
                                read by no later task) */                                                              \
  K(chain_corner_tail, 8)    /*   ... except the last this many panels, which keep chain_group */                      \
  K(chain_group_la, 2)       /* deferred (grouped) tile updates only for block columns at least this many columns      \
                                past the group's last panel */                                                         \
  K(asm_f32_fast, 1)       /* f32 K build of a single SE / MAT32 / MAT52 node: the interior tiles through f32_fast_kernel \
                              (f64 distances, f32 transcendentals; 0: every tile through the general f64 loop, A/B) */ \
  K(chain_group_eye, 8)    /* identity-augmented plans: panels per deferred tile update (0: chain_group's rule; 8: value + \
                              gradient N = 8192 11.33 vs 11.11 ms best, profiles/r06b_grad_sweep_8192.jsonl) */        \
  K(chain_xcd, 0)          /* persistent launch: the diagonal chain's tasks as a second list, claimed first by up to   \
                              chain_xcd_seats workgroups of XCD 0 (their hand-offs in one L2); 0: one list */          \
  K(chain_xcd_seats, 16)                                                                                               \
  K(asm_f32_chunk, 4)      /* f32_fast_kernel: consecutive lower tiles per workgroup (C3: 1 / 2 / 4 / 8 / 16 0.062 / 0.059 / \
                              0.059 / 0.063 / 0.073 ms, profiles/r06c_kb_c3_chunks.txt) */                             \
  K(chain_f32, 1)          /* f32 factorisations as one persistent launch too (chain_kernel<float>: f32 tile tasks, the \
                              diagonal blocks in f64 as the launch path's); 0: f32 keeps the launch path */            \
  K(chain_group_near, 2)   /* tile updates of the columns too near the diagonal for the deferred group: in sub-groups  \
                              of this many panels (same look-ahead rule; 1: panel by panel) */                         \
  K(chain_u128, 2)         /* the next panel's column below the next diagonal block: one 128 x 128 tile update per block \
                              row instead of four 32-row slice updates (1; 0: slice updates; 2 auto: slice updates only \
                              below 48 diagonal blocks on a grid of more than 2 workgroups per diagonal block) */      \
  K(chain_near_la, 1)      /* chain_group_near's sub-groups cover the columns at least this many past their last panel \
                              (1: C2 1866 -> 1884 evals/s, C3 474 -> 480, value + gradient N = 8192 10.6 -> 10.43 ms   \
                              against 2, profiles/r06u_near_la_ab.txt) */                                              \
  K(chain_s128, 2)         /* the panel solves below the next diagonal block: one task per block row (its slices one after \
                              another) instead of one per 32-row slice (1; 0: per slice; 2 auto: on a grid of at most 2 \
                              workgroups per diagonal block -- the CU-share launches side by side -- and for           \
                              identity-augmented plans of at least 64 diagonal blocks; N = 6144 within the spread either way) */ \
  K(cp_skip, 1)            /* K build of a tree with change-point window leaves: a window that is exactly 0.0 for all of a \
                              tile's row points or all of its column points skips its MUL sibling there (0: never, A/B; \
                              equal under == for finite sibling values) */

namespace gpk {

struct Tune {
#define GPK_TUNE_FIELD(field, dflt) int64_t field = dflt;
#define GPK_TUNE_FIELD_N(field, dflt, key, env) int64_t field = dflt;
  GPK_KNOBS(GPK_TUNE_FIELD, GPK_TUNE_FIELD_N)
#undef GPK_TUNE_FIELD
#undef GPK_TUNE_FIELD_N
};

// the integer value of an environment variable, dflt if it is unset or empty
int64_t env_i64(const char* name, int64_t dflt);

// The process-wide knobs: the table's defaults under the environment's overrides, read at the first call.
Tune& tune();

// the field a gpk_tune key names (nullptr: no such knob)
int64_t Tune::*knob_field(const char* key);

// The knobs in effect for one call on this thread: one snapshot per call, so a gpk_tune from
// another thread (ctypes releases the GIL during the enqueue) cannot change a decision midway.
Tune tune_now();

// Per-host-thread overrides (gpk_tune_thread): a caller that runs its own schedule -- e.g. the
// pipelined sweep's factorisations on several streams -- pins knobs for its own calls without
// changing them for other threads.  set: pin `value`, else drop the thread's override; *old_value / *old_set (may be
// null): the override in effect before the call (old_set 0: none, *old_value is then the global value).
void tune_thread_set(int64_t Tune::*field, int64_t value, bool set, int64_t* old_value, int32_t* old_set);

}  // namespace gpk
