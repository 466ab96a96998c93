// extern "C" entry points of libgpk.so (declared in include/gpk.h).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gpk_chain_plan.h"
#include "gpk_internal.h"
#include "gpk_kernels.h"
#include "gpk_launch_plan.h"
#include "gpk_tune.h"

#ifndef GPK_DIAG_PROF
#define GPK_DIAG_PROF 0
#endif

using namespace gpk;

namespace {

thread_local std::string g_err;

int fail_arg(int idx, const char* what) {
  g_err = std::string("invalid argument: ") + what;
  return -idx;
}

int fail_hip(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return (int)e > 0 ? (int)e : 1;
}

#define GPK_HIP(call, where)                         \
  do {                                               \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return fail_hip(e_, where); \
  } while (0)

// ------------------------------------------------------------------------------ event timing
struct TimedLaunch {
  int cls;
  hipEvent_t beg, end;
  double flops, bytes;
};

struct Timing {
  std::mutex mu;
  bool on = false;
  std::vector<TimedLaunch> pending;
  std::vector<hipEvent_t> pool;
  double ms[GPK_NUM_CLASSES] = {0};
  int64_t launches[GPK_NUM_CLASSES] = {0};
  double flops[GPK_NUM_CLASSES] = {0};
  double bytes[GPK_NUM_CLASSES] = {0};
};
Timing g_timing;

hipEvent_t take_event() {
  if (!g_timing.pool.empty()) {
    hipEvent_t e = g_timing.pool.back();
    g_timing.pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}

// Run `launch` bracketed by events on stream s when timing is on.
template <typename F>
hipError_t timed(int cls, double flops, double bytes, hipStream_t s, F&& launch) {
  if (!g_timing.on) return launch();
  std::lock_guard<std::mutex> lk(g_timing.mu);
  TimedLaunch t{cls, take_event(), take_event(), flops, bytes};
  hipEventRecord(t.beg, s);
  hipError_t e = launch();
  hipEventRecord(t.end, s);
  g_timing.pending.push_back(t);
  return e;
}

bool valid_kdesc(const gpk_kdesc* kd, int64_t d) {
  if (!kd || kd->n_nodes <= 0 || kd->n_nodes > GPK_MAX_NODES) return false;
  if (kd->n_hyp < 0 || kd->n_hyp > GPK_MAX_HYP || kd->dim != d) return false;
  if (kd->n_ard < 0 || kd->n_ard > GPK_MAX_ARD) return false;
  int sp = 0;
  for (int q = 0; q < kd->n_nodes; ++q) {
    const gpk_node& nd = kd->nodes[q];
    if (nd.op == GPK_OP_ADD || nd.op == GPK_OP_MUL) {
      if (sp < 2) return false;
      sp -= 1;
      continue;
    }
    // a leaf: its own flag rules, then its hyperparameters (node_params, gpk_kernels.h) inside the vector
    if (nd.op == GPK_OP_LIN) {
      // one offset per input dimension (+ sg); the node reads the raw points: no ARD slot, no distance form
      if (nd.flags & (GPK_NODE_ARD | GPK_NODE_SE_EXPANDED | GPK_NODE_STANDARD)) return false;
      if (nd.ard_slot != -1) return false;
    } else if (nd.op == GPK_OP_RQ) {
      // [l, a, (sg)]: the direct squared distance of the raw points only -- no ARD slot, no other distance form
      if (nd.flags & (GPK_NODE_ARD | GPK_NODE_SE_EXPANDED | GPK_NODE_STANDARD)) return false;
      if (nd.ard_slot != -1) return false;
    } else if (nd.op == GPK_OP_CPW) {
      // change-point window: 1-D inputs, one or two consecutive bounds, one mask form; reads the raw points
      if (kd->dim != 1) return false;
      if (cp_bounds(nd.flags) == 0) return false;
      if ((nd.flags & GPK_NODE_CP_SIGMOID) && (nd.flags & GPK_NODE_CP_APPROX)) return false;
      if (nd.flags & (GPK_NODE_SCALED | GPK_NODE_ARD | GPK_NODE_SE_EXPANDED | GPK_NODE_STANDARD)) return false;
      if (nd.ard_slot != -1) return false;
    } else if (nd.op == GPK_OP_SE || nd.op == GPK_OP_PER || nd.op == GPK_OP_MAT32 ||
               nd.op == GPK_OP_MAT52) {
      const bool ard = (nd.flags & GPK_NODE_ARD) != 0;
      if (ard && (nd.op == GPK_OP_PER || nd.ard_slot < 0 || nd.ard_slot >= kd->n_ard)) return false;
    } else {
      return false;
    }
    if (nd.hyp_offset < 0 || nd.hyp_offset + node_params(nd, (int)d) > kd->n_hyp) return false;
    if (++sp > 8) return false;
  }
  return sp == 1;
}

size_t elem_size(int dtype) { return dtype == GPK_F64 ? 8 : 4; }

// For every base node of the postfix program: the nodes (subtree roots) whose values multiply
// its value on the way to the root -- the siblings under each MUL ancestor.  d K / d k_node is
// the product of those values (ADD ancestors pass the adjoint through unchanged).
void adjoint_masks(const gpk_kdesc& kd, uint32_t* mask) {
  int left[GPK_MAX_NODES], right[GPK_MAX_NODES], stk[GPK_MAX_NODES];
  int sp = 0;
  for (int q = 0; q < kd.n_nodes; ++q) {
    left[q] = right[q] = -1;
    mask[q] = 0u;
    if (kd.nodes[q].op == GPK_OP_ADD || kd.nodes[q].op == GPK_OP_MUL) {
      right[q] = stk[--sp];
      left[q] = stk[--sp];
    }
    stk[sp++] = q;
  }
  for (int q = kd.n_nodes; q < GPK_MAX_NODES; ++q) mask[q] = 0u;
  // top-down: the root is the last node; children inherit the parent's mask (+ sibling at MUL)
  for (int q = kd.n_nodes - 1; q >= 0; --q) {
    if (left[q] < 0) continue;
    const bool mul = kd.nodes[q].op == GPK_OP_MUL;
    mask[left[q]] = mask[q] | (mul ? (1u << right[q]) : 0u);
    mask[right[q]] = mask[q] | (mul ? (1u << left[q]) : 0u);
  }
}

// Per host thread and device: the high-priority panel stream, the bulk-update stream (created
// with a CU mask that leaves tune().reserve_cus CUs to the panel chain, so that the
// diagonal-block kernel -- one workgroup of 150 KB LDS per batch member -- never waits for a CU
// to drain) and the fork / join events of gpk_potrf_aug; created on first use.
struct SideStream {
  hipStream_t panel_s = nullptr, bulk_s = nullptr, panel_np = nullptr;
  hipEvent_t fork = nullptr, panel = nullptr, bulk = nullptr, join_p = nullptr, join_b = nullptr;
};

// Every side stream ever created, destroyed by an atexit handler: registered after the HIP
// runtime's own start-up, it runs before the runtime tears down, and a CU-masked queue still
// alive at that point crashes rocprofv3's finalisation.
std::mutex g_side_mu;
std::vector<SideStream*> g_side_all;

void release_side_streams() {
  std::lock_guard<std::mutex> lk(g_side_mu);
  for (SideStream* ss : g_side_all) {
    if (ss->panel_s) hipStreamSynchronize(ss->panel_s);
    if (ss->bulk_s) hipStreamSynchronize(ss->bulk_s);
    if (ss->panel_np) hipStreamSynchronize(ss->panel_np);
    for (hipEvent_t e : {ss->fork, ss->panel, ss->bulk, ss->join_p, ss->join_b})
      if (e) hipEventDestroy(e);
    if (ss->panel_s) hipStreamDestroy(ss->panel_s);
    if (ss->bulk_s) hipStreamDestroy(ss->bulk_s);
    if (ss->panel_np) hipStreamDestroy(ss->panel_np);
    *ss = SideStream();
  }
  g_side_all.clear();
}

SideStream* side_stream() {
  thread_local std::vector<SideStream*> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
  if ((int)cache.size() <= dev) cache.resize(dev + 1, nullptr);
  if (!cache[dev]) {
    std::lock_guard<std::mutex> lk(g_side_mu);
    static bool registered = false;
    if (!registered) {
      std::atexit(release_side_streams);
      registered = true;
    }
    cache[dev] = new SideStream();  // owned by g_side_all (released at exit)
    g_side_all.push_back(cache[dev]);
  }
  SideStream& ss = *cache[dev];
  if (!ss.panel_s) {
    int least = 0, greatest = 0, ncu = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return nullptr;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return nullptr;
    if (hipStreamCreateWithPriority(&ss.panel_s, hipStreamNonBlocking, greatest) != hipSuccess) return nullptr;
    if (hipStreamCreateWithFlags(&ss.panel_np, hipStreamNonBlocking) != hipSuccess) return nullptr;
    const int64_t r = std::max<int64_t>(0, std::min<int64_t>(tune().reserve_cus, ncu / 2));
    if (r > 0) {
      std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
      for (int c = (int)r; c < ncu; ++c) mask[c / 32] |= 1u << (c % 32);
      if (hipExtStreamCreateWithCUMask(&ss.bulk_s, (uint32_t)mask.size(), mask.data()) != hipSuccess)
        return nullptr;
    } else if (hipStreamCreateWithFlags(&ss.bulk_s, hipStreamNonBlocking) != hipSuccess) {
      return nullptr;
    }
    for (hipEvent_t* e : {&ss.fork, &ss.panel, &ss.bulk, &ss.join_p, &ss.join_b})
      if (hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) return nullptr;
  }
  return &ss;
}

// Ticket counters of the fused panel solve (DiagArgs::ctr), one block of kFuseCtr (gpk_launch_plan.h) per (device,
// stream): launches on one stream never overlap.  Tickets are drawn with atomicInc(ctr, grid - 1), so
// the grid's last draw wraps the counter back to 0 by itself (no reset store).  A handle that stands
// for one stream per host thread (hipStreamPerThread) or a stream being captured does not get
// counters: its panel solve stays a separate launch (fuse_counters returns nullptr).  The null stream
// is one queue per device whatever thread launches on it (torch's default stream), so it keeps them.
std::mutex g_ctr_mu;
std::map<std::pair<int, hipStream_t>, int32_t*> g_ctr;

int32_t* fuse_counters(hipStream_t s) {
  if (s == hipStreamPerThread) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_ctr_mu);
  auto it = g_ctr.find({dev, s});
  if (it != g_ctr.end()) return it->second;
  int32_t* p = nullptr;
  if (hipMalloc(&p, kFuseCtr * sizeof(int32_t)) != hipSuccess) return nullptr;
  if (hipMemsetAsync(p, 0, kFuseCtr * sizeof(int32_t), s) != hipSuccess) {
    hipFree(p);
    return nullptr;
  }
  g_ctr[{dev, s}] = p;  // owned for the life of the process
  return p;
}

// Operand scratch of the folded panel solves (the planner's in-group mode 4: prep_kernel writes it, the solve that
// follows on the same stream reads it), one block per (device, stream) like the counters above and under the same
// rule: no block for hipStreamPerThread or a stream being captured (the factorisation then keeps mode 3's steps).
// Allocated at the stream's first folded factorisation, for the deepest operand of the batch and group size
// (launch_fold_bytes), so one block serves every shape of that batch.  A larger batch or group later gets a new block
// of at least twice the size; the old one is NOT freed: a thread that shares the stream may have fetched it and not
// launched yet (the counters above never move either).  Owned for the life of the process.
std::map<std::pair<int, hipStream_t>, std::pair<void*, size_t>> g_fold;

void* fold_scratch(hipStream_t s, size_t bytes) {
  if (s == hipStreamPerThread) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_ctr_mu);
  std::pair<void*, size_t>& blk = g_fold[{dev, s}];
  if (blk.second >= bytes) return blk.first;
  const size_t want = std::max(bytes, 2 * blk.second);
  void* p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) return nullptr;
  blk = {p, want};  // (a previous, smaller block stays allocated, see above)
  return p;
}

// ------------------------------------------------------------------------ persistent factorisation
// The task list of one shape on the device (its order: chain_order, gpk_chain_plan.h), uploaded at the shape's
// first call.
struct ChainPlan {
  int32_t* tasks = nullptr;  // device [ntasks + ntasks_b][4]: list A, then list B (chain_xcd)
  int32_t ntasks = 0, ntasks_b = 0;
  int32_t nblk = 0, nsl = 0, nbc = 0;
};
std::mutex g_chain_mu;
std::map<ChainPlanKey, ChainPlan> g_chain_plans;

// Counter scratch of the persistent launch, per (host thread, device, stream): the counters are zeroed
// by a memset enqueued before each launch, so two threads enqueueing on one stream (torch's null stream
// is shared by every thread) must never share them -- memset A, memset B, launch A, launch B would hand
// launch B counters already past its task count.  A thread's own calls on one stream are stream-ordered.
// The blocks are freed when their thread exits (hipFree waits for the device, so no launch still reads them).
struct ChainCtl {
  std::map<std::pair<int, hipStream_t>, std::pair<int32_t*, size_t>> blocks;
  ~ChainCtl() {
    for (auto& kv : blocks)
      if (kv.second.first) {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess && hipSetDevice(kv.first.first) == hipSuccess) {
          (void)hipFree(kv.second.first);
          (void)hipSetDevice(cur);
        }
      }
  }
};
thread_local ChainCtl t_chain_ctl;
std::atomic<int64_t> g_chain_launches{0};      // persistent launches enqueued
std::atomic<int64_t> g_chain_declined{0};      // auto mode: launch path taken, another stream busy
std::atomic<int64_t> g_chain_force_timeout{0};  // testing: the next N persistent launches time out
// gpk_tune "upd_tri" (GPK_UPD_TRI): uniform f64 128-tile group / half updates run their diagonal tiles (and the y
// row's live block) as lower-triangle work in update_tri_kernel -- 1: after the strictly lower tiles, 2: before them,
// 0: one gemm_kernel launch over all tiles.  The entry point's own knob, not a row of the knob table.
std::atomic<int64_t>& upd_tri_knob() {
  static std::atomic<int64_t> v{env_i64("GPK_UPD_TRI", 1)};
  return v;
}
thread_local bool t_chain_last = false;         // this thread's last factorisation was the persistent one

// Factorisations in flight per (device, stream): an event recorded on the caller's stream after every
// factorisation this library enqueues.  chain = 1 (auto) takes the launch path while a factorisation on
// another stream of the device has not finished: the persistent launch claims every CU and would
// serialise overlapped factorisations (C2 at 4 in flight: 1315 evals/s on the launch path, 779 with
// persistent launches).
std::mutex g_busy_mu;
std::map<std::pair<int, hipStream_t>, hipEvent_t> g_busy;

bool plain_stream(hipStream_t s) {
  if (s == hipStreamPerThread) return false;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
}

void note_factorisation(hipStream_t s) {
  int dev = 0;
  if (!plain_stream(s) || hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lk(g_busy_mu);
  hipEvent_t& e = g_busy[{dev, s}];
  if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
    e = nullptr;
    return;
  }
  hipEventRecord(e, s);
}

// (entries of other streams whose last factorisation has completed are dropped -- streams come and go, e.g. a
// pipelined sweep's -- once the map holds more than a few; the caller's own entry is kept for its next record)
bool other_stream_busy(hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return true;
  std::lock_guard<std::mutex> lk(g_busy_mu);
  const bool prune = g_busy.size() > 16;
  bool busy = false;
  for (auto it = g_busy.begin(); it != g_busy.end();) {
    const bool other = !(it->first.first == dev && it->first.second == s);
    const hipError_t q = it->second ? hipEventQuery(it->second) : hipSuccess;
    if (other && it->first.first == dev && q == hipErrorNotReady) busy = true;
    if (prune && other && q != hipErrorNotReady) {
      if (it->second) hipEventDestroy(it->second);
      it = g_busy.erase(it);
    } else {
      ++it;
    }
  }
  return busy;
}
int32_t* g_chain_trace = nullptr;  // GPK_CHAIN_TRACE=1: pinned host words the kernel writes its progress to
uint64_t* g_chain_times = nullptr;  // GPK_CHAIN_TIMES=1: device stamps per task of the last profiled launch
int64_t g_chain_times_n = 0;

// chain_kernel applies to one f64 member (or a small batch) without ragged rows -- identity extra rows
// included (chain_eye) --, on a stream that is not being captured (the first call of a shape uploads its task
// list), up to chain_max_p (identity rows: chain_max_p_eye) rows; f32 (chain_f32) without identity rows
bool chain_applies(const gpk_layout* lay, bool eye, const int64_t* n_dev, const int64_t* m_dev, const Tune& tn,
                   hipStream_t s) {
  const bool dt_ok = lay->dtype == GPK_F64 || (lay->dtype == GPK_F32 && tn.chain_f32 != 0 && !eye);
  if (!tn.chain || !dt_ok || (eye && !tn.chain_eye) || n_dev || m_dev) return false;
  if (lay->batch == 1 ? lay->p > (eye ? tn.chain_max_p_eye : tn.chain_max_p)
                      : (lay->batch > tn.chain_max_batch || lay->batch * lay->p > tn.chain_batch_max_rows))
    return false;
  if (tn.diag_dbg != 0 || tn.diag_version == 1) return false;
  if (!plain_stream(s)) return false;
  if (tn.chain == 1 && lay->p < (eye ? tn.chain_min_p_eye : tn.chain_min_p)) return false;
  if (tn.chain == 1 && other_stream_busy(s)) {
    ++g_chain_declined;
    return false;
  }
  return true;
}

int chain_potrf(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, const Tune& tn, hipStream_t s,
                bool eye) {
  int dev = 0, ncu = 0;
  GPK_HIP(hipGetDevice(&dev), "device");
  GPK_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev), "device");
  const int grid = tn.chain_grid > 0 ? (int)tn.chain_grid : ncu;
  ChainPlan plan;
  int32_t* ctl = nullptr;
  const ChainKnobs kn = chain_knobs(tn, lay->n_pad, eye, lay->dtype == GPK_F32, grid);
  {
    std::lock_guard<std::mutex> lk(g_chain_mu);
    const int nmem = lay->batch;
    // (two lists need workgroups of both roles: at least 8 per XCD)
    const int xcd = tn.chain_xcd != 0 && grid >= 64 ? 1 : 0;
    const ChainPlanKey key{dev, lay->n_pad, lay->y_row, grid, nmem, eye ? 1 : 0, xcd, kn};
    auto it = g_chain_plans.find(key);
    if (it == g_chain_plans.end()) {
      std::vector<int32_t> ord = chain_order(lay->n_pad, lay->y_row, grid, nmem, kn, eye);
      if (ord.empty()) {
        // (an internal failure, not a bad argument: reported like a HIP error, > 0)
        return fail_hip(hipErrorUnknown, "chain_order: a task exceeds the device's dependency bound");
      }
      ChainPlan p;
      p.ntasks_b = xcd ? chain_split_lists(ord) : 0;
      p.ntasks = (int32_t)(ord.size() / 4) - p.ntasks_b;
      p.nblk = (int32_t)(lay->n_pad / NB);
      p.nsl = (int32_t)(lay->y_row / 32 + 1);
      p.nbc = (int32_t)(lay->y_row / NB + 1);
      GPK_HIP(hipMalloc(&p.tasks, ord.size() * sizeof(int32_t)), "chain tasks");
      GPK_HIP(hipMemcpy(p.tasks, ord.data(), ord.size() * sizeof(int32_t), hipMemcpyHostToDevice), "chain tasks");
      it = g_chain_plans.emplace(key, p).first;  // owned for the life of the process
    }
    plan = it->second;
  }
  // counters of one member: dflag + hflag per block, sdone + qdone per (block, slice), ucnt per (slice, block column)
  const size_t ctl_stride = 2 * (size_t)plan.nblk + 2 * (size_t)plan.nblk * plan.nsl + (size_t)plan.nsl * plan.nbc;
  const size_t ctl_ints = (4 + (size_t)lay->batch * ctl_stride + 3) / 4 * 4;
  {
    auto& c = t_chain_ctl.blocks[{dev, s}];  // this thread's own (see t_chain_ctl)
    if (c.second < ctl_ints) {
      // (hipFree synchronises the device: no launch of this thread still uses the old block)
      if (c.first) GPK_HIP(hipFree(c.first), "chain scratch");
      c = {nullptr, 0};
      GPK_HIP(hipMalloc(&c.first, ctl_ints * sizeof(int32_t)), "chain scratch");
      c.second = ctl_ints;
    }
    ctl = c.first;
  }
  // every counter starts at zero in every call
  GPK_HIP(hipMemsetAsync(ctl, 0, ctl_ints * sizeof(int32_t), s), "chain memset");
  ChainArgs a;
  memset(&a, 0, sizeof(a));
  a.W = W;
  a.ld = lay->ld;
  a.Winv = Winv;
  a.info = info_dev;
  a.tasks = plan.tasks;
  a.ntasks = env_i64("GPK_CHAIN_MAX_TASKS", 0) > 0 ? (int32_t)std::min<int64_t>(plan.ntasks, env_i64("GPK_CHAIN_MAX_TASKS", 0)) : plan.ntasks;  // (debugging)
  a.ntasks_b = plan.ntasks_b;
  if (a.ntasks_b > 0) a.ntasks = plan.ntasks;  // (GPK_CHAIN_MAX_TASKS: one list only)
  a.xcd_b = plan.ntasks_b > 0 ? 0 : -1;
  a.b_seats = (int32_t)std::max<int64_t>(1, std::min<int64_t>(tn.chain_xcd_seats, grid / 16));
  a.dbg = (int32_t)env_i64("GPK_CHAIN_DBG", 0);
  a.ctl = ctl;
  a.dflag = ctl + 4;
  a.sdone = a.dflag + plan.nblk;
  a.ucnt = a.sdone + (size_t)plan.nblk * plan.nsl;
  a.qdone = a.ucnt + (size_t)plan.nsl * plan.nbc;
  a.hflag = a.qdone + (size_t)plan.nblk * plan.nsl;
  a.nsl = plan.nsl;
  a.nbc = plan.nbc;
  a.nmem = lay->batch;
  a.w_bs = lay->w_batch_stride;
  a.inv_bs = lay->inv_batch_stride;
  a.ctl_stride = (int64_t)ctl_stride;
  a.uq = (int32_t)kn.uq;
  // rows of L_kk^-1 behind D's early flag: later (more of the panel solve early) for short chains, where the
  // diagonal chain is all there is; earlier for long ones, where the S tasks' waiting CUs cost tile-update time
  // (N = 4096: 112 rows 1.501 vs 96 rows 1.515 ms; 6144 / 8192 2.42 / 4.44 vs 2.37 / 4.39, profiles/r04ab_*)
  a.half_step = (plan.nblk <= 32 ? GPK_CHAIN_SHALF_ROWS_SMALL : GPK_CHAIN_SHALF_ROWS) / 16;
  a.row_end = lay->y_row + 1;
  a.timeout = std::max<int64_t>(1, tn.chain_timeout_ms) * 100000;  // 100 MHz ticks
  for (int64_t f = g_chain_force_timeout.load(); f > 0;)
    if (g_chain_force_timeout.compare_exchange_weak(f, f - 1)) {
      a.force_abort = 1;
      break;
    }
  if (env_i64("GPK_CHAIN_TIMES", 0)) {
    std::lock_guard<std::mutex> lk(g_chain_mu);
    // (GPK_DIAG_PROF builds: the D tasks' phase stamps follow the task stamps, 8 steps x 8 waves x 6 per block,
    // read back as extra "tasks" of gpk_chain_times)
    const int64_t extra = GPK_DIAG_PROF ? (int64_t)plan.nblk * 8 * 8 : 0;
    const int64_t nt = (int64_t)a.ntasks + a.ntasks_b;
    if (g_chain_times_n < nt + extra) {
      if (g_chain_times) hipFree(g_chain_times);
      GPK_HIP(hipMalloc(&g_chain_times, (size_t)(nt + extra) * 6 * sizeof(uint64_t)), "chain times");
      g_chain_times_n = nt + extra;
    }
    a.times = g_chain_times;
    if (extra) a.dprof = g_chain_times + (size_t)nt * 6;
  }
  if (env_i64("GPK_CHAIN_TRACE", 0)) {
    std::lock_guard<std::mutex> lk(g_chain_mu);
    if (!g_chain_trace) GPK_HIP(hipHostMalloc(&g_chain_trace, 4096 * 32 * sizeof(int32_t), hipHostMallocCoherent), "trace");
    memset(g_chain_trace, 0xff, 4096 * 32 * sizeof(int32_t));
    a.trace = grid <= 4096 ? g_chain_trace : nullptr;
  }
  const double n3 = (double)lay->n_pad;
  GPK_HIP(timed(3, lay->batch * n3 * n3 * n3 / (eye ? 1.0 : 3.0), 0.0, s, [&] { return launch_chain(a, lay->dtype, grid, s); }),
          "chain");
  ++g_chain_launches;
  t_chain_last = true;
  return 0;
}

}  // namespace

extern "C" {

int gpk_abi_version(void) { return GPK_ABI_VERSION; }

int gpk_op_supported(int32_t op) {
  switch (op) {
    case GPK_OP_LIN: case GPK_OP_RQ: case GPK_OP_PER: case GPK_OP_SE: case GPK_OP_MAT32: case GPK_OP_MAT52:
    case GPK_OP_ADD: case GPK_OP_MUL: case GPK_OP_CPW:
      return 1;
    default:
      return 0;
  }
}

const char* gpk_last_error(void) { return g_err.c_str(); }

int gpk_plan(int dtype, int32_t batch, int64_t n, int64_t m, int64_t d, gpk_layout* out) {
  if (dtype != GPK_F64 && dtype != GPK_F32) return fail_arg(1, "dtype");
  if (batch <= 0) return fail_arg(2, "batch must be > 0");
  if (n <= 0) return fail_arg(3, "n must be > 0");
  if (m < 0) return fail_arg(4, "m must be >= 0");
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(5, "d must be in [1, 16]");
  if (!out) return fail_arg(6, "out");
  gpk_layout L;
  memset(&L, 0, sizeof(L));
  L.dtype = dtype;
  L.batch = batch;
  L.n = n;
  L.m = m;
  L.d = d;
  L.nb = NB;
  L.n_pad = (n + NB - 1) / NB * NB;
  L.y_row = L.n_pad + m;
  L.p = (L.y_row + 1 + NB - 1) / NB * NB;
  L.ld = L.p;
  L.w_batch_stride = L.p * L.ld;
  L.inv_batch_stride = (L.n_pad / NB) * NB * NB;
  L.w_bytes = (size_t)batch * (size_t)L.w_batch_stride * elem_size(dtype);
  L.inv_bytes = (size_t)batch * (size_t)L.inv_batch_stride * elem_size(dtype);
  *out = L;
  return 0;
}

static int check_layout(const gpk_layout* lay) {
  if (!lay) return fail_arg(1, "layout");
  if ((lay->dtype != GPK_F64 && lay->dtype != GPK_F32) || lay->batch <= 0 || lay->nb != NB ||
      lay->n_pad % NB != 0 || lay->p % NB != 0 || lay->ld < lay->p || lay->y_row >= lay->p ||
      lay->n <= 0 || lay->n > lay->n_pad)
    return fail_arg(1, "layout (use gpk_plan)");
  return 0;
}

static int assemble_impl(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                         int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                         const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride,
                         const double* E, int64_t e_bstride, const double* y, int64_t y_bstride,
                         void* W, bool eye, const int64_t* n_dev, const int64_t* m_dev, void* stream,
                         int64_t tcol_hi = 0) {
  if (int e = check_layout(lay)) return e;
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!noise_dev) return fail_arg(5, "noise_dev");
  if (!X) return fail_arg(7, "X");
  if (eye && lay->m != lay->n) return fail_arg(2, "identity extra rows need a layout planned with m = n");
  if (lay->m > 0 && !Xs && !E && !eye) return fail_arg(9, "Xs or E");
  if (!y) return fail_arg(13, "y");
  if (!W) return fail_arg(15, "W");
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.generic = tune_now().asm_generic != 0 ? 1 : 0;
  a.hyp = hyp_dev;
  a.hyp_stride = hyp_stride;
  a.noise = noise_dev;
  a.noise_stride = noise_stride;
  a.X = X;
  a.x_bs = x_bstride;
  a.Xs = Xs ? Xs : X;
  a.xs_bs = xs_bstride;
  a.E = (lay->m > 0) ? E : nullptr;
  a.e_bs = e_bstride;
  a.y = y;
  a.y_bs = y_bstride;
  a.W = W;
  a.ld = lay->ld;
  a.w_bs = lay->w_batch_stride;
  a.n = lay->n;
  a.m = lay->m;
  a.n_pad = lay->n_pad;
  a.y_row = lay->y_row;
  a.p = lay->p;
  a.d = (int32_t)lay->d;
  a.dp = padded_dim(lay->d);
  a.plain = 0;
  a.eye = eye ? 1 : 0;
  a.ntile = lay->p / ATILE;
  a.nb = n_dev;
  a.mb = m_dev;
  a.tcol_hi = tcol_hi;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double es = (double)elem_size(lay->dtype);
  const double cols = (tcol_hi > 0 && tcol_hi < a.ntile) ? (double)(tcol_hi * ATILE) : (double)lay->p;
  const double bytes = (double)lay->batch *
                       (es * (cols * (double)lay->p - cols * (cols - (double)ATILE) / 2.0) +
                        8.0 * (double)(lay->n + lay->m) * (double)lay->d + 8.0 * (double)lay->n);
  GPK_HIP(timed(0, 0.0, bytes, s, [&] { return launch_assemble(*kd, a, lay->dtype, lay->batch, s); }),
          "assemble");
  return 0;
}

int gpk_assemble(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                 int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                 const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride,
                 const double* E, int64_t e_bstride, const double* y, int64_t y_bstride,
                 void* W, void* stream) {
  return assemble_impl(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, Xs,
                       xs_bstride, E, e_bstride, y, y_bstride, W, false, nullptr, nullptr, stream);
}

int gpk_assemble_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                        int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                        const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride,
                        const double* y, int64_t y_bstride, const int64_t* n_dev, const int64_t* m_dev,
                        void* W, void* stream) {
  if (!n_dev) return fail_arg(13, "n_dev");
  if (lay && lay->m > 0 && !m_dev) return fail_arg(14, "m_dev (layout planned with m > 0)");
  return assemble_impl(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, Xs,
                       xs_bstride, nullptr, 0, y, y_bstride, W, false, n_dev, lay && lay->m > 0 ? m_dev : nullptr,
                       stream);
}

int gpk_assemble_inverse(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                         int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                         const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                         void* W, void* stream) {
  return assemble_impl(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, nullptr,
                       0, nullptr, 0, y, y_bstride, W, true, nullptr, nullptr, stream);
}

static int potrf_impl(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, int32_t flags,
                      const int64_t* n_dev, const int64_t* m_dev, void* stream, const GemmArgs* kb = nullptr) {
  if (int e = check_layout(lay)) return e;
  if (!W) return fail_arg(2, "W");
  if (!Winv) return fail_arg(3, "Winv");
  if (!info_dev) return fail_arg(4, "info_dev");
  if (flags & ~GPK_AUG_EXTRA_IDENTITY) return fail_arg(5, "flags");
  const bool eye = (flags & GPK_AUG_EXTRA_IDENTITY) != 0;
  if (eye && lay->m != lay->n) return fail_arg(1, "identity extra rows need a layout planned with m = n");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int dt = lay->dtype;
  const size_t es = elem_size(dt);

  // one snapshot of the knobs per call: a gpk_tune from another thread (ctypes releases the GIL during
  // the enqueue) must not change the fuse decision between a panel's diag(k) and trsm(k)
  const Tune tn = tune_now();
  const int64_t upd_tri = upd_tri_knob().load();
  t_chain_last = false;
  // a single evaluation: the whole factorisation as one persistent launch (no K build fused into it)
  if (!kb && chain_applies(lay, eye, n_dev, m_dev, tn, s)) {
    const int e = chain_potrf(lay, W, Winv, info_dev, tn, s, eye);
    if (!e) note_factorisation(s);
    return e;
  }
  // Checks, plan, issue: the schedule -- which launches, on which logical stream, between which event edges, with
  // what geometry and accounting -- is launch_plan's (gpk_launch_plan.cpp); here it meets the call's pointers,
  // strides and queues.
  const bool la = launch_lookahead(tn, lay->p);
  static const SideStream no_side;  // look-ahead off: no event step, every step on the caller's stream
  const SideStream* ss = &no_side;
  if (la) {
    ss = side_stream();
    if (!ss) return fail_hip(hipErrorInvalidValue, "side stream");
  }
  hipStream_t sp = !la ? s : tn.panel_stream == 1 ? s : tn.panel_stream == 2 ? ss->panel_np : ss->panel_s;
  const hipStream_t queue[3] = {s, sp, la ? ss->bulk_s : s};                                     // by LP_CALLER ..
  const hipEvent_t event[LP_NUM_EVENTS] = {ss->fork, ss->panel, ss->bulk, ss->join_p, ss->join_b};  // by LP_EV_*
  int32_t* const ctr = (dt == GPK_F64 && tn.fuse_trsm) ? fuse_counters(sp) : nullptr;

  thread_local std::vector<LaunchStep> steps;  // (reused: no allocation per call once it has grown)
  LaunchShape shape{dt == GPK_F32, lay->batch, lay->m, lay->n_pad, lay->y_row, lay->p, n_dev != nullptr, false};
  launch_plan(shape, eye, ctr != nullptr, kb != nullptr, tn, steps);
  // folded panel solves: their operand scratch on the panel stream, or the plan without them
  void* wop = nullptr;
  if (const int64_t fold_bytes = launch_fold_bytes(shape, eye, tn, steps)) {
    wop = fold_scratch(sp, (size_t)fold_bytes);
    if (!wop) {
      shape.no_fold = true;
      launch_plan(shape, eye, ctr != nullptr, kb != nullptr, tn, steps);
    }
  }

  DiagArgs dbase;
  memset(&dbase, 0, sizeof(dbase));
  dbase.W = W;
  dbase.ld = lay->ld;
  dbase.w_bs = lay->w_batch_stride;
  dbase.Winv = Winv;
  dbase.inv_bs = lay->inv_batch_stride;
  dbase.info = info_dev;
  dbase.dbg = (int32_t)tn.diag_dbg;
  dbase.version = (int32_t)tn.diag_version;
  GemmArgs base;
  memset(&base, 0, sizeof(base));
  base.W = W;
  base.ld = lay->ld;
  base.w_bs = lay->w_batch_stride;
  base.inv_bs = lay->inv_batch_stride;
  base.nb = n_dev;
  base.mb = m_dev;
  base.n_pad = lay->n_pad;
  base.y_row = lay->y_row;
  base.p = lay->p;
  static const char* const update_label[] = {"update", "update thin", "update half", "update look-ahead",
                                             "update bulk", "update"};  // by LP_ROLE_*
  for (const LaunchStep& st : steps) {
    const hipStream_t q = queue[st.stream];
    if (st.kind == LP_RECORD) {
      GPK_HIP(hipEventRecord(event[st.event], q), "event");
    } else if (st.kind == LP_WAIT) {
      GPK_HIP(hipStreamWaitEvent(q, event[st.event], 0), "event");
    } else if (st.kind == LP_DIAG) {
      DiagArgs da = dbase;
      da.j0 = st.j0;
      da.kblk = st.kblk;
      da.trsm_tiles = (int32_t)st.trsm_tiles;
      if (da.trsm_tiles > 0) {  // the panel solve inside the launch
        da.row0 = st.row0;
        da.p = lay->p;
        da.n_pad = lay->n_pad;
        da.y_row = lay->y_row;
        da.zlo = st.zlo;
        da.zhi = st.zhi;
        da.nb = n_dev;
        da.mb = m_dev;
        da.ctr = ctr;
      }
      GPK_HIP(timed((int)st.cls, st.flops, st.bytes, q, [&] { return launch_diag(da, dt, lay->batch, q); }), "diag");
    } else if (st.kind == LP_PREP) {  // the operand of the folded panel solve that follows on this stream
      PrepArgs pa;
      memset(&pa, 0, sizeof(pa));
      pa.W = W;
      pa.ld = lay->ld;
      pa.w_bs = lay->w_batch_stride;
      pa.Winv = Winv;
      pa.inv_bs = lay->inv_batch_stride;
      pa.kblk = st.kblk;
      pa.j0 = st.j0;
      pa.kdepth = (int32_t)st.kdepth;
      pa.Wop = wop;
      pa.ld_op = st.kdepth + NB;
      pa.op_bs = NB * pa.ld_op;
      GPK_HIP(timed((int)st.cls, st.flops, st.bytes, q, [&] { return launch_prep(pa, lay->batch, q); }), "prep");
    } else {
      GemmArgs ga = base;
      ga.j0 = st.j0;
      ga.row0 = st.row0;
      ga.kdepth = (int32_t)st.kdepth;
      ga.nt = (int32_t)st.nt;
      ga.c_lo = (int32_t)st.c_lo;
      ga.c_hi = (int32_t)st.c_hi;
      ga.zlo = st.zlo;
      ga.zhi = st.zhi;
      ga.bz0 = (int32_t)st.bz0;
      ga.bzn = (int32_t)st.bzn;
      ga.band = (int32_t)st.band;
      ga.row_end = st.row_end;
      const bool solve = st.kind == LP_TRSM;
      if (solve) ga.Binv = static_cast<const char*>(Winv) + (size_t)(st.j0 / NB) * NB * NB * es;
      if (solve && st.kdepth > NB) {  // folded: against the PREP step's operand, K = kdepth contiguous per row
        ga.Binv = wop;
        ga.inv_bs = NB * st.kdepth;
      }
      if (st.kbuild) {  // C is evaluated, not loaded (gpk_nlml's fused K build)
        ga.kbuild = 1;
        ga.d = kb->d;
        ga.n = kb->n;
        ga.node = kb->node;
        ga.hyp = kb->hyp;
        ga.hyp_stride = kb->hyp_stride;
        ga.noise = kb->noise;
        ga.noise_stride = kb->noise_stride;
        ga.X = kb->X;
        ga.x_bs = kb->x_bs;
        ga.y = kb->y;
        ga.y_bs = kb->y_bs;
      }
      // upd_tri: a uniform f64 128-tile update of a group's trailing matrix goes out as two kernels inside the one
      // counted launch -- gemm_kernel on the strictly lower tiles and update_tri_kernel on the lower 16 x 16 blocks of
      // the diagonal tiles.  When the last tile row (the y row's) has a single live 16-row block, that row leaves
      // gemm_kernel's grid too and each diagonal tile's workgroup takes its 8 blocks along (its B rows are staged
      // there anyway).  Thin in-group updates (a 64-workgroup launch of its own would only serialise the stream),
      // ragged and identity-augmented batches and the fused K build keep the single kernel.
      const bool split = !solve && upd_tri != 0 && dt == GPK_F64 && st.tile == 128 && !eye && !n_dev &&
                         st.row_end > 0 && !st.kbuild && st.bzn == 0 &&
                         (st.role == LP_ROLE_GROUP || st.role == LP_ROLE_LOOKAHEAD || st.role == LP_ROLE_BULK ||
                          st.role == LP_ROLE_HALF);
      GemmArgs gt = ga;
      if (split) {
        const bool fold = st.row_end - (st.row0 + (st.nt - 1) * NB) <= 16;
        gt.tri = fold ? 2 : 0;
        ga.tri = 1;
        if (fold) {
          ga.nt = gt.nt - 1;
          ga.c_hi = std::min(ga.c_hi, ga.nt);
        }
      }
      GPK_HIP(timed((int)st.cls, st.flops, st.bytes, q,
                    [&] {
                      if (split && upd_tri == 2)  // (A/B: the diagonal tiles first)
                        if (hipError_t e = launch_update_tri(gt, lay->batch, q)) return e;
                      if (hipError_t e = launch_gemm(ga, dt, solve ? GEMM_TRSM : GEMM_UPDATE, (int)st.tile, lay->batch, q))
                        return e;
                      return split && upd_tri != 2 ? launch_update_tri(gt, lay->batch, q) : hipSuccess;
                    }),
              solve ? "trsm" : update_label[st.role]);
    }
  }
  note_factorisation(s);
  return 0;
}

int gpk_potrf_aug_ex(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, int32_t flags,
                     void* stream) {
  return potrf_impl(lay, W, Winv, info_dev, flags, nullptr, nullptr, stream);
}

int gpk_potrf_aug(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, void* stream) {
  return potrf_impl(lay, W, Winv, info_dev, 0, nullptr, nullptr, stream);
}

int gpk_potrf_aug_ragged(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev,
                         const int64_t* n_dev, const int64_t* m_dev, void* stream) {
  if (!n_dev) return fail_arg(5, "n_dev");
  if (lay && lay->m > 0 && !m_dev) return fail_arg(6, "m_dev (layout planned with m > 0)");
  return potrf_impl(lay, W, Winv, info_dev, 0, n_dev, lay && lay->m > 0 ? m_dev : nullptr, stream);
}

static int finalize_impl(const gpk_layout* lay, const void* W, const int32_t* info_dev, const int64_t* n_dev,
                         double* out_dev, double* mu_dev, double* var_dev, void* stream) {
  if (int e = check_layout(lay)) return e;
  if (!W) return fail_arg(2, "W");
  if (!info_dev) return fail_arg(3, "info_dev");
  if (!out_dev) return fail_arg(4, "out_dev");
  FinArgs f;
  f.W = W;
  f.ld = lay->ld;
  f.w_bs = lay->w_batch_stride;
  f.n = lay->n;
  f.m = lay->m;
  f.n_pad = lay->n_pad;
  f.y_row = lay->y_row;
  f.info = info_dev;
  f.out = out_dev;
  f.mu = mu_dev;
  f.var = var_dev;
  f.nb = n_dev;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(timed(4, 0.0, 0.0, s, [&] { return launch_finalize(f, lay->dtype, lay->batch, s); }),
          "finalize");
  return 0;
}

int gpk_finalize(const gpk_layout* lay, const void* W, const int32_t* info_dev, double* out_dev,
                 double* mu_dev, double* var_dev, void* stream) {
  return finalize_impl(lay, W, info_dev, nullptr, out_dev, mu_dev, var_dev, stream);
}

int gpk_finalize_ragged(const gpk_layout* lay, const void* W, const int32_t* info_dev, const int64_t* n_dev,
                        double* out_dev, double* mu_dev, double* var_dev, void* stream) {
  if (!n_dev) return fail_arg(4, "n_dev");
  return finalize_impl(lay, W, info_dev, n_dev, out_dev, mu_dev, var_dev, stream);
}

int gpk_nlml_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                    const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                    const double* y, int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv,
                    int32_t* info_dev, double* out_dev, void* stream) {
  if (int e = check_layout(lay)) return e;
  if (lay->m != 0) return fail_arg(2, "gpk_nlml_ragged needs a layout planned with m = 0");
  if (!n_dev) return fail_arg(11, "n_dev");
  if (!info_dev) return fail_arg(14, "info_dev");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * lay->batch, s), "memset info");
  int e = gpk_assemble_ragged(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, nullptr, 0,
                              y, y_bstride, n_dev, nullptr, W, stream);
  if (e) return e;
  e = gpk_potrf_aug_ragged(lay, W, Winv, info_dev, n_dev, nullptr, stream);
  if (e) return e;
  return gpk_finalize_ragged(lay, W, info_dev, n_dev, out_dev, nullptr, nullptr, stream);
}

int gpk_nlml(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
             const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
             const double* y, int64_t y_bstride, void* W, void* Winv, int32_t* info_dev,
             double* out_dev, void* stream) {
  if (int e = check_layout(lay)) return e;
  if (lay->m != 0) return fail_arg(2, "gpk_nlml needs a layout planned with m = 0");
  if (!info_dev) return fail_arg(13, "info_dev");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * lay->batch, s), "memset info");
  // Fused K build (single SE / MAT32 / MAT52 nodes; any other single node, LIN and RQ included, takes the plain assemble
  // launch and the unfused factorisation below): only the first panel group's block columns are
  // assembled; the first trailing update evaluates its C tiles instead of reading them, so the
  // trailing part of K is never written to HBM and read back.
  const Tune tn = tune_now();
  const int64_t G0 = launch_first_group(tn, false, lay->n_pad);  // (a single group has no trailing matrix to build)
  const int op0 = kd ? kd->nodes[0].op : 0;
  if (tn.fuse_kbuild && lay->dtype == GPK_F64 && valid_kdesc(kd, lay->d) && kd->n_nodes == 1 && G0 < lay->n_pad / NB &&
      !chain_applies(lay, false, nullptr, nullptr, tn, s) &&
      (op0 == GPK_OP_SE || op0 == GPK_OP_MAT32 || op0 == GPK_OP_MAT52)) {
    int e = assemble_impl(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, nullptr, 0,
                          nullptr, 0, y, y_bstride, W, false, nullptr, nullptr, stream, G0 * NB / ATILE);
    if (e) return e;
    GemmArgs kb;
    memset(&kb, 0, sizeof(kb));
    kb.d = (int32_t)lay->d;
    kb.n = lay->n;
    kb.node = kd->nodes[0];
    kb.hyp = hyp_dev;
    kb.hyp_stride = hyp_stride;
    kb.noise = noise_dev;
    kb.noise_stride = noise_stride;
    kb.X = X;
    kb.x_bs = x_bstride;
    kb.y = y;
    kb.y_bs = y_bstride;
    e = potrf_impl(lay, W, Winv, info_dev, 0, nullptr, nullptr, stream, &kb);
    if (e) return e;
    return gpk_finalize(lay, W, info_dev, out_dev, nullptr, nullptr, stream);
  }
  int e = gpk_assemble(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, nullptr,
                       0, nullptr, 0, y, y_bstride, W, stream);
  if (e) return e;
  e = gpk_potrf_aug(lay, W, Winv, info_dev, stream);
  if (e) return e;
  return gpk_finalize(lay, W, info_dev, out_dev, nullptr, nullptr, stream);
}

// ------------------------------------------------------------- workspace-style convenience entries
// The flat signatures of SURVEY §8(b): the caller hands one scratch buffer instead of a layout and
// W / Winv; the calls carve the augmented layout out of it and run the same kernels.
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t gpk_workspace_bytes(int op, int dtype, int64_t n, int64_t m, int32_t batch) {
  (void)m;
  gpk_layout lay;
  if (n <= 0 || batch <= 0) return 0;
  if (op == GPK_WS_NLML) {
    if (gpk_plan(dtype, batch, n, 0, 1, &lay)) return 0;
    return align256(lay.w_bytes) + align256(lay.inv_bytes) + align256((size_t)batch * 4 * sizeof(double));
  }
  if (op == GPK_WS_POTRF) {
    if ((dtype != GPK_F64 && dtype != GPK_F32) || gpk_plan(dtype, 1, n, 0, 1, &lay)) return 0;
    return align256(lay.w_bytes) + align256(lay.inv_bytes) + align256(8 * sizeof(double)) +
           align256((size_t)n * sizeof(double));
  }
  const int64_t n_pad = (n + NB - 1) / NB * NB;
  const size_t winv = align256((size_t)n_pad * NB * sizeof(double));
  if (op == GPK_WS_TRSV) {
    if (dtype != GPK_F64) return 0;
    return winv + align256((size_t)n_pad * sizeof(double));
  }
  if (op == GPK_WS_POSTERIOR) {
    if (dtype != GPK_F64 || m <= 0) return 0;
    return winv + 2 * align256((size_t)n_pad * (size_t)m * sizeof(double)) + align256(8 * sizeof(double));
  }
  return 0;
}

int gpk_nlml_batched(const gpk_kdesc* kd, int32_t batch, const double* hyp_dev, const double* noise_dev, int dtype,
                     const double* X, const double* y, int64_t n, int32_t d, void* work, size_t work_bytes,
                     double* nlml_dev, int32_t* info_dev, void* stream) {
  if (!kd) return fail_arg(1, "kd");
  if (batch <= 0) return fail_arg(2, "batch");
  if (!nlml_dev) return fail_arg(12, "nlml_dev");
  gpk_layout lay;
  if (int e = gpk_plan(dtype, batch, n, 0, d, &lay)) return e;
  if (!work || work_bytes < gpk_workspace_bytes(GPK_WS_NLML, dtype, n, 0, batch)) return fail_arg(11, "work_bytes");
  char* w = reinterpret_cast<char*>(work);
  void* W = w;
  void* Winv = w + align256(lay.w_bytes);
  double* out = reinterpret_cast<double*>(w + align256(lay.w_bytes) + align256(lay.inv_bytes));
  if (int e = gpk_nlml(kd, &lay, hyp_dev, kd->n_hyp, noise_dev, 1, X, 0, y, 0, W, Winv, info_dev, out, stream))
    return e;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(hipMemcpy2DAsync(nlml_dev, sizeof(double), out, 4 * sizeof(double), sizeof(double), (size_t)batch,
                           hipMemcpyDeviceToDevice, s),
          "nlml_batched read-out");
  return 0;
}

static int potrf_lower_f32(float* A, int64_t n, int64_t lda, void* work, size_t work_bytes, int32_t* info_dev,
                           double* logdet_dev, void* stream) {
  gpk_layout lay;
  if (int e = gpk_plan(GPK_F32, 1, n, 0, 1, &lay)) return e;
  if (!work || work_bytes < gpk_workspace_bytes(GPK_WS_POTRF, GPK_F32, n, 0, 1)) return fail_arg(6, "work_bytes");
  char* w = reinterpret_cast<char*>(work);
  void* W = w;
  void* Winv = w + align256(lay.w_bytes);
  double* out = reinterpret_cast<double*>(w + align256(lay.w_bytes) + align256(lay.inv_bytes));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t), s), "memset info");
  GPK_HIP(launch_pack_lower(GPK_F32, A, lda, n, lay.n_pad, lay.p, W, s), "potrf_lower pack");
  if (int e = gpk_potrf_aug(&lay, W, Winv, info_dev, stream)) return e;
  if (int e = gpk_finalize(&lay, W, info_dev, out, nullptr, nullptr, stream)) return e;
  GPK_HIP(launch_unpack_lower(GPK_F32, W, lay.ld, n, A, lda, s), "potrf_lower unpack");
  if (logdet_dev) GPK_HIP(hipMemcpyAsync(logdet_dev, out + 2, sizeof(double), hipMemcpyDeviceToDevice, s), "logdet");
  return 0;
}

int gpk_potrf_lower(int dtype, void* A, int64_t n, int64_t lda, void* work, size_t work_bytes, int32_t* info_dev,
                    double* logdet_dev, void* stream) {
  if (dtype != GPK_F64 && dtype != GPK_F32) return fail_arg(1, "dtype");
  if (!A) return fail_arg(2, "A");
  if (n <= 0) return fail_arg(3, "n");
  if (lda < n) return fail_arg(4, "lda");
  if (!info_dev) return fail_arg(7, "info_dev");
  if (dtype == GPK_F32)
    return potrf_lower_f32(static_cast<float*>(A), n, lda, work, work_bytes, info_dev, logdet_dev, stream);
  gpk_layout lay;
  if (int e = gpk_plan(GPK_F64, 1, n, 0, 1, &lay)) return e;
  if (!work || work_bytes < gpk_workspace_bytes(GPK_WS_POTRF, GPK_F64, n, 0, 1)) return fail_arg(6, "work_bytes");
  char* w = reinterpret_cast<char*>(work);
  double* W = reinterpret_cast<double*>(w);
  void* Winv = w + align256(lay.w_bytes);
  double* out = reinterpret_cast<double*>(w + align256(lay.w_bytes) + align256(lay.inv_bytes));
  double* zeros = reinterpret_cast<double*>(w + align256(lay.w_bytes) + align256(lay.inv_bytes) +
                                            align256(8 * sizeof(double)));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(hipMemsetAsync(out, 0, 8 * sizeof(double), s), "potrf_lower scratch");
  GPK_HIP(hipMemsetAsync(zeros, 0, (size_t)n * sizeof(double), s), "potrf_lower scratch");
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t), s), "memset info");
  // noise 0 (out[4] is zero), y = 0: the augmented factorisation of A alone
  if (int e = gpk_assemble_dense(&lay, reinterpret_cast<const double*>(A), lda, 0, out + 4, 0, nullptr, 0, 0, zeros, 0,
                                 W, stream))
    return e;
  if (int e = gpk_potrf_aug(&lay, W, Winv, info_dev, stream)) return e;
  if (int e = gpk_finalize(&lay, W, info_dev, out, nullptr, nullptr, stream)) return e;
  GPK_HIP(launch_copy_lower(W, lay.ld, reinterpret_cast<double*>(A), lda, n, s), "potrf_lower copy");
  if (logdet_dev) GPK_HIP(hipMemcpyAsync(logdet_dev, out + 2, sizeof(double), hipMemcpyDeviceToDevice, s), "logdet");
  return 0;
}

size_t gpk_grad_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay) {
  if (!kd || !lay || lay->n <= 0 || lay->batch <= 0) return 0;
  if (!valid_kdesc(kd, lay->d)) return 0;  // (gpk_nlml_grad refuses such a program: no workspace to size)
  const int64_t nt = (lay->n + ATILE - 1) / ATILE;
  return (size_t)lay->batch * (size_t)(nt * (nt + 1) / 2) * (size_t)(kd->n_hyp + 1) * sizeof(double);
}

// the tile pass's arguments over the points of a layout planned with m = n (part: [batch][tiles][n_hyp + 1]; n_dev:
// ragged members' sizes or NULL); the caller adds what addresses the weights (W, ld, w_bs)
static GradArgs grad_args(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                          const double* X, int64_t x_bstride, const int64_t* n_dev, const int32_t* info_dev,
                          double* part, double* grad_dev) {
  GradArgs g;
  memset(&g, 0, sizeof(g));
  g.n = lay->n;
  g.n_pad = lay->n_pad;
  g.y_row = lay->y_row;
  g.hyp = hyp_dev;
  g.hyp_stride = hyp_stride;
  g.X = X;
  g.x_bs = x_bstride;
  g.d = (int32_t)lay->d;
  g.dp = padded_dim(lay->d);
  g.ntile = (lay->n + ATILE - 1) / ATILE;
  g.part = part;
  g.grad = grad_dev;
  g.info = info_dev;
  g.nb = n_dev;
  adjoint_masks(*kd, g.adj_mask);
  return g;
}

// the -LML tile pass on a factored identity-augmented W (the entries check their arguments first)
static int grad_pass(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                     const double* X, int64_t x_bstride, const int64_t* n_dev, const void* W, const int32_t* info_dev,
                     double* grad_dev, void* work, hipStream_t s) {
  GradArgs g = grad_args(kd, lay, hyp_dev, hyp_stride, X, x_bstride, n_dev, info_dev, static_cast<double*>(work),
                         grad_dev);
  g.W = W;
  g.ld = lay->ld;
  g.w_bs = lay->w_batch_stride;
  GPK_HIP(timed(6, 0.0, 0.0, s, [&] { return launch_grad(*kd, g, lay->dtype, lay->batch, s); }), "grad");
  return 0;
}

// info cleared, K build with identity extra rows, factorisation: uniform, or ragged with the members' sizes n_dev
static int factor_identity(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                           const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                           const double* y, int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv,
                           int32_t* info_dev, void* stream) {
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * lay->batch, reinterpret_cast<hipStream_t>(stream)),
          "memset info");
  if (n_dev) {
    if (int e = gpk_assemble_inverse_ragged(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, y,
                                            y_bstride, n_dev, W, stream))
      return e;
    return gpk_potrf_aug_ragged_ex(lay, W, Winv, info_dev, GPK_AUG_EXTRA_IDENTITY, n_dev, n_dev, stream);
  }
  if (int e = gpk_assemble_inverse(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, y, y_bstride,
                                   W, stream))
    return e;
  return gpk_potrf_aug_ex(lay, W, Winv, info_dev, GPK_AUG_EXTRA_IDENTITY, stream);
}

// the same with test points as extra rows (uniform, or ragged with n_dev and m_dev)
static int factor_test_rows(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                            const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                            const double* Xs, int64_t xs_bstride, const double* y, int64_t y_bstride,
                            const int64_t* n_dev, const int64_t* m_dev, void* W, void* Winv, int32_t* info_dev,
                            void* stream) {
  GPK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int32_t) * lay->batch, reinterpret_cast<hipStream_t>(stream)),
          "memset info");
  if (n_dev) {
    if (int e = gpk_assemble_ragged(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, Xs,
                                    xs_bstride, y, y_bstride, n_dev, m_dev, W, stream))
      return e;
    return gpk_potrf_aug_ragged(lay, W, Winv, info_dev, n_dev, m_dev, stream);
  }
  if (int e = gpk_assemble(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, Xs, xs_bstride,
                           nullptr, 0, y, y_bstride, W, stream))
    return e;
  return gpk_potrf_aug(lay, W, Winv, info_dev, stream);
}

int gpk_nlml_grad(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                  const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                  const double* y, int64_t y_bstride, void* W, void* Winv, int32_t* info_dev,
                  double* out_dev, double* grad_dev, void* work, size_t work_bytes, void* stream) {
  if (int e = check_layout(lay)) return e;
  if (lay->m != lay->n) return fail_arg(2, "gpk_nlml_grad needs a layout planned with m = n");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!info_dev) return fail_arg(13, "info_dev");
  if (!out_dev) return fail_arg(14, "out_dev");
  if (grad_dev && (!work || work_bytes < gpk_grad_workspace_bytes(kd, lay)))
    return fail_arg(16, "work (see gpk_grad_workspace_bytes)");
  if (int e = factor_identity(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, y, y_bstride,
                              nullptr, W, Winv, info_dev, stream))
    return e;
  if (int e = gpk_finalize(lay, W, info_dev, out_dev, nullptr, nullptr, stream)) return e;
  if (!grad_dev) return 0;
  return grad_pass(kd, lay, hyp_dev, hyp_stride, X, x_bstride, nullptr, W, info_dev, grad_dev, work,
                   reinterpret_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------- ragged identity-augmented batches
// Members of different sizes with identity extra rows: member b's extra rows t < n_b are e_t, the rest zero rows
// (m_b = n_b), its training rows past n_b identity padding.  assemble_impl, potrf_impl and finalize_impl take both
// modes at once; the gradient pass reads n_b per member (grad_kernel's ragged instantiation).
int gpk_assemble_inverse_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                                int64_t hyp_stride, const double* noise_dev, int64_t noise_stride,
                                const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                                const int64_t* n_dev, void* W, void* stream) {
  if (!n_dev) return fail_arg(11, "n_dev");
  return assemble_impl(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, nullptr, 0, nullptr, 0,
                       y, y_bstride, W, true, n_dev, n_dev, stream);
}

int gpk_potrf_aug_ragged_ex(const gpk_layout* lay, void* W, void* Winv, int32_t* info_dev, int32_t flags,
                            const int64_t* n_dev, const int64_t* m_dev, void* stream) {
  if (!n_dev) return fail_arg(6, "n_dev");
  if (lay && lay->m > 0 && !m_dev) return fail_arg(7, "m_dev (layout planned with m > 0)");
  return potrf_impl(lay, W, Winv, info_dev, flags, n_dev, lay && lay->m > 0 ? m_dev : nullptr, stream);
}

int gpk_grad_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                    const double* X, int64_t x_bstride, const int64_t* n_dev, const void* W,
                    const int32_t* info_dev, double* grad_dev, void* work, size_t work_bytes, void* stream) {
  if (int e = check_layout(lay)) return e == -1 ? fail_arg(2, "layout (use gpk_plan)") : e;
  if (lay->m != lay->n) return fail_arg(2, "gpk_grad_ragged needs a layout planned with m = n");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!X) return fail_arg(5, "X");
  if (!n_dev) return fail_arg(7, "n_dev");
  if (!W) return fail_arg(8, "W");
  if (!info_dev) return fail_arg(9, "info_dev");
  if (!grad_dev) return fail_arg(10, "grad_dev");
  if (!work || work_bytes < gpk_grad_workspace_bytes(kd, lay))
    return fail_arg(11, "work (see gpk_grad_workspace_bytes)");
  return grad_pass(kd, lay, hyp_dev, hyp_stride, X, x_bstride, n_dev, W, info_dev, grad_dev, work,
                   reinterpret_cast<hipStream_t>(stream));
}

int gpk_nlml_grad_ragged(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                         const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride,
                         const double* y, int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv,
                         int32_t* info_dev, double* out_dev, double* grad_dev, void* work, size_t work_bytes,
                         void* stream) {
  if (int e = check_layout(lay)) return e == -1 ? fail_arg(2, "layout (use gpk_plan)") : e;
  if (lay->m != lay->n) return fail_arg(2, "gpk_nlml_grad_ragged needs a layout planned with m = n");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!n_dev) return fail_arg(11, "n_dev");
  if (!info_dev) return fail_arg(14, "info_dev");
  if (!out_dev) return fail_arg(15, "out_dev");
  if (grad_dev && (!work || work_bytes < gpk_grad_workspace_bytes(kd, lay)))
    return fail_arg(17, "work (see gpk_grad_workspace_bytes)");
  if (int e = factor_identity(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, y, y_bstride,
                              n_dev, W, Winv, info_dev, stream))
    return e;
  if (int e = gpk_finalize_ragged(lay, W, info_dev, n_dev, out_dev, nullptr, nullptr, stream)) return e;
  if (!grad_dev) return 0;
  return gpk_grad_ragged(kd, lay, hyp_dev, hyp_stride, X, x_bstride, n_dev, W, info_dev, grad_dev, work, work_bytes,
                         stream);
}

// ------------------------------------------------------------------------- held-out MSE and its gradient
// workspace: [batch][2][n_pad] right-hand sides / solutions, [batch][m] residuals, [batch][tiles][n_hyp + 1] partials
static size_t mse_rhs_elems(const gpk_layout* lay) { return (size_t)lay->batch * 2 * (size_t)lay->n_pad; }
static size_t mse_res_elems(const gpk_layout* lay) { return (size_t)lay->batch * (size_t)lay->m; }

size_t gpk_mse_grad_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay) {
  if (!kd || !lay || lay->n <= 0 || lay->m <= 0 || lay->batch <= 0) return 0;
  if (!valid_kdesc(kd, lay->d)) return 0;  // (gpk_mse_backward refuses such a program: no workspace to size)
  return (mse_rhs_elems(lay) + mse_res_elems(lay) +
          (size_t)lay->batch * (size_t)mse_tiles(lay->n, lay->m) * (size_t)(kd->n_hyp + 1)) * sizeof(double);
}

int gpk_mse_backward(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                     const double* X, int64_t x_bstride, const double* Xs, int64_t xs_bstride, const double* ys,
                     int64_t ys_bstride, const int64_t* n_dev, const int64_t* m_dev, const void* W, const void* Winv,
                     const int32_t* info_dev, double* out_dev, double* grad_dev, void* work, size_t work_bytes,
                     void* stream) {
  if (int e = check_layout(lay)) return e == -1 ? fail_arg(2, "layout (use gpk_plan)") : e;
  if (lay->m < 1) return fail_arg(2, "the MSE needs a layout planned with m >= 1 test points");
  if (lay->dtype != GPK_F64) return fail_arg(30, "the MSE gradient is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!X) return fail_arg(5, "X");
  if (!Xs) return fail_arg(7, "Xs");
  if (!ys) return fail_arg(9, "ys");
  if ((n_dev == nullptr) != (m_dev == nullptr)) return fail_arg(11, "n_dev and m_dev: both or neither");
  if (!W) return fail_arg(13, "W");
  if (!Winv) return fail_arg(14, "Winv");
  if (!info_dev) return fail_arg(15, "info_dev");
  if (!out_dev) return fail_arg(16, "out_dev");
  if (!grad_dev) return fail_arg(17, "grad_dev");
  if (!work || work_bytes < gpk_mse_grad_workspace_bytes(kd, lay))
    return fail_arg(18, "work (see gpk_mse_grad_workspace_bytes)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MseArgs g;
  memset(&g, 0, sizeof(g));
  g.W = static_cast<const double*>(W);
  g.ld = lay->ld;
  g.w_bs = lay->w_batch_stride;
  g.n = lay->n;
  g.m = lay->m;
  g.n_pad = lay->n_pad;
  g.y_row = lay->y_row;
  g.hyp = hyp_dev;
  g.hyp_stride = hyp_stride;
  g.X = X;
  g.x_bs = x_bstride;
  g.Xs = Xs;
  g.xs_bs = xs_bstride;
  g.ys = ys;
  g.ys_bs = ys_bstride;
  g.d = (int32_t)lay->d;
  g.dp = padded_dim(lay->d);
  g.ntr = (lay->n + ATILE - 1) / ATILE;
  g.nte = (lay->m + ATILE - 1) / ATILE;
  g.rhs = static_cast<double*>(work);
  g.res = g.rhs + mse_rhs_elems(lay);
  g.part = g.res + mse_res_elems(lay);
  g.out = out_dev;
  g.grad = grad_dev;
  g.info = info_dev;
  g.nb = n_dev;
  g.mb = m_dev;
  adjoint_masks(*kd, g.adj_mask);
  // (timing classes: the residual kernel is this objective's read-out, class 4; the solves 5; the tile pass 6)
  GPK_HIP(timed(4, 0.0, 0.0, s, [&] { return launch_mse_residual(g, lay->batch, s); }), "mse residual");
  // q = L^-T c and alpha = L^-T z: the batched backward solve once per right-hand side (member stride 2 n_pad)
  const int64_t nblk = lay->n_pad / NB;
  TrsvArgs t;
  t.W = W;
  t.ld = lay->ld;
  t.w_bs = lay->w_batch_stride;
  t.Winv = Winv;
  t.inv_bs = lay->inv_batch_stride;
  t.x_bs = 2 * lay->n_pad;
  t.n_pad = lay->n_pad;
  t.trans = 1;
  t.n_valid = lay->n_pad;
  for (int rhs = 0; rhs < 2; ++rhs) {
    t.x = g.rhs + rhs * lay->n_pad;
    for (int64_t i = 0; i < nblk; ++i) {
      t.kblk = nblk - 1 - i;
      GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_diag(t, GPK_F64, lay->batch, s); }), "mse trsv_diag");
      GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_update(t, GPK_F64, lay->batch, s); }),
              "mse trsv_update");
    }
  }
  GPK_HIP(timed(6, 0.0, 0.0, s, [&] { return launch_mse_tiles(*kd, g, lay->batch, s); }), "mse tiles");
  return 0;
}

int gpk_mse_grad(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                 const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride, const double* Xs,
                 int64_t xs_bstride, const double* y, int64_t y_bstride, const double* ys, int64_t ys_bstride,
                 const int64_t* n_dev, const int64_t* m_dev, void* W, void* Winv, int32_t* info_dev, double* out_dev,
                 double* grad_dev, void* work, size_t work_bytes, void* stream) {
  if (int e = check_layout(lay)) return e == -1 ? fail_arg(2, "layout (use gpk_plan)") : e;
  if (lay->m < 1) return fail_arg(2, "the MSE needs a layout planned with m >= 1 test points");
  if (lay->dtype != GPK_F64) return fail_arg(30, "the MSE gradient is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!noise_dev) return fail_arg(5, "noise_dev");
  if (!X) return fail_arg(7, "X");
  if (!Xs) return fail_arg(9, "Xs");
  if (!y) return fail_arg(11, "y");
  if (!ys) return fail_arg(13, "ys");
  if ((n_dev == nullptr) != (m_dev == nullptr)) return fail_arg(15, "n_dev and m_dev: both or neither");
  if (!W) return fail_arg(17, "W");
  if (!Winv) return fail_arg(18, "Winv");
  if (!info_dev) return fail_arg(19, "info_dev");
  if (!out_dev) return fail_arg(20, "out_dev");
  if (!grad_dev) return fail_arg(21, "grad_dev");
  if (!work || work_bytes < gpk_mse_grad_workspace_bytes(kd, lay))
    return fail_arg(22, "work (see gpk_mse_grad_workspace_bytes)");
  if (int e = factor_test_rows(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, Xs, xs_bstride, y,
                               y_bstride, n_dev, m_dev, W, Winv, info_dev, stream))
    return e;
  // (the read-out: gpk_mse_backward's first kernel reads -mu from the corner's y row, where gpk_finalize reads it;
  // every argument it checks was checked above)
  return gpk_mse_backward(kd, lay, hyp_dev, hyp_stride, X, x_bstride, Xs, xs_bstride, ys, ys_bstride, n_dev, m_dev, W,
                          Winv, info_dev, out_dev, grad_dev, work, work_bytes, stream);
}

// ------------------------------------------------------------------------- leave-one-out cross-validation
// workspace: [batch][4][n_pad] per-point vectors, [batch][slabs][3] partial sums, [batch][n_pad + 1][n_pad] cotangent,
// [batch][lower tiles][n_hyp + 1] partials of the tile pass
static size_t loo_pts_elems(const gpk_layout* lay) { return (size_t)lay->batch * 4 * (size_t)lay->n_pad; }
static size_t loo_slab_elems(const gpk_layout* lay) { return (size_t)lay->batch * 3 * (size_t)loo_slabs(lay->n_pad); }
static size_t loo_cot_elems(const gpk_layout* lay) {
  return (size_t)lay->batch * (size_t)(lay->n_pad + 1) * (size_t)lay->n_pad;
}

size_t gpk_loo_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay) {
  if (!kd || !lay || lay->n <= 0 || lay->m != lay->n || lay->batch <= 0 || lay->dtype != GPK_F64) return 0;
  if (!valid_kdesc(kd, lay->d)) return 0;  // (gpk_loo_backward refuses such a program: no workspace to size)
  return (loo_pts_elems(lay) + loo_slab_elems(lay) + loo_cot_elems(lay)) * sizeof(double) +
         gpk_grad_workspace_bytes(kd, lay);
}

// the checks the two LOO entries share (argument numbers of loss, kd, lay are theirs in both)
static int loo_check(int32_t loss, const gpk_kdesc* kd, const gpk_layout* lay) {
  if (loss != GPK_LOO_LPD && loss != GPK_LOO_MSE) return fail_arg(1, "loss (GPK_LOO_LPD or GPK_LOO_MSE)");
  if (check_layout(lay)) return fail_arg(3, "layout (use gpk_plan)");
  if (lay->m != lay->n) return fail_arg(3, "leave-one-out needs a layout planned with m = n");
  if (lay->dtype != GPK_F64) return fail_arg(30, "leave-one-out is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(2, "kernel descriptor");
  return 0;
}

int gpk_loo_backward(int32_t loss, const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev,
                     int64_t hyp_stride, const double* X, int64_t x_bstride, const double* y, int64_t y_bstride,
                     const int64_t* n_dev, const void* W, const int32_t* info_dev, double* out_dev, double* mu_dev,
                     double* var_dev, double* grad_dev, void* work, size_t work_bytes, void* stream) {
  if (int e = loo_check(loss, kd, lay)) return e;
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(4, "hyp_dev");
  if (!X) return fail_arg(6, "X");
  if (!y) return fail_arg(8, "y");
  if (!W) return fail_arg(11, "W");
  if (!info_dev) return fail_arg(12, "info_dev");
  if (!out_dev) return fail_arg(13, "out_dev");
  if (!work || work_bytes < gpk_loo_workspace_bytes(kd, lay))
    return fail_arg(17, "work (see gpk_loo_workspace_bytes)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  LooArgs g;
  memset(&g, 0, sizeof(g));
  g.W = static_cast<const double*>(W);
  g.ld = lay->ld;
  g.w_bs = lay->w_batch_stride;
  g.n = lay->n;
  g.n_pad = lay->n_pad;
  g.y_row = lay->y_row;
  g.y = y;
  g.y_bs = y_bstride;
  g.loss = loss;
  g.pts = static_cast<double*>(work);
  g.slab = g.pts + loo_pts_elems(lay);
  g.cot = grad_dev ? g.slab + loo_slab_elems(lay) : nullptr;
  g.out = out_dev;
  g.mu = mu_dev;
  g.var = var_dev;
  g.info = info_dev;
  g.nb = n_dev;
  // (timing classes: the read-out 4, the matrix-vector product 5 like gpk_gemv, the cotangent 3 -- the class of the
  // factorisation's MFMA updates, with its flops -- and the tile pass 6)
  GPK_HIP(timed(4, 0.0, 0.0, s, [&] { return launch_loo_points(g, lay->batch, s); }), "loo points");
  if (!grad_dev) return 0;
  const double nn = (double)lay->n;
  GPK_HIP(timed(5, 2.0 * nn * nn * lay->batch, 8.0 * 0.5 * nn * nn * lay->batch, s,
                [&] { return launch_loo_symv(g, lay->batch, s); }),
          "loo symv");
  GPK_HIP(timed(3, nn * nn * nn * lay->batch, 0.0, s, [&] { return launch_loo_cot(g, lay->batch, s); }), "loo cot");
  const GradArgs gg = grad_args(kd, lay, hyp_dev, hyp_stride, X, x_bstride, n_dev, info_dev,
                                g.slab + loo_slab_elems(lay) + loo_cot_elems(lay), grad_dev);
  GPK_HIP(timed(6, 0.0, 0.0, s,
                [&] {
                  return launch_grad_cot(*kd, gg, g.cot, lay->n_pad, (lay->n_pad + 1) * lay->n_pad, lay->n_pad,
                                         lay->batch, s);
                }),
          "loo grad");
  return 0;
}

int gpk_loo_grad(int32_t loss, const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride,
                 const double* noise_dev, int64_t noise_stride, const double* X, int64_t x_bstride, const double* y,
                 int64_t y_bstride, const int64_t* n_dev, void* W, void* Winv, int32_t* info_dev, double* out_dev,
                 double* mu_dev, double* var_dev, double* grad_dev, void* work, size_t work_bytes, void* stream) {
  if (int e = loo_check(loss, kd, lay)) return e;
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(4, "hyp_dev");
  if (!noise_dev) return fail_arg(6, "noise_dev");
  if (!X) return fail_arg(8, "X");
  if (!y) return fail_arg(10, "y");
  if (!W) return fail_arg(13, "W");
  if (!Winv) return fail_arg(14, "Winv");
  if (!info_dev) return fail_arg(15, "info_dev");
  if (!out_dev) return fail_arg(16, "out_dev");
  if (!work || work_bytes < gpk_loo_workspace_bytes(kd, lay))
    return fail_arg(20, "work (see gpk_loo_workspace_bytes)");
  if (int e = factor_identity(kd, lay, hyp_dev, hyp_stride, noise_dev, noise_stride, X, x_bstride, y, y_bstride, n_dev,
                              W, Winv, info_dev, stream))
    return e;
  return gpk_loo_backward(loss, kd, lay, hyp_dev, hyp_stride, X, x_bstride, y, y_bstride, n_dev, W, info_dev, out_dev,
                          mu_dev, var_dev, grad_dev, work, work_bytes, stream);
}

int gpk_kernel_matrix(const gpk_kdesc* kd, const double* hyp_dev, int dtype, int uplo,
                      const double* X, int64_t n, const double* Y, int64_t m, int32_t d,
                      double diag_add, void* K, int64_t ldk, void* stream) {
  if (!valid_kdesc(kd, d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(2, "hyp_dev");
  if (dtype != GPK_F64 && dtype != GPK_F32) return fail_arg(3, "dtype");
  if (uplo != 0 && uplo != 1) return fail_arg(4, "uplo");
  if (!X) return fail_arg(5, "X");
  if (n <= 0) return fail_arg(6, "n");
  if (!Y) return fail_arg(7, "Y");
  if (m <= 0) return fail_arg(8, "m");
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(9, "d");
  if (!K) return fail_arg(11, "K");
  if (ldk < m) return fail_arg(12, "ldk");
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = hyp_dev;
  a.noise = nullptr;
  a.X = X;
  a.Xs = Y;
  a.W = K;
  a.ld = ldk;
  a.n = n;
  a.m = m;
  a.d = d;
  a.dp = padded_dim(d);
  a.plain = 1;
  a.uplo = uplo;
  a.diag_add = diag_add;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double bytes = (double)elem_size(dtype) * (double)n * (double)m;
  GPK_HIP(timed(0, 0.0, bytes, s, [&] { return launch_assemble(*kd, a, dtype, 1, s); }),
          "kernel_matrix");
  return 0;
}

int gpk_trsv(const gpk_layout* lay, int trans, const void* W, const void* Winv, double* x,
             void* stream) {
  if (int e = check_layout(lay)) return e;
  if (trans != 0 && trans != 1) return fail_arg(2, "trans");
  if (!W) return fail_arg(3, "W");
  if (!Winv) return fail_arg(4, "Winv");
  if (!x) return fail_arg(5, "x");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nblk = lay->n_pad / NB;
  TrsvArgs t;
  t.W = W;
  t.ld = lay->ld;
  t.w_bs = lay->w_batch_stride;
  t.Winv = Winv;
  t.inv_bs = lay->inv_batch_stride;
  t.x = x;
  t.x_bs = lay->n_pad;
  t.n_pad = lay->n_pad;
  t.trans = trans;
  t.n_valid = lay->n_pad;
  for (int64_t i = 0; i < nblk; ++i) {
    t.kblk = (trans == 0) ? i : nblk - 1 - i;
    GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_diag(t, lay->dtype, lay->batch, s); }),
            "trsv_diag");
    GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_update(t, lay->dtype, lay->batch, s); }),
            "trsv_update");
  }
  return 0;
}

int gpk_trsv_lower(int dtype, int trans, const double* L, int64_t n, int64_t ldl, double* x, void* work,
                   size_t work_bytes, void* stream) {
  if (dtype != GPK_F64) return fail_arg(1, "dtype (gpk_trsv_lower solves fp64)");
  if (trans != 0 && trans != 1) return fail_arg(2, "trans");
  if (!L) return fail_arg(3, "L");
  if (n <= 0) return fail_arg(4, "n");
  if (ldl < n) return fail_arg(5, "ldl");
  if (!x) return fail_arg(6, "x");
  if (!work || work_bytes < gpk_workspace_bytes(GPK_WS_TRSV, GPK_F64, n, 0, 1))
    return fail_arg(8, "work (gpk_workspace_bytes(GPK_WS_TRSV))");
  const int64_t n_pad = (n + NB - 1) / NB * NB, nblk = n_pad / NB;
  char* w = static_cast<char*>(work);
  double* Winv = reinterpret_cast<double*>(w);
  double* xp = reinterpret_cast<double*>(w + align256((size_t)n_pad * NB * sizeof(double)));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_trtri_blocks(L, ldl, n, Winv, s), "trsv_lower diagonal blocks");
  GPK_HIP(hipMemsetAsync(xp, 0, (size_t)n_pad * sizeof(double), s), "trsv_lower x");
  GPK_HIP(hipMemcpyAsync(xp, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s), "trsv_lower x");
  TrsvArgs t;
  t.W = L;
  t.ld = ldl;
  t.w_bs = 0;
  t.Winv = Winv;
  t.inv_bs = 0;
  t.x = xp;
  t.x_bs = n_pad;
  t.n_pad = n_pad;
  t.trans = trans;
  t.n_valid = n;
  for (int64_t i = 0; i < nblk; ++i) {
    t.kblk = (trans == 0) ? i : nblk - 1 - i;
    GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_diag(t, GPK_F64, 1, s); }), "trsv_lower diag");
    GPK_HIP(timed(5, 0.0, 0.0, s, [&] { return launch_trsv_update(t, GPK_F64, 1, s); }), "trsv_lower update");
  }
  GPK_HIP(hipMemcpyAsync(x, xp, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s), "trsv_lower x");
  return 0;
}

int gpk_posterior(const gpk_kdesc* kd, const double* hyp_dev, int dtype, const double* L, int64_t ldl,
                  const double* alpha, const double* X, int64_t n, const double* Xs, int64_t m, int32_t d,
                  int32_t var_mode, double* mu, double* var, int64_t ldv, void* work, size_t work_bytes,
                  void* stream) {
  if (!valid_kdesc(kd, d)) return fail_arg(1, "kernel descriptor");
  if (dtype != GPK_F64) return fail_arg(3, "dtype (gpk_posterior is fp64)");
  if (!L) return fail_arg(4, "L");
  if (ldl < n) return fail_arg(5, "ldl");
  if (!alpha && mu) return fail_arg(6, "alpha");
  if (!X) return fail_arg(7, "X");
  if (n <= 0) return fail_arg(8, "n");
  if (!Xs) return fail_arg(9, "Xs");
  if (m <= 0) return fail_arg(10, "m");
  if (var_mode != 0 && var_mode != 1) return fail_arg(12, "var_mode");
  if (var && var_mode == 1 && ldv < m) return fail_arg(15, "ldv");
  if (!work || work_bytes < gpk_workspace_bytes(GPK_WS_POSTERIOR, GPK_F64, n, m, 1))
    return fail_arg(16, "work (gpk_workspace_bytes(GPK_WS_POSTERIOR))");
  const int64_t n_pad = (n + NB - 1) / NB * NB, nblk = n_pad / NB;
  char* w = static_cast<char*>(work);
  double* Winv = reinterpret_cast<double*>(w);
  w += align256((size_t)n_pad * NB * sizeof(double));
  double* Ks = reinterpret_cast<double*>(w);
  w += align256((size_t)n_pad * (size_t)m * sizeof(double));
  double* V = reinterpret_cast<double*>(w);
  w += align256((size_t)n_pad * (size_t)m * sizeof(double));
  double* kdiag = reinterpret_cast<double*>(w);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // K_s = k(X, Xs) [n, m], zero padding rows
  if (n_pad > n)
    GPK_HIP(hipMemsetAsync(Ks + n * m, 0, (size_t)(n_pad - n) * (size_t)m * sizeof(double), s), "posterior pad");
  if (int e = gpk_kernel_matrix(kd, hyp_dev, GPK_F64, 0, X, n, Xs, m, d, 0.0, Ks, m, stream)) return e;
  if (mu) {  // mu = K_s^T alpha (S/Auxiliary.py:57-66)
    DgemmArgs g{1, 0, m, 1, n, Ks, m, 0, alpha, 1, 0, mu, 1, 0, 1.0, 0.0};
    GPK_HIP(launch_dgemm(g, 1, s), "posterior mu");
  }
  if (!var) return 0;
  // V = L^-1 K_s, blocked: V_k = L_kk^-1 K_s,k; K_s,below -= L_below,k V_k
  GPK_HIP(launch_trtri_blocks(L, ldl, n, Winv, s), "posterior diagonal blocks");
  for (int64_t kb = 0; kb < nblk; ++kb) {
    const int64_t j0 = kb * NB, nv = std::min<int64_t>(NB, n - j0);
    DgemmArgs g1{0, 0, NB, m, NB, Winv + kb * NB * NB, NB, 0, Ks + j0 * m, m, 0, V + j0 * m, m, 0, 1.0, 0.0};
    GPK_HIP(launch_dgemm(g1, 1, s), "posterior solve");
    if (j0 + NB < n) {
      DgemmArgs g2{0, 0, n - j0 - NB, m, nv, L + (j0 + NB) * ldl + j0, ldl, 0, V + j0 * m, m, 0,
                   Ks + (j0 + NB) * m, m, 0, -1.0, 1.0};
      GPK_HIP(launch_dgemm(g2, 1, s), "posterior update");
    }
  }
  if (var_mode == 1) {  // Sigma = K_ss - V^T V (S/Auxiliary.py:68-93)
    if (int e = gpk_kernel_matrix(kd, hyp_dev, GPK_F64, 0, Xs, m, Xs, m, d, 0.0, var, ldv, stream)) return e;
    DgemmArgs g{1, 0, m, m, n, V, m, 0, V, m, 0, var, ldv, 0, -1.0, 1.0};
    GPK_HIP(launch_dgemm(g, 1, s), "posterior covariance");
  } else {  // diag: k(x*, x*) is the same for every x* (every kernel of the descriptor is stationary)
    if (int e = gpk_kernel_matrix(kd, hyp_dev, GPK_F64, 0, Xs, 1, Xs, 1, d, 0.0, kdiag, 1, stream)) return e;
    GPK_HIP(launch_posterior_var(V, n, m, kdiag, var, s), "posterior variance");
  }
  return 0;
}

int gpk_gemv(const double* A, int64_t n, int64_t m, int64_t lda, const double* x, double* y, double alpha,
             double beta, void* stream) {
  if (!A) return fail_arg(1, "A");
  if (n < 0) return fail_arg(2, "n");
  if (m < 0) return fail_arg(3, "m");
  if (lda < m) return fail_arg(4, "lda");
  if (!x && m > 0) return fail_arg(5, "x");
  if (!y && n > 0) return fail_arg(6, "y");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(timed(5, 2.0 * (double)n * (double)m, 8.0 * (double)n * (double)m, s,
                [&] { return launch_gemv(A, n, m, lda, x, y, alpha, beta, s); }),
          "gemv");
  return 0;
}

// ------------------------------------------------------------------ approximation paths (§8f.4)
int gpk_assemble_dense(const gpk_layout* lay, const double* A, int64_t lda, int64_t a_bstride,
                       const double* noise_dev, int64_t noise_stride, const double* E, int64_t e_bstride,
                       int32_t eye, const double* y, int64_t y_bstride, void* W, void* stream) {
  if (int e = check_layout(lay)) return e;
  if (lay->dtype != GPK_F64) return fail_arg(1, "layout dtype (dense mode is fp64)");
  if (!A) return fail_arg(2, "A");
  if (lda < lay->n) return fail_arg(3, "lda");
  if (!noise_dev) return fail_arg(5, "noise_dev");
  if (eye && lay->m != lay->n) return fail_arg(9, "identity extra rows need a layout planned with m = n");
  if (lay->m > 0 && !E && !eye) return fail_arg(7, "E (extra rows) or eye");
  if (!y) return fail_arg(10, "y");
  if (!W) return fail_arg(12, "W");
  gpk_kdesc kd;
  memset(&kd, 0, sizeof(kd));
  kd.n_nodes = 1;
  kd.dim = 1;
  kd.nodes[0].op = GPK_OP_SE;
  AsmArgs a;
  memset(&a, 0, sizeof(a));
  a.noise = noise_dev;
  a.noise_stride = noise_stride;
  a.E = (lay->m > 0 && !eye) ? E : nullptr;
  a.e_bs = e_bstride;
  a.y = y;
  a.y_bs = y_bstride;
  a.W = W;
  a.ld = lay->ld;
  a.w_bs = lay->w_batch_stride;
  a.n = lay->n;
  a.m = lay->m;
  a.n_pad = lay->n_pad;
  a.y_row = lay->y_row;
  a.p = lay->p;
  a.d = 1;
  a.dp = 1;
  a.eye = eye ? 1 : 0;
  a.ntile = lay->p / ATILE;
  a.A = A;
  a.a_ld = lda;
  a.a_bs = a_bstride;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_assemble(kd, a, lay->dtype, lay->batch, s), "assemble_dense");
  return 0;
}

int gpk_dgemm(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, double alpha,
              const double* A, int64_t lda, int64_t a_bstride, const double* B, int64_t ldb, int64_t b_bstride,
              double beta, double* C, int64_t ldc, int64_t c_bstride, int32_t batch, void* stream) {
  if (M < 0) return fail_arg(3, "M");
  if (N < 0) return fail_arg(4, "N");
  if (K < 0) return fail_arg(5, "K");
  if (!A && M > 0 && K > 0) return fail_arg(7, "A");
  if (lda < (trans_a ? M : K)) return fail_arg(8, "lda");
  if (!B && N > 0 && K > 0) return fail_arg(10, "B");
  if (ldb < (trans_b ? K : N)) return fail_arg(11, "ldb");
  if (!C && M > 0 && N > 0) return fail_arg(14, "C");
  if (ldc < N) return fail_arg(15, "ldc");
  if (batch < 0) return fail_arg(17, "batch");
  DgemmArgs g{trans_a ? 1 : 0, trans_b ? 1 : 0, M, N, K, A, lda, a_bstride, B, ldb, b_bstride,
              C, ldc, c_bstride, alpha, beta};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(timed(5, 2.0 * (double)M * (double)N * (double)K * batch,
                8.0 * ((double)M * K + (double)K * N + 2.0 * (double)M * N) * batch, s,
                [&] { return launch_dgemm(g, batch, s); }),
          "dgemm");
  return 0;
}

size_t gpk_syevj_workspace_bytes(int64_t m, int32_t batch) {
  if (m <= 0 || batch <= 0) return 8;
  return (size_t)(4 * m * m * (int64_t)batch + 2) * sizeof(double);
}

int gpk_syevj(int64_t m, int32_t batch, const double* A, int64_t lda, int64_t a_bstride, double* V, double* lam,
              void* work, size_t work_bytes, int32_t max_sweeps, int32_t* sweeps_out, void* stream) {
  if (m < 0 || m > (1 << 20)) return fail_arg(1, "m");
  if (batch < 0) return fail_arg(2, "batch");
  if (m == 0 || batch == 0) {
    if (sweeps_out) *sweeps_out = 0;
    return 0;
  }
  if (!A) return fail_arg(3, "A");
  if (lda < m) return fail_arg(4, "lda");
  if (!V) return fail_arg(6, "V");
  if (!lam) return fail_arg(7, "lam");
  if (!work || work_bytes < gpk_syevj_workspace_bytes(m, batch)) return fail_arg(9, "work_bytes");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t blk = m * m * (int64_t)batch;
  double* buf = reinterpret_cast<double*>(work);
  double* Ab[2] = {buf, buf + blk};
  double* Vb[2] = {buf + 2 * blk, buf + 3 * blk};
  int32_t* flag = reinterpret_cast<int32_t*>(buf + 4 * blk);
  GPK_HIP(launch_jacobi_init(A, lda, a_bstride, (int)m, Ab[0], Vb[0], batch, s), "syevj init");
  // optional absolute threshold (gpk_tune("syevj_abs_tol_e3"), default 0 = the relative criterion
  // alone): pairs with |a_pq| below e3 * 1e-3 eps max|a_ii| are not rotated.  Measured on SE Gram
  // matrices (tools/diag_syevj.py): 1 eps saves 1 sweep of 31, 10 eps 7 sweeps with 4x the pinv error
  double* dmax = reinterpret_cast<double*>(flag) + 1;
  GPK_HIP(launch_diag_absmax(Ab[0], (int)m, batch, dmax, s), "syevj scale");
  double host_dmax = 0.0;
  GPK_HIP(hipMemcpyAsync(&host_dmax, dmax, sizeof(double), hipMemcpyDeviceToHost, s), "syevj scale read");
  GPK_HIP(hipStreamSynchronize(s), "syevj sync");
  const double tol_abs = (double)tune_now().syevj_abs_tol_e3 * 1e-3 * 2.220446049250313e-16 * host_dmax;
  const int mm = (int)(m + (m & 1));
  int cur = 0, sweeps = 0;
  for (; sweeps < (max_sweeps > 0 ? max_sweeps : 60); ++sweeps) {
    GPK_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s), "syevj flag");
    for (int r = 0; r < mm - 1; ++r) {
      JacobiArgs ja{Ab[cur], Ab[cur ^ 1], Vb[cur], Vb[cur ^ 1], (int32_t)m, mm, flag, tol_abs};
      GPK_HIP(launch_jacobi_round(ja, r, batch, s), "syevj round");
      cur ^= 1;
    }
    int32_t host_flag = 0;
    GPK_HIP(hipMemcpyAsync(&host_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, s), "syevj flag read");
    GPK_HIP(hipStreamSynchronize(s), "syevj sync");
    if (!host_flag) {
      ++sweeps;
      break;
    }
  }
  GPK_HIP(launch_jacobi_out(Ab[cur], Vb[cur], (int)m, V, lam, batch, s), "syevj out");
  if (sweeps_out) *sweeps_out = sweeps;
  return 0;
}

// ------------------------------------------------------------------- tridiagonal eigensolver (gpk_eig.hip)
namespace {
constexpr int kEigNb = 32;  // reflectors per compact-WY block of the back-transformation
// m^2 < 2^31: the eigensolver's kernels index a row-major m x m matrix with 32-bit products of two indices
#define GPK_SYEVD_MAX_M 46340

struct EigWs {  // carving of the gpk_syevd workspace
  double *W, *Qg, *U, *d, *e, *tau, *Y, *T1, *T2, *Gs, *S, *PV, *vg, *yg, *Sall;
  DcLevel L;
  size_t bytes;
};

EigWs eig_carve(int64_t m, void* base) {
  EigWs ws;
  memset(&ws, 0, sizeof(ws));
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) -> double* {
    double* r = reinterpret_cast<double*>(p ? p + off : nullptr);
    off += (n * sizeof(double) + 255) & ~(size_t)255;
    return r;
  };
  auto itake = [&](size_t n) -> int32_t* { return reinterpret_cast<int32_t*>(take((n + 1) / 2)); };
  const size_t mm = (size_t)m * (size_t)m, hp = (size_t)m / 2 + 1;
  ws.W = take(mm);
  ws.Qg = take(mm);
  ws.U = take(mm);
  ws.d = take(m);
  ws.e = take(m);
  ws.tau = take(m);
  ws.Y = take((size_t)m * kEigNb);
  ws.T1 = take((size_t)m * kEigNb);
  ws.T2 = take((size_t)m * kEigNb);
  ws.Gs = take((size_t)kEigNb * kEigNb);
  ws.S = take((size_t)kEigNb * kEigNb);
  ws.PV = take((size_t)3 * m * kEigNb);
  ws.Sall = take((size_t)(m / kEigNb + 1) * kEigNb * kEigNb);
  ws.vg = take(m);
  ws.yg = take(m);
  DcLevel& L = ws.L;
  L.dK = take(m);
  L.zK = take(m);
  L.rc = take(m);
  L.rs = take(m);
  L.root_t = take(m);
  L.zhat = take(m);
  L.rho = take(hp);
  L.idx = itake(m);
  L.ord = itake(m);
  L.rp = itake(m);
  L.rn = itake(m);
  L.root_o = itake(m);
  L.kcnt = itake(hp);
  L.rcnt = itake(hp);
  L.flip = itake(hp);
  L.gscr = take((size_t)5 * m);
  ws.bytes = off;
  return ws;
}

// C <- alpha op(A) op(B) + beta C (row-major, contiguous leading dimensions)
hipError_t eig_gemm(int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                    const double* B, int64_t ldb, double beta, double* C, int64_t ldc, hipStream_t s) {
  DgemmArgs g{ta, tb, M, N, K, A, lda, 0, B, ldb, 0, C, ldc, 0, alpha, beta};
  return launch_dgemm(g, 1, s);
}
}  // namespace

size_t gpk_syevd_workspace_bytes(int64_t m) {
  if (m <= 0) return 8;
  return eig_carve(m, nullptr).bytes;
}

int gpk_syevd(int64_t m, int32_t batch, const double* A, int64_t lda, int64_t a_bstride, double* V, double* lam,
              void* work, size_t work_bytes, void* stream) {
  if (m < 0 || m > GPK_SYEVD_MAX_M) return fail_arg(1, "m (gpk_syevd: m <= 46340)");
  if (batch < 0) return fail_arg(2, "batch");
  if (m == 0 || batch == 0) return 0;
  if (!A) return fail_arg(3, "A");
  if (lda < m) return fail_arg(4, "lda");
  if (!V) return fail_arg(6, "V");
  if (!lam) return fail_arg(7, "lam");
  if (!work || work_bytes < gpk_syevd_workspace_bytes(m)) return fail_arg(8, "work (gpk_syevd_workspace_bytes)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EigWs ws = eig_carve(m, work);
  const Tune tn = tune_now();
  const int mi = (int)m;
  const int64_t mm = m * m;
  for (int32_t b = 0; b < batch; ++b) {
    double* Vb = V + (int64_t)b * mm;
    double* lb = lam + (int64_t)b * m;
    GPK_HIP(launch_sym_copy(A + (int64_t)b * a_bstride, lda, mi, ws.W, s), "syevd copy");
    if (m == 1) {
      GPK_HIP(hipMemcpyAsync(lb, ws.W, sizeof(double), hipMemcpyDeviceToDevice, s), "syevd m=1");
      GPK_HIP(launch_eig_identity(Vb, 1, s), "syevd m=1");
      continue;
    }
    GPK_HIP(launch_eig_tridiag(ws.W, mi, ws.d, ws.e, ws.tau, ws.PV, ws.vg, ws.yg, (int)tn.trd_split_m, s),
            "syevd tridiag");
    // eigenvectors of T into V, eigenvalues into lam
    DcLevel L = ws.L;
    L.lam = lb;
    GPK_HIP(launch_eig_dc(ws.d, ws.e, mi, L, Vb, ws.Qg, ws.U, s), "syevd divide and conquer");
    // V <- Q V, Q = H_0 ... H_{m-2}: blocks of reflectors from the last to the first, V <- V - Y (S (Y^T V))
    if (eig_bt_fused(mi)) {
      GPK_HIP(launch_eig_backtransform(ws.W, ws.tau, mi, ws.Sall, Vb, s), "syevd back-transformation");
      continue;
    }
    const int nref = mi - 1;
    for (int k0 = ((nref - 1) / kEigNb) * kEigNb; k0 >= 0; k0 -= kEigNb) {
      const int nb = std::min(kEigNb, nref - k0);
      GPK_HIP(launch_eig_build_y(ws.W, mi, k0, nb, ws.Y, s), "syevd Y");
      GPK_HIP(eig_gemm(1, 0, nb, nb, m, 1.0, ws.Y, nb, ws.Y, nb, 0.0, ws.Gs, nb, s), "syevd Y^T Y");
      GPK_HIP(launch_eig_larft(ws.Gs, ws.tau, k0, nb, ws.S, s), "syevd larft");
      GPK_HIP(eig_gemm(1, 0, nb, m, m, 1.0, ws.Y, nb, Vb, m, 0.0, ws.T1, m, s), "syevd Y^T V");
      GPK_HIP(eig_gemm(0, 0, nb, m, nb, 1.0, ws.S, nb, ws.T1, m, 0.0, ws.T2, m, s), "syevd S (Y^T V)");
      GPK_HIP(eig_gemm(0, 0, m, m, nb, -1.0, ws.Y, nb, ws.T2, m, 1.0, Vb, m, s), "syevd V update");
    }
  }
  return 0;
}

int gpk_pinv_factor(int64_t m, int32_t batch, const double* V, const double* lam, double rcond, int32_t mode,
                    double* mu, double* U, int32_t* rank_dev, void* stream) {
  if (m <= 0) return fail_arg(1, "m");
  if (batch <= 0) return fail_arg(2, "batch");
  if (!V) return fail_arg(3, "V");
  if (!lam) return fail_arg(4, "lam");
  if (mode < 0 || mode > 2) return fail_arg(6, "mode (0, 1 or 2)");
  if (!mu) return fail_arg(7, "mu");
  if (!U) return fail_arg(8, "U");
  if (!rank_dev) return fail_arg(9, "rank_dev");
  if (rcond < 0.0) rcond = 10.0 * (double)m * 2.220446049250313e-16;  // tf.linalg.pinv's default
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_pinv_factor(V, lam, (int)m, rcond, mode, mu, U, rank_dev, batch, s), "pinv_factor");
  return 0;
}

int gpk_pinv_backward_scale(int64_t m, int32_t batch, const double* lam, const double* mu, double* T, void* stream) {
  if (m <= 0) return fail_arg(1, "m");
  if (batch <= 0) return fail_arg(2, "batch");
  if (!lam) return fail_arg(3, "lam");
  if (!mu) return fail_arg(4, "mu");
  if (!T) return fail_arg(5, "T");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_pinv_bwd_scale(lam, mu, (int)m, T, batch, s), "pinv_backward_scale");
  return 0;
}

int gpk_ski_weights(const double* X, int64_t n, const double* Z, int64_t m, int32_t d, double* Wm, double* work,
                    void* stream) {
  if (!X) return fail_arg(1, "X");
  if (n <= 0) return fail_arg(2, "n");
  if (!Z) return fail_arg(3, "Z");
  if (m <= 0) return fail_arg(4, "m");
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(5, "d");
  if (!Wm) return fail_arg(6, "Wm");
  if (!work) return fail_arg(7, "work");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_ski_weights(X, n, Z, m, d, Wm, work, s), "ski_weights");
  return 0;
}

int gpk_distance_matrix(int mode, const double* A, int64_t n, int64_t a_bstride, const double* B, int64_t m,
                        int64_t b_bstride, int32_t d, int32_t batch, double* out, int64_t ldo, int64_t o_bstride,
                        void* stream) {
  if (mode < 0 || mode > 2) return fail_arg(1, "mode (0 expanded-norm euclidean, 1 manhattan, 2 euclidean)");
  if (!A && n > 0) return fail_arg(2, "A");
  if (n < 0) return fail_arg(3, "n");
  if (!B && m > 0) return fail_arg(5, "B");
  if (m < 0) return fail_arg(6, "m");
  if (d <= 0) return fail_arg(8, "d");
  if (batch < 0) return fail_arg(9, "batch");
  if (!out && n > 0 && m > 0) return fail_arg(10, "out");
  if (ldo < m) return fail_arg(11, "ldo");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_distance(mode, A, n, a_bstride, B, m, b_bstride, d, batch, out, ldo, o_bstride, s), "distance");
  return 0;
}

size_t gpk_kernel_vjp_workspace_bytes(const gpk_kdesc* kd, int64_t n, int64_t m, int32_t d, int32_t want_z) {
  if (!kd || n <= 0 || m <= 0 || d <= 0) return 0;
  return vjp_workspace_elems(*kd, n, m, d, want_z != 0) * sizeof(double);
}

int gpk_kernel_vjp(const gpk_kdesc* kd, const double* hyp_dev, const double* X, int64_t n, const double* Z, int64_t m,
                   int32_t d, const double* G, int64_t ldg, const double* gu, const double* gv, double* grad_hyp,
                   double* grad_z, void* work, size_t work_bytes, void* stream) {
  if (!valid_kdesc(kd, d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(2, "hyp_dev");
  if (!X) return fail_arg(3, "X");
  if (n <= 0) return fail_arg(4, "n");
  if (!Z) return fail_arg(5, "Z");
  if (m <= 0) return fail_arg(6, "m");
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(7, "d");
  if (!G && !(gu && gv)) return fail_arg(8, "G (or the rank-1 weights gu, gv)");
  if (G && ldg < m) return fail_arg(9, "ldg");
  if (!grad_hyp && kd->n_hyp > 0) return fail_arg(12, "grad_hyp");
  if (!work || work_bytes < gpk_kernel_vjp_workspace_bytes(kd, n, m, d, grad_z != nullptr ? 1 : 0))
    return fail_arg(14, "work (see gpk_kernel_vjp_workspace_bytes)");
  VjpArgs g;
  memset(&g, 0, sizeof(g));
  g.hyp = hyp_dev;
  g.G = G;
  g.ldg = ldg;
  g.gu = gu;
  g.gv = gv;
  g.part_h = static_cast<double*>(work);
  adjoint_masks(*kd, g.adj_mask);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(timed(6, 0.0, 8.0 * (double)n * (double)m, s,
                [&] { return launch_vjp(*kd, g, X, n, Z, m, d, grad_hyp, grad_z, s); }),
          "kernel_vjp");
  return 0;
}

size_t gpk_kernel_jacobian_workspace_bytes(const gpk_kdesc* kd, int64_t n, int64_t m, int32_t d) {
  (void)kd, (void)n, (void)m, (void)d;
  return 0;  // the planes are written directly: no partial sums
}

int gpk_kernel_jacobian(const gpk_kdesc* kd, const double* hyp_dev, int64_t hyp_stride, int32_t batch, const double* X,
                        int64_t n, int64_t x_bstride, const double* Z, int64_t m, int64_t z_bstride, int32_t d,
                        double* J, int64_t ldj, int64_t plane_stride, int64_t j_bstride, void* work, size_t work_bytes,
                        void* stream) {
  (void)work, (void)work_bytes;
  if (!valid_kdesc(kd, d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(2, "hyp_dev");
  if (batch <= 0 || batch > 65535) return fail_arg(4, "batch (1 .. 65535)");
  if (batch > 1 && hyp_stride != 0 && hyp_stride < kd->n_hyp) return fail_arg(3, "hyp_stride");
  if (!X) return fail_arg(5, "X");
  if (n <= 0) return fail_arg(6, "n");
  if (batch > 1 && x_bstride != 0 && x_bstride < n * d) return fail_arg(7, "x_bstride");
  if (!Z) return fail_arg(8, "Z");
  if (m <= 0) return fail_arg(9, "m");
  if (batch > 1 && z_bstride != 0 && z_bstride < m * d) return fail_arg(10, "z_bstride");
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(11, "d");
  if (kd->n_hyp == 0) return 0;  // no plane to write
  if (!J) return fail_arg(12, "J");
  if (ldj < m) return fail_arg(13, "ldj");
  if (kd->n_hyp > 1 && plane_stride < (n - 1) * ldj + m) return fail_arg(14, "plane_stride");
  if (batch > 1 && j_bstride < (kd->n_hyp - 1) * plane_stride + (n - 1) * ldj + m) return fail_arg(15, "j_bstride");
  JacArgs g;
  memset(&g, 0, sizeof(g));
  g.hyp = hyp_dev;
  g.hyp_stride = hyp_stride;
  g.J = J;
  g.ldj = ldj;
  g.plane_stride = plane_stride;
  g.j_bs = j_bstride;
  adjoint_masks(*kd, g.adj_mask);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(timed(6, 0.0, 8.0 * (double)n * (double)m * kd->n_hyp * batch, s,
                [&] { return launch_jacobian(*kd, g, X, x_bstride, n, Z, z_bstride, m, d, 0, batch, s); }),
          "kernel_jacobian");
  return 0;
}

size_t gpk_fisher_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay) {
  if (!kd || !lay || lay->n <= 0 || lay->m != lay->n || lay->batch <= 0 || lay->dtype != GPK_F64) return 0;
  if (!valid_kdesc(kd, lay->d)) return 0;  // (gpk_fisher refuses such a program: no workspace to size)
  return fisher_workspace_elems(kd->n_hyp, lay->n) * sizeof(double);
}

int gpk_fisher(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, int64_t hyp_stride, const double* X,
               int64_t x_bstride, const void* W, const int32_t* info_dev, double* fisher_dev, void* work,
               size_t work_bytes, void* stream) {
  if (check_layout(lay)) return fail_arg(2, "layout (use gpk_plan)");
  if (lay->m != lay->n) return fail_arg(2, "gpk_fisher needs a layout planned with m = n");
  if (lay->dtype != GPK_F64) return fail_arg(2, "Fisher information is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!X) return fail_arg(5, "X");
  if (!W) return fail_arg(7, "W");
  if (!info_dev) return fail_arg(8, "info_dev");
  if (!fisher_dev) return fail_arg(9, "fisher_dev");
  if (!work || work_bytes < gpk_fisher_workspace_bytes(kd, lay))
    return fail_arg(11, "work (see gpk_fisher_workspace_bytes)");
  FisherArgs g;
  memset(&g, 0, sizeof(g));
  g.W = static_cast<const double*>(W);
  g.ld = lay->ld;
  g.w_bs = lay->w_batch_stride;
  g.n = lay->n;
  g.n_pad = lay->n_pad;
  g.d = (int32_t)lay->d;
  g.hyp = hyp_dev;
  g.hyp_stride = hyp_stride;
  g.X = X;
  g.x_bs = x_bstride;
  g.info = info_dev;
  g.fisher = fisher_dev;
  g.work = static_cast<double*>(work);
  adjoint_masks(*kd, g.adj_mask);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double nn = (double)lay->n;
  // (timing class 5, gpk_dgemm's: the products are the pass's flops)
  GPK_HIP(timed(5, 2.0 * kd->n_hyp * nn * nn * nn * lay->batch, 0.0, s,
                [&] { return launch_fisher(*kd, g, lay->batch, s); }),
          "fisher");
  return 0;
}

size_t gpk_predict_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay, int64_t rows) {
  if (!kd || !lay || lay->n <= 0 || lay->m != lay->n || lay->batch <= 0 || lay->dtype != GPK_F64) return 0;
  if (lay->n_pad < lay->n || lay->n_pad % NB != 0 || rows < 1 || rows > predict_max_rows()) return 0;
  if (!valid_kdesc(kd, lay->d)) return 0;  // (gpk_predict refuses such a program: no workspace to size)
  return predict_workspace_elems(lay->n, lay->n_pad, rows) * sizeof(double);
}

int gpk_predict(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, const double* X, const void* W,
                int32_t member, const double* Xs, int64_t m, double* mu, double* var, void* work, size_t work_bytes,
                void* stream) {
  if (check_layout(lay)) return fail_arg(2, "layout (use gpk_plan)");
  if (lay->m != lay->n) return fail_arg(2, "gpk_predict needs a layout planned with m = n");
  if (lay->dtype != GPK_F64) return fail_arg(2, "prediction is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!X) return fail_arg(4, "X");
  if (!W) return fail_arg(5, "W");
  if (member < 0 || member >= lay->batch) return fail_arg(6, "member (0 .. batch - 1)");
  if (!Xs) return fail_arg(7, "Xs");
  if (m <= 0) return fail_arg(8, "m");
  if (!mu && !var) return fail_arg(9, "mu and var (both NULL)");
  // as many test points per pass as the workspace holds: all of them, or a multiple of the 64-row tile
  const int64_t tile = std::min<int64_t>(m, ATILE);
  if (!work || work_bytes < gpk_predict_workspace_bytes(kd, lay, tile))
    return fail_arg(11, "work (see gpk_predict_workspace_bytes: at least one tile of 64 rows, or m rows)");
  int64_t rows = (int64_t)(work_bytes / gpk_predict_workspace_bytes(kd, lay, 1));
  rows = std::min<int64_t>(rows, predict_max_rows());
  rows = rows >= m ? m : rows / ATILE * ATILE;
  PredictArgs g;
  memset(&g, 0, sizeof(g));
  g.W = static_cast<const double*>(W) + (int64_t)member * lay->w_batch_stride;
  g.ld = lay->ld;
  g.n = lay->n;
  g.n_pad = lay->n_pad;
  g.y_row = lay->y_row;
  g.d = (int32_t)lay->d;
  g.hyp = hyp_dev;
  g.X = X;
  g.Xs = Xs;
  g.m = m;
  g.mu = mu;
  g.var = var;
  g.work = static_cast<double*>(work);
  g.rows = rows;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double nn = (double)lay->n;
  // (timing class 5, gpk_dgemm's: the triangular product is the pass's flops)
  GPK_HIP(timed(5, (var ? nn * nn : 0.0) * (double)m + 2.0 * nn * (double)m, 8.0 * nn * (double)m, s,
                [&] { return launch_predict(*kd, g, s); }),
          "predict");
  return 0;
}

size_t gpk_predict_vt_workspace_bytes(const gpk_kdesc* kd, const gpk_layout* lay, int64_t rows) {
  if (gpk_predict_workspace_bytes(kd, lay, rows) == 0) return 0;  // (the same refusals)
  return predict_vt_workspace_elems(lay->n_pad, rows) * sizeof(double);
}

int gpk_predict_vt(const gpk_kdesc* kd, const gpk_layout* lay, const double* hyp_dev, const double* X, const void* W,
                   int32_t member, const double* Xs, int64_t m, double* Vt, int64_t ldv, void* work, size_t work_bytes,
                   void* stream) {
  if (check_layout(lay)) return fail_arg(2, "layout (use gpk_plan)");
  if (lay->m != lay->n) return fail_arg(2, "gpk_predict_vt needs a layout planned with m = n");
  if (lay->dtype != GPK_F64) return fail_arg(2, "prediction is fp64 only (layout planned with GPK_F32)");
  if (!valid_kdesc(kd, lay->d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (!X) return fail_arg(4, "X");
  if (!W) return fail_arg(5, "W");
  if (member < 0 || member >= lay->batch) return fail_arg(6, "member (0 .. batch - 1)");
  if (!Xs) return fail_arg(7, "Xs");
  if (m <= 0) return fail_arg(8, "m");
  if (!Vt) return fail_arg(9, "Vt");
  if (ldv < lay->n) return fail_arg(10, "ldv (at least n)");
  // as many test points per pass as the workspace holds: all of them, or a multiple of the 64-row tile
  const int64_t tile = std::min<int64_t>(m, ATILE);
  if (!work || work_bytes < gpk_predict_vt_workspace_bytes(kd, lay, tile))
    return fail_arg(11, "work (see gpk_predict_vt_workspace_bytes: at least one tile of 64 rows, or m rows)");
  int64_t rows = (int64_t)(work_bytes / gpk_predict_vt_workspace_bytes(kd, lay, 1));
  rows = std::min<int64_t>(rows, predict_max_rows());
  rows = rows >= m ? m : rows / ATILE * ATILE;
  PredictVtArgs g;
  memset(&g, 0, sizeof(g));
  g.W = static_cast<const double*>(W) + (int64_t)member * lay->w_batch_stride;
  g.ld = lay->ld;
  g.n = lay->n;
  g.n_pad = lay->n_pad;
  g.d = (int32_t)lay->d;
  g.hyp = hyp_dev;
  g.X = X;
  g.Xs = Xs;
  g.m = m;
  g.V = Vt;
  g.ldv = ldv;
  g.work = static_cast<double*>(work);
  g.rows = rows;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double nn = (double)lay->n;
  // (timing class 5, gpk_dgemm's: the triangular product is the pass's flops)
  GPK_HIP(timed(5, nn * nn * (double)m, 8.0 * (2.0 * nn * (double)m + 0.5 * nn * nn), s,
                [&] { return launch_predict_vt(*kd, g, s); }),
          "predict_vt");
  return 0;
}

int gpk_predict_cov(const gpk_kdesc* kd, int32_t d, const double* hyp_dev, const double* Xa, int64_t ma,
                    const double* Va, int64_t lda, const double* Xb, int64_t mb, const double* Vb, int64_t ldb,
                    int64_t n, double* C, int64_t ldc, int32_t symmetric, void* stream) {
  if (d <= 0 || d > GPK_MAX_DIM) return fail_arg(2, "d");
  if (!valid_kdesc(kd, d)) return fail_arg(1, "kernel descriptor");
  if (!hyp_dev && kd->n_hyp > 0) return fail_arg(3, "hyp_dev");
  if (symmetric != 0 && symmetric != 1) return fail_arg(15, "symmetric (0 or 1)");
  if (n <= 0) return fail_arg(12, "n");
  if (!Xa) return fail_arg(4, "Xa");
  if (ma <= 0 || ma > predict_max_rows()) return fail_arg(5, "ma (1 .. 65535 * 64)");
  // (the symmetric launch is one block per lower tile in grid.x: 256 threads each, fewer than 2^32 in all)
  if (symmetric && (ma + ATILE - 1) / ATILE > 5792) return fail_arg(5, "ma (symmetric: at most 5792 * 64)");
  if (!Va) return fail_arg(6, "Va");
  if (lda < n) return fail_arg(7, "lda (at least n)");
  if (!Xb) return fail_arg(8, "Xb");
  if (symmetric && Xb != Xa) return fail_arg(8, "Xb (symmetric: Xb = Xa)");
  if (mb <= 0 || mb > predict_max_rows()) return fail_arg(9, "mb (1 .. 65535 * 64)");
  if (symmetric && mb != ma) return fail_arg(9, "mb (symmetric: mb = ma)");
  if (!Vb) return fail_arg(10, "Vb");
  if (symmetric && Vb != Va) return fail_arg(10, "Vb (symmetric: Vb = Va)");
  if (ldb < n) return fail_arg(11, "ldb (at least n)");
  if (symmetric && ldb != lda) return fail_arg(11, "ldb (symmetric: ldb = lda)");
  if (!C) return fail_arg(13, "C");
  if (ldc < mb) return fail_arg(14, "ldc (at least mb)");
  PredictCovArgs g;
  memset(&g, 0, sizeof(g));
  g.hyp = hyp_dev;
  g.d = d;
  g.Xa = Xa;
  g.ma = ma;
  g.Va = Va;
  g.lda = lda;
  g.Xb = Xb;
  g.mb = mb;
  g.Vb = Vb;
  g.ldb = ldb;
  g.n = n;
  g.C = C;
  g.ldc = ldc;
  g.symmetric = symmetric;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const double half = symmetric ? 0.5 : 1.0;
  // (timing class 5, gpk_dgemm's)
  GPK_HIP(timed(5, half * 2.0 * (double)ma * (double)mb * (double)n,
                8.0 * (((double)ma + (double)mb) * (double)n + 2.0 * (double)ma * (double)mb), s,
                [&] { return launch_predict_cov(*kd, g, s); }),
          "predict_cov");
  return 0;
}

int gpk_mean_op_supported(int32_t op) {
  return (mean_leaf_hyp(op, 1) > 0 || op == GPK_MOP_ADD || op == GPK_MOP_MUL) ? 1 : 0;
}

// the checks gpk_mean_eval and gpk_mean_vjp share (arguments 1 .. 7 of both)
static int check_mean_call(const gpk_mdesc* md, const double* hyp_dev, int64_t hyp_stride, const double* X, int64_t n,
                           int64_t x_bstride, int32_t batch) {
  if (const char* why = mean_desc_error(md)) return fail_arg(1, why);
  if (!hyp_dev && md->n_hyp > 0) return fail_arg(2, "hyp_dev");
  if (hyp_stride < 0) return fail_arg(3, "hyp_stride");
  if (!X) return fail_arg(4, "X");
  if (n < 1) return fail_arg(5, "n must be >= 1");
  if (x_bstride < 0) return fail_arg(6, "x_bstride");
  if (batch < 1) return fail_arg(7, "batch must be >= 1");
  if (mean_blocks(n) > (int64_t)0x7fffffff / batch) return fail_arg(5, "n x batch: too many workgroups for one launch");
  return 0;
}

int gpk_mean_eval(const gpk_mdesc* md, const double* hyp_dev, int64_t hyp_stride, const double* X, int64_t n,
                  int64_t x_bstride, int32_t batch, const double* y, int64_t y_bstride, double* out,
                  int64_t out_bstride, void* stream) {
  if (int e = check_mean_call(md, hyp_dev, hyp_stride, X, n, x_bstride, batch)) return e;
  if (y && y_bstride < 0) return fail_arg(9, "y_bstride");
  if (!out) return fail_arg(10, "out");
  if (out_bstride < (batch > 1 ? n : 0)) return fail_arg(11, "out_bstride");
  MeanArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = hyp_dev;
  a.hyp_stride = hyp_stride;
  a.X = X;
  a.x_bs = x_bstride;
  a.n = n;
  a.y = y;
  a.y_bs = y_bstride;
  a.out = out;
  a.out_bs = out_bstride;
  GPK_HIP(launch_mean_eval(*md, a, batch, reinterpret_cast<hipStream_t>(stream)), "mean_eval");
  return 0;
}

size_t gpk_mean_vjp_workspace_bytes(const gpk_mdesc* md, int64_t n, int32_t batch) {
  if (mean_desc_error(md) || n < 1 || batch < 1) return 0;
  return (size_t)batch * (size_t)mean_blocks(n) * (size_t)std::max<int32_t>(1, md->n_hyp) * sizeof(double);
}

int gpk_mean_vjp(const gpk_mdesc* md, const double* hyp_dev, int64_t hyp_stride, const double* X, int64_t n,
                 int64_t x_bstride, int32_t batch, const double* g, int64_t g_bstride, double* grad_hyp, void* work,
                 size_t work_bytes, void* stream) {
  if (int e = check_mean_call(md, hyp_dev, hyp_stride, X, n, x_bstride, batch)) return e;
  if (!g) return fail_arg(8, "g");
  if (g_bstride < 0) return fail_arg(9, "g_bstride");
  if (!grad_hyp) return fail_arg(10, "grad_hyp");
  if (!work || work_bytes < gpk_mean_vjp_workspace_bytes(md, n, batch))
    return fail_arg(11, "work (see gpk_mean_vjp_workspace_bytes)");
  MeanArgs a;
  memset(&a, 0, sizeof(a));
  a.hyp = hyp_dev;
  a.hyp_stride = hyp_stride;
  a.X = X;
  a.x_bs = x_bstride;
  a.n = n;
  a.g = g;
  a.g_bs = g_bstride;
  a.part = static_cast<double*>(work);
  GPK_HIP(launch_mean_vjp(*md, a, batch, grad_hyp, reinterpret_cast<hipStream_t>(stream)), "mean_vjp");
  return 0;
}

// ---------------------------------------------------------------------------- multi-start L-BFGS step
static const gpk_fit_opts kFitDefaults = {8, 200, 20, 0, 1e-4, 1e-5, 1e-9};

// the checks every gpk_fit_* entry shares: arguments 1 .. 3; *o receives the options in effect
static int check_fit_call(int n_par, int batch, const gpk_fit_opts* opts, gpk_fit_opts* o) {
  *o = opts ? *opts : kFitDefaults;
  if (n_par < 1 || n_par > GPK_FIT_MAX_PAR) return fail_arg(1, "n_par must be in [1, 65]");
  if (batch < 1) return fail_arg(2, "batch must be >= 1");
  if (o->m < 1 || o->m > GPK_FIT_MAX_HISTORY) return fail_arg(3, "opts: m (history) must be in [1, 16]");
  if (o->max_iter < 1) return fail_arg(3, "opts: max_iter must be >= 1");
  if (o->max_backtracks < 0) return fail_arg(3, "opts: max_backtracks must be >= 0");
  if (o->reserved != 0) return fail_arg(3, "opts: the reserved field must be 0");
  if (!(o->c1 > 0.0 && o->c1 < 1.0)) return fail_arg(3, "opts: c1 must be in (0, 1)");
  if (!(o->gtol >= 0.0)) return fail_arg(3, "opts: gtol must be >= 0");
  if (!(o->ftol >= 0.0)) return fail_arg(3, "opts: ftol must be >= 0");
  return 0;
}

size_t gpk_fit_state_bytes(int n_par, int batch, const gpk_fit_opts* opts) {
  gpk_fit_opts o;
  if (check_fit_call(n_par, batch, opts, &o)) return 0;
  return (size_t)batch * (size_t)fit_state_doubles(n_par, o.m) * sizeof(double);
}

int gpk_fit_init(int n_par, int batch, const gpk_fit_opts* opts, const double* x0_dev, int64_t x0_stride,
                 const double* lo_dev, const double* hi_dev, double* state_dev, double* x_trial_dev,
                 int64_t xt_stride, void* stream) {
  gpk_fit_opts o;
  if (int e = check_fit_call(n_par, batch, opts, &o)) return e;
  if (!x0_dev) return fail_arg(4, "x0_dev");
  if (x0_stride < n_par) return fail_arg(5, "x0_stride is smaller than n_par");
  if (!lo_dev) return fail_arg(6, "lo_dev");
  if (!hi_dev) return fail_arg(7, "hi_dev");
  if (!state_dev) return fail_arg(8, "state_dev");
  if (!x_trial_dev) return fail_arg(9, "x_trial_dev");
  if (xt_stride < n_par) return fail_arg(10, "xt_stride is smaller than n_par");
  FitArgs a;
  memset(&a, 0, sizeof(a));
  a.n_par = n_par;
  a.batch = batch;
  a.m = o.m;
  a.g = x0_dev;
  a.g_stride = x0_stride;
  a.lo = lo_dev;
  a.hi = hi_dev;
  a.state = state_dev;
  a.state_stride = fit_state_doubles(n_par, o.m);
  a.xt = x_trial_dev;
  a.xt_stride = xt_stride;
  GPK_HIP(launch_fit_init(a, reinterpret_cast<hipStream_t>(stream)), "fit_init");
  return 0;
}

int gpk_fit_step(int n_par, int batch, const gpk_fit_opts* opts, const double* f_dev, int64_t f_stride,
                 const double* g_dev, int64_t g_stride, const int32_t* info_dev, double* state_dev,
                 double* x_trial_dev, int64_t xt_stride, int32_t* status_dev, void* stream) {
  gpk_fit_opts o;
  if (int e = check_fit_call(n_par, batch, opts, &o)) return e;
  if (!f_dev) return fail_arg(4, "f_dev");
  if (f_stride < 1) return fail_arg(5, "f_stride is smaller than 1");
  if (!g_dev) return fail_arg(6, "g_dev");
  if (g_stride < n_par) return fail_arg(7, "g_stride is smaller than n_par");
  if (!state_dev) return fail_arg(9, "state_dev");
  if (!x_trial_dev) return fail_arg(10, "x_trial_dev");
  if (xt_stride < n_par) return fail_arg(11, "xt_stride is smaller than n_par");
  if (!status_dev) return fail_arg(12, "status_dev");
  FitArgs a;
  memset(&a, 0, sizeof(a));
  a.n_par = n_par;
  a.batch = batch;
  a.m = o.m;
  a.max_iter = o.max_iter;
  a.max_backtracks = o.max_backtracks;
  a.c1 = o.c1;
  a.gtol = o.gtol;
  a.ftol = o.ftol;
  a.f = f_dev;
  a.f_stride = f_stride;
  a.g = g_dev;
  a.g_stride = g_stride;
  a.info = info_dev;
  a.state = state_dev;
  a.xt = x_trial_dev;
  a.xt_stride = xt_stride;
  a.status = status_dev;
  GPK_HIP(launch_fit_step(a, reinterpret_cast<hipStream_t>(stream)), "fit_step");
  return 0;
}

int gpk_fit_current(int n_par, int batch, const double* state_dev, double* x_dev, int64_t x_stride, double* f_dev,
                    double* g_dev, int64_t g_stride, int32_t* iters_dev, void* stream) {
  if (n_par < 1 || n_par > GPK_FIT_MAX_PAR) return fail_arg(1, "n_par must be in [1, 65]");
  if (batch < 1) return fail_arg(2, "batch must be >= 1");
  if (!state_dev) return fail_arg(3, "state_dev");
  if (x_dev && x_stride < n_par) return fail_arg(5, "x_stride is smaller than n_par");
  if (g_dev && g_stride < n_par) return fail_arg(8, "g_stride is smaller than n_par");
  GPK_HIP(launch_fit_current(n_par, batch, state_dev, x_dev, x_stride, f_dev, g_dev, g_stride, iters_dev,
                             reinterpret_cast<hipStream_t>(stream)),
          "fit_current");
  return 0;
}

int gpk_add_diagonal(double* A, int64_t n, int64_t lda, int64_t a_bstride, int32_t batch, double value,
                     void* stream) {
  if (!A && n > 0) return fail_arg(1, "A");
  if (n < 0) return fail_arg(2, "n");
  if (lda < n) return fail_arg(3, "lda");
  if (batch < 0) return fail_arg(5, "batch");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GPK_HIP(launch_add_diag(A, n, lda, a_bstride, value, batch, s), "add_diagonal");
  return 0;
}

int gpk_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_timing.mu);
  g_timing.on = on != 0;
  return 0;
}

// profiling: the per-task stamps of the last chain launch with GPK_CHAIN_TIMES=1 (synchronises the device)
int gpk_chain_times(uint64_t* out, int64_t ntasks) {
  if (!g_chain_times || !out || ntasks > g_chain_times_n) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  return hipMemcpy(out, g_chain_times, (size_t)ntasks * 6 * sizeof(uint64_t), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// debugging: the progress words of the last traced chain launch (GPK_CHAIN_TRACE=1), host memory only
int gpk_chain_trace(int32_t* out, int64_t n) {
  if (!g_chain_trace || !out) return -1;
  memcpy(out, g_chain_trace, (size_t)std::min<int64_t>(n, 4096 * 32) * sizeof(int32_t));
  return 0;
}

namespace {
// gpk_chain_plan(_ex): ap = the argument positions of (tasks_out, cap, ntasks) in the entry point's own signature,
// so that -i names the caller's i-th argument (gpk.h's convention) for both entry points
int chain_plan_impl(int64_t n_pad, int64_t y_row, int32_t grid, int32_t flags, int32_t* tasks_out, int64_t cap,
                    int64_t* ntasks, int ap_cap, int ap_ntasks) {
  if (n_pad <= 0 || n_pad % NB != 0) return fail_arg(1, "n_pad (a positive multiple of 128)");
  if (y_row < n_pad) return fail_arg(2, "y_row (>= n_pad)");
  if (grid <= 0) return fail_arg(3, "grid");
  if (flags & ~(GPK_AUG_EXTRA_IDENTITY | GPK_CHAIN_PLAN_F32)) return fail_arg(4, "flags");
  const bool eye = (flags & GPK_AUG_EXTRA_IDENTITY) != 0;
  const bool f32 = (flags & GPK_CHAIN_PLAN_F32) != 0;
  if (eye && f32) return fail_arg(4, "flags (f32 plans have no identity rows)");
  if (eye && (y_row - n_pad < 1 || y_row - n_pad > n_pad))
    return fail_arg(2, "y_row (identity extra rows: n_pad + n with 0 < n <= n_pad)");
  if (!ntasks) return fail_arg(ap_ntasks, "ntasks");
  const std::vector<int32_t> ord = chain_order(n_pad, y_row, grid, 1, chain_knobs(tune_now(), n_pad, eye, f32, grid), eye);
  if (ord.empty()) {
    return fail_hip(hipErrorUnknown, "chain_order: a task exceeds the device's dependency bound");
  }
  *ntasks = (int64_t)(ord.size() / 4);
  if (tasks_out) {
    if (cap < *ntasks) return fail_arg(ap_cap, "cap (fewer than ntasks)");
    memcpy(tasks_out, ord.data(), ord.size() * sizeof(int32_t));
  }
  return 0;
}
}  // namespace

int gpk_chain_plan(int64_t n_pad, int64_t y_row, int32_t grid, int32_t* tasks_out, int64_t cap, int64_t* ntasks) {
  return chain_plan_impl(n_pad, y_row, grid, 0, tasks_out, cap, ntasks, 5, 6);
}

int gpk_chain_plan_ex(int64_t n_pad, int64_t y_row, int32_t grid, int32_t flags, int32_t* tasks_out, int64_t cap,
                      int64_t* ntasks) {
  return chain_plan_impl(n_pad, y_row, grid, flags, tasks_out, cap, ntasks, 6, 7);
}

int gpk_launch_plan(const gpk_layout* lay, int32_t flags, int32_t counters, int32_t kbuild, void* steps_out, int64_t cap,
                    int64_t* nsteps, int64_t* first_group) {
  static_assert(GPK_LAUNCH_STEP_WORDS == kLaunchStepWords, "gpk.h documents LaunchStep word by word");
  if (int e = check_layout(lay)) return e;
  if (flags & ~GPK_AUG_EXTRA_IDENTITY) return fail_arg(2, "flags");
  const bool eye = (flags & GPK_AUG_EXTRA_IDENTITY) != 0;
  if (eye && lay->m != lay->n) return fail_arg(1, "identity extra rows need a layout planned with m = n");
  if (!nsteps) return fail_arg(7, "nsteps");
  const Tune tn = tune_now();
  std::vector<LaunchStep> steps;
  // (a stream without the counters has no operand scratch either: fold_scratch's rule is fuse_counters')
  launch_plan({lay->dtype == GPK_F32, lay->batch, lay->m, lay->n_pad, lay->y_row, lay->p, false, counters == 0}, eye,
              counters != 0, kbuild != 0, tn, steps);
  *nsteps = (int64_t)steps.size();
  if (first_group) *first_group = launch_first_group(tn, eye, lay->n_pad);
  if (steps_out) {
    if (cap < *nsteps) return fail_arg(6, "cap (fewer than nsteps)");
    memcpy(steps_out, steps.data(), steps.size() * sizeof(LaunchStep));
  }
  return 0;
}

int gpk_tune(const char* key, int64_t value, int64_t* old) {
  if (!key) return fail_arg(1, "key");
  if (!strcmp(key, "chain_force_timeout")) {  // (testing: the next `value` persistent launches time out)
    const int64_t prev = g_chain_force_timeout.exchange(value);
    if (old) *old = prev;
    return 0;
  }
  if (!strcmp(key, "upd_tri")) {
    const int64_t prev = upd_tri_knob().exchange(value);
    if (old) *old = prev;
    return 0;
  }
  int64_t Tune::*f = knob_field(key);
  if (!f) return fail_arg(1, "key (unknown tuning knob)");
  Tune& t = tune();
  if (old) *old = t.*f;
  t.*f = value;
  return 0;
}

int gpk_tune_thread(const char* key, int64_t value, int32_t set, int64_t* old_value, int32_t* old_set) {
  if (!key) return fail_arg(1, "key");
  int64_t Tune::*f = knob_field(key);
  if (!f) return fail_arg(1, "key (unknown tuning knob)");
  tune_thread_set(f, value, set != 0, old_value, old_set);
  return 0;
}

int gpk_chain_stats(int64_t* out, int32_t n) {
  if (!out || n < 1) return fail_arg(1, "out");
  const int64_t v[4] = {g_chain_launches.load(), g_chain_declined.load(), t_chain_last ? 1 : 0,
                        g_chain_force_timeout.load()};
  for (int i = 0; i < n && i < 4; ++i) out[i] = v[i];
  if (n >= 5) {  // (a device read: waits for the work enqueued so far on the null stream's device)
    int64_t t = 0;
    GPK_HIP(chain_timeouts_read(&t), "chain timeouts");
    out[4] = t;
  }
  return 0;
}

int gpk_timing_reset(void) {
  std::lock_guard<std::mutex> lk(g_timing.mu);
  for (auto& t : g_timing.pending) {
    hipEventSynchronize(t.end);
    g_timing.pool.push_back(t.beg);
    g_timing.pool.push_back(t.end);
  }
  g_timing.pending.clear();
  for (int c = 0; c < GPK_NUM_CLASSES; ++c) {
    g_timing.ms[c] = 0;
    g_timing.launches[c] = 0;
    g_timing.flops[c] = 0;
    g_timing.bytes[c] = 0;
  }
  return 0;
}

int gpk_timing_read(double* ms_by_class, int64_t* launches_by_class, double* flops_by_class,
                    double* bytes_by_class) {
  std::lock_guard<std::mutex> lk(g_timing.mu);
  for (auto& t : g_timing.pending) {
    hipError_t e = hipEventSynchronize(t.end);
    if (e != hipSuccess) return fail_hip(e, "timing sync");
    float ms = 0.f;
    hipEventElapsedTime(&ms, t.beg, t.end);
    g_timing.ms[t.cls] += ms;
    g_timing.launches[t.cls] += 1;
    g_timing.flops[t.cls] += t.flops;
    g_timing.bytes[t.cls] += t.bytes;
    g_timing.pool.push_back(t.beg);
    g_timing.pool.push_back(t.end);
  }
  g_timing.pending.clear();
  for (int c = 0; c < GPK_NUM_CLASSES; ++c) {
    if (ms_by_class) ms_by_class[c] = g_timing.ms[c];
    if (launches_by_class) launches_by_class[c] = g_timing.launches[c];
    if (flops_by_class) flops_by_class[c] = g_timing.flops[c];
    if (bytes_by_class) bytes_by_class[c] = g_timing.bytes[c];
  }
  return 0;
}

}  // extern "C"
