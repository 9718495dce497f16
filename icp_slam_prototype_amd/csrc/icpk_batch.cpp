// icpk_batch.cpp -- the frame-batch mode, icpk_align_batch(_device): independent pairs in lock-step groups.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

// ---- frame-batch mode (the frame-pair formulation of icp.cpp:541-563) ----------
// Independent pairs, `batch_group` of them advancing in LOCK STEP: every stage of an iteration is
// ONE launch for the whole group (K1d and K2 with blockIdx.y = pair, the loop step with one
// workgroup per pair), so the two small kernels and the launch gaps of the dependent chain
// sweep -> reduce -> step, which leave most of the GPU idle for a single pair, are shared by the
// group.  Each pair lives in a slot (a child context: its own clouds, grid, loop state and a
// stream for its set-up work); two sets of slots alternate so that the set-up of the next group
// (uploads, grid build, query order) overlaps the loop of the current one.  Results are those
// of icpk_align on the same pair, bit for bit (same kernels' bodies, same canonical reduction
// geometry per pair).
namespace {

struct GroupRun {
  int first = 0, count = 0, set = 0;  // pairs [first, first + count) live in slots [set * G, ...)
  std::vector<int> rc;                // per pair: set-up status (< 0: failed, not in the loop)
};

}  // namespace

namespace icpk {

bool batch_eligible(const icpk_ctx* ctx, const icpk_params* p) {
  return p->nn_mode == ICPK_NN_GRID && !p->host_loop && !ctx->log_fn && !ctx->robust_on && p->profile <= 1 &&
         (p->solve == ICPK_SOLVE_REFERENCE || p->solve == ICPK_SOLVE_KABSCH) && p->max_iterations >= 0 &&
         p->max_iterations <= LOOP_MAX_ITER && p->min_pairs >= 1;
}

int ensure_slots(icpk_ctx* ctx, int n) {
  if (n > 2 * BATCH_MAX) return fail(ctx, ICPK_E_ARG, "too many frame-batch slots");
  int rc = ctx->slot_states.reserve(ctx, 2 * BATCH_MAX);
  if (!rc) rc = ctx->slot_states_host.reserve(ctx, 2 * BATCH_MAX);
  if (rc) return rc;
  while ((int)ctx->slots.size() < n) {
    icpk_ctx* sl = make_context(ctx->device, ctx);
    if (!sl) return fail(ctx, ICPK_E_HIP, "frame-batch slot allocation failed");
    // the slot's loop state lives in the parent's pools (one copy brings a whole group's states back): its own goes
    const size_t k = ctx->slots.size();
    (void)sl->st_dev_mem.release();
    (void)sl->st_host_mem.release();
    sl->st_dev = ctx->slot_states + k;
    sl->st_host = ctx->slot_states_host + k;
    ctx->slots.push_back(sl);
  }
  return ICPK_OK;
}

}  // namespace icpk

namespace {

// uploads + everything up to (not including) the first host wait of the pair's set-up
// device-resident pair into a slot: one launch per cloud (planes, padding and, for the source,
// the working copy) instead of the seven copies and six fills of the general upload path
int slot_ingest_device(icpk_ctx* sl, const icpk_pair& pr) {
  if (pr.nt < 0 || pr.ns < 0 || (pr.nt > 0 && (!pr.tx || !pr.ty || !pr.tz)) || (pr.ns > 0 && (!pr.sx || !pr.sy || !pr.sz)))
    return fail(sl, ICPK_E_ARG, "bad cloud pointers/size");
  ICPK_HIP(sl, hipSetDevice(sl->device));
  int rc = ensure_cloud(sl, sl->tgt, pr.nt);
  if (rc == ICPK_OK) rc = ensure_cloud(sl, sl->src0, pr.ns);
  if (rc == ICPK_OK) rc = ensure_cloud(sl, sl->src, pr.ns);
  if (rc) return rc;
  launch_ingest_cloud(IngestArgs{pr.tx, pr.ty, pr.tz, pr.nt, sl->tgt.cap, __builtin_inff(), sl->tgt.cap, sl->tgt.base, nullptr, 0, 0},
                      sl->stream);
  // (src.cap <= src0.cap always; both paddings reach their own capacity's first NN_TILE multiple above n)
  const int spad = round_up(pr.ns < 1 ? 1 : pr.ns, NN_TILE);
  launch_ingest_cloud(IngestArgs{pr.sx, pr.sy, pr.sz, pr.ns, spad, 0.f, sl->src0.cap, sl->src0.base, sl->src.base, sl->src.cap, 0},
                      sl->stream);
  ICPK_HIP(sl, hipGetLastError());
  sl->have_src = true;
  sl->have_qperm = false;
  target_changed(sl, false);
  return ICPK_OK;
}

int slot_setup_phase1(icpk_ctx* sl, const icpk_pair& pr, hipMemcpyKind kind) {
  int rc;
  if (kind == hipMemcpyDeviceToDevice) {
    rc = slot_ingest_device(sl, pr);
  } else {
    rc = set_target_impl(sl, pr.tx, pr.ty, pr.tz, pr.nt, kind, false);
    if (rc == ICPK_OK) rc = set_source_impl(sl, pr.sx, pr.sy, pr.sz, pr.ns, kind, false);
  }
  if (rc) return rc;
  rc = check_ready(sl);
  if (rc) return rc;
  if (sl->src.n <= 0) return ICPK_OK;  // an empty source takes the single-pair path
  sl->have_seed = false;
  sl->have_qperm = false;
  sl->rec_pending = false;
  return ensure_assoc(sl, sl->src.n);
}

}  // namespace

namespace icpk {

// grid of the target (waits for its 36-byte info), query order, scan-order queries and seeds,
// initial loop state: the slot is then ready for the group's first sweep
int slot_setup_phase2(icpk_ctx* sl, const icpk_params* p, GridSweepArgs& first, bool throttled) {
  int rc = device_loop_begin(sl, p, throttled);
  if (rc) return rc;
  NnArgs a = base_nn_args(sl);
  NnBoxes bx{};
  int recheck = 0;
  rc = prepare_sorted_sweep(sl, ICPK_NN_GRID, a, bx, recheck);
  if (rc) return rc;
  first = grid_sweep_args(sl, a, bx);
  after_grid_sweep(sl);
  sl->rec_pending = true;  // planes / keys come from qm4 / rec on demand (icpk_get_associations)
  sl->src_pristine = false;  // (the loop moves the working copy)
  // (while the launches are being recorded the group's set-up event, recorded after the flush, takes its place)
  if (!setup_recorder()) ICPK_HIP(sl, hipEventRecord(sl->ready_ev, sl->stream));
  return ICPK_OK;
}

ReduceArgs slot_reduce_args(const icpk_ctx* sl) {
  ReduceArgs r{};
  r.best = sl->best;
  r.ax = sl->src.x();
  r.ay = sl->src.y();
  r.az = sl->src.z();
  r.tx = sl->tgt.x();
  r.ty = sl->tgt.y();
  r.tz = sl->tgt.z();
  r.o4 = sl->have_grid ? sl->grid.o4.get() : nullptr;
  r.rec = sl->rec;
  r.partial = sl->partial;
  r.pcount = sl->pcount;
  r.st = sl->st_dev;
  r.nq = sl->src.n;
  r.nblocks = red_blocks(sl->src.n);
  return r;
}

// the whole loop of a group on the parent's stream, then the read-back of every loop state
// throttled: every slot's loop was begun throttled (its steps publish LoopState::progress); the iterations are enqueued
// loop_ahead ahead of the slowest pair and no further once every pair has exited -- what align_device_loop does for
// one pair.  Whatever would have followed is a no-op for every pair: same results either way.
static int wait_group_progress(icpk_ctx* ctx, const std::vector<icpk_ctx*>& act, int steps, bool* all_exited) {
  bool all = false;
  const int rc = spin_until(ctx, [&] {
    all = true;
    for (const icpk_ctx* sl : act) {
      const volatile int* pr = sl->progress;
      const int e = sl->loop_epoch;
      const int w0 = __atomic_load_n(&pr[0], __ATOMIC_ACQUIRE), w1 = pr[1];
      const bool exited = (w1 >> 2) == e && (w1 & 1);
      all = all && exited;
      if (!exited && !((w0 >> 10) == e && (w0 & 1023) >= steps)) return false;
    }
    return true;
  }, "frame-batch group loop made no progress");
  *all_exited = all;
  return rc;
}

int enqueue_group_loop(icpk_ctx* ctx, const icpk_params* p, const std::vector<icpk_ctx*>& act,
                       const std::vector<GridSweepArgs>& first, int set, const std::vector<bool>& own_event,
                       bool throttled) {
  const int n = (int)act.size();
  if (n == 0) return ICPK_OK;
  const int nsum = loop_nsum(p);
  const int nact = nsum == NSUM_REF ? NSUM_REF : NSUM;
  long long nq_total = 0;
  bool group_event = false;
  for (int k = 0; k < n; ++k) {
    icpk_ctx* sl = act[k];
    if (own_event[k])
      ICPK_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl->ready_ev, 0));
    else
      group_event = true;  // set up by the group's batched launches
    nq_total += sl->src.n;
  }
  if (group_event) ICPK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->setup_ev[set], 0));
  // lanes per query: a single pair is latency-bound and wants 8; a group that fills the GPU
  // several times over is issue-bound and does better with fewer, longer lanes (measured on
  // 8 config-2 pairs: 43.4k iter/s with 8, 50.6k with 4, 48.2k with 2)
  int slices = ctx->tune.grid_slices ? ctx->tune.grid_slices : (nq_total >= 300000 ? 4 : 8);
  GridSweepBatch gb{};
  ReduceBatch rb{};
  StepBatch sb{};
  for (int k = 0; k < n; ++k) {
    gb.p[k] = first[k];
    rb.p[k] = slot_reduce_args(act[k]);
    sb.p[k].partial = act[k]->partial;
    sb.p[k].pcount = act[k]->pcount;
    sb.p[k].nblocks = rb.p[k].nblocks;
    sb.p[k].st = act[k]->st_dev;
  }
  // params.profile = 1: ONE of the group's max_iterations + 1 batched sweeps (rotating from group to group)
  // is bracketed by two HIP events on this stream; finish_group adds the time to the group's first pair
  int timed = -1;
  ctx->batch_timed[set] = false;
  if (p->profile == 1) {
    for (hipEvent_t* e : {&ctx->batch_t0[set], &ctx->batch_t1[set]})
      if (!*e) ICPK_HIP(ctx, hipEventCreate(e));
    timed = ctx->profile_phase++ % (p->max_iterations + 1);
    ctx->batch_timed[set] = true;
  }
  // the pairs still in the group's launches.  Throttled: a pair whose loop is done (its progress word says so) leaves
  // them -- from then on its sweep, reduce and step would return before writing anything but the step counter, so
  // results are the same; the launches of the group's slowest pairs stop paying for its finished ones' grids.
  std::vector<int> live(n);
  for (int k = 0; k < n; ++k) live[k] = k;
  GridSweepBatch gl{};
  ReduceBatch rl{};
  StepBatch sl{};
  // (lanes per query follow the pairs still launched: a lone slow pair is latency-bound again and wants 8; the
  // lane count decides the speed of a sweep, not its result)
  auto pack = [&]() {
    long long nq_live = 0;
    for (size_t j = 0; j < live.size(); ++j) {
      gl.p[j] = gb.p[live[j]];
      rl.p[j] = rb.p[live[j]];
      sl.p[j] = sb.p[live[j]];
      nq_live += act[live[j]]->src.n;
    }
    if (!ctx->tune.grid_slices) slices = nq_live >= 300000 ? 4 : 8;
  };
  auto sweep = [&](int nth, int expand) -> int {
    if (nth == timed) ICPK_HIP(ctx, hipEventRecord(ctx->batch_t0[set], ctx->stream));
    launch_nn_grid_batch(throttled ? gl : gb, throttled ? (int)live.size() : n, slices, expand, ctx->stream);
    if (nth == timed) ICPK_HIP(ctx, hipEventRecord(ctx->batch_t1[set], ctx->stream));
    return ICPK_OK;
  };
  if (throttled) pack();
  int src_ = sweep(0, 1);  // icp.cpp:98 (expanding search from element 0)
  if (src_) return src_;
  launch_assoc_reduce_batch(throttled ? rl : rb, throttled ? (int)live.size() : n, p->max_nn_dist, nact, ctx->stream);
  const int ahead = ctx->tune.loop_ahead;
  for (int i = 0; i < p->max_iterations; ++i) {
    if (throttled && i >= ahead) {
      bool all_exited = false;
      const int rc = wait_group_progress(ctx, act, i - ahead + 1, &all_exited);
      if (rc) return rc;
      if (all_exited) break;  // (every launch from here on would find every pair done)
      size_t w = 0;
      for (const int k : live) {
        const int w1 = ((const volatile int*)act[k]->progress)[1];
        if (!((w1 >> 2) == act[k]->loop_epoch && (w1 & 2))) live[w++] = k;
      }
      live.resize(w);
      if (live.empty()) break;  // (every pair finished between the wait and this look)
      pack();
    }
    if (throttled)
      launch_loop_step_batch(sl, (int)live.size(), nsum, 0, ctx->stream);
    else
      launch_loop_step_batch(sb, n, nsum, 0, ctx->stream);
    for (const int k : live) {  // pointer rotation only: nothing is enqueued for a chained sweep
      icpk_ctx* sl_k = act[k];
      NnArgs a = base_nn_args(sl_k);
      NnBoxes bx{};
      int recheck = 0;
      int rc = prepare_sorted_sweep(sl_k, ICPK_NN_GRID, a, bx, recheck);
      if (rc) {
        ctx->err = sl_k->err;
        return rc;
      }
      gb.p[k] = grid_sweep_args(sl_k, a, bx);
      after_grid_sweep(sl_k);
      rb.p[k].best = sl_k->best;
    }
    if (throttled) pack();
    src_ = sweep(i + 1, 0);  // icp.cpp:255, K3 fused
    if (src_) return src_;
    launch_assoc_reduce_batch(throttled ? rl : rb, throttled ? (int)live.size() : n, p->max_nn_dist, nact, ctx->stream);
  }
  launch_loop_step_batch(sb, n, nsum, 1, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  {  // the group's loop states: ONE copy (the slots' states are consecutive entries of the parent's pool)
    size_t lo = (size_t)-1, hi = 0;
    for (icpk_ctx* sl : act) {
      const size_t k = (size_t)(sl->st_dev - ctx->slot_states);
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
    }
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->slot_states_host + lo, ctx->slot_states + lo, (hi - lo + 1) * sizeof(LoopState),
                                 hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipEventRecord(ctx->group_ev[set], ctx->stream));
  return ICPK_OK;
}

}  // namespace icpk

namespace {

int align_batch_impl(icpk_ctx* ctx, int32_t n_pairs, const icpk_pair* pairs, const icpk_params* p, float* T_out,
                     icpk_stats* stats, hipMemcpyKind kind) {
  if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!pairs || !T_out)) || !p) return ICPK_E_ARG;
  if (p->max_iterations < 0 || p->solve < ICPK_SOLVE_REFERENCE || p->solve > ICPK_SOLVE_POINT_TO_PLANE)
    return fail(ctx, ICPK_E_ARG, "bad params");
  if (p->min_pairs < 1) return fail(ctx, ICPK_E_ARG, "min_pairs must be >= 1");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int worst = ICPK_OK;
  auto note = [&](int rc) {
    if (rc < 0 && worst >= 0) worst = rc;
    if (rc > 0 && worst >= 0 && rc > worst) worst = rc;
  };
  for (int32_t b = 0; b < n_pairs; ++b) {
    reset_outputs(T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
  }
  auto fetch_assoc = [&](icpk_ctx* c, const icpk_pair& pr) -> int {
    if (!pr.idx_out && !pr.dist_out) return ICPK_OK;
    return icpk_get_associations(c, pr.idx_out, pr.dist_out);
  };
  if (!batch_eligible(ctx, p)) {
    // other kernels / flavours / a log callback: the pairs one after the other on this context
    for (int32_t b = 0; b < n_pairs; ++b) {
      int rc = set_target_impl(ctx, pairs[b].tx, pairs[b].ty, pairs[b].tz, pairs[b].nt, kind);
      if (rc == ICPK_OK) rc = set_source_impl(ctx, pairs[b].sx, pairs[b].sy, pairs[b].sz, pairs[b].ns, kind);
      if (rc == ICPK_OK) {
        rc = icpk_align(ctx, p, T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
        if (rc >= 0) {
          const int r2 = fetch_assoc(ctx, pairs[b]);
          if (r2 < 0) rc = r2;
        }
      } else if (stats) {
        stats[b].status = rc;
      }
      note(rc);
    }
    return worst;
  }

  const int G = ctx->tune.batch_group < 1 ? 1 : (ctx->tune.batch_group > BATCH_MAX ? BATCH_MAX : ctx->tune.batch_group);
  const int ngroups = (n_pairs + G - 1) / G;
  int rc = ensure_slots(ctx, ngroups > 1 ? 2 * G : (n_pairs < G ? n_pairs : G));
  if (rc) return rc;

  auto finish_group = [&](const GroupRun& g) -> int {
    bool any = false;
    for (int k = 0; k < g.count; ++k) any |= g.rc[k] == ICPK_OK;
    if (any) ICPK_HIP(ctx, hipEventSynchronize(ctx->group_ev[g.set]));
    float timed_ms = -1.f;
    if (any && ctx->batch_timed[g.set] && hipEventElapsedTime(&timed_ms, ctx->batch_t0[g.set], ctx->batch_t1[g.set]) != hipSuccess)
      timed_ms = -1.f;
    for (int k = 0; k < g.count; ++k) {
      const int b = g.first + k;
      icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
      int r = g.rc[k];
      if (r == ICPK_OK) {
        r = device_loop_finish(sl, p, T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
        if (stats && timed_ms >= 0.f) {  // the group's one timed launch, booked on its first pair (it covers ALL the group's pairs)
          stats[b].nn_ms_total = timed_ms;
          stats[b].nn_timed_launches = 1;
          timed_ms = -1.f;
        }
        if (r >= 0) {
          const int r2 = fetch_assoc(sl, pairs[b]);
          if (r2 < 0) r = r2;
        }
      } else if (r >= 100) {  // ran on the single-pair path during set-up: outputs already written
        r -= 100;
      } else if (stats) {
        stats[b].status = r;
      }
      if (r < 0) ctx->err = sl->err;
      note(r);
    }
    return ICPK_OK;
  };

  // ICPK_BATCH_TRACE=1 (diagnostic): host time per group in set-up phase 1 / phase 2 / loop
  // enqueue / waiting for the previous group, on stderr
  const bool trace = std::getenv("ICPK_BATCH_TRACE") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
  };
  GroupRun prev;
  bool have_prev = false;
  std::vector<icpk_ctx*> unfinished;  // slots whose set-up stopped half-way (see the end of this function)
  // Every way out of the loop below, error or not, goes through the same tail: the previous group's results are
  // delivered, and nothing of this call is still in flight when it returns -- set-up kernels may be reading the
  // caller's device-resident clouds, uploads may be reading the caller's host buffers or a slot's staging area.
  auto drain = [&]() {
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t st : {ctx->setup_stream[0], ctx->setup_stream[1]})
      if (st) (void)hipStreamSynchronize(st);
    for (icpk_ctx* sl : ctx->slots) (void)hipStreamSynchronize(sl->stream);
  };
  auto bail = [&](int code) {
    if (have_prev) finish_group(prev);
    have_prev = false;
    drain();
    return code;
  };
#define ICPK_HIP_BAIL(call)                                                      \
  do {                                                                           \
    hipError_t e__ = (call);                                                     \
    if (e__ != hipSuccess) {                                                     \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);             \
      return bail(ICPK_E_HIP);                                                   \
    }                                                                            \
  } while (0)
  for (int gi = 0; gi < ngroups; ++gi) {
    const auto t0 = now();
        GroupRun g;
    g.first = gi * G;
    g.count = n_pairs - g.first < G ? n_pairs - g.first : G;
    g.set = ngroups > 1 ? (gi & 1) : 0;
    g.rc.assign(g.count, ICPK_OK);
    // set-up of the group's pairs: independent per slot (own buffers, own stream), so a few host
    // threads share the ~35 runtime calls per pair -- with 8 pairs per GPU (config 4 at 8 GPUs)
    // there is no previous group whose loop could hide this host time
    std::vector<GridSweepArgs> fargs(g.count);
    auto setup_one = [&](int k) {
      icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
      const int b = g.first + k;
      int r = slot_setup_phase1(sl, pairs[b], kind);
      if (r != ICPK_OK) {
        g.rc[k] = r;
        return;
      }
      if (sl->src.n <= 0) {  // no queries: the single-pair path handles it (icp.cpp:163-182 fallback)
        r = icpk_align(sl, p, T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
        g.rc[k] = r < 0 ? r : 100 + r;
        return;
      }
      r = slot_setup_phase2(sl, p, fargs[k], false);
      if (r != ICPK_OK) device_loop_disarm(sl);
      g.rc[k] = r;
    };
    // Device-resident pairs: the set-up launches of the whole group are RECORDED (icpk_internal.h, SetupRecorder)
    // and issued as one launch per step on the set's set-up stream -- 13 launches instead of 13 per pair.
    std::vector<bool> recorded(g.count, false);
    // (host buffers: only when several groups follow each other -- 64 pairs 20.4 -> 17.8 ms; for a single group
    // the uploads of the pairs would queue up on the one set-up stream in front of everything else: 8 pairs
    // 3.1 -> 3.3 ms, tools/probe_host_batch.py)
    const bool batched = ctx->tune.batch_setup != 0 && (kind == hipMemcpyDeviceToDevice || ngroups > 1 || ctx->tune.batch_setup >= 2);
    // (host buffers: one thread -- concurrent host-to-device copies from several threads stall for
    // ~9 ms at random on this runtime, tools/one_align.py --batch under ICPK_BATCH_TRACE)
    const int nthreads = batched || kind == hipMemcpyHostToDevice ? 1 : (g.count < ctx->tune.batch_threads ? g.count : ctx->tune.batch_threads);
    if (batched) {
      if (!ctx->setup_stream[g.set]) {
        ICPK_HIP_BAIL(hipStreamCreateWithFlags(&ctx->setup_stream[g.set], hipStreamNonBlocking));
        ICPK_HIP_BAIL(hipEventCreateWithFlags(&ctx->setup_ev[g.set], hipEventDisableTiming));
      }
      const hipStream_t ss = ctx->setup_stream[g.set];
      std::vector<SetupRecorder> recs(g.count);
      for (int k = 0; k < g.count; ++k) {
        icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
        if (pairs[g.first + k].ns <= 0) {  // goes down the single-pair path at once: nothing to defer
          setup_one(k);
          continue;
        }
        const hipStream_t own = sl->stream;
        sl->stream = ss;  // whatever is not recorded (first-use clears) must precede the flushed launches
        setup_recorder() = &recs[k];
        setup_one(k);
        setup_recorder() = nullptr;
        sl->stream = own;
        if (g.rc[k] == ICPK_OK && recs[k].overflow) {
          // more set-up steps than the recorder holds: the launches beyond its capacity were never issued --
          // the pair must not run on half a set-up
          device_loop_disarm(sl);
          g.rc[k] = fail(sl, ICPK_E_HIP, "frame-batch set-up recorder overflow (SETUP_MAX_CALLS)");
        }
        recorded[k] = g.rc[k] == ICPK_OK;
      }
      std::vector<SetupRecorder> ok;
      for (int k = 0; k < g.count; ++k)
        if (recorded[k]) ok.push_back(recs[k]);
      if (!ok.empty()) {
        if (ctx->tune.batch_setup == 3 /* test hook: the pair-by-pair replay */ || !flush_setup_batches(ok.data(), (int)ok.size(), ss))
          for (const SetupRecorder& r : ok) replay_setup(r, ss);
        ICPK_HIP_BAIL(hipGetLastError());
        ICPK_HIP_BAIL(hipEventRecord(ctx->setup_ev[g.set], ss));
      }
    } else if (nthreads <= 1) {
      for (int k = 0; k < g.count; ++k) setup_one(k);
    } else {
      std::vector<std::thread> pool;
      for (int t = 1; t < nthreads; ++t)
        pool.emplace_back([&, t] {
          for (int k = t; k < g.count; k += nthreads) setup_one(k);
        });
      for (int k = 0; k < g.count; k += nthreads) setup_one(k);
      for (std::thread& th : pool) th.join();
    }
    const auto t1 = now();
    std::vector<icpk_ctx*> act;
    std::vector<GridSweepArgs> first;
    std::vector<bool> own_event;
    for (int k = 0; k < g.count; ++k) {
      if (g.rc[k] != ICPK_OK) {
        if (g.rc[k] < 0) unfinished.push_back(ctx->slots[(size_t)g.set * G + k]);
        continue;
      }
      act.push_back(ctx->slots[(size_t)g.set * G + k]);
      first.push_back(fargs[k]);
      own_event.push_back(!recorded[k]);
    }
    const auto t2 = now();
    rc = enqueue_group_loop(ctx, p, act, first, g.set, own_event, false);
    if (rc) {  // enqueue failed: nothing of this group can be trusted (the previous group's results still are)
      for (icpk_ctx* sl : act) device_loop_disarm(sl);
      return bail(rc);
    }
    const auto t3 = now();
    if (have_prev) finish_group(prev);
    if (trace)
      std::fprintf(stderr, "icpk batch group %d: set-up %.0f us (%d host threads), loop enqueue %.0f us, wait+finish prev %.0f us\n",
                   gi, us(t0, t1), nthreads, us(t2, t3), us(t3, now()));
    prev = g;
    have_prev = true;
  }
  const auto te0 = now();
  if (have_prev) finish_group(prev);
  const auto te1 = now();
  // host input buffers were read asynchronously: everything has landed before we return.  A pair that went
  // through the loop has: its slot's stream reached `ready_ev` before the group's loop started, and the loop
  // has been waited for.  Only slots whose set-up FAILED may still have copies in flight.
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (icpk_ctx* sl : unfinished) ICPK_HIP(ctx, hipStreamSynchronize(sl->stream));
  if (!unfinished.empty())  // (with the batched set-up their uploads went to the set's set-up stream)
    for (hipStream_t st : {ctx->setup_stream[0], ctx->setup_stream[1]})
      if (st) ICPK_HIP(ctx, hipStreamSynchronize(st));
  if (trace) std::fprintf(stderr, "icpk batch tail: wait+finish last group %.0f us, stream syncs %.0f us\n", us(te0, te1), us(te1, now()));
#undef ICPK_HIP_BAIL
  return worst;
}

}  // namespace

extern "C" {

int icpk_align_batch(icpk_ctx* ctx, int32_t n_pairs, const icpk_pair* pairs, const icpk_params* p, float* T_out,
                     icpk_stats* stats) {
  if (ctx && p && p->nn_mode == ICPK_NN_MAP) return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP has no frame-batch mode");
  return align_batch_impl(ctx, n_pairs, pairs, p, T_out, stats, hipMemcpyHostToDevice);
}

int icpk_align_batch_device(icpk_ctx* ctx, int32_t n_pairs, const icpk_pair* pairs, const icpk_params* p,
                            float* T_out, icpk_stats* stats) {
  if (ctx && p && p->nn_mode == ICPK_NN_MAP) return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP has no frame-batch mode");
  return align_batch_impl(ctx, n_pairs, pairs, p, T_out, stats, hipMemcpyDeviceToDevice);
}

}  // extern "C"
