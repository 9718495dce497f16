// icpk_align.cpp -- the ICP loop (icp.cpp:98-268 in its frame-pair formulation): icpk_align with its device-side
// loop (kernels_loop.hip, the default) and its host loop, and the query-sharded loop icpk_align_query_sharded.
//
// The host loop sees exactly one small device->host copy per iteration (19 sums + count, 160 bytes, pinned) and
// sends the next 3x4 transform as kernel arguments.
#include <chrono>
#include <cstring>
#include <utility>
#include <vector>

#include "icpk_ctx.h"
#include "solve_impl.h"

using namespace icpk;

namespace {

hipEvent_t get_event(icpk_ctx* ctx, size_t k) {
  while (ctx->events.size() <= k) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ctx->events.push_back(e);
  }
  return ctx->events[k];
}

void log_delta(icpk_ctx* ctx, int key, int quantity) {
  if (!ctx->log_fn) return;
  const auto now = std::chrono::steady_clock::now();
  const double us = std::chrono::duration<double, std::micro>(now - ctx->log_last).count();
  ctx->log_last = now;
  ctx->log_fn(key, quantity, us, ctx->log_user);
}

float mse_from(const double* sums, int64_t n) {
  // icp.cpp:622-638: (mean distance)^2, evaluated from the double sum
  if (n <= 0) return 0.f;
  const float m = (float)(sums[12] / (double)n);
  return (float)((double)m * (double)m);
}

// params.profile: HIP events on the context's stream, summed into icpk_stats at the end.  Two tightly around every
// sampled K1 launch (1: every profile_stride-th sweep, successive alignments bracketing different sweeps for an
// unbiased sample; 2: every sweep), and with 2 a pair around every other stage too (stamp).
struct Profiler {
  icpk_ctx* ctx;
  const icpk_params* p;
  bool on, all;
  int phase;
  int nsweep = 0;
  size_t nev = 0;
  std::vector<size_t> nn, red, tr;  // indices of (start, stop) pairs

  Profiler(icpk_ctx* c, const icpk_params* prm)
      : ctx(c), p(prm), on(prm->profile != 0), all(prm->profile >= 2), phase(c->profile_phase++) {}

  // one event (list: it starts a span that the next one ends)
  int stamp(std::vector<size_t>* list) {
    if (!on) return ICPK_OK;
    hipEvent_t e = get_event(ctx, nev);
    if (!e) return fail(ctx, ICPK_E_HIP, "hipEventCreate failed");
    ICPK_HIP(ctx, hipEventRecord(e, ctx->stream));
    if (list) list->push_back(nev);
    ++nev;
    return ICPK_OK;
  }

  // enqueue_nn, bracketed if this sweep is sampled
  int sweep(int nn_mode) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int nth = nsweep++;
    if (on && (all || p->profile_stride <= 1 || (nth + phase) % p->profile_stride == 0)) {
      e0 = get_event(ctx, nev);
      e1 = get_event(ctx, nev + 1);
      if (!e0 || !e1) return fail(ctx, ICPK_E_HIP, "hipEventCreate failed");
      nn.push_back(nev);
      nev += 2;
    }
    return enqueue_nn(ctx, nn_mode, e0, e1);
  }

  // after the stream has drained
  void book(icpk_stats* stats) const {
    stats->nn_timed_launches = (int32_t)nn.size();
    if (!on || nev < 2) return;
    auto span = [&](size_t a, size_t b) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ctx->events[a], ctx->events[b]);
      return ms;
    };
    for (size_t e : nn) stats->nn_ms_total += span(e, e + 1);
    for (size_t e : red) stats->reduce_ms_total += span(e, e + 1);
    for (size_t e : tr) stats->transform_ms_total += span(e, e + 1);
    stats->total_ms = span(0, nev - 1);
  }
};

// every way out of an alignment that has armed the device loop disarms it
struct LoopGuard {
  icpk_ctx* c;
  ~LoopGuard() { device_loop_disarm(c); }
};

// T_out of an alignment: the reference flavour's rotation product and its LAST offset (icp.cpp:266-268), the
// accumulated [R|t] otherwise
void pack_pose(float T_out[16], int solve, const float Trot[9], const float offset[3], const double Tk[12]) {
  if (solve == ICPK_SOLVE_REFERENCE) {
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_out[4 * r + c] = Trot[3 * r + c];
      T_out[4 * r + 3] = offset[r];
    }
  } else {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T_out[4 * r + c] = (float)Tk[4 * r + c];
  }
  T_out[12] = T_out[13] = T_out[14] = 0.f;
  T_out[15] = 1.f;
}

// every alignment starts from the source as set / committed, with no seeds or query order of an earlier pose.
// rec_loop: a device loop of grid sweeps follows -- it neither reads nor writes the working planes (the set-up takes the
// queries from the committed source, the sweeps keep records, the unpack rewrites every point), so a copy that
// copy_src0_to_src has deferred stays deferred; every other loop gets its planes here
int begin_alignment(icpk_ctx* ctx, bool rec_loop) {
  int rc = copy_src0_to_src(ctx);
  if (!rc && !(rec_loop && ctx->src.n > 0)) rc = ensure_unpacked(ctx);
  if (rc) return rc;
  ctx->src_pristine = false;  // (the loop moves the working copy)
  ctx->have_seed = false;     // matches of an earlier alignment belong to a different source pose
  ctx->have_qperm = false;
  clear_trace(ctx);
  return ICPK_OK;
}

}  // namespace

namespace icpk {

// ---- device-side loop: begin / finish, shared by the single-pair and the frame-batch path ----
// sums the loop step of this flavour consumes: the reference flavour reads [0..12] only
int loop_nsum(const icpk_params* p) {
  if (p->solve == ICPK_SOLVE_POINT_TO_PLANE || p->solve == ICPK_SOLVE_PLANE_TO_PLANE) return NP2L;  // (solve_p2l's layout)
  return p->solve == ICPK_SOLVE_REFERENCE ? NSUM_REF : NSUM;
}

// initial LoopState -> device (on ctx->stream), stop flags armed
// defer: the launch is left to the first set-up launch that can carry it (build_grid_and_order, enqueue_cell_order)
// or, failing that, to flush_loop_init right before the first kernel that reads the state
int device_loop_begin(icpk_ctx* ctx, const icpk_params* p, bool throttled, bool mirror, bool defer) {
  LoopInitArgs a{};
  a.st = ctx->st_dev;
  if (throttled || mirror) {
    ctx->loop_epoch = (ctx->loop_epoch % 1000000) + 1;  // (<< 10 must fit an int)
    a.epoch = ctx->loop_epoch;
    a.progress = ctx->progress_dev;
    a.mirror = mirror ? ctx->st_mirror_dev : nullptr;
  }
  a.throttled = throttled;  // (only then does a step store its progress words: nothing reads them otherwise)
  a.max_iterations = p->max_iterations;
  a.min_pairs = p->min_pairs;
  a.solve = p->solve;
  a.fixed_iterations = p->fixed_iterations;
  a.threshold = p->threshold;
  std::memcpy(a.last_rotation, p->last_rotation, sizeof(a.last_rotation));
  std::memcpy(a.last_translation, p->last_translation, sizeof(a.last_translation));
  if (defer) {
    ctx->pending_init = a;
    ctx->init_pending = true;
  } else {
    launch_loop_init(a, ctx->stream);  // (values travel in the kernel arguments: no staging copy)
    ICPK_HIP(ctx, hipGetLastError());
  }
  const int nsum = loop_nsum(p);
  ctx->loop_nact = nsum == NSUM_REF ? NSUM_REF : NSUM;
  // the stop flags are only meaningful while this alignment is being enqueued
  ctx->stop = &ctx->st_dev->done;
  ctx->st_active = ctx->st_dev;
  ctx->grid_chain = false;
  ctx->best_of_sweep.clear();
  return ICPK_OK;
}

void device_loop_disarm(icpk_ctx* ctx) {
  ctx->init_pending = false;
  ctx->stop = nullptr;
  ctx->st_active = nullptr;
  ctx->grid_chain = false;
}

// after the LoopState has landed in ctx->st_host: outputs of the alignment
int device_loop_finish(icpk_ctx* ctx, const icpk_params* p, float T_out[16], icpk_stats* stats, const LoopState* h) {
  device_loop_disarm(ctx);
  if (!h) h = ctx->st_host;
  // the associations of the last EXECUTED sweep are the result
  const int k = h->sweeps;
  if (k >= 1 && k <= (int)ctx->best_of_sweep.size()) {
    // (every sweep wrote one of the two buffers that trade places as best / seed)
    if (ctx->best_of_sweep[k - 1] != ctx->best) std::swap(ctx->seed, ctx->best);
  }
  ctx->have_seed_m = false;  // the Morton-ordered copy may belong to a skipped sweep: re-gather on demand
  const int it = h->iterations;
  pack_pose(T_out, p->solve, h->Trot, h->offset, h->Tk);
  ctx->trace_R.assign(h->trace_R, h->trace_R + 9 * it);
  ctx->trace_t.assign(h->trace_t, h->trace_t + 3 * it);
  ctx->trace_mse.assign(h->trace_mse, h->trace_mse + it);
  ctx->trace_pairs.assign(h->trace_pairs, h->trace_pairs + it);
  if (stats) {
    stats->iterations = it;
    stats->status = h->status;
    stats->final_pairs = (int32_t)h->pairs;
    stats->final_mse = h->mse;
    stats->nn_launches = k;
  }
  return h->status;
}

}  // namespace icpk

namespace {

// host side of LoopState::progress: returns once `steps` loop steps have run on the device or the loop has
// exited (the wait is a fraction of one iteration).  steps < 0: returns once the loop's outputs have landed in
// ctx->st_mirror (progress word 2).
int wait_loop_progress(icpk_ctx* ctx, int steps, bool* exited) {
  volatile int* pr = ctx->progress;
  const int e = ctx->loop_epoch;
  auto look = [&]() -> int {  // 1: the loop has exited, 2: `steps` steps have run, 0: neither yet
    if (steps < 0) return __atomic_load_n(&pr[2], __ATOMIC_ACQUIRE) == ((e << 1) | 1) ? 1 : 0;
    const int w0 = __atomic_load_n(&pr[0], __ATOMIC_ACQUIRE), w1 = pr[1];
    if ((w1 >> 2) == e && (w1 & 1)) return 1;
    return ((w0 >> 10) == e && (w0 & 1023) >= steps) ? 2 : 0;
  };
  int got = 0;
  const int rc = spin_until(ctx, [&] { return (got = look()) != 0; }, "device loop made no progress");
  *exited = got == 1;
  return rc;
}

// Whole alignment enqueued up front (or, when the loop may leave early, a few iterations ahead of the
// device); loop test, solve and pose accumulation run on the device (kernels_loop.hip).  Same results
// as the host loop below.
int align_device_loop(icpk_ctx* ctx, const icpk_params* p, float T_out[16], icpk_stats* stats) {
  const bool prof = p->profile != 0;
  const bool prof_all = p->profile >= 2;  // 1: NN kernels only (2 events per sweep); 2: every stage
  const bool p2l = p->solve == ICPK_SOLVE_POINT_TO_PLANE;
  const bool gicp = p->solve == ICPK_SOLVE_PLANE_TO_PLANE;  // (never robust: icpk_align refuses the combination)
  const bool colored = colored_step(ctx, p);                // (nor this: the joint step in place of K5, K17)
  const bool fused = p->nn_mode == ICPK_NN_PRUNED || p->nn_mode == ICPK_NN_GRID;  // K3 runs inside the sweep
  const bool robust = ctx->robust_on;
  const int nsum = robust ? (p2l ? NP2L_W : NSUM_W) : loop_nsum(p);
  const int B = red_blocks(ctx->src.n);
  const LoopGuard guard{ctx};
  // a loop that may leave early is enqueued loop_ahead iterations ahead of the device, not all at once
  const int ahead = ctx->tune.loop_ahead;
  const bool throttled = !p->fixed_iterations && !prof && ahead > 0 && p->max_iterations > ahead;
  // the outputs come back through the host-visible mirror the last step writes (LoopState::mirror): no copy kernel,
  // and in a throttled loop no stream wait either -- the call returns when the deciding step has run
  const bool mirror = ctx->tune.result_mirror && !prof;
  int rc = device_loop_begin(ctx, p, throttled, mirror, /*defer=*/p->nn_mode == ICPK_NN_GRID && !prof);
  if (rc) return rc;

  Profiler pf(ctx, p);
  // throttled loop: LoopState::progress word 1 of this loop, bit 1 (exited: done, or stopping after the fallback
  // motion) or 2 (done).  A glance at pinned memory before a launch: whatever would be enqueued after the exit is a
  // no-op that still costs its dispatch (4-5 us each).
  auto progress_bit = [&](int bit) -> bool {
    if (!throttled) return false;
    const int w1 = ((const volatile int*)ctx->progress)[1];
    return (w1 >> 2) == ctx->loop_epoch && (w1 & bit);
  };
  auto sweep = [&]() -> int {
    int r = pf.sweep(p->nn_mode);
    if (r) return r;
    if (!loop_rec(ctx)) ctx->best_of_sweep.push_back(ctx->best);  // (grid sweeps keep ONE set of records: a sweep that runs at all supersedes the previous one)
    if (progress_bit(1)) return ICPK_OK;  // (the loop has exited meanwhile: K2 would be a no-op launch)
    if (prof_all && (r = pf.stamp(&pf.red))) return r;
    if (gicp)  // (R_acc is read from the loop state)
      r = enqueue_reduce_gicp(ctx, p->max_nn_dist, nullptr);
    else if (colored)
      r = enqueue_reduce_colored(ctx, p->max_nn_dist);
    else
      r = robust ? enqueue_reduce_robust(ctx, p->max_nn_dist, p2l)
                 : (p2l ? enqueue_reduce_p2l(ctx, p->max_nn_dist) : enqueue_reduce(ctx, p->max_nn_dist));
    if (r) return r;
    return prof_all ? pf.stamp(nullptr) : ICPK_OK;
  };
  rc = sweep();  // icp.cpp:98
  if (rc) return rc;
  if ((rc = flush_loop_init(ctx))) return rc;  // (normally carried by the set-up or flushed before the sweep already)
  for (int i = 0; i < p->max_iterations; ++i) {
    if (throttled && i >= ahead) {
      bool exited = false;
      rc = wait_loop_progress(ctx, i - ahead + 1, &exited);
      if (rc) return rc;
      if (exited) break;  // everything from here on would find `done` set and do nothing
    }
    launch_loop_step(ctx->partial, ctx->pcount, B, nsum, ctx->st_dev, 0, ctx->stream, ctx->rsel, ctx->robust_trace_dev);
    // (done only: a step that fell back to the caller's last motion stops AFTER the next transform, which the fused
    // sweep applies -- the working source must receive it)
    if (progress_bit(2)) break;
    if (!fused) {  // the pruned sweep applies the transform itself (K3 fused into K1c)
      if (prof_all && (rc = pf.stamp(&pf.tr))) return rc;
      launch_transform_state(ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->src.n, ctx->st_dev, ctx->stream);
      if (prof_all && (rc = pf.stamp(nullptr))) return rc;
    }
    rc = sweep();  // icp.cpp:255
    if (rc) return rc;
  }
  // a step that set `done` has published the outputs already: the statistics-only step would be a no-op launch
  const bool done_seen = mirror && progress_bit(2);
  if (!done_seen)
    launch_loop_step(ctx->partial, ctx->pcount, B, nsum, ctx->st_dev, 1, ctx->stream, ctx->rsel, ctx->robust_trace_dev);
  if (loop_rec(ctx)) {  // the caller-order planes and keys the grid sweeps did not keep current: once, and only if asked for
    ctx->rec_pending = true;
    if (!ctx->tune.lazy_unpack && (rc = ensure_unpacked(ctx))) return rc;
  }
  ICPK_HIP(ctx, hipGetLastError());
  const LoopState* result = nullptr;
  if (mirror) {
    // a loop enqueued whole is waited for the same way when it is short (well under a millisecond of device time: the
    // host would otherwise sleep through the unpack and its own wake-up); long ones leave the core alone
    const bool brief = (long long)ctx->src.n * p->max_iterations <= 8000000ll;
    if (throttled || brief) {  // (what is still enqueued -- a no-op sweep, the unpack -- is stream-ordered before whatever comes next)
      bool ready = false;
      rc = wait_loop_progress(ctx, -1, &ready);
      if (rc) return rc;
    } else {
      ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (__atomic_load_n(&ctx->progress[2], __ATOMIC_ACQUIRE) != ((ctx->loop_epoch << 1) | 1))
        return fail(ctx, ICPK_E_HIP, "device loop ended without publishing its result");
    }
    result = ctx->st_mirror;
  } else {
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->st_host, ctx->st_dev, sizeof(LoopState), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }

  rc = device_loop_finish(ctx, p, T_out, stats, result);
  if (robust)  // (written by the loop steps into mapped memory before the result was published)
    ctx->robust_trace.assign(ctx->robust_trace_pin.get(), ctx->robust_trace_pin.get() + ctx->trace_pairs.size());
  if (stats) pf.book(stats);
  return rc;
}

}  // namespace

extern "C" {

// Query-sharded alignment of ONE pair over the ranks of the context's communicator ("single huge
// pair"; the frame-pair formulation icp.cpp:541-563 with the queries split): the target is the same on every rank
// (icpk_comm_broadcast_target), the source is this rank's slice of the queries.  The whole loop is enqueued: per
// iteration the grid sweep (K3 fused) and K2 on the slice, the canonical second tree stage, ONE in-stream float64
// all-reduce of the 19 sums + the pair count (160 bytes), and the loop step on the reduced sums -- replicated, so
// every rank applies the same transform, takes the same exit and returns the same T.  No host round trip and no
// host copy per iteration (the host-driven loop of round 2 paid a stream sync + two staging copies each).
// Results agree with icpk_align on the whole pair to ~1e-6 on T (the sums of the ranks are added by the collective:
// another order than the single-GPU canonical tree); with one rank they are bit-identical.
int icpk_align_query_sharded(icpk_ctx* ctx, const icpk_params* p, float T_out[16], icpk_stats* stats) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  if (!p || !T_out) return ICPK_E_ARG;
  if (p->nn_mode == ICPK_NN_MAP) return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP is single-context only");
  if (p->solve == ICPK_SOLVE_PLANE_TO_PLANE) return fail(ctx, ICPK_E_ARG, "the query-sharded loop has no plane-to-plane flavour");
  if (colored_step(ctx, p)) return fail(ctx, ICPK_E_ARG, "the query-sharded loop has no colored flavour (icpk_set_colored is on)");
  if (!ctx->comm) return fail(ctx, ICPK_E_NOT_SET, "icpk_comm_init_rccl has not been called");
  if (p->solve != ICPK_SOLVE_REFERENCE && p->solve != ICPK_SOLVE_KABSCH)
    return fail(ctx, ICPK_E_ARG, "the query-sharded loop supports the reference and Kabsch flavours");
  if (p->max_iterations < 0 || p->max_iterations > LOOP_MAX_ITER) return fail(ctx, ICPK_E_ARG, "max_iterations out of range");
  if (p->min_pairs < 1) return fail(ctx, ICPK_E_ARG, "min_pairs must be >= 1");
  if (ctx->robust_on) return fail(ctx, ICPK_E_ARG, "robust alignment is not available in the query-sharded loop");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  reset_outputs(T_out, stats);
  icpk_params q = *p;
  q.nn_mode = ICPK_NN_GRID;
  rc = begin_alignment(ctx, false);  // (this loop unpacks into the planes itself)
  if (rc) return rc;
  const LoopGuard guard{ctx};
  rc = device_loop_begin(ctx, &q, false);
  if (rc) return rc;
  ctx->loop_nact = NSUM;  // both flavours through the full 19 sums: one message shape
  const int B = red_blocks(ctx->src.n);
  auto sweep = [&]() -> int {
    // (an empty slice still takes part: its sums are zero)
    int r = enqueue_nn(ctx, ICPK_NN_GRID);
    if (r) return r;
    r = enqueue_reduce(ctx, q.max_nn_dist);
    if (r) return r;
    launch_reduce_final_shard(ctx->partial, ctx->pcount, B, ctx->red_out, ctx->st_dev, ctx->stream);
    return icpk_comm_allreduce_device(ctx, ctx->red_out, NSUM + 1);
  };
  rc = sweep();
  for (int i = 0; rc == ICPK_OK && i < q.max_iterations; ++i) {
    launch_loop_step(ctx->red_out, nullptr, -1, NSUM, ctx->st_dev, 0, ctx->stream);
    rc = sweep();
  }
  if (rc) {
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  launch_loop_step(ctx->red_out, nullptr, -1, NSUM, ctx->st_dev, 1, ctx->stream);
  if (loop_rec(ctx))
    launch_grid_unpack(ctx->qm4, ctx->rec, ctx->src.n, ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->best, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->st_host, ctx->st_dev, sizeof(LoopState), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return device_loop_finish(ctx, &q, T_out, stats);
}

int icpk_align(icpk_ctx* ctx, const icpk_params* p, float T_out[16], icpk_stats* stats) {
  reset_outputs(T_out, stats);  // (what a failure returns)
  if (!ctx || !p || !T_out) return ICPK_E_ARG;
  if (p->max_iterations < 0 || p->solve < ICPK_SOLVE_REFERENCE || p->solve > ICPK_SOLVE_PLANE_TO_PLANE)
    return fail(ctx, ICPK_E_ARG, "bad params");
  // min_pairs < 1 would let a sweep with no pairs reach the solve, which divides by the zero count (a NaN transform)
  if (p->min_pairs < 1) return fail(ctx, ICPK_E_ARG, "min_pairs must be >= 1");
  if (p->solve == ICPK_SOLVE_POINT_TO_PLANE && ctx && !ctx->have_normals)
    return fail(ctx, ICPK_E_NOT_SET, "point-to-plane needs target normals");
  const bool gicp = p->solve == ICPK_SOLVE_PLANE_TO_PLANE;
  if (p->nn_mode == ICPK_NN_MAP && (p->solve == ICPK_SOLVE_POINT_TO_PLANE || gicp || !(p->max_nn_dist <= ICPK_MAX_NN_DISTANCE)))
    return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP: reference or Kabsch flavour and max_nn_dist <= 0.75");
  if (gicp && ctx->robust_on) return fail(ctx, ICPK_E_ARG, "plane-to-plane has no robust form (icpk_set_robust is on)");
  if (gicp && (!ctx->have_normals || !ctx->have_src_normals))
    return fail(ctx, ICPK_E_NOT_SET, "plane-to-plane needs source and target normals");
  const bool colored = colored_step(ctx, p);  // (ICPK_NN_MAP has been refused with point-to-plane above)
  if (colored && ctx->robust_on) return fail(ctx, ICPK_E_ARG, "colored ICP has no robust form (icpk_set_robust is on)");
  if (colored && (!ctx->have_src_colors || !ctx->have_tgt_colors || !ctx->have_color_gradients))
    return fail(ctx, ICPK_E_NOT_SET, "colored ICP needs source colours, target colours and target colour gradients");
  // the bug-for-bug solve has no weighted form
  if (ctx->robust_on && p->solve == ICPK_SOLVE_REFERENCE)
    return fail(ctx, ICPK_E_ARG, "robust alignment needs the Kabsch or point-to-plane flavour");
  int rc = check_ready(ctx);
  if (rc) {
    if (stats) stats->status = rc;
    return rc;
  }
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool device_loop = !p->host_loop && !ctx->log_fn && p->max_iterations <= LOOP_MAX_ITER;  // (and a source that is not empty)
  rc = begin_alignment(ctx, device_loop && p->nn_mode == ICPK_NN_GRID);
  if (rc) return rc;
  const bool robust = ctx->robust_on;
  if (robust && ctx->src.n > 0 && (rc = ensure_robust(ctx, ctx->src.n))) return rc;
  if (device_loop && ctx->src.n > 0) return align_device_loop(ctx, p, T_out, stats);

  Profiler pf(ctx, p);
  const bool p2l = p->solve == ICPK_SOLVE_POINT_TO_PLANE;
  const int nsum = robust ? (p2l ? NP2L_W : NSUM_W) : (p2l || gicp ? NP2L : NSUM);
  double Tk[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  double sums[NSUM_MAX];
  int64_t npairs = 0, kept = 0;  // kept: pairs with a weight > 0 (robust; else the accepted ones)
  double wsum = 0.0;             // W = sum w (robust; else the pair count)
  RobustSel sel{};
  float mse = 0.f;
  auto sweep = [&]() -> int {
    int r = pf.sweep(p->nn_mode);
    if (r) return r;
    r = pf.stamp(&pf.red);  // start of reduce
    if (r) return r;
    if (ctx->src.n > 0) {
      if (gicp) {  // R_acc: the floats T_out would hold now, as the device loop's kernel reads them from its state
        float Racc[9];
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) Racc[3 * a + b] = (float)Tk[4 * a + b];
        r = enqueue_reduce_gicp(ctx, p->max_nn_dist, Racc);
      } else if (colored) {
        r = enqueue_reduce_colored(ctx, p->max_nn_dist);
      } else {
        r = robust ? enqueue_reduce_robust(ctx, p->max_nn_dist, p2l)
                   : (p2l ? enqueue_reduce_p2l(ctx, p->max_nn_dist) : enqueue_reduce(ctx, p->max_nn_dist));
      }
      if (r) return r;
    }
    r = pf.stamp(nullptr);  // end of reduce
    if (r) return r;
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->src.n > 0) {
      std::memcpy(sums, ctx->red_host, nsum * sizeof(double));
      std::memcpy(&npairs, ctx->red_host + nsum, sizeof(int64_t));
      if (robust) sel = *ctx->rsel_host;
    } else {
      std::memset(sums, 0, sizeof(sums));
      npairs = 0;
    }
    kept = robust ? (int64_t)sums[nsum - 1] : npairs;
    wsum = robust ? sums[nsum - 2] : (double)npairs;
    if (p2l || gicp) {  // distance sum sits in the last slot
      const float m = npairs > 0 ? (float)(sums[27] / (double)npairs) : 0.f;
      mse = (float)((double)m * (double)m);
    } else {
      mse = mse_from(sums, npairs);
    }
    log_delta(ctx, ICPK_LOG_NEAREST_NEIGHBOR, (int)npairs);  // icp.cpp:561
    log_delta(ctx, ICPK_LOG_MSE, (int)npairs);               // icp.cpp:635
    return ICPK_OK;
  };
  auto apply = [&](const float R[9], const float t[3]) -> int {
    Rt rt;
    std::memcpy(rt.R, R, sizeof(rt.R));
    std::memcpy(rt.t, t, sizeof(rt.t));
    int r = pf.stamp(&pf.tr);
    if (r) return r;
    launch_transform(ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->src.n, rt, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    return pf.stamp(nullptr);
  };

  ctx->log_last = std::chrono::steady_clock::now();
  rc = sweep();  // icp.cpp:98
  if (rc) return rc;

  float Trot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  float offset[3] = {0, 0, 0};
  // the motion of a Kabsch / point-to-plane solve: applied and recorded in float, accumulated into Tk in double
  auto take = [&](const double Rd[9], const double td[3]) -> int {
    float Rf[9], tf[3];
    for (int k = 0; k < 9; ++k) Rf[k] = (float)Rd[k];
    for (int k = 0; k < 3; ++k) tf[k] = (float)td[k];
    if (const int e = apply(Rf, tf)) return e;
    ctx->trace_R.insert(ctx->trace_R.end(), Rf, Rf + 9);
    ctx->trace_t.insert(ctx->trace_t.end(), tf, tf + 3);
    double Tn[12];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (double)Rf[3 * r + k] * Tk[4 * k + c];
        Tn[4 * r + c] = s + (c == 3 ? (double)tf[r] : 0.0);
      }
    std::memcpy(Tk, Tn, sizeof(Tk));
    return ICPK_OK;
  };
  int status = ICPK_OK;
  int i = 0;
  while ((p->fixed_iterations || mse > p->threshold) && i < p->max_iterations) {  // icp.cpp:155
    if (kept < p->min_pairs) {  // icp.cpp:163-182: reuse the caller's last motion
      rc = apply(p->last_rotation, p->last_translation);
      if (rc) return rc;
      for (int k = 0; k < 3; ++k) offset[k] = -p->last_translation[k];
      status = ICPK_W_TOO_FEW_PAIRS;
      break;
    }
    ctx->trace_pairs.push_back((int32_t)npairs);
    ctx->trace_mse.push_back(mse);
    if (robust) ctx->robust_trace.push_back(RobustTraceEntry{(int)kept, sel.cut, sel.c, wsum});
    double Rd[9], td[3];
    if (p->solve == ICPK_SOLVE_REFERENCE) {
      float M[9], R[9], Rinv[9], neg[3];
      for (int k = 0; k < 9; ++k) M[k] = (float)sums[k];  // icp.cpp:212 (CV_32F result)
      log_delta(ctx, ICPK_LOG_RECONSTRUCT_POINT_CLOUDS, 0);  // icp.cpp:210
      solve_reference(M, R);                                 // icp.cpp:215-223
      log_delta(ctx, ICPK_LOG_SVD, 0);                       // icp.cpp:225
      if (i == 0)
        std::memcpy(Trot, R, sizeof(Trot));  // icp.cpp:227-229
      else
        mul3f(R, Trot, Trot);  // icp.cpp:231-232
      invert3f(R, Rinv);       // icp.cpp:235
      for (int k = 0; k < 3; ++k) {
        offset[k] = (float)(sums[9 + k] / (double)npairs);  // icp.cpp:240 (pre-rotation pairs)
        neg[k] = -offset[k];
      }
      rc = apply(Rinv, neg);  // icp.cpp:236,245
      if (rc) return rc;
      ctx->trace_R.insert(ctx->trace_R.end(), R, R + 9);
      ctx->trace_t.insert(ctx->trace_t.end(), offset, offset + 3);
    } else if (p2l || gicp) {
      if (!solve_p2l(sums, Rd, td)) {
        // not a completed iteration: it leaves no entry in the trace or the robust trace (as the device loop's step)
        ctx->trace_pairs.pop_back();
        ctx->trace_mse.pop_back();
        if (robust) ctx->robust_trace.pop_back();
        status = ICPK_W_DEGENERATE;
        break;
      }
      log_delta(ctx, ICPK_LOG_SVD, 0);
      if ((rc = take(Rd, td))) return rc;
    } else {
      double sa[3], sb[3], sab[9];
      for (int k = 0; k < 3; ++k) {
        sa[k] = sums[13 + k];
        sb[k] = sums[16 + k];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sab[3 * r + c] = sums[3 * c + r];  // sum a_r b_c = M^T
      log_delta(ctx, ICPK_LOG_RECONSTRUCT_POINT_CLOUDS, 0);
      solve_kabsch(wsum, sa, sb, sab, Rd, td);
      log_delta(ctx, ICPK_LOG_SVD, 0);
      if ((rc = take(Rd, td))) return rc;
    }
    log_delta(ctx, ICPK_LOG_ROTATE, 0);  // icp.cpp:250
    rc = sweep();                        // icp.cpp:255
    if (rc) return rc;
    ++i;  // icp.cpp:257
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));

  pack_pose(T_out, p->solve, Trot, offset, Tk);
  if (stats) {
    stats->iterations = i;
    stats->status = status;
    stats->final_pairs = (int32_t)npairs;
    stats->final_mse = mse;
    stats->nn_launches = pf.nsweep;
    pf.book(stats);
  }
  return status;
}

}  // extern "C"
