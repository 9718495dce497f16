// icpk_frames_batch.cpp -- icpk_align_frames_batch: icpk_backproject_pair + icpk_align for many independent depth
// streams, their pairs advancing in the lock-step groups of the frame-batch mode (icpk_batch.cpp).
//
// Per group of up to BATCH_MAX jobs, on the slot set's set-up stream: the new images cross PCIe from one pinned
// staging buffer (the counting pass reads them there when the filter is off, as icpk_backproject_pair does), ONE
// filter launch for every image that needs it, ONE count / scan / scatter launch each for all 2 x n images -- the
// scatter writes straight into the slots' clouds and pixel maps -- then ONE host wait for all 2 x n point counts (the
// reduce geometry needs them), the recorded batched set-up of the slots (icpk_internal.h, SetupRecorder) and the
// group's loop (enqueue_group_loop).  Same kernels' bodies as the single path: same bits.
#include <algorithm>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

constexpr int FB_WORDS = 2 * BATCH_MAX;  // published point counts per slot set: two images per job

// icpk_backproject_pair's anchor rule (cv::dilate / cv::erode default (-1, -1): the element's centre)
int check_anchor(icpk_ctx* ctx, int morph, int& ax, int& ay) {
  if (ax < 0) ax = 2;
  if (ay < 0) ay = 2;
  if (morph != 0 && (ax > 4 || ay > 4)) return fail(ctx, ICPK_E_ARG, "anchor outside the 5x5 element");
  return ICPK_OK;
}

// the subsample key of the next image of this stream: a stream draws its patterns as a context of its own would
unsigned long long next_stream_key(const icpk_ctx* ctx, FrameStream& fs) {
  const unsigned long long k = fs.sub_images++;
  return ctx->sub_seed + (k + 1ull) * 0x9E3779B97F4A7C15ull;
}

struct FrameGroup {
  int first = 0, count = 0, set = 0;
  std::vector<int> rc;  // per job: ICPK_OK (in the loop), 100 + status (ran the single-pair path), or the failure
};

int align_frames_impl(icpk_ctx* ctx, int32_t n_jobs, const icpk_frame_job* jobs, int32_t rows, int32_t cols, float fx,
                      float cx, const float offset[3], int32_t filter, int32_t max_d, int32_t min_d, int32_t morph,
                      int32_t anchor_x, int32_t anchor_y, const icpk_params* p, float* T_out, icpk_stats* stats) {
  if (!ctx || !p || n_jobs < 0 || (n_jobs > 0 && (!jobs || !T_out)) || rows <= 0 || cols <= 0 ||
      (int64_t)rows * cols > (1 << 27))
    return fail(ctx, ICPK_E_ARG, "bad arguments");
  if (p->max_iterations < 0 || p->solve < ICPK_SOLVE_REFERENCE || p->solve > ICPK_SOLVE_POINT_TO_PLANE)
    return fail(ctx, ICPK_E_ARG, "bad params");
  if (p->min_pairs < 1) return fail(ctx, ICPK_E_ARG, "min_pairs must be >= 1");
  if (ctx->robust_on) return fail(ctx, ICPK_E_ARG, "robust alignment is not available in lock-step frame batches");
  if (!batch_eligible(ctx, p))
    return fail(ctx, ICPK_E_ARG,
                "icpk_align_frames_batch: ICPK_NN_GRID, device-side loop, reference or Kabsch flavour, no log callback");
  int ax = anchor_x, ay = anchor_y;
  if (filter && check_anchor(ctx, morph, ax, ay)) return ICPK_E_ARG;
  {
    std::vector<bool> seen(ICPK_MAX_FRAME_STREAMS, false);
    for (int32_t b = 0; b < n_jobs; ++b) {
      const int s = jobs[b].stream;
      if (s < 0 || s >= ICPK_MAX_FRAME_STREAMS) return fail(ctx, ICPK_E_ARG, "stream id out of range");
      if (seen[s]) return fail(ctx, ICPK_E_ARG, "a stream appears twice in one call");
      if (!jobs[b].depth_source) return fail(ctx, ICPK_E_ARG, "null depth_source");
      seen[s] = true;
    }
  }
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  for (int32_t b = 0; b < n_jobs; ++b) reset_outputs(T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
  ctx->frames_trace.assign((size_t)n_jobs, FrameTrace{});
  if (n_jobs == 0) return ICPK_OK;
  if (ctx->frame_streams.empty()) ctx->frame_streams.resize(ICPK_MAX_FRAME_STREAMS);

  const int G = ctx->tune.batch_group < 1 ? 1 : (ctx->tune.batch_group > BATCH_MAX ? BATCH_MAX : ctx->tune.batch_group);
  const int ngroups = (n_jobs + G - 1) / G;
  int rc = ensure_slots(ctx, ngroups > 1 ? 2 * G : (n_jobs < G ? n_jobs : G));
  if (rc) return rc;
  const int npix = rows * cols;
  const int nblocks = (npix + 1023) / 1024;
  const int per_image = nblocks + 2;
  const size_t bytes = (size_t)npix * sizeof(uint16_t);
  rc = ctx->fb_stage.reserve(ctx, (size_t)2 * G * npix);
  for (int s = 0; s < 2 && !rc; ++s) rc = ctx->fb_counts[s].reserve(ctx, (size_t)2 * G * per_image);
  if (!rc) rc = ctx->fb_n_dev.reserve(ctx, 2 * FB_WORDS);
  if (!rc && !ctx->fb_n_mapped) {
    rc = ctx->fb_n.reserve(ctx, 2 * FB_WORDS);
    const hipError_t e = rc ? hipSuccess : hipHostGetDevicePointer((void**)&ctx->fb_n_mapped, ctx->fb_n, 0);
    if (e != hipSuccess) {  // (no half-made state: the next call starts again from the allocation)
      ctx->fb_n_mapped = nullptr;
      (void)ctx->fb_n.release();
      rc = hip_failure(ctx, "hipHostGetDevicePointer(fb_n)", e);
    }
  }
  if (rc) return rc;
  for (int s = 0; s < 2; ++s)
    if (!ctx->setup_stream[s]) {
      ICPK_HIP(ctx, hipStreamCreateWithFlags(&ctx->setup_stream[s], hipStreamNonBlocking));
      ICPK_HIP(ctx, hipEventCreateWithFlags(&ctx->setup_ev[s], hipEventDisableTiming));
    }
  const int fset[6] = {filter != 0, max_d, min_d, morph != 0, ax, ay};
  // without the filter the images are not copied at all: the counting pass reads them from the staging buffer
  const bool zero_copy = !filter && ctx->tune.zero_copy_upload;
  const uint16_t* stage_dev = nullptr;
  if (zero_copy) ICPK_HIP(ctx, hipHostGetDevicePointer((void**)&stage_dev, ctx->fb_stage, 0));
  const float ox = offset ? offset[0] : 0.f, oy = offset ? offset[1] : 0.f, oz = offset ? offset[2] : 0.f;
  // job k's icpk_params: the caller's with the stream's last motion (icp.cpp:163-182)
  std::vector<icpk_params> pj((size_t)n_jobs, *p);
  for (int32_t b = 0; b < n_jobs; ++b) {
    std::memcpy(pj[b].last_rotation, jobs[b].last_rotation, sizeof(pj[b].last_rotation));
    std::memcpy(pj[b].last_translation, jobs[b].last_translation, sizeof(pj[b].last_translation));
  }

  int worst = ICPK_OK;
  auto note = [&](int r) {
    if (r < 0 && worst >= 0) worst = r;
    if (r > 0 && worst >= 0 && r > worst) worst = r;
  };
  auto keep_trace = [&](int b, const icpk_ctx* sl) {
    FrameTrace& tr = ctx->frames_trace[(size_t)b];
    tr.R = sl->trace_R;
    tr.t = sl->trace_t;
    tr.mse = sl->trace_mse;
    tr.pairs = sl->trace_pairs;
  };
  // the group's results; a failed wait for its loop fails every job that was in it (their outputs stay reset)
  auto finish_group = [&](const FrameGroup& g) -> int {
    bool any = false;
    for (int k = 0; k < g.count; ++k) any |= g.rc[k] == ICPK_OK;
    const hipError_t we = any ? hipEventSynchronize(ctx->group_ev[g.set]) : hipSuccess;
    if (we != hipSuccess) {
      const int code = hip_failure(ctx, "hipEventSynchronize(frame-batch group)", we);
      for (int k = 0; k < g.count; ++k)
        if (g.rc[k] == ICPK_OK) {
          device_loop_disarm(ctx->slots[(size_t)g.set * G + k]);
          if (stats) stats[g.first + k].status = code;
          note(code);
        }
      return code;
    }
    for (int k = 0; k < g.count; ++k) {
      const int b = g.first + k;
      icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
      int r = g.rc[k];
      if (r == ICPK_OK) {
        r = device_loop_finish(sl, p, T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
        keep_trace(b, sl);
      } else if (r >= 100) {  // ran on the single-pair path during set-up: outputs already written
        r -= 100;
        keep_trace(b, sl);
      } else if (stats) {
        stats[b].status = r;
      }
      if (r < 0 && worst >= 0) ctx->err = sl->err.empty() ? ctx->err : sl->err;
      note(r);
    }
    return ICPK_OK;
  };
  auto drain = [&]() {
    (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t st : {ctx->setup_stream[0], ctx->setup_stream[1]})
      if (st) (void)hipStreamSynchronize(st);
    for (icpk_ctx* sl : ctx->slots) (void)hipStreamSynchronize(sl->stream);
  };
  FrameGroup prev;
  bool have_prev = false;
  auto bail = [&](int code) {
    if (have_prev) (void)finish_group(prev);  // (the first error is the one reported)
    drain();
    return code;
  };

  for (int gi = 0; gi < ngroups; ++gi) {
    FrameGroup g;
    g.first = gi * G;
    g.count = n_jobs - g.first < G ? n_jobs - g.first : G;
    g.set = ngroups > 1 ? (gi & 1) : 0;
    g.rc.assign(g.count, ICPK_OK);
    const hipStream_t ss = ctx->setup_stream[g.set];
    // Threshold mode, last group of the call: the loop is enqueued a few iterations ahead of its slowest pair and ends
    // when every pair has exited (enqueue_group_loop), instead of running the no-op tail to max_iterations -- a batched
    // sweep of exited pairs still dispatches its whole grid.  The host then waits inside the loop's enqueue, which an
    // earlier group must not do: the next group's set-up overlaps its loop.
    const bool throttled = gi == ngroups - 1 && !p->fixed_iterations && p->profile == 0 &&
                           ctx->tune.loop_ahead > 0 && p->max_iterations > ctx->tune.loop_ahead;
    // ---- back-projection of the group's pairs: one launch per pass -------------------------------------------------
    BpFrameBatch bb{};
    DfBatch df{};
    int m = 0, ndf = 0, staged = 0;
    std::vector<int> bp_job;           // batch entry -> job of the group
    std::vector<int> new_slot(g.count, -1);  // image slot the job's source frame went to
    std::vector<std::pair<uint16_t*, const uint16_t*>> copies, uploads;  // host -> staging, staging -> device
    for (int k = 0; k < g.count; ++k) {
      const icpk_frame_job& job = jobs[g.first + k];
      FrameStream& fs = ctx->frame_streams[(size_t)job.stream];
      icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
      const bool resident = job.depth_target == nullptr;
      const bool fits = (size_t)2 * npix <= fs.raw.capacity();
      if (resident && (fs.slot < 0 || fs.rows != rows || fs.cols != cols || !fits)) {
        g.rc[k] = fail(sl, ICPK_E_NOT_SET, "no resident previous frame of this size for this stream (pass depth_target)");
        continue;
      }
      bool grown = false;
      int r = reserve_group(sl, &grown, need(fs.raw, (size_t)2 * npix), need(fs.flt, (size_t)2 * npix));
      if (grown) fs.slot = -1;
      for (Cloud* c : {&sl->src0, &sl->src, &sl->tgt})
        if (!r) r = ensure_cloud(sl, *c, npix);  // worst case: every pixel valid
      if (!r) r = reserve_group(sl, nullptr, need(sl->pix_tidx, (size_t)npix), need(sl->pix_src, (size_t)npix));
      if (r) {
        g.rc[k] = r;
        continue;
      }
      const int tslot = resident ? fs.slot : 1;
      const int sslot = 1 - tslot;
      uint16_t* const raw_s = fs.raw + (size_t)sslot * npix;
      uint16_t* const raw_t = fs.raw + (size_t)tslot * npix;
      uint16_t* const flt_s = fs.flt + (size_t)sslot * npix;
      uint16_t* const flt_t = fs.flt + (size_t)tslot * npix;
      const bool refilter = !resident || std::memcmp(fset, fs.filter, sizeof(fset)) != 0;
      fs.slot = -1;  // (nothing is resident until the group's counts are back)
      BpFramePair& f = bb.p[m];
      const int si = staged++;
      copies.push_back({ctx->fb_stage + (size_t)si * npix, job.depth_source});
      int ti = -1;
      if (!resident) {
        ti = staged++;
        copies.push_back({ctx->fb_stage + (size_t)ti * npix, job.depth_target});
      }
      f.depth[0] = raw_s;
      f.depth[1] = raw_t;
      if (zero_copy) {
        f.host_src[0] = stage_dev + (size_t)si * npix;
        f.raw_out[0] = raw_s;
        if (!resident) {
          f.host_src[1] = stage_dev + (size_t)ti * npix;
          f.raw_out[1] = raw_t;
        }
      } else {
        uploads.push_back({raw_s, ctx->fb_stage + (size_t)si * npix});
        if (!resident) uploads.push_back({raw_t, ctx->fb_stage + (size_t)ti * npix});
      }
      if (filter) {  // SLAM.cpp:229,553-574; the resident frame's filtered copy is reused when its settings match
        df.in[ndf] = raw_s;
        df.out[ndf++] = flt_s;
        if (refilter) {
          df.in[ndf] = raw_t;
          df.out[ndf++] = flt_t;
        }
        f.depth[0] = flt_s;
        f.depth[1] = flt_t;
      }
      f.src0 = sl->src0.base;
      f.src = sl->src.base;
      f.tgt = sl->tgt.base;
      f.src0_cap = sl->src0.cap;
      f.src_cap = sl->src.cap;
      f.tgt_cap = sl->tgt.cap;
      f.counts = ctx->fb_counts[g.set] + (size_t)m * 2 * per_image;
      f.pix_src = sl->pix_src;
      f.pix_tidx = sl->pix_tidx;
      // (icp.cpp:38-39 builds the cloud of `data` first, then that of `previous`: the source draws its pattern first)
      f.sub_key[0] = next_stream_key(ctx, fs);
      f.sub_key[1] = next_stream_key(ctx, fs);
      f.sub_factor = ctx->sub_factor;
      std::memcpy(f.rt.R, job.R, sizeof(f.rt.R));
      std::memcpy(f.rt.t, job.t, sizeof(f.rt.t));
      new_slot[k] = sslot;
      bp_job.push_back(k);
      ++m;
    }
    // the images into the staging buffer: 0.6 MB each at Kinect size, so a few host threads share them
    const int nthreads = (int)std::min<size_t>(copies.size(), copies.size() * bytes >= ((size_t)4 << 20) ? 4 : 1);
    if (nthreads > 1) {
      std::vector<std::thread> pool;
      for (int t = 1; t < nthreads; ++t)
        pool.emplace_back([&, t] {
          for (size_t c = t; c < copies.size(); c += nthreads) std::memcpy(copies[c].first, copies[c].second, bytes);
        });
      for (size_t c = 0; c < copies.size(); c += nthreads) std::memcpy(copies[c].first, copies[c].second, bytes);
      for (std::thread& th : pool) th.join();
    } else {
      for (const auto& c : copies) std::memcpy(c.first, c.second, bytes);
    }
    for (const auto& u : uploads) {
      const hipError_t e = hipMemcpyAsync(u.first, u.second, bytes, hipMemcpyHostToDevice, ss);
      if (e != hipSuccess) return bail(hip_failure(ctx, "hipMemcpyAsync(frame upload)", e));
    }
    volatile int* const nw = ctx->fb_n + (size_t)g.set * FB_WORDS;
    if (m > 0) {
      if (ndf > 0) launch_depth_filter_batch(df, ndf, rows, cols, min_d, max_d, ax, ay, morph != 0, ss);
      for (int i = 0; i < 2 * m; ++i) nw[i] = -1;
      __atomic_thread_fence(__ATOMIC_SEQ_CST);
      int* const n_dev = ctx->fb_n_dev + (size_t)g.set * FB_WORDS;
      launch_backproject_frames(bb, m, rows, cols, fx, cx, ox, oy, oz, n_dev,
                                ctx->tune.result_mirror ? ctx->fb_n_mapped + (size_t)g.set * FB_WORDS : nullptr, ss);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return bail(hip_failure(ctx, "launch_backproject_frames", e));
      // the one host wait of the group: every image's point count
      if (ctx->tune.result_mirror) {
        rc = spin_until(ctx, [&] {
          for (int i = 0; i < 2 * m; ++i)
            if (nw[i] < 0) return false;
          return true;
        }, "frame-batch back-projection ended without its counts", ss);
        if (rc) return bail(rc);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
      } else {
        hipError_t e2 = hipMemcpyAsync(ctx->fb_n + (size_t)g.set * FB_WORDS, n_dev, 2 * m * sizeof(int),
                                       hipMemcpyDeviceToHost, ss);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(ss);
        if (e2 != hipSuccess) return bail(hip_failure(ctx, "frame-batch counts", e2));
      }
    }
    // ---- the slots take the clouds; set-up recorded and flushed as one launch per step --------------------------
    std::vector<SetupRecorder> recs(g.count);
    std::vector<GridSweepArgs> fargs(g.count);
    std::vector<bool> recorded(g.count, false);
    for (int i = 0; i < m; ++i) {
      const int k = bp_job[i], b = g.first + k;
      icpk_ctx* sl = ctx->slots[(size_t)g.set * G + k];
      FrameStream& fs = ctx->frame_streams[(size_t)jobs[b].stream];
      fs.slot = new_slot[k];
      fs.rows = rows;
      fs.cols = cols;
      std::memcpy(fs.filter, fset, sizeof(fset));
      sl->src0.n = sl->src.n = nw[2 * i];
      sl->tgt.n = nw[2 * i + 1];
      sl->src_pristine = true;   // (the scatter wrote the committed and the working copy of the source at once)
      sl->have_pix_seed = true;  // (... and which pixel every point came from)
      sl->pix_rows = rows;
      sl->pix_cols = cols;
      sl->have_src = true;
      sl->have_qperm = false;
      target_changed(sl, false);
      int r = check_ready(sl);
      if (r) {
        g.rc[k] = r;
        continue;
      }
      const hipStream_t own = sl->stream;
      sl->stream = ss;  // (behind the scatter; whatever is not recorded -- first-use clears -- precedes the flush)
      if (sl->src.n <= 0) {  // no queries: the single-pair path (icp.cpp:163-182 fallback), as icpk_align_batch
        r = icpk_align(sl, &pj[b], T_out + 16 * (size_t)b, stats ? stats + b : nullptr);
        sl->stream = own;
        g.rc[k] = r < 0 ? r : 100 + r;
        continue;
      }
      sl->have_seed = false;
      sl->rec_pending = false;
      r = ensure_assoc(sl, sl->src.n);
      if (!r) {
        setup_recorder() = &recs[k];
        r = slot_setup_phase2(sl, &pj[b], fargs[k], throttled);
        setup_recorder() = nullptr;
      }
      sl->stream = own;
      if (!r && recs[k].overflow) r = fail(sl, ICPK_E_HIP, "frame-batch set-up recorder overflow (SETUP_MAX_CALLS)");
      if (r) device_loop_disarm(sl);
      g.rc[k] = r;
      recorded[k] = r == ICPK_OK;
    }
    std::vector<SetupRecorder> ok;
    std::vector<icpk_ctx*> act;
    std::vector<GridSweepArgs> first;
    for (int k = 0; k < g.count; ++k)
      if (recorded[k]) {
        ok.push_back(recs[k]);
        act.push_back(ctx->slots[(size_t)g.set * G + k]);
        first.push_back(fargs[k]);
      }
    if (!ok.empty()) {
      if (ctx->tune.batch_setup == 3 /* test hook: the pair-by-pair replay */ || !flush_setup_batches(ok.data(), (int)ok.size(), ss))
        for (const SetupRecorder& r : ok) replay_setup(r, ss);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipEventRecord(ctx->setup_ev[g.set], ss);
      if (e != hipSuccess) {
        for (icpk_ctx* sl : act) device_loop_disarm(sl);
        return bail(hip_failure(ctx, "frame-batch set-up", e));
      }
    }
    rc = enqueue_group_loop(ctx, p, act, first, g.set, std::vector<bool>(act.size(), false), throttled);
    if (rc) {
      for (icpk_ctx* sl : act) device_loop_disarm(sl);
      return bail(rc);
    }
    if (have_prev && (rc = finish_group(prev))) {
      have_prev = false;
      return bail(rc);
    }
    prev = g;
    have_prev = true;
  }
  if (have_prev && (rc = finish_group(prev))) {
    drain();
    return rc;
  }
  // the staging buffer and the caller's images have been consumed (the counts came from them); nothing of this call
  // is left in flight when it returns
  drain();
  return worst;
}

}  // namespace

extern "C" {

int icpk_align_frames_batch(icpk_ctx* ctx, int32_t n_jobs, const icpk_frame_job* jobs, int32_t rows, int32_t cols,
                            float fx, float cx, const float offset[3], int32_t filter, int32_t max_d, int32_t min_d,
                            int32_t morph, int32_t anchor_x, int32_t anchor_y, const icpk_params* p, float* T_out,
                            icpk_stats* stats) {
  return align_frames_impl(ctx, n_jobs, jobs, rows, cols, fx, cx, offset, filter, max_d, min_d, morph, anchor_x,
                           anchor_y, p, T_out, stats);
}

int icpk_get_frames_trace(icpk_ctx* ctx, int32_t job, int32_t* n_iter, float* R_out, float* t_out, int32_t* pairs_out,
                          float* mse_out) {
  if (!ctx || !n_iter) return ICPK_E_ARG;
  if (job < 0 || (size_t)job >= ctx->frames_trace.size()) return fail(ctx, ICPK_E_ARG, "no such job in the last call");
  const FrameTrace& tr = ctx->frames_trace[(size_t)job];
  const size_t n = tr.R.size() / 9;  // completed solves (a fallback iteration records none)
  *n_iter = (int32_t)n;
  if (R_out && n) std::memcpy(R_out, tr.R.data(), n * 9 * sizeof(float));
  if (t_out && n) std::memcpy(t_out, tr.t.data(), n * 3 * sizeof(float));
  if (pairs_out && n) std::memcpy(pairs_out, tr.pairs.data(), n * sizeof(int32_t));
  if (mse_out && n) std::memcpy(mse_out, tr.mse.data(), n * sizeof(float));
  return ICPK_OK;
}

int icpk_release_frame_streams(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  for (hipStream_t st : {ctx->setup_stream[0], ctx->setup_stream[1], ctx->stream})  // (nothing may still read an image)
    if (st) ICPK_HIP(ctx, hipStreamSynchronize(st));
  ctx->frame_streams.clear();  // (each stream's buffers free themselves)
  return ICPK_OK;
}

}  // extern "C"
