// icpk_api.cpp -- host side of libicpk.so: the context (one GPU + one HIP stream) and its tuning, the clouds it holds,
// and the small entry points of the C ABI of include/icpk.h.  The NN sweeps live in icpk_sweep.cpp, the alignment
// loops in icpk_align.cpp, the frame-batch mode in icpk_batch.cpp and the depth front end in icpk_frontend.cpp.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "icpk_ctx.h"
#include "solve_impl.h"

using namespace icpk;

namespace {

// pad value: +inf for targets (a padded target is never nearer than a real
// one), 0 for sources (padded queries are computed and discarded)
int upload_cloud(icpk_ctx* ctx, Cloud& c, const float* x, const float* y, const float* z, int n, float pad,
                 hipMemcpyKind kind, bool sync = true) {
  if (n < 0 || (n > 0 && (!x || !y || !z))) return fail(ctx, ICPK_E_ARG, "bad cloud pointers/size");
  int rc = ensure_cloud(ctx, c, n);
  if (rc) return rc;
  if (n > 0 && kind == hipMemcpyHostToDevice && !sync) {
    // frame-batch slots: pageable host memory crosses PCIe through a staging copy inside the
    // runtime, one plane after the other and synchronously; copying into the slot's own pinned
    // buffer here (the set-up threads do it in parallel) leaves ONE truly asynchronous DMA per cloud
    PinnedBuf<float>& stage = (&c == &ctx->tgt) ? ctx->stage_t : ctx->stage_s;
    if ((rc = stage.reserve(ctx, (size_t)3 * c.cap))) return rc;
    std::memcpy(stage, x, (size_t)n * sizeof(float));
    std::memcpy(stage + c.cap, y, (size_t)n * sizeof(float));
    std::memcpy(stage + 2 * (size_t)c.cap, z, (size_t)n * sizeof(float));
    // (the planes sit at the device cloud's own stride: one contiguous copy; the tails are padded below)
    ICPK_HIP(ctx, hipMemcpyAsync(c.base, stage, ((size_t)2 * c.cap + n) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  } else if (n > 0) {
    ICPK_HIP(ctx, hipMemcpyAsync(c.x(), x, (size_t)n * sizeof(float), kind, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(c.y(), y, (size_t)n * sizeof(float), kind, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(c.z(), z, (size_t)n * sizeof(float), kind, ctx->stream));
  }
  launch_fill_f32(c.x() + n, c.cap - n, pad, ctx->stream);
  launch_fill_f32(c.y() + n, c.cap - n, pad, ctx->stream);
  launch_fill_f32(c.z() + n, c.cap - n, pad, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  // host buffers are only valid for the duration of the call (the frame-batch entry points
  // keep theirs alive until they return and synchronise once at the end)
  if (sync) ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// the first n points of c into host planes (waits for them)
int download_planes(icpk_ctx* ctx, const Cloud& c, int n, float* x, float* y, float* z) {
  const size_t b = (size_t)n * sizeof(float);
  if (b) {
    ICPK_HIP(ctx, hipMemcpyAsync(x, c.x(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(y, c.y(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(z, c.z(), b, hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// the environment knobs (struct Tuning), each with its range check
Tuning tuning_from_env() {
  Tuning t;
  if (const char* e = std::getenv("ICPK_NN_TARGET_BLOCKS")) {
    const int v = std::atoi(e);
    if (v > 0) t.target_blocks = v;
  }
  if (const char* e = std::getenv("ICPK_NN_SLICES")) {
    const int v = std::atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) t.slices = v;
  }
  if (const char* e = std::getenv("ICPK_GRID_PPC")) {
    const float v = (float)std::atof(e);
    if (v > 0.f) t.grid_ppc = v;
  }
  if (const char* e = std::getenv("ICPK_GRID_XDIV")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= 64) t.grid_xdiv = v;
  }
  if (const char* e = std::getenv("ICPK_GRID_SLICES")) {
    const int v = std::atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8) t.grid_slices = v;
  }
  if (const char* e = std::getenv("ICPK_MERGED_SETUP")) t.merged_setup = std::atoi(e);  // 0: the two sorts of a fresh pair one after the other
  if (const char* e = std::getenv("ICPK_NN_Q")) {
    const int v = std::atoi(e);
    if (v == 1 || v == 2) t.q_per_lane = v;
  }
  if (const char* e = std::getenv("ICPK_BATCH_GROUP")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= BATCH_MAX) t.batch_group = v;
  }
  if (const char* e = std::getenv("ICPK_BATCH_THREADS")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= 16) t.batch_threads = v;
  }
  if (const char* e = std::getenv("ICPK_BATCH_SETUP")) t.batch_setup = std::atoi(e);  // 0: per-pair launches; 2: batched launches for single-group host-pointer batches too; 3: as 2, replayed pair by pair
  if (const char* e = std::getenv("ICPK_PRISTINE_SKIP")) t.pristine_skip = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_PIXEL_SEEDS")) t.pixel_seeds = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_LAZY_UNPACK")) t.lazy_unpack = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_IMAGE_ORDER")) t.image_order = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_ZERO_COPY_UPLOAD")) t.zero_copy_upload = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_RESULT_MIRROR")) t.result_mirror = std::atoi(e) != 0;
  if (const char* e = std::getenv("ICPK_LOOP_AHEAD")) {  // 0: enqueue every iteration up front
    const int v = std::atoi(e);
    if (v >= 0 && v <= LOOP_MAX_ITER) t.loop_ahead = v;
  }
  return t;
}

}  // namespace

namespace icpk {

// stream + the fixed-size buffers every context owns; `parent` != nullptr: a frame-batch slot
// (inherits the tuning knobs)
icpk_ctx* make_context(int device_id, const icpk_ctx* parent) {
  icpk_ctx* ctx = new icpk_ctx();
  ctx->device = device_id;
  bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && ctx->partial.reserve(ctx, (size_t)RED_MAX_BLOCKS * NSUM_MAX) == ICPK_OK;
  ok = ok && ctx->pcount.reserve(ctx, RED_MAX_BLOCKS) == ICPK_OK;
  ok = ok && ctx->red_out.reserve(ctx, NSUM_MAX + 1) == ICPK_OK;
  ok = ok && ctx->red_host.reserve(ctx, NSUM_MAX + 1) == ICPK_OK;
  ok = ok && ctx->bp_n_host.reserve(ctx, 2) == ICPK_OK;
  ok = ok && ctx->st_dev_mem.reserve(ctx, 1) == ICPK_OK;
  ok = ok && ctx->st_host_mem.reserve(ctx, 1) == ICPK_OK;
  ctx->st_dev = ctx->st_dev_mem;
  ctx->st_host = ctx->st_host_mem;
  ok = ok && ctx->progress.reserve(ctx, 64 / sizeof(int)) == ICPK_OK;
  ok = ok && hipHostGetDevicePointer((void**)&ctx->progress_dev, ctx->progress, 0) == hipSuccess;
  ok = ok && ctx->st_mirror.reserve(ctx, 1) == ICPK_OK;
  ok = ok && hipHostGetDevicePointer((void**)&ctx->st_mirror_dev, ctx->st_mirror, 0) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ctx->ready_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ctx->group_ev[0], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&ctx->group_ev[1], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    icpk_destroy(ctx);
    return nullptr;
  }
  if (parent) {
    ctx->tune = parent->tune;
    ctx->grid_max_cells = GRID_MAX_CELLS_SLOT;
  }
  ctx->log_last = std::chrono::steady_clock::now();
  return ctx;
}

int set_target_impl(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, hipMemcpyKind k,
                    bool sync) {
  if (!ctx) return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int rc = upload_cloud(ctx, ctx->tgt, x, y, z, n, __builtin_inff(), k, sync);
  if (rc) return rc;
  target_changed(ctx, false);
  return ICPK_OK;
}

int set_source_impl(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, hipMemcpyKind k,
                    bool sync) {
  if (!ctx) return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int rc = upload_cloud(ctx, ctx->src0, x, y, z, n, 0.f, k, sync);
  if (rc) return rc;
  ctx->have_src = true;
  ctx->have_assoc = false;
  ctx->have_seed = false;
  ctx->have_qperm = false;
  // (no second wait: the host buffers have been consumed by upload_cloud; the device-side copy of the
  // working source, made when something first reads it, is stream-ordered like any other)
  return copy_src0_to_src(ctx);
}

int copy_src0_to_src(icpk_ctx* ctx) {
  // src_pristine: the working copy is known to hold the committed source already (icpk_backproject_pair writes both
  // at once; nothing has touched either since) -- the frame path's icpk_align starts without this copy
  // (the working source is overwritten, or holds the committed one already: nothing of the last loop's is wanted)
  ctx->rec_pending = false;
  if (ctx->src_pristine && ctx->tune.pristine_skip && ctx->src.n == ctx->src0.n) return ICPK_OK;
  int rc = ensure_cloud(ctx, ctx->src, ctx->src0.n);
  if (rc) return rc;
  ctx->src_pristine = true;
  // The copy itself waits for a reader (ensure_unpacked): the next alignment's device loop of grid sweeps is none, so a
  // tracker that sets a source and aligns never pays it.  ICPK_PRISTINE_SKIP=0 copies here and now, as ever.
  ctx->src_deferred = ctx->tune.pristine_skip;
  return ctx->src_deferred ? ICPK_OK : copy_source_planes(ctx, false);
}

int copy_source_planes(icpk_ctx* ctx, bool tail_only) {
  const Cloud &a = ctx->src0, &b = ctx->src;
  const int m = round_up(a.n < 1 ? 1 : a.n, NN_TILE);
  if (tail_only) {  // the padding behind the n points an unpack is about to rewrite
    if (m == a.n) return ICPK_OK;
    const size_t bytes = (size_t)(m - a.n) * sizeof(float);
    ICPK_HIP(ctx, hipMemcpyAsync(b.x() + a.n, a.x() + a.n, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(b.y() + a.n, a.y() + a.n, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(b.z() + a.n, a.z() + a.n, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  } else if (a.cap == b.cap) {
    ICPK_HIP(ctx, hipMemcpyAsync(b.base, a.base, (size_t)3 * a.cap * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  } else {  // capacities can differ after a shrink: copy plane by plane, padded part included
    ICPK_HIP(ctx, hipMemcpyAsync(b.x(), a.x(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(b.y(), a.y(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(b.z(), a.z(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  }
  return ICPK_OK;
}

int check_ready(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_tgt || !ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source or target cloud not set");
  if (ctx->tgt.n <= 0) return fail(ctx, ICPK_E_EMPTY_TARGET, "target cloud is empty");
  return ICPK_OK;
}

int pad_target(icpk_ctx* ctx) {
  Cloud& c = ctx->tgt;
  const int padded = round_up(c.n < 1 ? 1 : c.n, NN_TILE);
  launch_fill_f32(c.x() + c.n, padded - c.n, __builtin_inff(), ctx->stream);
  launch_fill_f32(c.y() + c.n, padded - c.n, __builtin_inff(), ctx->stream);
  launch_fill_f32(c.z() + c.n, padded - c.n, __builtin_inff(), ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

void target_changed(icpk_ctx* ctx, bool keep_normals) {
  ctx->have_tgt = true;
  ctx->have_assoc = false;
  ctx->have_dec = false;
  ctx->have_boxes = false;
  ctx->have_grid = false;
  ctx->tgt_lookup = false;
  ctx->have_seed = false;
  if (!keep_normals) ctx->have_normals = false;
  ctx->have_nstats = false;  // (icpk_get_normal_stats speaks of the target it was estimated on)
  ctx->have_score_assoc = false;  // (as icpk_get_score_associations of the target it scored against)
  fpfh_dropped(ctx, 1);           // (and K16's descriptors of the target and its normals)
  // K17: a target that was only moved keeps its intensities and its (rotated) colour gradients; the integer sums
  // behind them were taken along the old axes
  ctx->have_cg_sums = false;
  if (!keep_normals) ctx->have_tgt_colors = ctx->have_color_gradients = false;
}

void reset_outputs(float T_out[16], icpk_stats* stats) {
  if (T_out)
    for (int k = 0; k < 16; ++k) T_out[k] = (k % 5 == 0) ? 1.f : 0.f;
  if (stats) std::memset(stats, 0, sizeof(*stats));
}

void clear_trace(icpk_ctx* ctx) {
  ctx->trace_R.clear();
  ctx->trace_t.clear();
  ctx->trace_mse.clear();
  ctx->trace_pairs.clear();
  ctx->robust_trace.clear();
}

}  // namespace icpk

extern "C" {

const char* icpk_version(void) { return ICPK_VERSION_STRING; }

void icpk_default_params(icpk_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = ICPK_DEFAULT_MAX_ITERATIONS;
  p->threshold = ICPK_DEFAULT_THRESHOLD;
  p->max_nn_dist = ICPK_MAX_NN_DISTANCE;
  p->min_pairs = ICPK_MIN_PAIRS;
  p->solve = ICPK_SOLVE_REFERENCE;
  p->nn_mode = ICPK_NN_GRID;  // same results as ICPK_NN_EXACT (tests), fastest
  p->last_rotation[0] = p->last_rotation[4] = p->last_rotation[8] = 1.f;
}

int icpk_create(icpk_ctx** out, int device_id) {
  if (!out) return ICPK_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ICPK_E_NO_DEVICE;
  if (device_id < 0 || device_id >= ndev) return ICPK_E_NO_DEVICE;
  if (hipSetDevice(device_id) != hipSuccess) return ICPK_E_NO_DEVICE;
  icpk_ctx* ctx = make_context(device_id, nullptr);
  if (!ctx) return ICPK_E_HIP;
  ctx->tune = tuning_from_env();
  *out = ctx;
  return ICPK_OK;
}

void icpk_destroy(icpk_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  icpk_comm_release(ctx);
  icpk_map_free(ctx);
  icpk_fast_free(ctx);
  icpk_tsdf_free(ctx);
  icpk_frame_view_free(ctx);
  icpk_esdf_free(ctx);
  icpk_brief_free(ctx);
  for (icpk_ctx* sl : ctx->slots) icpk_destroy(sl);  // (before the pools their loop states point into)
  ctx->slots.clear();
  for (hipStream_t st : {ctx->setup_stream[0], ctx->setup_stream[1]})
    if (st) (void)hipStreamDestroy(st);
  for (hipEvent_t e : {ctx->ready_ev, ctx->group_ev[0], ctx->group_ev[1], ctx->setup_ev[0], ctx->setup_ev[1], ctx->batch_t0[0],
                       ctx->batch_t0[1], ctx->batch_t1[0], ctx->batch_t1[1]})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
  for (const icpk_ctx::HostRange& r : ctx->registered) (void)hipHostUnregister(const_cast<char*>(r.host));
  ctx->registered.clear();
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;  // (its buffers free themselves)
}

const char* icpk_last_error(const icpk_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int icpk_set_log_callback(icpk_ctx* ctx, icpk_log_fn fn, void* user) {
  if (!ctx) return ICPK_E_ARG;
  ctx->log_fn = fn;
  ctx->log_user = user;
  ctx->log_last = std::chrono::steady_clock::now();
  return ICPK_OK;
}

void* icpk_stream(icpk_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int icpk_set_target(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n) {
  return set_target_impl(ctx, x, y, z, n, hipMemcpyHostToDevice);
}
int icpk_set_source(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n) {
  return set_source_impl(ctx, x, y, z, n, hipMemcpyHostToDevice);
}
int icpk_set_target_device(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n) {
  return set_target_impl(ctx, x, y, z, n, hipMemcpyDeviceToDevice);
}
int icpk_set_source_device(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n) {
  return set_source_impl(ctx, x, y, z, n, hipMemcpyDeviceToDevice);
}

int icpk_reset_source(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int rc = copy_src0_to_src(ctx);
  if (rc) return rc;
  ctx->have_assoc = false;
  ctx->have_seed = false;
  ctx->have_qperm = false;
  return ICPK_OK;  // (the device-side copy is left to whoever reads the working source first: no host wait)
}

int icpk_commit_source(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  const Cloud &a = ctx->src, &b = ctx->src0;  // src0.cap >= src.cap by construction
  const int m = round_up(a.n < 1 ? 1 : a.n, NN_TILE);
  ICPK_HIP(ctx, hipMemcpyAsync(b.x(), a.x(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(b.y(), a.y(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(b.z(), a.z(), (size_t)m * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
  ctx->src_pristine = a.n == b.n;  // (the two copies are equal again)
  ctx->have_src_normals = false;   // (the uploaded source is another cloud now)
  fpfh_dropped(ctx, 0);
  ctx->have_score_assoc = false;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_source(icpk_ctx* ctx, float* x, float* y, float* z) {
  if (!ctx || !x || !y || !z) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  return download_planes(ctx, ctx->src, ctx->src.n, x, y, z);
}

int icpk_get_target(icpk_ctx* ctx, float* x, float* y, float* z) {
  if (!ctx || !x || !y || !z) return ICPK_E_ARG;
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  return download_planes(ctx, ctx->tgt, ctx->tgt.n, x, y, z);
}

int32_t icpk_source_size(const icpk_ctx* ctx) { return ctx && ctx->have_src ? ctx->src0.n : 0; }
int32_t icpk_target_size(const icpk_ctx* ctx) { return ctx && ctx->have_tgt ? ctx->tgt.n : 0; }

int icpk_transform_source(icpk_ctx* ctx, const float R[9], const float t[3]) {
  if (!ctx || !R || !t) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  Rt rt;
  std::memcpy(rt.R, R, sizeof(rt.R));
  std::memcpy(rt.t, t, sizeof(rt.t));
  ctx->src_pristine = false;
  launch_transform(ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->src.n, rt, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_assoc = false;
  return ICPK_OK;  // (R and t travel by value in the kernel arguments: no host wait)
}

int icpk_transform_target(icpk_ctx* ctx, const float R[9], const float t[3]) {
  if (!ctx || !R || !t) return ICPK_E_ARG;
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  Rt rt;
  std::memcpy(rt.R, R, sizeof(rt.R));
  std::memcpy(rt.t, t, sizeof(rt.t));
  Cloud& c = ctx->tgt;
  launch_transform(c.x(), c.y(), c.z(), c.n, rt, ctx->stream);
  const int rc = pad_target(ctx);  // (the kernel works on whole float4s: restore the +inf padding it touched)
  if (rc) return rc;
  if (ctx->have_normals) {  // normals rotate with the cloud (no translation)
    Rt rn = rt;
    rn.t[0] = rn.t[1] = rn.t[2] = 0.f;
    launch_transform(ctx->nrm.x(), ctx->nrm.y(), ctx->nrm.z(), c.n, rn, ctx->stream);
  }
  if (ctx->have_color_gradients) {  // as do the colour gradients (K17)
    Rt rn = rt;
    rn.t[0] = rn.t[1] = rn.t[2] = 0.f;
    launch_transform(ctx->cgrad.x(), ctx->cgrad.y(), ctx->cgrad.z(), c.n, rn, ctx->stream);
  }
  ICPK_HIP(ctx, hipGetLastError());
  target_changed(ctx, true);
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_trace(icpk_ctx* ctx, int32_t* n_iter, float* R_out, float* t_out, int32_t* pairs_out, float* mse_out) {
  if (!ctx || !n_iter) return ICPK_E_ARG;
  const size_t n = ctx->trace_R.size() / 9;  // completed solves (a fallback iteration records none)
  *n_iter = (int32_t)n;
  if (R_out && n) std::memcpy(R_out, ctx->trace_R.data(), n * 9 * sizeof(float));
  if (t_out && n) std::memcpy(t_out, ctx->trace_t.data(), n * 3 * sizeof(float));
  if (pairs_out && n) std::memcpy(pairs_out, ctx->trace_pairs.data(), n * sizeof(int32_t));
  if (mse_out && n) std::memcpy(mse_out, ctx->trace_mse.data(), n * sizeof(float));
  return ICPK_OK;
}

int icpk_set_robust(icpk_ctx* ctx, const icpk_robust* r) {
  if (!ctx) return ICPK_E_ARG;
  if (!r) {
    ctx->robust_on = false;
    return ICPK_OK;
  }
  if (r->kernel < ICPK_ROBUST_NONE || r->kernel > ICPK_ROBUST_TUKEY)
    return fail(ctx, ICPK_E_ARG, "unknown robust kernel");
  if (r->scale_mode != ICPK_SCALE_FIXED && r->scale_mode != ICPK_SCALE_MEDIAN)
    return fail(ctx, ICPK_E_ARG, "unknown robust scale mode");
  if (!(r->scale > 0.f) || !std::isfinite(r->scale)) return fail(ctx, ICPK_E_ARG, "robust scale must be finite and > 0");
  if (!(r->trim_fraction > 0.f && r->trim_fraction <= 1.f)) return fail(ctx, ICPK_E_ARG, "trim_fraction must lie in (0, 1]");
  ctx->robust = *r;
  ctx->robust_on = true;
  return ICPK_OK;
}

int icpk_get_robust_trace(icpk_ctx* ctx, int32_t* n_iter, int32_t* kept_out, float* cut_out, double* c_out,
                          double* wsum_out) {
  if (!ctx || !n_iter) return ICPK_E_ARG;
  const size_t n = ctx->robust_trace.size();
  *n_iter = (int32_t)n;
  for (size_t i = 0; i < n; ++i) {
    const icpk::RobustTraceEntry& e = ctx->robust_trace[i];
    if (kept_out) kept_out[i] = e.kept;
    if (cut_out) cut_out[i] = e.cut;
    if (c_out) c_out[i] = e.c;
    if (wsum_out) wsum_out[i] = e.wsum;
  }
  return ICPK_OK;
}

int icpk_set_target_normals(icpk_ctx* ctx, const float* nx, const float* ny, const float* nz, int32_t n) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  if (n != ctx->tgt.n) return fail(ctx, ICPK_E_ARG, "normal count differs from the target size");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int rc = upload_cloud(ctx, ctx->nrm, nx, ny, nz, n, 0.f, hipMemcpyHostToDevice);
  if (rc) return rc;
  ctx->have_normals = true;
  ctx->have_nstats = false;
  fpfh_dropped(ctx, 1);
  return ICPK_OK;
}

int icpk_get_target_normals(icpk_ctx* ctx, float* nx, float* ny, float* nz) {
  if (!ctx || !nx || !ny || !nz) return ICPK_E_ARG;
  if (!ctx->have_normals) return fail(ctx, ICPK_E_NOT_SET, "no target normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  return download_planes(ctx, ctx->nrm, ctx->tgt.n, nx, ny, nz);
}

int icpk_solve_point_to_plane(const double sums[28], double R[9], double t[3]) {
  return solve_p2l(sums, R, t) ? ICPK_OK : ICPK_W_DEGENERATE;
}

/* test hook: icp.cpp:606-620 (point3 == 0) or :595-602 (point3 == 1) on n pairs; a and b are host xyz-SoA [3][n] */
static int pair_distance_impl(icpk_ctx* ctx, const float* a, const float* b, float* out, int32_t n, int point3) {
  if (!ctx || n < 0 || (n > 0 && (!a || !b || !out))) return ICPK_E_ARG;
  if (n == 0) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf<float> da, db, dout;  // (freed on every return)
  int rc = da.reserve(ctx, (size_t)3 * n);
  if (!rc) rc = db.reserve(ctx, (size_t)3 * n);
  if (!rc) rc = dout.reserve(ctx, n);
  if (rc) return rc;
  ICPK_HIP(ctx, hipMemcpyAsync(da, a, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(db, b, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  launch_pair_distance(da, db, dout, n, point3, ctx->stream);
  ICPK_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_pair_distance(icpk_ctx* ctx, const float* a, const float* b, float* out, int32_t n) {
  return pair_distance_impl(ctx, a, b, out, n, 0);
}
int icpk_pair_distance3(icpk_ctx* ctx, const float* a, const float* b, float* out, int32_t n) {
  return pair_distance_impl(ctx, a, b, out, n, 1);
}
float icpk_distance3(const float a[3], const float b[3]) {
  return a && b ? distance3(a[0], a[1], a[2], b[0], b[1], b[2]) : __builtin_nanf("");
}

void icpk_make_rotation_matrix(float x, float y, float z, float out[9]) { make_rotation_matrix(x, y, z, out); }
void icpk_matrix_to_quaternion(const float m[9], float q[4]) { matrix_to_quaternion(m, q); }
void icpk_quaternion_to_euler(const float q[4], float e[3]) { quaternion_to_euler(q, e); }
void icpk_solve_reference(const float M[9], float R[9]) { solve_reference(M, R); }
void icpk_solve_kabsch(int64_t n, const double sa[3], const double sb[3], const double sab[9], double R[9], double t[3]) {
  solve_kabsch(n, sa, sb, sab, R, t);
}

}  // extern "C"
