// icpk_frontend.cpp -- the depth front end (SLAM.cpp, pointcloud.cpp): depth filter, bilateral filter (K22; its host-only
// half is icpk_bilateral.cpp), back-projection of one image or
// of a frame pair (with the frame kept resident for the next call), subsampling, registered host buffers, and the
// key-point entry points icpk_associate_keypoints and icpk_backproject_keypoints.
#include <cmath>
#include <cstring>

#include "icpk_ctx.h"

using namespace icpk;

extern "C" {

struct DepthFilter {  // SLAM.cpp:553-574 filterDepthImage
  int max_d, min_d, morph, ax, ay;
};
static int check_filter(icpk_ctx* ctx, int morph, int& ax, int& ay) {
  if (ax < 0) ax = 2;  // cv::dilate / cv::erode default anchor (-1,-1): the element's centre
  if (ay < 0) ay = 2;
  if (morph != 0 && (ax > 4 || ay > 4)) return fail(ctx, ICPK_E_ARG, "anchor outside the 5x5 element");
  return ICPK_OK;
}

// raw + filtered depth images on the device (`count` pixels each) and `ints` block-count words
// the subsample key of the next image this context back-projects (kernels_backproject.hip: bp_keep)
static unsigned long long next_subsample_key(icpk_ctx* ctx) {
  const unsigned long long k = ctx->sub_stream++;
  return ctx->sub_seed + (k + 1ull) * 0x9E3779B97F4A7C15ull;
}

// caller memory that icpk_register_host_buffer pinned: the device address of [p, p + bytes) or nullptr
static const void* registered_device_pointer(const icpk_ctx* ctx, const void* p, size_t bytes) {
  const char* c = static_cast<const char*>(p);
  for (const icpk_ctx::HostRange& r : ctx->registered)
    if (c >= r.host && c + bytes <= r.host + r.bytes) return r.dev + (c - r.host);
  return nullptr;
}

int icpk_register_host_buffer(icpk_ctx* ctx, const void* ptr, size_t bytes) {
  if (!ctx || !ptr || bytes == 0) return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (registered_device_pointer(ctx, ptr, bytes)) return ICPK_OK;
  ICPK_HIP(ctx, hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterMapped));
  void* dev = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&dev, const_cast<void*>(ptr), 0);
  if (e != hipSuccess) {
    (void)hipHostUnregister(const_cast<void*>(ptr));
    return fail(ctx, ICPK_E_HIP, hipGetErrorString(e));
  }
  ctx->registered.push_back({static_cast<const char*>(ptr), bytes, static_cast<const char*>(dev)});
  return ICPK_OK;
}

int icpk_unregister_host_buffer(icpk_ctx* ctx, const void* ptr) {
  if (!ctx || !ptr) return ICPK_E_ARG;
  for (size_t k = 0; k < ctx->registered.size(); ++k)
    if (ctx->registered[k].host == static_cast<const char*>(ptr)) {
      ICPK_HIP(ctx, hipSetDevice(ctx->device));
      ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (nothing in flight may still read it)
      ICPK_HIP(ctx, hipHostUnregister(const_cast<void*>(ptr)));
      ctx->registered.erase(ctx->registered.begin() + k);
      return ICPK_OK;
    }
  return fail(ctx, ICPK_E_ARG, "not a registered buffer");
}

int icpk_set_subsample(icpk_ctx* ctx, int32_t factor, uint64_t seed) {
  if (!ctx || factor < 0) return ICPK_E_ARG;
  ctx->sub_factor = factor;
  ctx->sub_seed = seed;
  ctx->sub_stream = 0;
  for (icpk::FrameStream& fs : ctx->frame_streams) fs.sub_images = 0;  // (icpk_align_frames_batch: per stream)
  return ICPK_OK;
}

static int ensure_depth_buffers(icpk_ctx* ctx, int count, int ints) {
  bool grown = false;
  const int rc = reserve_group(ctx, &grown, need(ctx->depth_dev, count), need(ctx->depth_flt, count));
  if (grown) ctx->frame_slot = -1;
  return rc ? rc : ctx->bp_counts.reserve(ctx, ints);
}

// K22: params (NULL: the defaults) checked into *p
static int check_bilateral(icpk_ctx* ctx, const icpk_bilateral_params* params, icpk_bilateral_params* p) {
  if (params)
    *p = *params;
  else
    icpk_default_bilateral_params(p);
  if (icpk_bilateral_tables(p, nullptr, nullptr, nullptr) != ICPK_OK)
    return fail(ctx, ICPK_E_ARG, "bilateral parameters outside their ranges (see THE BILATERAL RULE)");
  return ICPK_OK;
}

// the tables of `p` (checked) on the device.  A change of parameters waits for the stream first: an earlier upload may
// still be reading the host copy that is about to be rewritten.
static int ensure_bilateral_tables(icpk_ctx* ctx, const icpk_bilateral_params& p) {
  if (ctx->bil_params.radius != 0 && std::memcmp(&ctx->bil_params, &p, sizeof(p)) == 0) return ICPK_OK;
  constexpr int side_max = 2 * ICPK_BILATERAL_MAX_RADIUS + 1;
  constexpr size_t words = side_max * side_max + ICPK_BILATERAL_MAX_RANGE;
  const int rc = ctx->bil_tables.reserve(ctx, words);
  if (rc) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->bil_params.radius = 0;
  ctx->bil_tables_host.resize(words);
  uint16_t* const h = ctx->bil_tables_host.data();
  const int n_ws = (2 * p.radius + 1) * (2 * p.radius + 1);
  int32_t K = 0;
  icpk_bilateral_tables(&p, h, h + n_ws, &K);
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->bil_tables, h, (size_t)(n_ws + K) * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  ctx->bil_params = p;
  ctx->bil_K = K;
  return ICPK_OK;
}

static int backproject_impl(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols, float fx, float cx,
                            const float offset[3], int32_t which, int normals_mode /* <0: none */,
                            const DepthFilter* flt = nullptr, const icpk_bilateral_params* bil = nullptr /* checked */,
                            const uint16_t* dev_image = nullptr /* K24: an image on the device in place of `depth` */) {
  if (!ctx || (!depth && !dev_image) || rows <= 0 || cols <= 0 || (which != 0 && which != 1) || (int64_t)rows * cols > (1 << 28) ||
      normals_mode > ICPK_NORMALS_REFERENCE)
    return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int npix = rows * cols;
  const int nblocks = (npix + 1023) / 1024;
  int rc = ensure_depth_buffers(ctx, dev_image ? 0 : npix, nblocks + 2);
  if (rc) return rc;
  Cloud& c = which == 0 ? ctx->src0 : ctx->tgt;
  rc = ensure_cloud(ctx, c, npix);  // worst case: every pixel valid
  if (rc) return rc;
  if (bil && (rc = ensure_bilateral_tables(ctx, *bil))) return rc;
  ctx->frame_slot = -1;  // (the image buffers are shared with icpk_backproject_pair's resident frame)
  if (!dev_image)
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->depth_dev, depth, (size_t)npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  const uint16_t* dimg = dev_image ? dev_image : ctx->depth_dev.get();
  if (bil) {  // K22: the cloud (and its normals) come from the smoothed frame
    launch_depth_bilateral(ctx->depth_dev, ctx->depth_flt, rows, cols, bil->radius, ctx->bil_K, ctx->bil_tables, ctx->stream);
    dimg = ctx->depth_flt;
  }
  if (flt) {  // SLAM.cpp:229,553-574: the frame is filtered before it is back-projected
    launch_depth_filter(ctx->depth_dev, ctx->depth_flt, rows, cols, flt->min_d, flt->max_d, flt->ax, flt->ay, flt->morph,
                        ctx->stream);
    dimg = ctx->depth_flt;
  }
  const float ox = offset ? offset[0] : 0.f, oy = offset ? offset[1] : 0.f, oz = offset ? offset[2] : 0.f;
  // the total lands in bp_counts[nblocks + 1] (device) and is read back pinned
  float *nxp = nullptr, *nyp = nullptr, *nzp = nullptr;
  if (normals_mode >= 0) {
    rc = ensure_cloud(ctx, ctx->nrm, npix);
    if (rc) return rc;
    nxp = ctx->nrm.x();
    nyp = ctx->nrm.y();
    nzp = ctx->nrm.z();
  }
  launch_backproject(dimg, rows, cols, fx, cx, ox, oy, oz, c.x(), c.y(), c.z(), nxp, nyp, nzp,
                     normals_mode < 0 ? 0 : normals_mode, ctx->bp_counts, ctx->bp_counts + nblocks + 1, next_subsample_key(ctx),
                     ctx->sub_factor, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->bp_n_host, ctx->bp_counts + nblocks + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = *ctx->bp_n_host;
  c.n = n;
  const float pad = which == 0 ? 0.f : __builtin_inff();
  const int padded = round_up(n < 1 ? 1 : n, NN_TILE);
  launch_fill_f32(c.x() + n, padded - n, pad, ctx->stream);
  launch_fill_f32(c.y() + n, padded - n, pad, ctx->stream);
  launch_fill_f32(c.z() + n, padded - n, pad, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_assoc = false;
  ctx->have_seed = false;
  ctx->have_qperm = false;
  if (which == 0) {
    ctx->have_src = true;
    rc = copy_src0_to_src(ctx);
    if (rc) return rc;
  } else {
    target_changed(ctx, false);
    ctx->have_normals = normals_mode >= 0;
    if (ctx->have_normals) ctx->nrm.n = n;
  }
  return n;  // (the depth image was consumed before the count came back: no second host wait)
}

int icpk_backproject_pair(icpk_ctx* ctx, const uint16_t* depth_source, const uint16_t* depth_target, int32_t rows,
                          int32_t cols, float fx, float cx, const float offset[3], const float R[9], const float t[3],
                          int32_t filter, int32_t max_d, int32_t min_d, int32_t morph, int32_t anchor_x, int32_t anchor_y,
                          int32_t* n_source, int32_t* n_target) {
  if (!ctx || !depth_source || rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 27) || (!R != !t))
    return ICPK_E_ARG;
  int ax = anchor_x, ay = anchor_y;
  int rc = filter ? check_filter(ctx, morph, ax, ay) : ICPK_OK;
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int npix = rows * cols;
  const int nblocks = (npix + 1023) / 1024;
  const int per_image = nblocks + 2;
  const int fset[6] = {filter != 0, max_d, min_d, morph != 0, ax, ay};
  // depth_target == NULL: the previous frame is the one this context saw as `depth_source` last time (SLAM.cpp:305,
  // previous = filtered.clone()): its image -- and its filtered copy -- are still on the device
  const bool resident = depth_target == nullptr;
  const bool fits = (size_t)2 * npix <= ctx->depth_dev.capacity();
  if (resident && (ctx->frame_slot < 0 || ctx->frame_rows != rows || ctx->frame_cols != cols || !fits))
    return fail(ctx, ICPK_E_NOT_SET, "no resident previous frame of this size (pass depth_target)");
  if (!resident && !fits) ctx->frame_slot = -1;  // (the buffers are about to be replaced)
  rc = ensure_depth_buffers(ctx, 2 * npix, 2 * per_image + 2);
  if (rc) return rc;
  for (Cloud* c : {&ctx->src0, &ctx->src, &ctx->tgt}) {
    rc = ensure_cloud(ctx, *c, npix);  // worst case: every pixel valid
    if (rc) return rc;
  }
  // two image slots; the new frame goes where the resident one is not
  const int tslot = resident ? ctx->frame_slot : 1;
  const int sslot = 1 - tslot;
  uint16_t* const raw_s = ctx->depth_dev + (size_t)sslot * npix;
  uint16_t* const raw_t = ctx->depth_dev + (size_t)tslot * npix;
  uint16_t* const flt_s = ctx->depth_flt + (size_t)sslot * npix;
  uint16_t* const flt_t = ctx->depth_flt + (size_t)tslot * npix;
  const size_t bytes = (size_t)npix * sizeof(uint16_t);
  ctx->frame_slot = -1;  // (nothing is resident until this call has enqueued everything)
  // The images cross PCIe from the context's own pinned staging buffer, in halves: the copy engine moves one half
  // while the host copies the next one in.  (Handing the caller's pageable buffer to hipMemcpyAsync leaves the staging
  // to the runtime -- one blocking copy, then the transfer -- and was seen to take 70 us in one process and 340 us in
  // the next for the same 614 KB.)  The buffer is free again when this call returns: the counts it waits for are made
  // from the uploaded images.
  if ((rc = ctx->stage_depth.reserve(ctx, (size_t)2 * npix))) return rc;
  // without the filter the images are not copied at all: the counting pass reads them from the staging buffer
  const bool zero_copy = !filter && ctx->tune.zero_copy_upload;
  // (an image inside memory the caller has registered -- icpk_register_host_buffer -- is read where it lies: no copy at all)
  const uint16_t* reg_s = zero_copy ? static_cast<const uint16_t*>(registered_device_pointer(ctx, depth_source, bytes)) : nullptr;
  const uint16_t* reg_t =
      zero_copy && !resident ? static_cast<const uint16_t*>(registered_device_pointer(ctx, depth_target, bytes)) : nullptr;
  auto upload = [&](uint16_t* dev, const uint16_t* host, uint16_t* stage) -> int {
    if (zero_copy) {
      if (!(host == depth_source ? reg_s : reg_t)) std::memcpy(stage, host, bytes);
      return ICPK_OK;
    }
    const int parts = npix >= 65536 ? 2 : 1;  // (more parts cost more in copy commands than they hide)
    for (int k = 0; k < parts; ++k) {
      const size_t a0 = (size_t)npix * k / parts, a1 = (size_t)npix * (k + 1) / parts;
      std::memcpy(stage + a0, host + a0, (a1 - a0) * sizeof(uint16_t));
      ICPK_HIP(ctx, hipMemcpyAsync(dev + a0, stage + a0, (a1 - a0) * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    }
    return ICPK_OK;
  };
  if ((rc = upload(raw_s, depth_source, ctx->stage_depth))) return rc;
  if (!resident && (rc = upload(raw_t, depth_target, ctx->stage_depth + npix))) return rc;
  const uint16_t *img_s = raw_s, *img_t = raw_t;
  if (filter) {  // SLAM.cpp:229,553-574: the frames are filtered before they are back-projected
    launch_depth_filter(raw_s, flt_s, rows, cols, min_d, max_d, ax, ay, morph != 0, ctx->stream);
    // (the resident frame's filtered copy is reused when it was made with the same settings)
    if (!resident || std::memcmp(fset, ctx->frame_filter, sizeof(fset)) != 0)
      launch_depth_filter(raw_t, flt_t, rows, cols, min_d, max_d, ax, ay, morph != 0, ctx->stream);
    img_s = flt_s;
    img_t = flt_t;
  }
  if ((rc = reserve_group(ctx, nullptr, need(ctx->pix_tidx, npix), need(ctx->pix_src, npix)))) return rc;
  BpPair b;
  const uint16_t* stage_dev = nullptr;
  if (zero_copy) ICPK_HIP(ctx, hipHostGetDevicePointer((void**)&stage_dev, ctx->stage_depth, 0));
  b.im[0] = BpImage{img_s, ctx->src0.x(), ctx->src0.y(), ctx->src0.z(), ctx->src.x(), ctx->src.y(), ctx->src.z(),
                    ctx->bp_counts, 0.f, ctx->pix_src, nullptr, zero_copy ? (reg_s ? reg_s : stage_dev) : nullptr, raw_s, 0, 0, 0};
  b.im[1] = BpImage{img_t, ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), nullptr, nullptr, nullptr,
                    ctx->bp_counts + per_image, __builtin_inff(), nullptr, ctx->pix_tidx,
                    zero_copy && !resident ? (reg_t ? reg_t : stage_dev + npix) : nullptr, raw_t, 0, 0, 0};
  // (icp.cpp:38-39 builds the cloud of `data` first, then that of `previous`: the source draws its pattern first)
  b.im[0].sub_key = next_subsample_key(ctx);
  b.im[1].sub_key = next_subsample_key(ctx);
  b.im[0].sub_factor = b.im[1].sub_factor = ctx->sub_factor;
  Rt rt{};
  if (R) {
    std::memcpy(rt.R, R, sizeof(rt.R));
    std::memcpy(rt.t, t, sizeof(rt.t));
  }
  int* n_dev = ctx->bp_counts + 2 * per_image;
  // the one host wait: both counts (and both images consumed).  The scan writes them into pinned, mapped words as
  // well (progress words 4, 5), the host spins on those and returns while the scatter is still running -- whatever
  // comes next is stream-ordered behind it.  ICPK_RESULT_MIRROR=0: copy them back and wait for the stream.
  volatile int* const nw = ctx->progress + 4;
  nw[0] = nw[1] = -1;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  launch_backproject_pair(b, rows, cols, fx, cx, offset ? offset[0] : 0.f, offset ? offset[1] : 0.f,
                          offset ? offset[2] : 0.f, rt, R != nullptr, n_dev, ctx->tune.result_mirror ? ctx->progress_dev + 4 : nullptr,
                          ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  if (ctx->tune.result_mirror) {
    rc = spin_until(ctx, [&] { return nw[0] >= 0 && nw[1] >= 0; }, "back-projection ended without its counts");
    if (rc) return rc;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    ctx->bp_n_host[0] = nw[0];
    ctx->bp_n_host[1] = nw[1];
  } else {
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->bp_n_host, n_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  ctx->src0.n = ctx->src.n = ctx->bp_n_host[0];
  ctx->tgt.n = ctx->bp_n_host[1];
  ctx->src_pristine = true;  // (the scatter wrote the committed and the working copy of the source at once)
  ctx->have_pix_seed = true;  // (... and which pixel every point came from)
  ctx->pix_rows = rows;
  ctx->pix_cols = cols;
  ctx->have_src = true;
  ctx->have_qperm = false;
  target_changed(ctx, false);
  ctx->frame_slot = sslot;
  ctx->frame_rows = rows;
  ctx->frame_cols = cols;
  std::memcpy(ctx->frame_filter, fset, sizeof(fset));
  if (n_source) *n_source = ctx->src.n;
  if (n_target) *n_target = ctx->tgt.n;
  return ICPK_OK;
}

int icpk_backproject_filtered(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols, float fx, float cx,
                              const float offset[3], int32_t which, int32_t normals_mode, int32_t max_d,
                              int32_t min_d, int32_t morph, int32_t anchor_x, int32_t anchor_y) {
  if (!ctx) return ICPK_E_ARG;
  if (normals_mode >= 0 && which != 1) return fail(ctx, ICPK_E_ARG, "normals belong to the target cloud");
  int ax = anchor_x, ay = anchor_y;
  int rc = check_filter(ctx, morph, ax, ay);
  if (rc) return rc;
  const DepthFilter f{max_d, min_d, morph != 0, ax, ay};
  return backproject_impl(ctx, depth, rows, cols, fx, cx, offset, which, normals_mode < 0 ? -1 : normals_mode, &f);
}

int icpk_filter_depth_image(icpk_ctx* ctx, const uint16_t* depth_in, uint16_t* depth_out, int32_t rows, int32_t cols,
                            int32_t max_d, int32_t min_d, int32_t morph, int32_t anchor_x, int32_t anchor_y) {
  if (!ctx || !depth_in || !depth_out || rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  int ax = anchor_x, ay = anchor_y;
  int rc = check_filter(ctx, morph, ax, ay);
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int npix = rows * cols;
  rc = ensure_depth_buffers(ctx, npix, 0);
  if (rc) return rc;
  ctx->frame_slot = -1;  // (the image buffers are shared with icpk_backproject_pair's resident frame)
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->depth_dev, depth_in, (size_t)npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  launch_depth_filter(ctx->depth_dev, ctx->depth_flt, rows, cols, min_d, max_d, ax, ay, morph != 0, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(depth_out, ctx->depth_flt, (size_t)npix * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_bilateral_depth_image(icpk_ctx* ctx, const icpk_bilateral_params* params, const uint16_t* depth_in,
                               uint16_t* depth_out, int32_t rows, int32_t cols) {
  if (!ctx || !depth_in || !depth_out || rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  icpk_bilateral_params p;
  int rc = check_bilateral(ctx, params, &p);
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int npix = rows * cols;
  rc = ensure_depth_buffers(ctx, npix, 0);
  if (rc) return rc;
  if ((rc = ensure_bilateral_tables(ctx, p))) return rc;
  ctx->frame_slot = -1;  // (the image buffers are shared with icpk_backproject_pair's resident frame)
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->depth_dev, depth_in, (size_t)npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  launch_depth_bilateral(ctx->depth_dev, ctx->depth_flt, rows, cols, p.radius, ctx->bil_K, ctx->bil_tables, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(depth_out, ctx->depth_flt, (size_t)npix * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_backproject_smoothed(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols, float fx, float cx,
                              const float offset[3], int32_t which, int32_t normals_mode,
                              const icpk_bilateral_params* params) {
  if (!ctx) return ICPK_E_ARG;
  if (normals_mode >= 0 && which != 1) return fail(ctx, ICPK_E_ARG, "normals belong to the target cloud");
  icpk_bilateral_params p;
  const int rc = check_bilateral(ctx, params, &p);
  if (rc) return rc;
  return backproject_impl(ctx, depth, rows, cols, fx, cx, offset, which, normals_mode < 0 ? -1 : normals_mode, nullptr, &p);
}

// ---- K24: the depth pyramid (include/icpk.h, THE PYRAMID RULE; its host-only half is icpk_pyramid.cpp) ----
int icpk_depth_pyramid_build(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols,
                             const icpk_pyramid_params* params, const icpk_bilateral_params* smooth) {
  if (!ctx || !depth || rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  icpk_pyramid_params p;
  if (params)
    p = *params;
  else
    icpk_default_pyramid_params(&p);
  if (p.levels < 1 || p.levels > ICPK_PYRAMID_MAX_LEVELS || p.range_cutoff < 1 || p.range_cutoff > 65536)
    return fail(ctx, ICPK_E_ARG, "pyramid parameters outside their ranges (see THE PYRAMID RULE)");
  icpk_bilateral_params bil;
  int rc = smooth ? check_bilateral(ctx, smooth, &bil) : ICPK_OK;
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int lr[ICPK_PYRAMID_MAX_LEVELS], lc[ICPK_PYRAMID_MAX_LEVELS];
  size_t off[ICPK_PYRAMID_MAX_LEVELS], total = 0;
  for (int l = 0; l < p.levels; ++l) {
    lr[l] = l ? (lr[l - 1] + 1) / 2 : rows;
    lc[l] = l ? (lc[l - 1] + 1) / 2 : cols;
    off[l] = total;
    total += (size_t)lr[l] * lc[l];
  }
  const size_t npix = (size_t)rows * cols;
  if (smooth) {
    if ((rc = ensure_depth_buffers(ctx, (int)npix, 0))) return rc;
    if ((rc = ensure_bilateral_tables(ctx, bil))) return rc;
  }
  if (total > ctx->pyr.capacity()) ctx->pyr_levels = 0;  // (the old pyramid goes with its memory)
  if ((rc = ctx->pyr.reserve(ctx, total))) return rc;
  ctx->pyr_levels = 0;  // (nothing is resident until this call has enqueued everything)
  ctx->pyr_have_int = false;  // (K26: the intensity levels belong to the pyramid they were set beside)
  ctx->fern_code_current = false;  // (K27: and so does the current fern code; the database stays)
  uint16_t* const base = ctx->pyr;
  if (smooth) {  // K22 writes level 0
    ctx->frame_slot = -1;  // (the image buffers are shared with icpk_backproject_pair's resident frame)
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->depth_dev, depth, npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    launch_depth_bilateral(ctx->depth_dev, base, rows, cols, bil.radius, ctx->bil_K, ctx->bil_tables, ctx->stream);
  } else {
    ICPK_HIP(ctx, hipMemcpyAsync(base, depth, npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  }
  // two levels per launch from the deepest level written; a last odd level with the second stage switched off
  for (int l = 0; l + 1 < p.levels; l += 2)
    launch_depth_pyramid(base + off[l], lr[l], lc[l], base + off[l + 1], l + 2 < p.levels ? base + off[l + 2] : nullptr,
                         p.range_cutoff, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's image has been consumed)
  for (int l = 0; l < p.levels; ++l) {
    ctx->pyr_rows[l] = lr[l];
    ctx->pyr_cols[l] = lc[l];
    ctx->pyr_off[l] = off[l];
  }
  ctx->pyr_levels = p.levels;
  ctx->pyr_K = p.range_cutoff;
  return ICPK_OK;
}

// ---- K26: the intensity pyramid beside it (include/icpk.h, THE INTENSITY PYRAMID RULE) ----
int icpk_depth_pyramid_set_intensity(icpk_ctx* ctx, const float* intensity, int32_t rows, int32_t cols) {
  if (!ctx || !intensity) return ICPK_E_ARG;
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  if (rows != ctx->pyr_rows[0] || cols != ctx->pyr_cols[0]) return fail(ctx, ICPK_E_ARG, "the image's shape is not level 0's");
  const size_t npix = (size_t)rows * cols;
  for (size_t i = 0; i < npix; ++i)
    if (!(intensity[i] >= 0.f && intensity[i] <= 1.f)) return fail(ctx, ICPK_E_ARG, "an intensity is not in [0, 1]");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int L = ctx->pyr_levels;
  const size_t total = ctx->pyr_off[L - 1] + (size_t)ctx->pyr_rows[L - 1] * ctx->pyr_cols[L - 1];
  if (total > ctx->pyr_int.capacity()) ctx->pyr_have_int = false;  // (the old levels go with their memory)
  if (int rc = ctx->pyr_int.reserve(ctx, total)) return rc;
  ctx->pyr_have_int = false;
  float* const base = ctx->pyr_int;
  ICPK_HIP(ctx, hipMemcpyAsync(base, intensity, npix * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  for (int l = 0; l + 1 < L; ++l)
    launch_intensity_pyramid(ctx->pyr + ctx->pyr_off[l], base + ctx->pyr_off[l], ctx->pyr_rows[l], ctx->pyr_cols[l],
                             base + ctx->pyr_off[l + 1], ctx->pyr_K, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's image has been consumed)
  ctx->pyr_have_int = true;
  return ICPK_OK;
}

int icpk_depth_pyramid_get_intensity(icpk_ctx* ctx, int32_t level, float* out) {
  if (!ctx || !out) return ICPK_E_ARG;
  if (ctx->pyr_levels == 0 || !ctx->pyr_have_int)
    return fail(ctx, ICPK_E_NOT_SET, "no intensity pyramid (icpk_depth_pyramid_set_intensity)");
  if (level < 0 || level >= ctx->pyr_levels) return fail(ctx, ICPK_E_ARG, "the pyramid has no such level");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipMemcpyAsync(out, ctx->pyr_int + ctx->pyr_off[level],
                               (size_t)ctx->pyr_rows[level] * ctx->pyr_cols[level] * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// the resident pyramid has this level
static int check_pyramid_level(icpk_ctx* ctx, int32_t level) {
  if (!ctx) return ICPK_E_ARG;
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  if (level < 0 || level >= ctx->pyr_levels) return fail(ctx, ICPK_E_ARG, "the pyramid has no such level");
  return ICPK_OK;
}

int icpk_depth_pyramid_shape(icpk_ctx* ctx, int32_t level, int32_t* rows, int32_t* cols) {
  const int rc = check_pyramid_level(ctx, level);
  if (rc) return rc;
  if (rows) *rows = ctx->pyr_rows[level];
  if (cols) *cols = ctx->pyr_cols[level];
  return ICPK_OK;
}

int icpk_depth_pyramid_get(icpk_ctx* ctx, int32_t level, uint16_t* out) {
  if (!ctx || !out) return ICPK_E_ARG;
  const int rc = check_pyramid_level(ctx, level);
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipMemcpyAsync(out, ctx->pyr + ctx->pyr_off[level],
                               (size_t)ctx->pyr_rows[level] * ctx->pyr_cols[level] * sizeof(uint16_t), hipMemcpyDeviceToHost,
                               ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_depth_pyramid_backproject(icpk_ctx* ctx, int32_t level, float fx, float cx, const float offset[3], int32_t which,
                                   int32_t normals_mode) {
  const int rc = check_pyramid_level(ctx, level);
  if (rc) return rc;
  if (normals_mode >= 0 && which != 1) return fail(ctx, ICPK_E_ARG, "normals belong to the target cloud");
  const float scale = (float)(1 << level);  // (a power of two: both quotients are exact)
  return backproject_impl(ctx, nullptr, ctx->pyr_rows[level], ctx->pyr_cols[level], fx / scale, cx / scale, offset, which,
                          normals_mode < 0 ? -1 : normals_mode, nullptr, nullptr, ctx->pyr + ctx->pyr_off[level]);
}

/* icp.cpp:488-515 on the context's clouds (source = the frame's key points, target = the map's) */
int icpk_associate_keypoints(icpk_ctx* ctx, int32_t nn_mode, float max_dist, int32_t* assoc_query,
                             int32_t* assoc_target, float* assoc_dist, int32_t* n_assoc, int32_t* rejected_query,
                             int32_t rejected_capacity, int32_t* n_rejected) {
  if (!ctx || !n_assoc || !n_rejected || *n_rejected < 0 || rejected_capacity < *n_rejected) return ICPK_E_ARG;
  if (!ctx->have_tgt || !ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source or target cloud not set");
  // icp.cpp:490-491: an empty map returns BEFORE errors / associations are cleared: nothing is touched
  if (ctx->tgt.n <= 0) return ICPK_W_EMPTY_MAP;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  const int nq = ctx->src.n;
  if (nq == 0) {  // icp.cpp:497-498: the lists are cleared, nothing is appended
    *n_assoc = 0;
    return ICPK_OK;
  }
  if (!assoc_query || !assoc_target || !assoc_dist || (!rejected_query && rejected_capacity > 0)) return ICPK_E_ARG;
  if (nn_mode == ICPK_NN_MAP && !(max_dist <= ICPK_MAX_NN_DISTANCE))
    return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP: max_dist <= 0.75");
  int rc = enqueue_nn(ctx, nn_mode);
  if (rc) return rc;
  if ((rc = ctx->ks_buf.reserve(ctx, (size_t)4 * round_up(nq, NN_TILE)))) return rc;
  const int nblocks = (nq + 1023) / 1024;
  rc = ensure_depth_buffers(ctx, 0, nblocks + 2);
  if (rc) return rc;
  const size_t ks = ctx->ks_buf.capacity() / 4;  // entries per list
  int32_t* dq = ctx->ks_buf;
  int32_t* dt = dq + ks;
  float* dd = reinterpret_cast<float*>(dt + ks);
  int32_t* dr = dt + 2 * ks;
  launch_assoc_split(ctx->best, nq, max_dist, ctx->bp_counts, ctx->bp_counts + nblocks + 1, dq, dt, dd, dr, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->bp_n_host, ctx->bp_counts + nblocks + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int na = *ctx->bp_n_host, nr = nq - na;
  if (*n_rejected + nr > rejected_capacity)
    return fail(ctx, ICPK_E_ARG, "rejected_capacity too small for the appended queries");
  if (na > 0) {
    ICPK_HIP(ctx, hipMemcpyAsync(assoc_query, dq, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(assoc_target, dt, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(assoc_dist, dd, (size_t)na * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (nr > 0)
    ICPK_HIP(ctx, hipMemcpyAsync(rejected_query + *n_rejected, dr, (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost,
                                 ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_assoc = na;           // icp.cpp:497-498: errors / associations are rebuilt by every call
  *n_rejected += nr;       // icp.cpp:507-509: nonAssociations only ever grows
  return ICPK_OK;
}

int icpk_backproject(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols, float fx, float cx,
                     const float offset[3], int32_t which) {
  return backproject_impl(ctx, depth, rows, cols, fx, cx, offset, which, -1);
}

int icpk_backproject_with_normals(icpk_ctx* ctx, const uint16_t* depth, int32_t rows, int32_t cols, float fx, float cx,
                                  const float offset[3], int32_t normals_mode) {
  if (normals_mode < 0) return ICPK_E_ARG;
  return backproject_impl(ctx, depth, rows, cols, fx, cx, offset, 1, normals_mode);
}
int icpk_backproject_keypoints(const uint16_t* depth, int32_t rows, int32_t cols, const float* kp_xy, int32_t n, float fx,
                               float cx, float* out_xyz, int32_t* kept) {
  if (!depth || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!kp_xy || !out_xyz))) return ICPK_E_ARG;
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const float fxp = kp_xy[2 * i], fyp = kp_xy[2 * i + 1];
    if (!(fxp > -1.f && fxp < (float)cols + 1.f && fyp > -1.f && fyp < (float)rows + 1.f)) continue;  // (NaN, far outside)
    const long x = std::lrint(fxp), y = std::lrint(fyp);  // cvRound: to nearest, ties to even (default rounding mode)
    if (x < 0 || x >= cols || y < 0 || y >= rows) continue;
    const uint16_t d = depth[(size_t)y * cols + x];
    if (d == 0) continue;  // pointcloud.cpp:67-70
    const float pz = ((float)d) / 5000.0f;            // pointcloud.cpp:86
    const float px = ((float)x - cx) * pz / fx;       // :87 (an int minus the float constant)
    const float py = ((float)y - cx) * pz / fx;       // :88 (CX, FX)
    out_xyz[3 * m] = px;
    out_xyz[3 * m + 1] = py;
    out_xyz[3 * m + 2] = pz;
    if (kept) kept[m] = i;
    ++m;
  }
  return m;
}

}  // extern "C"
