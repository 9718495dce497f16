// icpk_fast.cpp -- host side of K8 (kernels_fast.hip; icpk_bgr_to_gray, icpk_detect_fast, icpk_detected_to_cloud in
// include/icpk.h).
//
// A detection is one upload of the image, 3 launches and one host wait for the count; the key points stay on the
// device as the context's detected list.  icpk_detected_to_cloud turns that list into the context's source or target
// with one launch, the depth image read where it lies in pinned host memory (only the key points' pixels cross
// PCIe), and one host wait on a mapped count word.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <string>
#include <thread>

#include "icpk.h"
#include "icpk_ctx.h"
#include "icpk_internal.h"

using namespace icpk;

struct icpk_fast_state {
  DevBuf<uint8_t> img;       // the uploaded image (rows x cols x channels)
  PinnedBuf<uint8_t> stage;  // the image on its way to the device
  DevBuf<uint8_t> score;     // rows x cols (the score of every kept pixel; grey output of icpk_bgr_to_gray)
  DevBuf<unsigned long long> masks;  // rows x tile columns
  DevBuf<int> counts;                // rows x tile columns, then the total (total_word)
  DevBuf<float> kp;    // the detected list, (x, y) per key point ...
  DevBuf<float> resp;  // ... and its response
  PinnedBuf<int> total_host;
  MappedBuf<uint16_t> dstage;  // the depth image of icpk_detected_to_cloud
  int n = -1;  // key points in the detected list (-1: no detection yet)
  int rows = 0, cols = 0, channels = 0;  // of the image the list was detected in: img holds it while n >= 0 (K32 reads it)
};

namespace {

int ensure_fast(icpk_ctx* ctx) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->fast) ctx->fast = new icpk_fast_state();
  return ctx->fast->total_host.reserve(ctx, 1);
}

int* total_word(const icpk_fast_state* f) { return f->counts + (f->counts.capacity() - 1); }

bool bad_size(int32_t rows, int32_t cols) { return rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 27); }

// the image into the device buffer through the pinned staging buffer
int upload_image(icpk_ctx* ctx, const uint8_t* image, size_t bytes) {
  icpk_fast_state* f = ctx->fast;
  int rc = f->stage.reserve(ctx, bytes);
  if (!rc) rc = f->img.reserve(ctx, bytes);
  if (rc) return rc;
  std::memcpy(f->stage, image, bytes);
  ICPK_HIP(ctx, hipMemcpyAsync(f->img, f->stage, bytes, hipMemcpyHostToDevice, ctx->stream));
  return ICPK_OK;
}

// per-(row, tile column) masks and counts (+ the total), and a detected list with room for every pixel
int ensure_lists(icpk_ctx* ctx, size_t ents, size_t npix) {
  icpk_fast_state* f = ctx->fast;
  int rc = reserve_group(ctx, nullptr, need(f->masks, ents), need(f->counts, ents + 1));
  if (rc) return rc;
  bool grown = false;
  rc = reserve_group(ctx, &grown, need(f->kp, 2 * npix), need(f->resp, npix));
  if (grown) f->n = -1;
  return rc;
}

}  // namespace

void icpk_fast_free(icpk_ctx* ctx) {
  icpk_fast_state* f = ctx ? ctx->fast : nullptr;
  if (!f) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete f;  // (its buffers free themselves)
  ctx->fast = nullptr;
}

namespace icpk {

FastResident fast_resident(const icpk_ctx* ctx) {
  const icpk_fast_state* f = ctx->fast;
  if (!f || f->n < 0 || f->channels == 0) return FastResident{nullptr, 0, 0, 0, nullptr, -1};
  return FastResident{f->img, f->rows, f->cols, f->channels, f->kp, f->n};
}

int keypoints_to_cloud(icpk_ctx* ctx, const float* kp, int n, const uint16_t* depth, int32_t d_rows, int32_t d_cols, float fx,
                       float cx, const float R[9], const float t[3], int32_t which, int* map, int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!depth || bad_size(d_rows, d_cols) || !R || !t) return fail(ctx, ICPK_E_ARG, "bad depth image, size or pose");
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (int rc = ensure_fast(ctx)) return rc;  // (the depth staging and the count word live with K8's state)
  icpk_fast_state* f = ctx->fast;
  const size_t npix = (size_t)d_rows * d_cols;
  // the depth image is read where it lies, in pinned host memory: only the key points' pixels cross PCIe.  The buffer
  // is free again when this call returns (the count is written after the last read).
  int rc = f->dstage.reserve(ctx, npix);
  if (!rc) rc = ensure_lists(ctx, 1, 0);  // (the count word, should the detection have had no candidate pixel)
  if (rc) return rc;
  std::memcpy(f->dstage, depth, npix * sizeof(uint16_t));
  const uint16_t* ddev = nullptr;
  ICPK_HIP(ctx, hipHostGetDevicePointer((void**)&ddev, f->dstage, 0));
  Rt rt;
  std::memcpy(rt.R, R, sizeof(rt.R));
  std::memcpy(rt.t, t, sizeof(rt.t));
  // room for every key point; the planes are written as icpk_set_source / icpk_set_target leave them (a source:
  // committed and working copy, padding 0; a target: padding +inf)
  Cloud* c = which == 0 ? &ctx->src0 : &ctx->tgt;
  rc = ensure_cloud(ctx, *c, n);
  if (!rc && which == 0) rc = ensure_cloud(ctx, ctx->src, n);
  if (rc) return rc;
  Cloud* c2 = which == 0 ? &ctx->src : nullptr;
  int* n_dev = total_word(f);  // (the detection's total is read from f->n: the word is free)
  volatile int* const nw = ctx->tune.result_mirror && ctx->progress ? ctx->progress + 6 : nullptr;
  if (nw) {
    nw[0] = -1;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
  }
  launch_fast_cloud(kp, n, ddev, d_rows, d_cols, fx, cx, rt, c->x(), c->y(), c->z(), c2 ? c2->x() : nullptr,
                    c2 ? c2->y() : nullptr, c2 ? c2->z() : nullptr, which == 0 ? 0.f : __builtin_inff(), n_dev,
                    nw ? ctx->progress_dev + 6 : nullptr, map, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  int m = 0;
  if (nw) {  // the one host wait, on the mapped word (as icpk_backproject_pair)
    rc = spin_until(ctx, [&] { return nw[0] >= 0; }, "key-point back-projection ended without its count");
    if (rc) return rc;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    m = nw[0];
  } else {
    ICPK_HIP(ctx, hipMemcpyAsync(f->total_host, n_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m = *f->total_host;
  }
  if (which == 0) {  // what set_source leaves behind
    ctx->src0.n = ctx->src.n = m;
    ctx->src_pristine = true;  // (both copies were written at once)
    ctx->have_src = true;
    ctx->have_assoc = ctx->have_seed = ctx->have_qperm = false;
  } else {  // what set_target leaves behind
    ctx->tgt.n = m;
    target_changed(ctx, false);
  }
  if (n_out) *n_out = m;
  return ICPK_OK;
}

}  // namespace icpk

extern "C" {

int icpk_bgr_to_gray(icpk_ctx* ctx, const uint8_t* bgr, int32_t rows, int32_t cols, uint8_t* gray_out) {
  if (!ctx) return ICPK_E_ARG;
  if (!bgr || !gray_out || bad_size(rows, cols)) return fail(ctx, ICPK_E_ARG, "bad image or size");
  int rc = ensure_fast(ctx);
  if (rc) return rc;
  icpk_fast_state* f = ctx->fast;
  const size_t npix = (size_t)rows * cols;
  f->rows = f->cols = f->channels = 0;  // (the image of the detected list is overwritten: K32 refuses to describe against it)
  rc = upload_image(ctx, bgr, 3 * npix);
  if (!rc) rc = f->score.reserve(ctx, npix);
  if (rc) return rc;
  launch_bgr_to_gray(f->img, (int)npix, f->score, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(gray_out, f->score, npix, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_detect_fast(icpk_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t channels,
                     int32_t threshold, int32_t nonmax, int32_t type, int32_t capacity, float* kp_xy, float* response,
                     int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!ctx) return ICPK_E_ARG;
  if (!image || bad_size(rows, cols)) return fail(ctx, ICPK_E_ARG, "bad image or size");
  if (channels != 1 && channels != 3) return fail(ctx, ICPK_E_ARG, "channels must be 1 (grey) or 3 (BGR)");
  if (type != ICPK_FAST_TYPE_7_12 && type != ICPK_FAST_TYPE_9_16)
    return fail(ctx, ICPK_E_ARG, "FAST type must be ICPK_FAST_TYPE_7_12 or ICPK_FAST_TYPE_9_16");
  if (capacity < 0) return fail(ctx, ICPK_E_ARG, "negative capacity");
  int rc = ensure_fast(ctx);
  if (rc) return rc;
  icpk_fast_state* f = ctx->fast;
  f->n = 0;
  f->rows = rows, f->cols = cols, f->channels = channels;
  if (rows < 7 || cols < 7) return ICPK_OK;  // no candidate pixel (3 <= y <= rows - 4, 3 <= x <= cols - 4)
  f->n = -1;  // (a failed call below leaves no list)
  const int t = threshold < 0 ? 0 : (threshold > 255 ? 255 : threshold);  // fast.cpp: std::min(std::max(threshold, 0), 255)
  const size_t npix = (size_t)rows * cols;
  const size_t ents = (size_t)rows * fast_tiles_x(cols);
  rc = upload_image(ctx, image, (size_t)channels * npix);
  if (!rc) rc = f->score.reserve(ctx, npix);
  if (!rc) rc = ensure_lists(ctx, ents, npix);
  if (rc) return rc;
  int* total = total_word(f);
  launch_fast_detect(f->img, rows, cols, channels, t, nonmax != 0, type == ICPK_FAST_TYPE_9_16 ? 16 : 12, f->masks, f->counts,
                     f->score, total, f->kp, f->resp, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(f->total_host, total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = *f->total_host;
  f->n = n;
  const int m = n < capacity ? n : capacity;
  if (m > 0 && (kp_xy || response)) {
    if (kp_xy) ICPK_HIP(ctx, hipMemcpyAsync(kp_xy, f->kp, (size_t)2 * m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (response) ICPK_HIP(ctx, hipMemcpyAsync(response, f->resp, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (n_out) *n_out = n;
  return ICPK_OK;
}

int icpk_detected_to_cloud(icpk_ctx* ctx, const uint16_t* depth, int32_t d_rows, int32_t d_cols, float fx, float cx,
                           const float R[9], const float t[3], int32_t which, int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!ctx) return ICPK_E_ARG;
  if (!depth || bad_size(d_rows, d_cols) || !R || !t) return fail(ctx, ICPK_E_ARG, "bad depth image, size or pose");
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (!ctx->fast || ctx->fast->n < 0) return fail(ctx, ICPK_E_NOT_SET, "no detected key points (icpk_detect_fast)");
  return keypoints_to_cloud(ctx, ctx->fast->kp, ctx->fast->n, depth, d_rows, d_cols, fx, cx, R, t, which, nullptr, n_out);
}

}  // extern "C"
