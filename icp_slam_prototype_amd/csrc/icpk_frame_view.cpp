// icpk_frame_view.cpp -- K28, host side of the frame view (include/icpk.h, THE FRAME VIEW RULE; kernels_frame_view.hip):
// the snapshot the context owns -- per level of the resident pyramid (K24, K26) eight planes in the ray cast's layout,
// in world coordinates at a given pose --, the rule over a host image through the header the kernel includes
// (icpk_frame_view_pixels: no context, no device), THE VIEW GRADIENT RULE's kernel run on a level of it, and the
// resolver that decides which planes the projective calls (icpk_projective.cpp) read.  The snapshot lies outside the
// TSDF state: no volume is needed, and neither a pyramid build nor any TSDF call touches it.
#include <cmath>
#include <cstring>

#include "frame_view_rule.h"
#include "icpk_ctx.h"

using namespace icpk;

static_assert(FRAME_VIEW_MAX_LEVELS == ICPK_PYRAMID_MAX_LEVELS, "one table entry per level a pyramid can have");

struct icpk_frame_view_state {
  // level l: eight planes of rows[l] cols[l] floats from planes + 8 off[l]; its gradients, three planes from
  // grad + 3 off[l] (off[l]: the pixels of the levels before l)
  DevBuf<float> planes, grad;
  DevBuf<int> slots;   // 2 per workgroup of the build
  DevBuf<int> totals;  // 2 per level
  PinnedBuf<int> totals_host;
  bool have = false;
  int levels = 0;
  int rows[ICPK_PYRAMID_MAX_LEVELS] = {0}, cols[ICPK_PYRAMID_MAX_LEVELS] = {0};
  size_t off[ICPK_PYRAMID_MAX_LEVELS + 1] = {0};
  bool color = false;  // the intensity planes hold the intensity pyramid's values
  bool have_grad[ICPK_PYRAMID_MAX_LEVELS] = {false};
  float fx = 0.f, cx = 0.f;  // the LEVEL-0 intrinsics and the pose the snapshot was built with
  double pose[16] = {0};
  size_t npix(int l) const { return (size_t)rows[l] * cols[l]; }
};

void icpk_frame_view_free(icpk_ctx* ctx) {
  delete ctx->fview;  // (its buffers free themselves)
  ctx->fview = nullptr;
}

namespace {

bool finite_pose(const double* pose) {
  if (!pose) return false;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return false;
  return true;
}

bool good_camera(float fx, float cx) { return std::isfinite(fx) && fx > 0.f && std::isfinite(cx); }

// the snapshot and its level, or ICPK_E_NOT_SET / ICPK_E_ARG with the reason
int level_of(icpk_ctx* ctx, int32_t level, icpk_frame_view_state** out) {
  if (level < 0 || level >= ICPK_PYRAMID_MAX_LEVELS) return fail(ctx, ICPK_E_ARG, "a level no frame view can have");
  icpk_frame_view_state* v = ctx->fview;
  if (!v || !v->have) return fail(ctx, ICPK_E_NOT_SET, "no frame view (icpk_frame_view_build)");
  if (level >= v->levels) return fail(ctx, ICPK_E_NOT_SET, "the frame view has no such level");
  *out = v;
  return ICPK_OK;
}

}  // namespace

int icpk::projective_view(icpk_ctx* ctx, TsdfRayView* out) {
  if (ctx->proj_view_which != ICPK_VIEW_FRAME) return tsdf_raycast_view(ctx, out);
  icpk_frame_view_state* v = nullptr;
  const int l = ctx->proj_view_level;
  if (int rc = level_of(ctx, l, &v)) return rc;
  const float scale = (float)(1 << l);  // (a power of two: both quotients are exact)
  out->maps = v->planes + 8 * v->off[l];
  out->rows = v->rows[l], out->cols = v->cols[l];
  out->fx = v->fx / scale, out->cx = v->cx / scale;
  std::memcpy(out->pose, v->pose, sizeof(out->pose));
  return ICPK_OK;
}

void icpk::projective_color_view(icpk_ctx* ctx, bool* color, const float** grad) {
  if (ctx->proj_view_which != ICPK_VIEW_FRAME) return tsdf_raycast_color_view(ctx, color, grad);
  // (after projective_view has succeeded: the snapshot has the selected level)
  const icpk_frame_view_state* v = ctx->fview;
  const int l = ctx->proj_view_level;
  *color = v->color;
  *grad = v->have_grad[l] ? v->grad + 3 * v->off[l] : nullptr;
}

extern "C" {

int icpk_frame_view_build(icpk_ctx* ctx, float fx, float cx, const double pose[16], int32_t* n_valid, int32_t* n_no_normal) {
  if (!ctx) return ICPK_E_ARG;
  if (!finite_pose(pose)) return fail(ctx, ICPK_E_ARG, "the pose is NULL or not finite");
  if (!good_camera(fx, cx)) return fail(ctx, ICPK_E_ARG, "fx must be finite and > 0, cx finite");
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->fview) ctx->fview = new icpk_frame_view_state();
  icpk_frame_view_state* v = ctx->fview;
  const int L = ctx->pyr_levels;
  FrameViewArgs a{};
  size_t total = 0;
  a.block0[0] = 0;
  for (int l = 0; l < L; ++l) {
    const int npix = ctx->pyr_rows[l] * ctx->pyr_cols[l];  // (a level has at most 2^28 pixels)
    a.block0[l + 1] = a.block0[l] + frame_view_blocks(npix);
    total += (size_t)npix;
  }
  const int grid = a.block0[L];
  // (buffers are reused while the shape fits; one that grows takes the old snapshot with it)
  bool grown = false;
  int rc = v->planes.reserve(ctx, 8 * total, &grown);
  if (!rc) rc = v->slots.reserve(ctx, 2 * (size_t)grid);
  if (!rc) rc = v->totals.reserve(ctx, 2 * ICPK_PYRAMID_MAX_LEVELS);
  if (!rc) rc = v->totals_host.reserve(ctx, 2 * ICPK_PYRAMID_MAX_LEVELS);
  if (rc) {
    if (grown) v->have = false;
    return rc;
  }
  v->have = false;  // (nothing is a snapshot until this call has enqueued everything)
  std::memset(v->have_grad, 0, sizeof(v->have_grad));  // (the gradients are those of the planes they were made from)
  size_t off = 0;
  for (int l = 0; l < L; ++l) {
    const float scale = (float)(1 << l);  // (a power of two: both quotients are exact)
    v->rows[l] = ctx->pyr_rows[l], v->cols[l] = ctx->pyr_cols[l], v->off[l] = off;
    FrameViewLevel& lv = a.level[l];
    lv.depth = ctx->pyr + ctx->pyr_off[l];
    lv.inten = ctx->pyr_have_int ? ctx->pyr_int + ctx->pyr_off[l] : nullptr;
    lv.planes = v->planes + 8 * off;
    lv.rows = v->rows[l], lv.cols = v->cols[l];
    lv.fx = fx / scale, lv.cx = cx / scale;
    off += v->npix(l);
  }
  v->off[L] = off;
  a.levels = L;
  proj_round_pose(pose, a.R, a.t);
  a.slots = v->slots;
  launch_frame_view(a, v->totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  v->levels = L;
  v->color = ctx->pyr_have_int;
  v->fx = fx, v->cx = cx;
  std::memcpy(v->pose, pose, sizeof(v->pose));
  v->have = true;
  if (!n_valid && !n_no_normal) return ICPK_OK;  // (nothing is asked: the call does not wait)
  ICPK_HIP(ctx, hipMemcpyAsync(v->totals_host, v->totals, 2 * (size_t)L * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int l = 0; l < L; ++l) {
    if (n_valid) n_valid[l] = v->totals_host[2 * l];
    if (n_no_normal) n_no_normal[l] = v->totals_host[2 * l + 1];
  }
  return ICPK_OK;
}

int icpk_frame_view_levels(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  return ctx->fview && ctx->fview->have ? ctx->fview->levels : 0;
}

int icpk_frame_view_shape(icpk_ctx* ctx, int32_t level, int32_t* rows, int32_t* cols) {
  if (!ctx) return ICPK_E_ARG;
  icpk_frame_view_state* v = nullptr;
  if (int rc = level_of(ctx, level, &v)) return rc;
  if (rows) *rows = v->rows[level];
  if (cols) *cols = v->cols[level];
  return ICPK_OK;
}

int icpk_frame_view_get(icpk_ctx* ctx, int32_t level, float* const planes[8]) {
  if (!ctx || !planes) return ICPK_E_ARG;
  icpk_frame_view_state* v = nullptr;
  if (int rc = level_of(ctx, level, &v)) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = v->npix(level);
  const float* base = v->planes + 8 * v->off[level];
  for (int k = 0; k < 8; ++k)
    if (planes[k])
      ICPK_HIP(ctx, hipMemcpyAsync(planes[k], base + (size_t)k * npix, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_frame_view_release(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->fview) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (nothing enqueued still reads the planes)
  icpk_frame_view_free(ctx);
  return ICPK_OK;
}

int icpk_frame_view_color_gradients(icpk_ctx* ctx, int32_t level, float radius, int32_t min_neighbors, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (!(std::isfinite(radius) && radius > 0.f) || min_neighbors < 1 || flags != 0)
    return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0, min_neighbors >= 1, flags 0");
  icpk_frame_view_state* v = nullptr;
  if (int rc = level_of(ctx, level, &v)) return rc;
  if (!v->color) return fail(ctx, ICPK_E_NOT_SET, "the frame view was built without an intensity pyramid");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  bool grown = false;
  if (int rc = v->grad.reserve(ctx, 3 * v->off[v->levels], &grown)) {
    if (grown) std::memset(v->have_grad, 0, sizeof(v->have_grad));
    return rc;
  }
  if (grown) std::memset(v->have_grad, 0, sizeof(v->have_grad));  // (the other levels' planes went with the old memory)
  v->have_grad[level] = false;
  launch_raycast_color_gradients(v->planes + 8 * v->off[level], v->rows[level], v->cols[level], radius, min_neighbors,
                                 v->grad + 3 * v->off[level], nullptr, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  v->have_grad[level] = true;
  return ICPK_OK;
}

int icpk_frame_view_get_color_gradients(icpk_ctx* ctx, int32_t level, float* gx, float* gy, float* gz) {
  if (!ctx) return ICPK_E_ARG;
  icpk_frame_view_state* v = nullptr;
  if (int rc = level_of(ctx, level, &v)) return rc;
  if (!v->have_grad[level])
    return fail(ctx, ICPK_E_NOT_SET, "no colour gradients of this frame-view level (icpk_frame_view_color_gradients)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = v->npix(level);
  const float* base = v->grad + 3 * v->off[level];
  float* const out[3] = {gx, gy, gz};
  for (int k = 0; k < 3; ++k)
    if (out[k])
      ICPK_HIP(ctx, hipMemcpyAsync(out[k], base + (size_t)k * npix, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_projective_set_view(icpk_ctx* ctx, int32_t which, int32_t view_level) {
  if (!ctx) return ICPK_E_ARG;
  if (which != ICPK_VIEW_RAYCAST && which != ICPK_VIEW_FRAME) return fail(ctx, ICPK_E_ARG, "an unknown view");
  if (which == ICPK_VIEW_RAYCAST) {  // (view_level says nothing about a ray cast)
    ctx->proj_view_which = ICPK_VIEW_RAYCAST, ctx->proj_view_level = 0;
    return ICPK_OK;
  }
  icpk_frame_view_state* v = nullptr;
  if (int rc = level_of(ctx, view_level, &v)) return rc;
  ctx->proj_view_which = ICPK_VIEW_FRAME, ctx->proj_view_level = view_level;
  return ICPK_OK;
}

int icpk_frame_view_pixels(float fx, float cx, int32_t level, const double pose[16], const uint16_t* depth,
                           const float* intensity, int32_t rows, int32_t cols, int64_t first, int32_t count, float* out,
                           int32_t* n_no_normal) {
  if (!depth || !out || count < 0 || first < 0) return ICPK_E_ARG;
  if (!finite_pose(pose) || !good_camera(fx, cx)) return ICPK_E_ARG;
  if (level < 0 || level >= ICPK_PYRAMID_MAX_LEVELS) return ICPK_E_ARG;
  if (rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  if (first + count > (int64_t)rows * cols) return ICPK_E_ARG;
  const float scale = (float)(1 << level);
  const ProjLevel lv{depth, rows, cols, fx / scale, cx / scale};
  ProjPose P;
  proj_round_pose(pose, P.R, P.t);
  int listed = 0, none = 0;
  for (int32_t e = 0; e < count; ++e) {
    const int64_t i = first + e;
    float px[8];
    const int what = frame_view_pixel(lv, P, (int)(i / cols), (int)(i % cols), intensity ? intensity[i] : 0.f, px);
    listed += what == FRAME_VIEW_LISTED, none += what == FRAME_VIEW_NO_NORMAL;
    for (int k = 0; k < 8; ++k) out[(size_t)k * count + e] = px[k];
  }
  if (n_no_normal) *n_no_normal = none;
  return listed;
}

}  // extern "C"
