// icpk_normals.cpp -- host side of the target normals from the target's own geometry (K12; kernels_normals.hip):
// icpk_estimate_target_normals fits a plane to every target point's neighbours within a radius and writes the normals
// where icpk_set_target_normals would; the per-point counts, curvatures and moments stay on the device for
// icpk_get_normal_stats.
#include <cmath>

#include "icpk_ctx.h"

using namespace icpk;

extern "C" {

int icpk_estimate_target_normals(icpk_ctx* ctx, float radius, int32_t min_neighbors, const float viewpoint[3],
                                 int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (!(radius > 0.f) || !std::isfinite(radius)) return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0");
  if (min_neighbors < 3) return fail(ctx, ICPK_E_ARG, "min_neighbors must be at least 3");
  if (flags & ~ICPK_NORMALS_KEEP_MOMENTS) return fail(ctx, ICPK_E_ARG, "unknown normals flag");
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ctx->have_nstats = false;
  fpfh_dropped(ctx, 1);
  const int n = ctx->tgt.n;
  const size_t cap = n < 1 ? 1 : (size_t)n;
  int rc = ctx->nrm_moments.reserve(ctx, cap * NRM_MOMENTS);
  if (!rc) rc = ctx->nrm_count.reserve(ctx, cap);
  if (!rc) rc = ctx->nrm_curv.reserve(ctx, cap);
  if (!rc) rc = ctx->nrm_valid.reserve(ctx, 1);
  if (!rc) rc = ctx->nrm_valid_host.reserve(ctx, 1);
  if (!rc) rc = ensure_cloud(ctx, ctx->nrm, n);
  if (rc) return rc;
  ctx->have_normals = false;  // (the planes are about to be rewritten)
  const Cloud& c = ctx->nrm;
  ICPK_HIP(ctx, hipMemsetAsync(ctx->nrm_valid, 0, sizeof(int), ctx->stream));
  if (n > 0) {
    // K1d's index of the target: built here if the target has none yet, and then valid for the alignment that follows
    GridView v;
    if ((rc = index_target(ctx, &v))) return rc;
    NormalsArgs a{};
    a.index = v;
    a.x = ctx->tgt.x(), a.y = ctx->tgt.y(), a.z = ctx->tgt.z();
    a.n = n;
    a.radius = radius;
    a.min_neighbors = min_neighbors;
    a.has_viewpoint = viewpoint != nullptr;
    for (int k = 0; k < 3; ++k) a.viewpoint[k] = viewpoint ? viewpoint[k] : 0.f;
    a.moments = ctx->nrm_moments;
    a.nx = c.x(), a.ny = c.y(), a.nz = c.z();
    a.count = ctx->nrm_count;
    a.curvature = ctx->nrm_curv;
    a.n_valid = ctx->nrm_valid;
    launch_estimate_normals(a, ctx->stream);
  }
  float* const planes[3] = {c.x(), c.y(), c.z()};
  for (int k = 0; k < 3; ++k) launch_fill_f32(planes[k] + n, c.cap - n, 0.f, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_normals = true;
  ctx->nstats_n = n;
  ctx->nstats_moments = (flags & ICPK_NORMALS_KEEP_MOMENTS) != 0;
  ctx->have_nstats = true;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_normal_stats(icpk_ctx* ctx, int32_t* n, int32_t* n_valid, int32_t* count, float* curvature,
                          int64_t* moments) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_nstats) return fail(ctx, ICPK_E_NOT_SET, "no normals estimated for the current target");
  if (moments && !ctx->nstats_moments)
    return fail(ctx, ICPK_E_ARG, "the moments were not kept (ICPK_NORMALS_KEEP_MOMENTS)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)ctx->nstats_n;
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->nrm_valid_host, ctx->nrm_valid, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (count && m) ICPK_HIP(ctx, hipMemcpyAsync(count, ctx->nrm_count, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (curvature && m)
    ICPK_HIP(ctx, hipMemcpyAsync(curvature, ctx->nrm_curv, m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (moments && m)
    ICPK_HIP(ctx, hipMemcpyAsync(moments, ctx->nrm_moments, m * NRM_MOMENTS * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = ctx->nstats_n;
  if (n_valid) *n_valid = ctx->nrm_valid_host[0];
  return ICPK_OK;
}

}  // extern "C"
