// icpk_gicp.cpp -- host side of the plane-to-plane flavour (ICPK_SOLVE_PLANE_TO_PLANE, K14; kernels_gicp.hip): the
// normals of the uploaded source (estimated by K12's kernels over an index of the source in the context's aux_grid, or
// taken from the host), the epsilon setting and the test hook icpk_reduce_plane_to_plane.  The loop itself is
// icpk_align's (icpk_align.cpp).
#include <cmath>
#include <cstring>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

// the planes of ctx->snrm beyond n, up to the capacity: zero (no normal)
int pad_source_normals(icpk_ctx* ctx, int n) {
  const Cloud& c = ctx->snrm;
  float* const planes[3] = {c.x(), c.y(), c.z()};
  for (int k = 0; k < 3; ++k) launch_fill_f32(planes[k] + n, c.cap - n, 0.f, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

}  // namespace

extern "C" {

int icpk_estimate_source_normals(icpk_ctx* ctx, float radius, int32_t min_neighbors, const float viewpoint[3],
                                 int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (!(radius > 0.f) || !std::isfinite(radius)) return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0");
  if (min_neighbors < 3) return fail(ctx, ICPK_E_ARG, "min_neighbors must be at least 3");
  if (flags != 0) return fail(ctx, ICPK_E_ARG, "unknown normals flag");
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int n = ctx->src0.n;
  const size_t cap = n < 1 ? 1 : (size_t)n;
  int rc = ctx->sn_moments.reserve(ctx, cap * NRM_MOMENTS);
  if (!rc) rc = ctx->sn_count.reserve(ctx, cap);
  if (!rc) rc = ctx->sn_curv.reserve(ctx, cap);
  if (!rc) rc = ctx->sn_valid.reserve(ctx, 1);
  if (!rc) rc = ensure_cloud(ctx, ctx->snrm, n);
  if (rc) return rc;
  ctx->have_src_normals = false;  // (the planes are about to be rewritten)
  fpfh_dropped(ctx, 0);
  const Cloud& c = ctx->snrm;
  if (n > 0) {
    GridView v;  // (the uploaded source's index, in aux_grid: the target's is not disturbed)
    if ((rc = index_aux(ctx, ctx->src0, &v))) return rc;
    ICPK_HIP(ctx, hipMemsetAsync(ctx->sn_valid, 0, sizeof(int), ctx->stream));
    NormalsArgs a{};
    a.index = v;
    a.x = ctx->src0.x(), a.y = ctx->src0.y(), a.z = ctx->src0.z();
    a.n = n;
    a.radius = radius;
    a.min_neighbors = min_neighbors;
    a.has_viewpoint = viewpoint != nullptr;
    for (int k = 0; k < 3; ++k) a.viewpoint[k] = viewpoint ? viewpoint[k] : 0.f;
    a.moments = ctx->sn_moments;
    a.nx = c.x(), a.ny = c.y(), a.nz = c.z();
    a.count = ctx->sn_count;
    a.curvature = ctx->sn_curv;
    a.n_valid = ctx->sn_valid;
    launch_estimate_normals(a, ctx->stream);  // K12's two kernels, K12's rule
  }
  if ((rc = pad_source_normals(ctx, n))) return rc;
  ctx->have_src_normals = true;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_set_source_normals(icpk_ctx* ctx, const float* nx, const float* ny, const float* nz, int32_t n) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  if (n != ctx->src0.n) return fail(ctx, ICPK_E_ARG, "normal count differs from the source size");
  if (n > 0 && (!nx || !ny || !nz)) return fail(ctx, ICPK_E_ARG, "bad normal pointers");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_cloud(ctx, ctx->snrm, n);
  if (rc) return rc;
  ctx->have_src_normals = false;
  fpfh_dropped(ctx, 0);
  const Cloud& c = ctx->snrm;
  const float* const from[3] = {nx, ny, nz};
  float* const planes[3] = {c.x(), c.y(), c.z()};
  for (int k = 0; k < 3; ++k)
    if (n > 0) ICPK_HIP(ctx, hipMemcpyAsync(planes[k], from[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = pad_source_normals(ctx, n))) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the host arrays are the caller's again)
  ctx->have_src_normals = true;
  return ICPK_OK;
}

int icpk_get_source_normals(icpk_ctx* ctx, float* nx, float* ny, float* nz) {
  if (!ctx || !nx || !ny || !nz) return ICPK_E_ARG;
  if (!ctx->have_src_normals) return fail(ctx, ICPK_E_NOT_SET, "no source normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const Cloud& c = ctx->snrm;
  const size_t b = (size_t)ctx->src0.n * sizeof(float);
  if (b) {
    ICPK_HIP(ctx, hipMemcpyAsync(nx, c.x(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(ny, c.y(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(nz, c.z(), b, hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_set_plane_to_plane(icpk_ctx* ctx, float epsilon) {
  if (!ctx) return ICPK_E_ARG;
  if (!std::isfinite(epsilon) || !(epsilon > 0.f && epsilon <= 1.f))
    return fail(ctx, ICPK_E_ARG, "epsilon must be finite and in (0, 1]");
  ctx->gicp_epsilon = epsilon;
  return ICPK_OK;
}

int icpk_reduce_plane_to_plane(icpk_ctx* ctx, float max_dist, const float R_acc[9], double sums[28], int64_t* count) {
  if (!ctx || !sums) return ICPK_E_ARG;
  if (!ctx->have_assoc) return fail(ctx, ICPK_E_NOT_SET, "no nearest-neighbour sweep has run");
  if (!ctx->have_normals || !ctx->have_src_normals)
    return fail(ctx, ICPK_E_NOT_SET, "plane-to-plane needs source and target normals");
  if (ctx->src.n != ctx->src0.n) return fail(ctx, ICPK_E_ARG, "the working source differs in size from the uploaded one");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  if (ctx->src.n == 0) {
    std::memset(sums, 0, NP2L * sizeof(double));
    if (count) *count = 0;
    return ICPK_OK;
  }
  const int rc = enqueue_reduce_gicp(ctx, max_dist, R_acc);
  if (rc) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(sums, ctx->red_host, NP2L * sizeof(double));
  if (count) std::memcpy(count, ctx->red_host + NP2L, sizeof(int64_t));
  return ICPK_OK;
}

}  // extern "C"
