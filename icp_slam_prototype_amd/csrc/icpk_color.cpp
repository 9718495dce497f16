// icpk_color.cpp -- host side of colored ICP (K17; kernels_color.hip): one intensity per point of the target and of the
// uploaded source, the target's colour gradients (icpk_estimate_target_color_gradients), the setting
// (icpk_set_colored) and the test hook icpk_reduce_colored.  The loop itself is icpk_align's (icpk_align.cpp): the
// point-to-plane path with another reduction.
#include <cmath>
#include <cstring>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

// every value finite and in [0, 1]: the bound the integer sums of the gradient estimate rest on
bool intensities_ok(const float* v, int32_t n) {
  for (int32_t i = 0; i < n; ++i)
    if (!(v[i] >= 0.f && v[i] <= 1.f)) return false;  // (false for NaN)
  return true;
}

int upload_colors(icpk_ctx* ctx, DevBuf<float>& buf, const float* v, int32_t n) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = buf.reserve(ctx, n < 1 ? 1 : (size_t)n)) return rc;
  if (n > 0) ICPK_HIP(ctx, hipMemcpyAsync(buf, v, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the host array is the caller's again)
  return ICPK_OK;
}

int download_colors(icpk_ctx* ctx, const DevBuf<float>& buf, float* v, int32_t n) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (n > 0) ICPK_HIP(ctx, hipMemcpyAsync(v, buf, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

}  // namespace

extern "C" {

void icpk_intensity_from_bgr(const uint8_t* bgr, int32_t n, float* out) {
  if (!bgr || !out) return;
  for (int32_t i = 0; i < n; ++i)
    out[i] = (float)(((double)bgr[3 * (size_t)i] + (double)bgr[3 * (size_t)i + 1] + (double)bgr[3 * (size_t)i + 2]) / 765.0);
}

int icpk_set_target_colors(icpk_ctx* ctx, const float* intensity, int32_t n) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  if (n != ctx->tgt.n) return fail(ctx, ICPK_E_ARG, "intensity count differs from the target size");
  if (n > 0 && !intensity) return fail(ctx, ICPK_E_ARG, "bad intensity pointer");
  if (!intensities_ok(intensity, n)) return fail(ctx, ICPK_E_ARG, "intensities must be finite and in [0, 1]");
  ctx->have_tgt_colors = false;
  ctx->have_color_gradients = false;  // (they describe the intensities that are being replaced)
  ctx->have_cg_sums = false;
  if (int rc = upload_colors(ctx, ctx->tcol, intensity, n)) return rc;
  ctx->have_tgt_colors = true;
  return ICPK_OK;
}

int icpk_set_source_colors(icpk_ctx* ctx, const float* intensity, int32_t n) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  if (n != ctx->src0.n) return fail(ctx, ICPK_E_ARG, "intensity count differs from the source size");
  if (n > 0 && !intensity) return fail(ctx, ICPK_E_ARG, "bad intensity pointer");
  if (!intensities_ok(intensity, n)) return fail(ctx, ICPK_E_ARG, "intensities must be finite and in [0, 1]");
  ctx->have_src_colors = false;
  if (int rc = upload_colors(ctx, ctx->scol, intensity, n)) return rc;
  ctx->have_src_colors = true;
  return ICPK_OK;
}

int icpk_get_target_colors(icpk_ctx* ctx, float* intensity) {
  if (!ctx || !intensity) return ICPK_E_ARG;
  if (!ctx->have_tgt_colors) return fail(ctx, ICPK_E_NOT_SET, "no target colours");
  return download_colors(ctx, ctx->tcol, intensity, ctx->tgt.n);
}

int icpk_get_source_colors(icpk_ctx* ctx, float* intensity) {
  if (!ctx || !intensity) return ICPK_E_ARG;
  if (!ctx->have_src_colors) return fail(ctx, ICPK_E_NOT_SET, "no source colours");
  return download_colors(ctx, ctx->scol, intensity, ctx->src0.n);
}

int icpk_estimate_target_color_gradients(icpk_ctx* ctx, float radius, int32_t min_neighbors, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (!(radius > 0.f) || !std::isfinite(radius)) return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0");
  if (min_neighbors < 1) return fail(ctx, ICPK_E_ARG, "min_neighbors must be at least 1");
  if (flags & ~ICPK_COLOR_KEEP_SUMS) return fail(ctx, ICPK_E_ARG, "unknown colour gradient flag");
  if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  if (!ctx->have_normals) return fail(ctx, ICPK_E_NOT_SET, "no target normals");
  if (!ctx->have_tgt_colors) return fail(ctx, ICPK_E_NOT_SET, "no target colours");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int n = ctx->tgt.n;
  const size_t cap = n < 1 ? 1 : (size_t)n;
  int rc = ctx->cg_sums.reserve(ctx, cap * COLOR_SUMS);
  if (!rc) rc = ctx->tcol_sorted.reserve(ctx, cap);
  if (!rc) rc = ensure_cloud(ctx, ctx->cgrad, n);
  if (rc) return rc;
  ctx->have_color_gradients = false;  // (the planes are about to be rewritten)
  ctx->have_cg_sums = false;
  const Cloud& c = ctx->cgrad;
  if (n > 0) {
    // K1d's index of the target: built here if the target has none yet, and then valid for the alignment that follows
    GridView v;
    if ((rc = index_target(ctx, &v))) return rc;
    ColorGradArgs a{};
    a.index = v;
    a.nx = ctx->nrm.x(), a.ny = ctx->nrm.y(), a.nz = ctx->nrm.z();
    a.col = ctx->tcol;
    a.col_sorted = ctx->tcol_sorted;
    a.n = n;
    a.radius = radius;
    a.min_neighbors = min_neighbors;
    a.sums = ctx->cg_sums;
    a.gx = c.x(), a.gy = c.y(), a.gz = c.z();
    launch_color_gradients(a, ctx->stream);
  }
  float* const planes[3] = {c.x(), c.y(), c.z()};
  for (int k = 0; k < 3; ++k) launch_fill_f32(planes[k] + n, c.cap - n, 0.f, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_color_gradients = true;
  ctx->have_cg_sums = (flags & ICPK_COLOR_KEEP_SUMS) != 0;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_target_color_gradients(icpk_ctx* ctx, float* gx, float* gy, float* gz) {
  if (!ctx || !gx || !gy || !gz) return ICPK_E_ARG;
  if (!ctx->have_color_gradients) return fail(ctx, ICPK_E_NOT_SET, "no target colour gradients");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const Cloud& c = ctx->cgrad;
  const size_t b = (size_t)ctx->tgt.n * sizeof(float);
  if (b) {
    ICPK_HIP(ctx, hipMemcpyAsync(gx, c.x(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(gy, c.y(), b, hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(gz, c.z(), b, hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_get_color_gradient_sums(icpk_ctx* ctx, int64_t* sums) {
  if (!ctx || !sums) return ICPK_E_ARG;
  if (!ctx->have_cg_sums)
    return fail(ctx, ICPK_E_NOT_SET, "no colour gradient sums kept for the current target (ICPK_COLOR_KEEP_SUMS)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t b = (size_t)ctx->tgt.n * COLOR_SUMS * sizeof(int64_t);
  if (b) ICPK_HIP(ctx, hipMemcpyAsync(sums, ctx->cg_sums, b, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_set_colored(icpk_ctx* ctx, int32_t on, float lambda_geometric) {
  if (!ctx) return ICPK_E_ARG;
  if (!std::isfinite(lambda_geometric) || !(lambda_geometric >= 0.f && lambda_geometric <= 1.f))
    return fail(ctx, ICPK_E_ARG, "lambda_geometric must be finite and in [0, 1]");
  ctx->colored_on = on != 0;
  ctx->lambda_geometric = lambda_geometric;
  return ICPK_OK;
}

int icpk_reduce_colored(icpk_ctx* ctx, float max_dist, double sums[28], int64_t* count) {
  if (!ctx || !sums) return ICPK_E_ARG;
  if (!ctx->have_assoc) return fail(ctx, ICPK_E_NOT_SET, "no nearest-neighbour sweep has run");
  if (!ctx->have_normals || !ctx->have_src_colors || !ctx->have_tgt_colors || !ctx->have_color_gradients)
    return fail(ctx, ICPK_E_NOT_SET, "colored ICP needs target normals, both clouds' colours and the target's colour gradients");
  if (ctx->src.n != ctx->src0.n) return fail(ctx, ICPK_E_ARG, "the working source differs in size from the uploaded one");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  if (ctx->src.n == 0) {
    std::memset(sums, 0, NP2L * sizeof(double));
    if (count) *count = 0;
    return ICPK_OK;
  }
  const int rc = enqueue_reduce_colored(ctx, max_dist);
  if (rc) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(sums, ctx->red_host, NP2L * sizeof(double));
  if (count) std::memcpy(count, ctx->red_host + NP2L, sizeof(int64_t));
  return ICPK_OK;
}

}  // extern "C"
