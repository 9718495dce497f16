// icpk_filter.cpp -- host side of the outlier removal (K13; kernels_filter.hip): icpk_remove_outliers computes the
// statistical or the radius filter's per-point value over K1d's index of the cloud, thresholds and compacts on the
// device, and replaces the cloud through the path icpk_set_*_device take; the statistics stay on the device for
// icpk_get_outlier_stats.
#include <cmath>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

// the record of a call on a cloud of n_in points (the contents of a previous call are given up) and the scratch
int ensure_filter_buffers(icpk_ctx* ctx, int n_in, bool normals) {
  ctx->have_flt = false;
  const size_t n = n_in < 1 ? 1 : (size_t)n_in;
  int rc = ctx->flt_value.reserve(ctx, n);
  if (!rc) rc = ctx->flt_kth.reserve(ctx, n);
  if (!rc) rc = ctx->flt_oidx.reserve(ctx, n);
  if (!rc) rc = ctx->flt_summary.reserve(ctx, 4);
  if (!rc) rc = ctx->flt_summary_host.reserve(ctx, 4);
  if (!rc) rc = ctx->flt_partial.reserve(ctx, 2 * (size_t)RED_MAX_BLOCKS);
  if (!rc) rc = ctx->flt_pcount.reserve(ctx, RED_MAX_BLOCKS);
  if (!rc) rc = ctx->flt_bsum.reserve(ctx, (n + 1023) / 1024);
  if (!rc) rc = ctx->flt_counts.reserve(ctx, 2);
  if (!rc) rc = ctx->flt_counts_host.reserve(ctx, 2);
  if (!rc) rc = ctx->flt_out.reserve(ctx, (size_t)(normals ? 6 : 3) * n);
  return rc;
}

}  // namespace

extern "C" {

int icpk_remove_outliers(icpk_ctx* ctx, int32_t which, const icpk_outlier_filter* f, int32_t flags, int32_t* n_out,
                         int32_t* n_dropped) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (!f) return fail(ctx, ICPK_E_ARG, "no filter given");
  if (flags & ~ICPK_FILTER_STATS_ONLY) return fail(ctx, ICPK_E_ARG, "unknown filter flag");
  if (f->kind == ICPK_FILTER_STATISTICAL) {
    if (f->k < 1 || f->k > ICPK_FILTER_MAX_K) return fail(ctx, ICPK_E_ARG, "k must be in 1 .. ICPK_FILTER_MAX_K");
    if (!(f->std_ratio >= 0.f) || !std::isfinite(f->std_ratio))
      return fail(ctx, ICPK_E_ARG, "std_ratio must be finite and >= 0");
  } else if (f->kind == ICPK_FILTER_RADIUS) {
    if (!(f->radius > 0.f) || !std::isfinite(f->radius)) return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0");
    if (f->min_neighbors < 1) return fail(ctx, ICPK_E_ARG, "min_neighbors must be at least 1");
  } else {
    return fail(ctx, ICPK_E_ARG, "unknown filter kind");
  }
  if (which == 0 ? !ctx->have_src : !ctx->have_tgt)
    return fail(ctx, ICPK_E_NOT_SET, which == 0 ? "source cloud not set" : "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (which == 0)
    if (int ru = ensure_unpacked(ctx)) return ru;  // (the call reads the working source)
  const Cloud& in = which == 0 ? ctx->src : ctx->tgt;
  const int n = in.n;
  const bool stats_only = (flags & ICPK_FILTER_STATS_ONLY) != 0;
  const bool normals = which == 1 && ctx->have_normals && !stats_only;
  int rc = ensure_filter_buffers(ctx, n, normals);
  if (rc) return rc;
  int counts[2] = {0, 0};
  float* o = nullptr;
  ICPK_HIP(ctx, hipMemsetAsync(ctx->flt_summary, 0, 4 * sizeof(double), ctx->stream));
  if (n > 0) {
    // the index: the target's own (built here if it has none yet, and then valid for the alignment that follows), or
    // one of the working source in aux_grid (the target's have_grid state is not touched)
    GridView v;
    if ((rc = which == 1 ? index_target(ctx, &v) : index_aux(ctx, ctx->src, &v))) return rc;
    ICPK_HIP(ctx, hipMemsetAsync(ctx->flt_counts, 0, 2 * sizeof(int), ctx->stream));
    if (f->kind == ICPK_FILTER_STATISTICAL) {
      KnnArgs q{};
      q.q4 = v.t4;  // every point against its own cloud
      q.nq = n;
      q.k = f->k;
      q.r0_scale = 2.5f / (3.14159265f * ctx->tune.grid_ppc);
      q.index = v;
      q.mean = ctx->flt_value;
      q.kth = ctx->flt_kth;
      launch_knn_mean(q, ctx->stream);
    } else {
      launch_radius_count(v, n, f->radius, ctx->flt_value, ctx->stream);
    }
    o = ctx->flt_out;
    FilterArgs a{};
    a.x = in.x(), a.y = in.y(), a.z = in.z();
    if (normals) a.nx = ctx->nrm.x(), a.ny = ctx->nrm.y(), a.nz = ctx->nrm.z();
    a.n = n;
    a.kind = f->kind;
    a.min_neighbors = f->min_neighbors;
    a.std_ratio = f->std_ratio;
    a.value = ctx->flt_value;
    a.partial = ctx->flt_partial;
    a.pcount = ctx->flt_pcount;
    a.summary = ctx->flt_summary;
    a.bsum = ctx->flt_bsum;
    a.counts = ctx->flt_counts;
    a.ox = o, a.oy = o + n, a.oz = o + 2 * (size_t)n;
    if (normals) a.onx = o + 3 * (size_t)n, a.ony = o + 4 * (size_t)n, a.onz = o + 5 * (size_t)n;
    a.out_index = ctx->flt_oidx;
    launch_filter_compact(a, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    // the one host wait of the call: the size of the new cloud
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->flt_counts_host, ctx->flt_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    counts[0] = ctx->flt_counts_host[0];
    counts[1] = ctx->flt_counts_host[1];
    if (counts[0] < 0 || counts[0] > n || counts[1] < 0 || counts[1] > n)
      return fail(ctx, ICPK_E_HIP, "outlier filter: impossible output size");
  }
  const int m = counts[0];
  if (!stats_only) {
    // the new cloud takes the way of icpk_set_*_device, which drops everything derived from the old one (the copies
    // out of flt_out are stream-ordered; nothing writes flt_out before the next filter on this stream)
    if (which == 0) {
      rc = set_source_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
    } else {
      rc = set_target_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
      if (!rc && normals) {
        if ((rc = ensure_cloud(ctx, ctx->nrm, m))) return rc;
        const Cloud& c = ctx->nrm;
        float* const planes[3] = {c.x(), c.y(), c.z()};
        for (int k = 0; k < 3; ++k) {
          if (m > 0)
            ICPK_HIP(ctx, hipMemcpyAsync(planes[k], o + (3 + k) * (size_t)n, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice,
                                         ctx->stream));
          launch_fill_f32(planes[k] + m, c.cap - m, 0.f, ctx->stream);
        }
        ICPK_HIP(ctx, hipGetLastError());
        ctx->have_normals = true;
      }
    }
    if (rc) return rc;
  }
  ctx->flt_n_in = n;
  ctx->flt_n_out = m;
  ctx->flt_kind = f->kind;
  ctx->flt_min_neighbors = f->min_neighbors;
  ctx->flt_n_finite = n - counts[1];
  ctx->have_flt = true;
  if (n_out) *n_out = m;
  if (n_dropped) *n_dropped = counts[1];
  return ICPK_OK;
}

int icpk_get_outlier_stats(icpk_ctx* ctx, int32_t* n_in, int32_t* n_out, double* value, float* kth, int32_t* out_index,
                           double summary[4]) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_flt) return fail(ctx, ICPK_E_NOT_SET, "no outlier filter has run on this context");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->flt_n_in;
  const bool stat = ctx->flt_kind == ICPK_FILTER_STATISTICAL;
  if (value && n) ICPK_HIP(ctx, hipMemcpyAsync(value, ctx->flt_value, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (kth && n && stat) ICPK_HIP(ctx, hipMemcpyAsync(kth, ctx->flt_kth, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (out_index && n)
    ICPK_HIP(ctx, hipMemcpyAsync(out_index, ctx->flt_oidx, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (summary && stat)
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->flt_summary_host, ctx->flt_summary, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_in) *n_in = ctx->flt_n_in;
  if (n_out) *n_out = ctx->flt_n_out;
  if (summary) {
    if (stat) {
      for (int k = 0; k < 4; ++k) summary[k] = ctx->flt_summary_host[k];
    } else {
      summary[0] = (double)ctx->flt_n_finite, summary[1] = 0.0, summary[2] = 0.0;
      summary[3] = (double)ctx->flt_min_neighbors;
    }
  }
  return ICPK_OK;
}

}  // extern "C"
