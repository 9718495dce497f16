// icpk_sdf_track.cpp -- K29, host side of tracking depth frames directly against the TSDF (include/icpk.h, THE SDF
// TRACKING RULE; kernels_sdf_track.hip): the defaults, the refusals, the rule over host arrays through the header the
// kernel includes (icpk_sdf_pixels -- the host-only half: it needs no context and no device), and the three entry points
// that run on the device over a level of the resident pyramid (K24) and the volume's two planes (K19) with its current
// origin (K23).  They read both where they lie and write only the scratch the context keeps for THIS family: the loop's
// state block has K25's type and its step launch is K25's, but the block, the partials and the trace are their own, so
// that the record of the last icpk_align_projective stays as it was.
#include <cmath>
#include <cstring>

#include "icpk_ctx.h"
#include "sdf_track_rule.h"

using namespace icpk;

static_assert(SDF_NO_DEPTH == ICPK_SDF_NO_DEPTH && SDF_OUTSIDE == ICPK_SDF_OUTSIDE && SDF_UNKNOWN == ICPK_SDF_UNKNOWN &&
                  SDF_TOO_FAR == ICPK_SDF_TOO_FAR && SDF_NO_GRADIENT == ICPK_SDF_NO_GRADIENT &&
                  SDF_NO_NORMAL == ICPK_SDF_NO_NORMAL && SDF_NORMAL == ICPK_SDF_NORMAL,
              "the rule's codes are the header's");
static_assert(sizeof(icpk_projective_iter) == sizeof(ProjIter), "the device writes the trace in the ABI's layout");
static_assert(ICPK_TSDF_MAX_VOXELS <= (1 << 30), "an accepted pixel's cell index fits an int32 below 2^30");

namespace {

// nullptr: fine; else what is wrong (the refusals that need no context)
const char* check_params(const icpk_sdf_params& p, const double* pose) {
  if (!pose) return "the pose is NULL";
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return "the pose is not finite";
  if (p.level < 0 || p.level >= ICPK_PYRAMID_MAX_LEVELS) return "a level the pyramid does not have";
  if (!(std::isfinite(p.fx) && p.fx > 0.f) || !std::isfinite(p.cx)) return "fx must be finite and > 0, cx finite";
  if (!(p.max_abs_tsdf > 0.f && p.max_abs_tsdf <= 1.f)) return "max_abs_tsdf must be in (0, 1]";
  if (p.min_weight < 1 || p.min_weight > 65535) return "min_weight outside 1 .. 65535";
  if (p.min_normal_cos != p.min_normal_cos) return "min_normal_cos is NaN";
  if (p.min_pairs < 1) return "min_pairs < 1";
  if (p.max_iterations < 1 || p.max_iterations > ICPK_PROJECTIVE_MAX_ITERATIONS)
    return "max_iterations outside 1 .. ICPK_PROJECTIVE_MAX_ITERATIONS";
  return nullptr;
}

icpk_sdf_params params_or_defaults(const icpk_sdf_params* params) {
  icpk_sdf_params p;
  icpk_default_sdf_params(&p);
  if (params) p = *params;
  return p;
}

TsdfPlanes planes_of(const icpk_tsdf_params& t, const float* tsdf, const uint16_t* weight, int min_weight) {
  TsdfPlanes v{};
  v.tsdf = tsdf, v.weight = weight, v.intensity = nullptr;
  for (int k = 0; k < 3; ++k) v.dims[k] = t.dims[k], v.origin[k] = t.origin[k];
  v.voxel = t.voxel;
  v.min_weight = min_weight;
  return v;
}

// Everything a device call needs, checked in the header's order of refusals: nothing of the context has changed when
// this fails.  a.partial / a.pcount / a.st are left for begin_state.
int prepare(icpk_ctx* ctx, const icpk_sdf_params& p, const double* pose, SdfArgs* a) {
  if (const char* why = check_params(p, pose)) return fail(ctx, ICPK_E_ARG, why);
  TsdfVolumeView vol;
  if (int rc = tsdf_volume_view(ctx, &vol)) return rc;
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  if (p.level >= ctx->pyr_levels) return fail(ctx, ICPK_E_ARG, "a level the pyramid does not have");
  const float scale = (float)(1 << p.level);  // (a power of two: both quotients are exact)
  a->depth = ctx->pyr + ctx->pyr_off[p.level];
  a->rows = ctx->pyr_rows[p.level], a->cols = ctx->pyr_cols[p.level];
  a->fx = p.fx / scale, a->cx = p.cx / scale;
  a->vol = planes_of(vol.p, vol.tsdf, vol.weight, p.min_weight);
  a->trunc = vol.p.trunc, a->max_abs_tsdf = p.max_abs_tsdf, a->min_normal_cos = p.min_normal_cos;
  return ICPK_OK;
}

// the scratch of the reduction and the loop's block; E_0 into the block's staging copy and on its way to the device
int begin_state(icpk_ctx* ctx, const double pose[16], SdfArgs* a) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ctx->sdf_partial.reserve(ctx, (size_t)NP2L * RED_MAX_BLOCKS)) return rc;
  if (int rc = ctx->sdf_pcount.reserve(ctx, RED_MAX_BLOCKS)) return rc;
  if (int rc = ctx->sdf_out.reserve(ctx, NP2L + 1)) return rc;
  if (int rc = ctx->sdf_out_host.reserve(ctx, NP2L + 1)) return rc;
  if (int rc = ctx->sdf_block.reserve(ctx, 1)) return rc;
  if (int rc = ctx->sdf_block_host.reserve(ctx, 1)) return rc;
  ProjState& st = ctx->sdf_block_host.get()->st;
  std::memset(&st, 0, sizeof(st));
  proj_round_pose(pose, st.R, st.t);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) st.E[4 * r + c] = pose[4 * r + c];
  // (the staging copy is read by this copy alone, and every call ends with a wait on the stream)
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->sdf_block.get(), &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  a->partial = ctx->sdf_partial, a->pcount = ctx->sdf_pcount;
  a->st = &ctx->sdf_block.get()->st;
  return ICPK_OK;
}

}  // namespace

extern "C" {

void icpk_default_sdf_params(icpk_sdf_params* p) {
  if (!p) return;
  p->level = 0;
  p->fx = 468.60f, p->cx = 318.27f;
  p->max_iterations = 10;
  p->max_abs_tsdf = 1.0f;
  p->min_weight = 1;
  p->min_normal_cos = -2.f;
  p->min_pairs = 6;
}

int icpk_sdf_pixels(const icpk_sdf_params* params, const icpk_tsdf_params* volume, const double pose[16],
                    const uint16_t* level, int32_t rows_s, int32_t cols_s, const float* tsdf, const uint16_t* weight,
                    int64_t first, int32_t count, int32_t* cell, float* value, double* terms) {
  if (!volume || !level || !tsdf || !weight || !cell || !value || count < 0 || first < 0) return ICPK_E_ARG;
  const icpk_sdf_params p = params_or_defaults(params);
  if (check_params(p, pose)) return ICPK_E_ARG;
  long long n = 1;
  for (int a = 0; a < 3; ++a) {
    if (volume->dims[a] < 1) return ICPK_E_ARG;
    n *= volume->dims[a];  // (each factor < 2^31 and the running product is checked: no overflow)
    if (n > ICPK_TSDF_MAX_VOXELS || !std::isfinite(volume->origin[a])) return ICPK_E_ARG;
  }
  if (!(std::isfinite(volume->voxel) && volume->voxel > 0.f) || !(std::isfinite(volume->trunc) && volume->trunc > 0.f))
    return ICPK_E_ARG;
  if (rows_s < 1 || cols_s < 1 || (int64_t)rows_s * cols_s > (1 << 28)) return ICPK_E_ARG;
  if (first + count > (int64_t)rows_s * cols_s) return ICPK_E_ARG;
  const float scale = (float)(1 << p.level);
  const ProjLevel lv{level, rows_s, cols_s, p.fx / scale, p.cx / scale};
  const TsdfPlanes vol = planes_of(*volume, tsdf, weight, p.min_weight);
  ProjPose E;
  proj_round_pose(pose, E.R, E.t);
  const SdfGate g{volume->trunc, p.max_abs_tsdf, p.min_normal_cos};
  const bool with_normal = p.min_normal_cos > -1.f;
  int accepted = 0;
  for (int32_t e = 0; e < count; ++e) {
    const int64_t i = first + e;
    const int r = (int)(i / cols_s), c = (int)(i % cols_s);
    SdfHit h;
    const int at = with_normal ? sdf_pixel<true>(lv, vol, E, g, r, c, level[i], &h)
                               : sdf_pixel<false>(lv, vol, E, g, r, c, level[i], &h);
    cell[e] = at;
    value[e] = at >= 0 ? h.D : 0.f;
    accepted += at >= 0;
    if (terms) {
      double v[28] = {0.0};
      if (at >= 0) sdf_add_terms(h, v);
      std::memcpy(terms + (size_t)e * 28, v, sizeof(v));
    }
  }
  return accepted;
}

int icpk_sdf_associate(icpk_ctx* ctx, const icpk_sdf_params* params, const double pose[16], int32_t* cell, float* value) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_sdf_params p = params_or_defaults(params);
  SdfArgs a{};
  if (int rc = prepare(ctx, p, pose, &a)) return rc;
  if (int rc = begin_state(ctx, pose, &a)) return rc;
  const size_t npix = (size_t)a.rows * a.cols;
  if (int rc = ctx->sdf_cell.reserve(ctx, npix)) return rc;
  if (int rc = ctx->sdf_value.reserve(ctx, npix)) return rc;
  launch_sdf_associate(a, ctx->sdf_cell, ctx->sdf_value, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  if (cell)
    ICPK_HIP(ctx, hipMemcpyAsync(cell, ctx->sdf_cell.get(), npix * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (value)
    ICPK_HIP(ctx, hipMemcpyAsync(value, ctx->sdf_value.get(), npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_sdf_reduce(icpk_ctx* ctx, const icpk_sdf_params* params, const double pose[16], double sums[28], int64_t* count) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_sdf_params p = params_or_defaults(params);
  SdfArgs a{};
  if (int rc = prepare(ctx, p, pose, &a)) return rc;
  if (int rc = begin_state(ctx, pose, &a)) return rc;
  launch_sdf_reduce(a, ctx->stream);
  launch_reduce_final(a.partial, a.pcount, red_blocks(a.rows * a.cols), NP2L, ctx->sdf_out, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->sdf_out_host.get(), ctx->sdf_out.get(), (NP2L + 1) * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (sums) std::memcpy(sums, ctx->sdf_out_host.get(), NP2L * sizeof(double));
  if (count) std::memcpy(count, ctx->sdf_out_host.get() + NP2L, sizeof(int64_t));
  return ICPK_OK;
}

int icpk_align_sdf(icpk_ctx* ctx, const icpk_sdf_params* params, const double pose_in[16], double pose_out[16],
                   icpk_projective_result* result) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_sdf_params p = params_or_defaults(params);
  SdfArgs a{};
  if (int rc = prepare(ctx, p, pose_in, &a)) return rc;
  if (int rc = begin_state(ctx, pose_in, &a)) return rc;
  // every launch of every iteration up front; once the state says done the rest are no-ops
  const int B = red_blocks(a.rows * a.cols);
  for (int k = 0; k < p.max_iterations; ++k) {
    launch_sdf_reduce(a, ctx->stream);
    launch_proj_step(a.partial, a.pcount, B, ctx->sdf_block, k, p.min_pairs, ctx->stream);
  }
  ICPK_HIP(ctx, hipGetLastError());
  // one copy (state + the trace entries that can have been written) and one wait
  ProjBlock* h = ctx->sdf_block_host;
  const size_t bytes = offsetof(ProjBlock, trace) + (size_t)p.max_iterations * sizeof(ProjIter);
  ICPK_HIP(ctx, hipMemcpyAsync(h, ctx->sdf_block.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int evaluated = h->st.done ? h->st.iterations + 1 : h->st.iterations;
  ctx->sdf_trace.resize((size_t)evaluated);
  if (evaluated > 0) std::memcpy(ctx->sdf_trace.data(), h->trace, (size_t)evaluated * sizeof(ProjIter));
  if (pose_out) {
    std::memcpy(pose_out, h->st.E, 12 * sizeof(double));
    pose_out[12] = pose_out[13] = pose_out[14] = 0.0, pose_out[15] = 1.0;
  }
  if (result) {
    const ProjIter& last = h->trace[evaluated - 1];  // (max_iterations >= 1: at least one was evaluated)
    result->status = h->st.status;
    result->iterations = h->st.iterations;
    result->count = last.count;
    result->mean_dist = last.count > 0 ? last.sums[27] / (double)last.count : 0.0;
  }
  return h->st.status;
}

int icpk_get_sdf_trace(icpk_ctx* ctx, icpk_projective_iter* out, int32_t cap) {
  if (!ctx || cap < 0 || (cap > 0 && !out)) return ICPK_E_ARG;
  const size_t n = ctx->sdf_trace.size() < (size_t)cap ? ctx->sdf_trace.size() : (size_t)cap;
  if (n) std::memcpy(out, ctx->sdf_trace.data(), n * sizeof(icpk_projective_iter));
  return (int)n;
}

}  // extern "C"
