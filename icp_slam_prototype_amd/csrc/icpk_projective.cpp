// icpk_projective.cpp -- K25, host side of the projective frame-to-model alignment (include/icpk.h, THE PROJECTIVE RULE;
// kernels_projective.hip): the defaults, the refusals, the rule over host images through the header the kernel includes
// (icpk_projective_pixels -- the host-only half: it needs no context and no device), and the three entry points that
// run on the device over a level of the resident pyramid (K24) and the maps of the last ray cast (K20) -- or, when
// icpk_projective_set_view says so, a level of the frame view (K28; icpk_frame_view.cpp resolves which).  They read
// both where they lie and write only the scratch the context keeps for them.  K26's coloured entry points
// (icpk_projective_reduce_colored, icpk_align_projective_colored, icpk_projective_pixels_colored) share every line with
// them but the refusals of their own and the choice of rule 9.
#include <cmath>
#include <cstring>
#include <vector>

#include "icpk_ctx.h"
#include "projective_rule.h"

using namespace icpk;

static_assert(sizeof(icpk_projective_iter) == sizeof(ProjIter) && offsetof(icpk_projective_iter, sums) == offsetof(ProjIter, sums) &&
                  offsetof(icpk_projective_iter, count) == offsetof(ProjIter, count) &&
                  offsetof(icpk_projective_iter, status) == offsetof(ProjIter, status),
              "the device writes the trace in the ABI's layout");
static_assert(PROJ_MAX_ITER == ICPK_PROJECTIVE_MAX_ITERATIONS && PROJ_NO_DEPTH == ICPK_PROJ_NO_DEPTH &&
                  PROJ_BEHIND == ICPK_PROJ_BEHIND && PROJ_OUTSIDE == ICPK_PROJ_OUTSIDE && PROJ_NO_MODEL == ICPK_PROJ_NO_MODEL &&
                  PROJ_TOO_FAR == ICPK_PROJ_TOO_FAR && PROJ_NO_NORMAL == ICPK_PROJ_NO_NORMAL && PROJ_NORMAL == ICPK_PROJ_NORMAL,
              "the rule's codes are the header's");

namespace {

// nullptr: fine; else what is wrong (the refusals that need no context)
const char* check_params(const icpk_projective_params& p, const double* pose) {
  if (!pose) return "the pose is NULL";
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return "the pose is not finite";
  if (p.level < 0 || p.level >= ICPK_PYRAMID_MAX_LEVELS) return "a level the pyramid does not have";
  if (!(std::isfinite(p.fx) && p.fx > 0.f) || !std::isfinite(p.cx)) return "fx must be finite and > 0, cx finite";
  if (!(p.max_dist > 0.f)) return "max_dist must be > 0";
  if (p.min_normal_cos != p.min_normal_cos) return "min_normal_cos is NaN";
  if (p.min_pairs < 1) return "min_pairs < 1";
  if (p.max_iterations < 1 || p.max_iterations > ICPK_PROJECTIVE_MAX_ITERATIONS)
    return "max_iterations outside 1 .. ICPK_PROJECTIVE_MAX_ITERATIONS";
  return nullptr;
}

icpk_projective_params params_or_defaults(const icpk_projective_params* params) {
  icpk_projective_params p;
  icpk_default_projective_params(&p);
  if (params) p = *params;
  return p;
}

// Everything a device call needs, checked in the header's order of refusals: nothing of the context has changed when
// this fails.  a.partial / a.pcount / a.st are left for the caller.
int prepare(icpk_ctx* ctx, const icpk_projective_params& p, const double* pose, ProjArgs* a) {
  if (const char* why = check_params(p, pose)) return fail(ctx, ICPK_E_ARG, why);
  TsdfRayView view;
  if (int rc = projective_view(ctx, &view)) return rc;  // (K28: the ray cast's planes, or a level of the frame view)
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  if (p.level >= ctx->pyr_levels) return fail(ctx, ICPK_E_ARG, "a level the pyramid does not have");
  const float scale = (float)(1 << p.level);  // (a power of two: both quotients are exact)
  a->depth = ctx->pyr + ctx->pyr_off[p.level];
  a->rows = ctx->pyr_rows[p.level], a->cols = ctx->pyr_cols[p.level];
  a->fx = p.fx / scale, a->cx = p.cx / scale;
  a->maps = view.maps;
  a->rows_v = view.rows, a->cols_v = view.cols, a->fx_v = view.fx, a->cx_v = view.cx;
  if (icpk_tsdf_invert_pose(view.pose, a->Q, a->s) != ICPK_OK) return fail(ctx, ICPK_E_ARG, "the view's pose is not finite");
  a->max_dist = p.max_dist, a->min_normal_cos = p.min_normal_cos;
  return ICPK_OK;
}

// the scratch of the reduction and the loop's block; E_0 into the block's staging copy and on its way to the device
int begin_state(icpk_ctx* ctx, const double pose[16], ProjArgs* a) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = ctx->proj_partial.reserve(ctx, (size_t)NP2L * RED_MAX_BLOCKS)) return rc;
  if (int rc = ctx->proj_pcount.reserve(ctx, RED_MAX_BLOCKS)) return rc;
  if (int rc = ctx->proj_out.reserve(ctx, NP2L + 1)) return rc;
  if (int rc = ctx->proj_out_host.reserve(ctx, NP2L + 1)) return rc;
  if (int rc = ctx->proj_block.reserve(ctx, 1)) return rc;
  if (int rc = ctx->proj_block_host.reserve(ctx, 1)) return rc;
  ProjState& st = ctx->proj_block_host.get()->st;
  std::memset(&st, 0, sizeof(st));
  proj_round_pose(pose, st.R, st.t);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) st.E[4 * r + c] = pose[4 * r + c];
  // (the staging copy is read by this copy alone, and every call ends with a wait on the stream)
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->proj_block.get(), &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  a->partial = ctx->proj_partial, a->pcount = ctx->proj_pcount;
  a->st = &ctx->proj_block.get()->st;
  return ICPK_OK;
}

bool lambda_ok(float l) { return std::isfinite(l) && l >= 0.f && l <= 1.f; }

icpk_projective_color_params color_or_defaults(const icpk_projective_color_params* color) {
  icpk_projective_color_params c;
  icpk_default_projective_color_params(&c);
  if (color) c = *color;
  return c;
}

// K26: prepare's refusals first, unchanged; then what the coloured step needs beside them
int prepare_colored(icpk_ctx* ctx, const icpk_projective_params& p, const icpk_projective_color_params& c, const double* pose,
                    ProjArgs* a) {
  if (!lambda_ok(c.lambda_geometric)) return fail(ctx, ICPK_E_ARG, "lambda_geometric must be finite and in [0, 1]");
  if (int rc = prepare(ctx, p, pose, a)) return rc;
  bool color = false;
  const float* grad = nullptr;
  const bool frame = ctx->proj_view_which == ICPK_VIEW_FRAME;
  projective_color_view(ctx, &color, &grad);
  if (!color && frame) return fail(ctx, ICPK_E_NOT_SET, "the frame view was built without an intensity pyramid");
  if (!color) return fail(ctx, ICPK_E_ARG, "the volume keeps no intensities");
  if (!ctx->pyr_have_int) return fail(ctx, ICPK_E_NOT_SET, "no intensity pyramid (icpk_depth_pyramid_set_intensity)");
  if (!grad && frame)
    return fail(ctx, ICPK_E_NOT_SET, "no colour gradients of this frame-view level (icpk_frame_view_color_gradients)");
  if (!grad) return fail(ctx, ICPK_E_NOT_SET, "no colour gradients of this ray cast (icpk_tsdf_raycast_color_gradients)");
  a->inten = ctx->pyr_int + ctx->pyr_off[p.level];
  a->grad = grad;
  a->lambda_geometric = c.lambda_geometric;
  return ICPK_OK;
}

// one evaluation at the state's pose: a.grad decides the step
int reduce_impl(icpk_ctx* ctx, ProjArgs& a, const double* pose, double sums[28], int64_t* count) {
  if (int rc = begin_state(ctx, pose, &a)) return rc;
  launch_proj_reduce(a, ctx->stream);
  launch_reduce_final(a.partial, a.pcount, red_blocks(a.rows * a.cols), NP2L, ctx->proj_out, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->proj_out_host.get(), ctx->proj_out.get(), (NP2L + 1) * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (sums) std::memcpy(sums, ctx->proj_out_host.get(), NP2L * sizeof(double));
  if (count) std::memcpy(count, ctx->proj_out_host.get() + NP2L, sizeof(int64_t));
  return ICPK_OK;
}

// the loop: a.grad decides the reduce launch, everything else is one code
int align_impl(icpk_ctx* ctx, const icpk_projective_params& p, ProjArgs& a, const double* pose_in, double pose_out[16],
               icpk_projective_result* result) {
  if (int rc = begin_state(ctx, pose_in, &a)) return rc;
  // every launch of every iteration up front; once the state says done the rest are no-ops
  const int B = red_blocks(a.rows * a.cols);
  for (int k = 0; k < p.max_iterations; ++k) {
    launch_proj_reduce(a, ctx->stream);
    launch_proj_step(a.partial, a.pcount, B, ctx->proj_block, k, p.min_pairs, ctx->stream);
  }
  ICPK_HIP(ctx, hipGetLastError());
  // one copy (state + the trace entries that can have been written) and one wait
  ProjBlock* h = ctx->proj_block_host;
  const size_t bytes = offsetof(ProjBlock, trace) + (size_t)p.max_iterations * sizeof(ProjIter);
  ICPK_HIP(ctx, hipMemcpyAsync(h, ctx->proj_block.get(), bytes, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int evaluated = h->st.done ? h->st.iterations + 1 : h->st.iterations;
  ctx->proj_trace.resize((size_t)evaluated);
  if (evaluated > 0) std::memcpy(ctx->proj_trace.data(), h->trace, (size_t)evaluated * sizeof(ProjIter));
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

// rules 1 - 9 over host images; cv == nullptr: the geometric terms
struct HostColor {
  const float *level_intensity, *view_intensity, *gx, *gy, *gz;
  double lg, lc;
};
int pixels_impl(const icpk_projective_params* params, const double pose[16], const uint16_t* level, int32_t rows_s,
                int32_t cols_s, const float* const view[7], int32_t rows_v, int32_t cols_v, float fx_v, float cx_v,
                const double view_pose[16], int64_t first, int32_t count, int32_t* pixel, float* dist, double* terms,
                const HostColor* cv) {
  if (!level || !view || !view_pose || !pixel || !dist || count < 0 || first < 0) return ICPK_E_ARG;
  for (int k = 0; k < 7; ++k)
    if (!view[k]) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  if (check_params(p, pose)) return ICPK_E_ARG;
  if (rows_s < 1 || cols_s < 1 || (int64_t)rows_s * cols_s > (1 << 28) || rows_v < 1 || cols_v < 1 ||
      (int64_t)rows_v * cols_v > (1 << 28))
    return ICPK_E_ARG;
  if (!(std::isfinite(fx_v) && fx_v > 0.f) || !std::isfinite(cx_v)) return ICPK_E_ARG;
  if (first + count > (int64_t)rows_s * cols_s) return ICPK_E_ARG;
  const float scale = (float)(1 << p.level);
  const ProjLevel lv{level, rows_s, cols_s, p.fx / scale, p.cx / scale};
  ProjView vw{view[0], view[1], view[2], view[3], view[4], view[5], view[6], rows_v, cols_v, fx_v, cx_v, {}, {}};
  if (icpk_tsdf_invert_pose(view_pose, vw.Q, vw.s) != ICPK_OK) return ICPK_E_ARG;
  ProjPose E;
  proj_round_pose(pose, E.R, E.t);
  const ProjGate g{p.max_dist, p.min_normal_cos};
  const bool with_normal = p.min_normal_cos > -1.f;
  int pairs = 0;
  for (int32_t e = 0; e < count; ++e) {
    const int64_t i = first + e;
    const int r = (int)(i / cols_s), c = (int)(i % cols_s);
    ProjPair pr;
    const int j = with_normal ? proj_pixel<true>(lv, vw, E, g, r, c, level[i], &pr)
                              : proj_pixel<false>(lv, vw, E, g, r, c, level[i], &pr);
    pixel[e] = j;
    dist[e] = j >= 0 ? pr.dist : 0.f;
    pairs += j >= 0;
    if (terms) {
      double v[28] = {0.0};
      if (j >= 0 && cv) {
        const ProjColor pc{{cv->gx[j], cv->gy[j], cv->gz[j]}, cv->view_intensity[j], cv->level_intensity[i]};
        proj_add_terms_colored(pr, pc, cv->lg, cv->lc, v);
      } else if (j >= 0) {
        proj_add_terms(pr, v);
      }
      std::memcpy(terms + (size_t)e * 28, v, sizeof(v));
    }
  }
  return pairs;
}

}  // namespace

extern "C" {

void icpk_default_projective_color_params(icpk_projective_color_params* c) {
  if (!c) return;
  c->lambda_geometric = 0.968f;
}

void icpk_default_projective_params(icpk_projective_params* p) {
  if (!p) return;
  p->level = 0;
  p->fx = 468.60f, p->cx = 318.27f;
  p->max_iterations = 10;
  p->max_dist = 0.5f;
  p->min_normal_cos = -2.f;
  p->min_pairs = 6;
}

int icpk_projective_pixels(const icpk_projective_params* params, const double pose[16], const uint16_t* level,
                           int32_t rows_s, int32_t cols_s, const float* const view[7], int32_t rows_v, int32_t cols_v,
                           float fx_v, float cx_v, const double view_pose[16], int64_t first, int32_t count,
                           int32_t* pixel, float* dist, double* terms) {
  return pixels_impl(params, pose, level, rows_s, cols_s, view, rows_v, cols_v, fx_v, cx_v, view_pose, first, count, pixel, dist,
                     terms, nullptr);
}

int icpk_projective_pixels_colored(const icpk_projective_params* params, const double pose[16], const uint16_t* level,
                                   int32_t rows_s, int32_t cols_s, const float* const view[7], int32_t rows_v,
                                   int32_t cols_v, float fx_v, float cx_v, const double view_pose[16], int64_t first,
                                   int32_t count, int32_t* pixel, float* dist, double* terms, const float* level_intensity,
                                   const float* view_intensity, const float* const gradient[3],
                                   const icpk_projective_color_params* color) {
  if (!level_intensity || !view_intensity || !gradient || !gradient[0] || !gradient[1] || !gradient[2]) return ICPK_E_ARG;
  const icpk_projective_color_params c = color_or_defaults(color);
  if (!lambda_ok(c.lambda_geometric)) return ICPK_E_ARG;
  const double lg = (double)c.lambda_geometric;
  const HostColor cv{level_intensity, view_intensity, gradient[0], gradient[1], gradient[2], lg, 1.0 - lg};
  return pixels_impl(params, pose, level, rows_s, cols_s, view, rows_v, cols_v, fx_v, cx_v, view_pose, first, count, pixel, dist,
                     terms, &cv);
}

int icpk_projective_associate(icpk_ctx* ctx, const icpk_projective_params* params, const double pose[16], int32_t* pixel,
                              float* dist) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  ProjArgs a{};
  if (int rc = prepare(ctx, p, pose, &a)) return rc;
  if (int rc = begin_state(ctx, pose, &a)) return rc;
  const size_t npix = (size_t)a.rows * a.cols;
  if (int rc = ctx->proj_pixel.reserve(ctx, npix)) return rc;
  if (int rc = ctx->proj_dist.reserve(ctx, npix)) return rc;
  launch_proj_associate(a, ctx->proj_pixel, ctx->proj_dist, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  if (pixel)
    ICPK_HIP(ctx, hipMemcpyAsync(pixel, ctx->proj_pixel.get(), npix * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (dist)
    ICPK_HIP(ctx, hipMemcpyAsync(dist, ctx->proj_dist.get(), npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_projective_reduce(icpk_ctx* ctx, const icpk_projective_params* params, const double pose[16], double sums[28],
                           int64_t* count) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  ProjArgs a{};
  if (int rc = prepare(ctx, p, pose, &a)) return rc;
  return reduce_impl(ctx, a, pose, sums, count);
}

int icpk_projective_reduce_colored(icpk_ctx* ctx, const icpk_projective_params* params,
                                   const icpk_projective_color_params* color, const double pose[16], double sums[28],
                                   int64_t* count) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  ProjArgs a{};
  if (int rc = prepare_colored(ctx, p, color_or_defaults(color), pose, &a)) return rc;
  return reduce_impl(ctx, a, pose, sums, count);
}

int icpk_align_projective(icpk_ctx* ctx, const icpk_projective_params* params, const double pose_in[16], double pose_out[16],
                          icpk_projective_result* result) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  ProjArgs a{};
  if (int rc = prepare(ctx, p, pose_in, &a)) return rc;
  return align_impl(ctx, p, a, pose_in, pose_out, result);
}

int icpk_align_projective_colored(icpk_ctx* ctx, const icpk_projective_params* params,
                                  const icpk_projective_color_params* color, const double pose_in[16], double pose_out[16],
                                  icpk_projective_result* result) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_projective_params p = params_or_defaults(params);
  ProjArgs a{};
  if (int rc = prepare_colored(ctx, p, color_or_defaults(color), pose_in, &a)) return rc;
  return align_impl(ctx, p, a, pose_in, pose_out, result);
}

int icpk_get_projective_trace(icpk_ctx* ctx, icpk_projective_iter* out, int32_t cap) {
  if (!ctx || cap < 0 || (cap > 0 && !out)) return ICPK_E_ARG;
  const size_t n = ctx->proj_trace.size() < (size_t)cap ? ctx->proj_trace.size() : (size_t)cap;
  if (n) std::memcpy(out, ctx->proj_trace.data(), n * sizeof(icpk_projective_iter));
  return (int)n;
}

}  // extern "C"
