// icpk_score.cpp -- host side of pose scoring (K15; kernels_score.hip): icpk_score_poses finds, for every candidate pose,
// the exact partner of every source point within max_dist and the eleven sums fitness, RMSE and the information matrix
// are made of; icpk_get_score_associations returns a pose's partners; icpk_score_metrics / icpk_information_matrix
// turn the sums into what the caller asked for (host only).
#include <cmath>
#include <cstring>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

static_assert(NSCORE == ICPK_NSCORE, "kernel and ABI agree on the number of sums");

extern "C" {

int icpk_score_poses(icpk_ctx* ctx, int32_t n_poses, const float* T, float max_dist, int32_t flags, double* sums,
                     int64_t* inliers) {
  if (!ctx) return ICPK_E_ARG;
  if (n_poses < 1 || n_poses > ICPK_SCORE_MAX_POSES) return fail(ctx, ICPK_E_ARG, "n_poses outside 1 .. ICPK_SCORE_MAX_POSES");
  if (!T && n_poses != 1) return fail(ctx, ICPK_E_ARG, "T == NULL scores the working source: n_poses must be 1");
  if (!(max_dist > 0.f) || !std::isfinite(max_dist)) return fail(ctx, ICPK_E_ARG, "max_dist must be finite and > 0");
  if (flags & ~ICPK_SCORE_KEEP_ASSOC) return fail(ctx, ICPK_E_ARG, "unknown score flag");
  if (!sums || !inliers) return fail(ctx, ICPK_E_ARG, "sums and inliers must not be NULL");
  if (int rc = check_ready(ctx)) return rc;  // ICPK_E_NOT_SET; an empty target: what icpk_nn returns for it
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool keep = (flags & ICPK_SCORE_KEEP_ASSOC) != 0;
  // T == NULL: the working source as it stands (a device loop may have left it to be unpacked: the same cloud)
  if (!T)
    if (int ru = ensure_unpacked(ctx)) return ru;
  const Cloud& src = T ? ctx->src0 : ctx->src;
  const int ns = src.n;
  const size_t per_pose = ns < 1 ? 1 : (size_t)ns;
  size_t by_keys = SCORE_CHUNK_KEYS / per_pose;
  if (by_keys < 1) by_keys = 1;
  int chunk = n_poses < SCORE_CHUNK_POSES ? n_poses : SCORE_CHUNK_POSES;
  if ((size_t)chunk > by_keys) chunk = (int)by_keys;
  // kept associations live in a buffer of their own: a later call without the flag leaves them retrievable
  if (keep) ctx->have_score_assoc = false;  // (they are about to be rewritten)
  int rc = keep ? ctx->score_kept.reserve(ctx, (size_t)n_poses * per_pose) : ctx->score_keys.reserve(ctx, (size_t)chunk * per_pose);
  if (!rc) rc = ctx->score_partial.reserve(ctx, (size_t)chunk * NSCORE * RED_MAX_BLOCKS);
  if (!rc) rc = ctx->score_pcount.reserve(ctx, (size_t)chunk * RED_MAX_BLOCKS);
  if (!rc) rc = ctx->score_out.reserve(ctx, (size_t)n_poses * (NSCORE + 1));
  if (!rc) rc = ctx->score_out_host.reserve(ctx, (size_t)n_poses * (NSCORE + 1));
  if (!rc && T) rc = ctx->score_T.reserve(ctx, (size_t)n_poses * 16);
  if (!rc && T) rc = ctx->score_T_host.reserve(ctx, (size_t)n_poses * 16);
  if (rc) return rc;
  // K1d's index of the target: built here if the target has none yet, and then valid for the alignment that follows
  GridView v;
  if ((rc = index_target(ctx, &v))) return rc;
  if (T) {
    std::memcpy(ctx->score_T_host, T, (size_t)n_poses * 16 * sizeof(float));
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->score_T, ctx->score_T_host, (size_t)n_poses * 16 * sizeof(float),
                                 hipMemcpyHostToDevice, ctx->stream));
  }
  ScoreArgs a{};
  a.sx = src.x(), a.sy = src.y(), a.sz = src.z();
  a.ns = ns;
  a.max_dist = max_dist;
  a.index = v;
  a.o4 = ctx->grid.o4;
  a.partial = ctx->score_partial;
  a.pcount = ctx->score_pcount;
  for (int k0 = 0; k0 < n_poses; k0 += chunk) {
    const int m = n_poses - k0 < chunk ? n_poses - k0 : chunk;
    a.T = T ? ctx->score_T + 16 * (size_t)k0 : nullptr;
    a.keys = keep ? ctx->score_kept + (size_t)k0 * per_pose : ctx->score_keys.get();
    a.out = ctx->score_out + (size_t)k0 * (NSCORE + 1);
    launch_score_poses(a, m, ctx->stream);
  }
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->score_out_host, ctx->score_out, (size_t)n_poses * (NSCORE + 1) * sizeof(double),
                               hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the one host wait
  for (int k = 0; k < n_poses; ++k) {
    const double* o = ctx->score_out_host + (size_t)k * (NSCORE + 1);
    std::memcpy(sums + (size_t)k * NSCORE, o, NSCORE * sizeof(double));
    std::memcpy(inliers + k, o + NSCORE, sizeof(int64_t));
  }
  if (keep) {
    ctx->score_n_poses = n_poses;
    ctx->score_ns = ns;
    ctx->have_score_assoc = true;
  }
  return ICPK_OK;
}

int icpk_get_score_associations(icpk_ctx* ctx, int32_t pose, int32_t* idx_out, float* dist_out) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_score_assoc)
    return fail(ctx, ICPK_E_NOT_SET, "no icpk_score_poses call with ICPK_SCORE_KEEP_ASSOC on the current clouds");
  if (pose < 0 || pose >= ctx->score_n_poses) return fail(ctx, ICPK_E_ARG, "pose outside the last icpk_score_poses call");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ns = (size_t)ctx->score_ns;
  if (!ns) return ICPK_OK;
  std::vector<nn_key_t> keys(ns);
  const size_t per_pose = ns;  // (ns >= 1 here: the stride icpk_score_poses used)
  ICPK_HIP(ctx, hipMemcpyAsync(keys.data(), ctx->score_kept + (size_t)pose * per_pose, ns * sizeof(nn_key_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < ns; ++i) {
    const bool none = keys[i] == NN_KEY_INIT;
    const uint32_t bits = (uint32_t)(keys[i] >> 32);
    float d;
    std::memcpy(&d, &bits, sizeof(d));
    if (idx_out) idx_out[i] = none ? -1 : (int32_t)(uint32_t)(keys[i] & 0xffffffffu);
    if (dist_out) dist_out[i] = none ? __builtin_inff() : d;
  }
  return ICPK_OK;
}

void icpk_score_metrics(const double sums[ICPK_NSCORE], int64_t inliers, int32_t n_source, float* fitness,
                        float* inlier_rmse, float* mean_dist) {
  const double n = (double)inliers;
  const bool any = sums && inliers > 0;
  if (fitness) *fitness = (float)(n_source > 0 ? n / (double)n_source : 0.0);
  if (inlier_rmse) *inlier_rmse = (float)(any ? std::sqrt(sums[1] / n) : 0.0);
  if (mean_dist) *mean_dist = (float)(any ? sums[0] / n : 0.0);
}

void icpk_information_matrix(const double sums[ICPK_NSCORE], int64_t inliers, double info[36]) {
  if (!sums || !info) return;
  const double sx = sums[2], sy = sums[3], sz = sums[4];
  const double xx = sums[5], xy = sums[6], xz = sums[7], yy = sums[8], yz = sums[9], zz = sums[10];
  const double n = (double)inliers;
  // sum G^T G, G = [-[q]x | I]: upper triangle, then mirrored
  const double u[6][6] = {{yy + zz, -xy, -xz, 0.0, -sz, sy},  //
                          {0.0, xx + zz, -yz, sz, 0.0, -sx},  //
                          {0.0, 0.0, xx + yy, -sy, sx, 0.0},  //
                          {0.0, 0.0, 0.0, n, 0.0, 0.0},       //
                          {0.0, 0.0, 0.0, 0.0, n, 0.0},       //
                          {0.0, 0.0, 0.0, 0.0, 0.0, n}};
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) info[6 * r + c] = r <= c ? u[r][c] : u[c][r];
}

}  // extern "C"
