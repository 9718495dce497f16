// icpk_global.cpp -- global registration (K16): a seeded RANSAC over the feature matches of icpk_match_features.  The
// hypotheses are drawn, checked and solved on the host (icpk_global_hypotheses, no device work); the valid ones are
// scored by K15 (icpk_score_poses) in chunks of ICPK_SCORE_MAX_POSES, and the best pose is the result icpk_align can
// then refine.  No scoring code of its own.
#include <cmath>
#include <cstring>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

constexpr int GLOBAL_DRAWS = 16;

// draw d of hypothesis h: the finaliser icpk_set_subsample documents
inline uint32_t draw(uint64_t seed, uint64_t h, uint64_t d) {
  uint64_t z = seed + (h + 1) * 0x9E3779B97F4A7C15ull + d * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

struct Clouds {
  const int32_t *ms, *mt;
  int32_t n_matches;
  const float *sx, *sy, *sz, *tx, *ty, *tz;
};

void identity(float T[16]) {
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
}

// hypothesis h of the rule in include/icpk.h: sample[3] (match indices, -1 where the draws gave none), T (the identity
// unless valid); returns validity
bool hypothesis(const Clouds& c, uint64_t seed, float e, uint64_t h, int32_t sample[3], float T[16]) {
  sample[0] = sample[1] = sample[2] = -1;
  identity(T);
  int got = 0;
  for (int d = 0; d < GLOBAL_DRAWS && got < 3; ++d) {
    const int32_t k = (int32_t)(draw(seed, h, (uint64_t)d) % (uint32_t)c.n_matches);
    bool seen = false;
    for (int u = 0; u < got; ++u) seen = seen || sample[u] == k;
    if (!seen) sample[got++] = k;
  }
  if (got < 3) return false;
  float a[3][3], b[3][3];
  for (int u = 0; u < 3; ++u) {
    const int32_t i = c.ms[sample[u]], j = c.mt[sample[u]];
    a[u][0] = c.sx[i], a[u][1] = c.sy[i], a[u][2] = c.sz[i];
    b[u][0] = c.tx[j], b[u][1] = c.ty[j], b[u][2] = c.tz[j];
  }
  const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
  for (const auto& pr : pairs) {
    const float ls = icpk_distance3(a[pr[0]], a[pr[1]]), lt = icpk_distance3(b[pr[0]], b[pr[1]]);
    if (!(ls >= e * lt && lt >= e * ls)) return false;
  }
  // Kabsch on the three pairs, the sums added in sample order from +0.0 (a = source, b = target, as icpk_reduce's
  // Kabsch path feeds the solve: the pose moves source onto target)
  double sa[3] = {0.0, 0.0, 0.0}, sb[3] = {0.0, 0.0, 0.0}, sab[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int u = 0; u < 3; ++u)
    for (int r = 0; r < 3; ++r) {
      sa[r] += (double)a[u][r];
      sb[r] += (double)b[u][r];
      for (int q = 0; q < 3; ++q) sab[3 * r + q] += (double)a[u][r] * (double)b[u][q];
    }
  double R[9], t[3];
  icpk_solve_kabsch(3, sa, sb, sab, R, t);
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) T[4 * r + q] = (float)R[3 * r + q];
    T[4 * r + 3] = (float)t[r];
  }
  return true;
}

}  // namespace

extern "C" {

void icpk_default_global_params(icpk_global_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_hypotheses = 4096;
  p->max_dist = ICPK_MAX_NN_DISTANCE;
  p->edge_similarity = 0.9f;
}

int icpk_global_hypotheses(const int32_t* match_src, const int32_t* match_tgt, int32_t n_matches, const float* sx,
                           const float* sy, const float* sz, int32_t ns, const float* tx, const float* ty,
                           const float* tz, int32_t nt, uint64_t seed, float edge_similarity, int64_t h0, int32_t count,
                           int32_t* samples, uint8_t* valid, float* T) {
  if (n_matches < 0 || count < 0 || h0 < 0 || ns < 0 || nt < 0) return ICPK_E_ARG;
  if (!(edge_similarity >= 0.f && edge_similarity <= 1.f)) return ICPK_E_ARG;
  if (n_matches > 0 && (!match_src || !match_tgt || !sx || !sy || !sz || !tx || !ty || !tz)) return ICPK_E_ARG;
  for (int32_t k = 0; k < n_matches; ++k)
    if (match_src[k] < 0 || match_src[k] >= ns || match_tgt[k] < 0 || match_tgt[k] >= nt) return ICPK_E_ARG;
  const Clouds c{match_src, match_tgt, n_matches, sx, sy, sz, tx, ty, tz};
  for (int32_t k = 0; k < count; ++k) {
    int32_t smp[3] = {-1, -1, -1};
    float Tk[16];
    identity(Tk);
    const bool ok = n_matches >= 3 && hypothesis(c, seed, edge_similarity, (uint64_t)h0 + (uint64_t)k, smp, Tk);
    if (samples) std::memcpy(samples + 3 * (size_t)k, smp, sizeof(smp));
    if (valid) valid[k] = ok ? 1 : 0;
    if (T) std::memcpy(T + 16 * (size_t)k, Tk, sizeof(Tk));
  }
  return ICPK_OK;
}

int icpk_register_global(icpk_ctx* ctx, const icpk_global_params* p, icpk_global_result* out) {
  if (!ctx) return ICPK_E_ARG;
  if (!p || !out) return fail(ctx, ICPK_E_ARG, "params and result must not be NULL");
  if (p->n_hypotheses < 1 || p->n_hypotheses > ICPK_GLOBAL_MAX_HYPOTHESES)
    return fail(ctx, ICPK_E_ARG, "n_hypotheses outside 1 .. ICPK_GLOBAL_MAX_HYPOTHESES");
  if (!(p->max_dist > 0.f) || !std::isfinite(p->max_dist)) return fail(ctx, ICPK_E_ARG, "max_dist must be finite and > 0");
  if (!(p->edge_similarity >= 0.f && p->edge_similarity <= 1.f))
    return fail(ctx, ICPK_E_ARG, "edge_similarity must lie in [0, 1]");
  std::memset(out, 0, sizeof(*out));
  identity(out->T);
  out->hypothesis = -1;
  if (!ctx->have_matches) return fail(ctx, ICPK_E_NOT_SET, "no icpk_match_features call on the current descriptors");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  // the matches and the two clouds they index, to the host
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->match_n_host, ctx->match_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t nm = ctx->match_n_host[0];
  out->n_matches = nm;
  if (nm < 3) return ICPK_W_TOO_FEW_PAIRS;  // (an empty cloud on either side ends here too: it has no matches)
  if (int rc = check_ready(ctx)) return rc;
  const int ns = ctx->src0.n, nt = ctx->tgt.n;
  std::vector<int32_t> ms(nm), mt(nm);
  std::vector<float> sp(3 * (size_t)ns), tp(3 * (size_t)nt);
  ICPK_HIP(ctx, hipMemcpyAsync(ms.data(), ctx->match_src, (size_t)nm * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(mt.data(), ctx->match_tgt, (size_t)nm * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  const float* const from[6] = {ctx->src0.x(), ctx->src0.y(), ctx->src0.z(), ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z()};
  for (int k = 0; k < 3; ++k) {
    ICPK_HIP(ctx, hipMemcpyAsync(sp.data() + (size_t)k * ns, from[k], (size_t)ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(tp.data() + (size_t)k * nt, from[3 + k], (size_t)nt * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const Clouds c{ms.data(), mt.data(), nm, sp.data(), sp.data() + ns, sp.data() + 2 * (size_t)ns,
                 tp.data(), tp.data() + nt, tp.data() + 2 * (size_t)nt};
  // valid hypotheses in order of h, scored a chunk at a time; the best: most inliers, then the smallest sums[1], then
  // the lowest h (a chunk's poses come in order of h, so "strictly better" keeps the lowest)
  std::vector<float> Tc((size_t)ICPK_SCORE_MAX_POSES * 16);
  std::vector<int32_t> hc(ICPK_SCORE_MAX_POSES);
  std::vector<double> sums((size_t)ICPK_SCORE_MAX_POSES * ICPK_NSCORE);
  std::vector<int64_t> inl(ICPK_SCORE_MAX_POSES);
  int filled = 0;
  bool any = false;
  auto flush = [&]() -> int {
    if (!filled) return ICPK_OK;
    const int rc = icpk_score_poses(ctx, filled, Tc.data(), p->max_dist, 0, sums.data(), inl.data());
    if (rc) return rc;
    for (int k = 0; k < filled; ++k) {
      const double* s = sums.data() + (size_t)k * ICPK_NSCORE;
      const bool better = !any || inl[k] > out->inliers || (inl[k] == out->inliers && s[1] < out->sums[1]);
      if (!better) continue;
      any = true;
      std::memcpy(out->T, Tc.data() + 16 * (size_t)k, 16 * sizeof(float));
      std::memcpy(out->sums, s, ICPK_NSCORE * sizeof(double));
      out->inliers = inl[k];
      out->hypothesis = hc[k];
    }
    filled = 0;
    return ICPK_OK;
  };
  for (int32_t h = 0; h < p->n_hypotheses; ++h) {
    int32_t smp[3];
    if (!hypothesis(c, p->seed, p->edge_similarity, (uint64_t)h, smp, Tc.data() + 16 * (size_t)filled)) continue;
    hc[filled++] = h;
    ++out->n_valid;
    if (filled == ICPK_SCORE_MAX_POSES)
      if (int rc = flush()) return rc;
  }
  if (int rc = flush()) return rc;
  if (!any) {
    identity(out->T);
    return ICPK_W_TOO_FEW_PAIRS;
  }
  return ICPK_OK;
}

}  // extern "C"
