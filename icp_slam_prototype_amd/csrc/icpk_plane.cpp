// icpk_plane.cpp -- host side of the RANSAC plane segmentation (K34; kernels_plane.hip): icpk_segment_planes runs the
// rounds of THE PLANE RULE on one of the context's clouds -- one host wait per round, for the round's count block --,
// selects and compacts on the device, and replaces the cloud through the path icpk_remove_outliers takes; the record stays
// on the device for icpk_get_planes.  icpk_segment_planes_host is the rule once more as a literal O(P H n) program over
// plane_rule.h, host only; icpk_plane_fit_host is the refit alone.
#include <cmath>
#include <vector>

#include "icpk_ctx.h"
#include "plane_rule.h"

using namespace icpk;

static_assert(PL_MAX_PLANES == ICPK_PLANE_MAX_PLANES, "one count block per possible round");

namespace {

constexpr int32_t PLANE_FLAGS = ICPK_PLANE_LABELS_ONLY | ICPK_PLANE_KEEP_INLIERS;

// what both entry points refuse (nullptr: the parameters are good)
const char* bad_params(const icpk_plane_params* p, int32_t flags) {
  if (flags & ~PLANE_FLAGS) return "unknown plane flag";
  if (!p) return "no plane parameters given";
  if (!(p->distance_threshold > 0.f) || !std::isfinite(p->distance_threshold)) return "distance_threshold must be finite and > 0";
  if (p->n_hypotheses < 1 || p->n_hypotheses > ICPK_PLANE_MAX_HYPOTHESES) return "n_hypotheses out of range";
  if (p->max_planes < 1 || p->max_planes > ICPK_PLANE_MAX_PLANES) return "max_planes out of range";
  if (p->min_inliers < 3) return "min_inliers must be at least 3";
  if (p->select_plane < -1 || p->select_plane >= ICPK_PLANE_MAX_PLANES) return "select_plane out of range";
  if (p->select_plane >= 0 && !(flags & ICPK_PLANE_KEEP_INLIERS)) return "select_plane needs ICPK_PLANE_KEEP_INLIERS";
  return nullptr;
}

// the record of a call on a cloud of n_in points (the contents of a previous call are given up) and the scratch
int ensure_plane_buffers(icpk_ctx* ctx, int n_in, int H, bool normals) {
  ctx->have_pl = false;
  const size_t n = n_in < 1 ? 1 : (size_t)n_in;
  int rc = ctx->pl_labels.reserve(ctx, n);
  if (!rc) rc = ctx->pl_oidx.reserve(ctx, n);
  if (!rc) rc = ctx->pl_E.reserve(ctx, n);
  if (!rc) rc = ctx->pl_bsum.reserve(ctx, (n + 1023) / 1024);
  if (!rc) rc = ctx->pl_counts.reserve(ctx, (size_t)(PL_MAX_PLANES + 1) * PL_COUNTS);
  if (!rc) rc = ctx->pl_counts_host.reserve(ctx, PL_COUNTS);
  if (!rc) rc = ctx->pl_hyp.reserve(ctx, (size_t)H * (sizeof(PlaneHyp) / sizeof(double)));
  if (!rc) rc = ctx->pl_hidx.reserve(ctx, (size_t)H * 3);
  if (!rc) rc = ctx->pl_hcount.reserve(ctx, (size_t)H);
  if (!rc) rc = ctx->pl_partial.reserve(ctx, (size_t)9 * RED_MAX_BLOCKS);
  if (!rc) rc = ctx->pl_pcount.reserve(ctx, RED_MAX_BLOCKS);
  if (!rc) rc = ctx->pl_model.reserve(ctx, (size_t)PL_MAX_PLANES * 8);
  if (!rc) rc = ctx->pl_info.reserve(ctx, (size_t)PL_MAX_PLANES * 6);
  if (!rc) rc = ctx->pl_sums.reserve(ctx, (size_t)PL_MAX_PLANES * 9);
  if (!rc) rc = ctx->pl_out.reserve(ctx, (size_t)(normals ? 6 : 3) * n);
  return rc;
}

// what a selection keeps, from the rounds' counts alone: no wait for the selection's own count
int selected_count(const icpk_plane_params* p, int32_t flags, int n_planes, const int* finals, int unassigned) {
  if (!(flags & ICPK_PLANE_KEEP_INLIERS)) return unassigned;
  int kept = 0;
  for (int r = 0; r < n_planes; ++r)
    if (p->select_plane < 0 || p->select_plane == r) kept += finals[r];
  return kept;
}

// ---- the canonical tree of include/icpk.h (ICPK_RED_*) on the host, for icpk_segment_planes_host --------------------
// one workgroup's 256 lanes of NS sums each: the wave64 butterfly (32, 16, ..., 1), then ((w0 + w1) + w2) + w3
void host_tree256(const double* lanes /*[256][9]*/, double out[9]) {
  double w[4][9];
  for (int wave = 0; wave < 4; ++wave) {
    double v[64][9], u[64][9];
    for (int l = 0; l < 64; ++l)
      for (int s = 0; s < 9; ++s) v[l][s] = lanes[(size_t)(wave * 64 + l) * 9 + s];
    for (int msk = 32; msk >= 1; msk >>= 1) {
      for (int l = 0; l < 64; ++l)
        for (int s = 0; s < 9; ++s) u[l][s] = v[l][s] + v[l ^ msk][s];
      for (int l = 0; l < 64; ++l)
        for (int s = 0; s < 9; ++s) v[l][s] = u[l][s];
    }
    for (int s = 0; s < 9; ++s) w[wave][s] = v[0][s];
  }
  for (int s = 0; s < 9; ++s) out[s] = ((w[0][s] + w[1][s]) + w[2][s]) + w[3][s];
}

// terms[n][9] (a row of +0.0 where a point adds nothing) -> the nine sums: red_blocks(n) blocks, lane g adds rows g,
// g + 256 B, ... in order from +0.0, the tree per block, and once more over the block sums padded to 256 slots
void host_canonical(const std::vector<double>& terms, int n, double out[9]) {
  const int B = red_blocks(n);
  const size_t P = (size_t)B * RED_THREADS;
  std::vector<double> acc(P * 9, 0.0), slots((size_t)RED_MAX_BLOCKS * 9, 0.0);
  for (size_t i = 0; i < (size_t)n; ++i)
    for (int s = 0; s < 9; ++s) acc[(i % P) * 9 + s] += terms[i * 9 + s];
  for (int b = 0; b < B; ++b) host_tree256(acc.data() + (size_t)b * RED_THREADS * 9, slots.data() + (size_t)b * 9);
  host_tree256(slots.data(), out);
}

}  // namespace

extern "C" {

void icpk_default_plane_params(icpk_plane_params* p) {
  if (!p) return;
  p->seed = 0;
  p->distance_threshold = 0.01f;
  p->n_hypotheses = 256;
  p->max_planes = 4;
  p->min_inliers = 1000;
  p->select_plane = -1;
  p->reserved = 0;
}

int icpk_segment_planes(icpk_ctx* ctx, int32_t which, const icpk_plane_params* p, int32_t flags, int32_t* n_planes,
                        int32_t* n_unassigned, int32_t* n_out) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (const char* why = bad_params(p, flags)) return fail(ctx, ICPK_E_ARG, why);
  if (which == 0 ? !ctx->have_src : !ctx->have_tgt)
    return fail(ctx, ICPK_E_NOT_SET, which == 0 ? "source cloud not set" : "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (which == 0)
    if (int ru = ensure_unpacked(ctx)) return ru;  // (the call reads the working source)
  const Cloud& in = which == 0 ? ctx->src : ctx->tgt;
  const int n = in.n;
  const bool labels_only = (flags & ICPK_PLANE_LABELS_ONLY) != 0;
  const bool normals = which == 1 && ctx->have_normals && !labels_only;
  int rc = ensure_plane_buffers(ctx, n, p->n_hypotheses, normals);
  if (rc) return rc;
  int planes = 0, unassigned = 0, finals[PL_MAX_PLANES] = {};
  float* o = nullptr;
  if (n > 0) {
    ICPK_HIP(ctx, hipMemsetAsync(ctx->pl_counts, 0, (size_t)(PL_MAX_PLANES + 1) * PL_COUNTS * sizeof(int), ctx->stream));
    ICPK_HIP(ctx, hipMemsetAsync(ctx->pl_labels, 0xff, (size_t)n * sizeof(int), ctx->stream));  // every label -1
    o = ctx->pl_out;
    PlaneArgs a{};
    a.x = in.x(), a.y = in.y(), a.z = in.z();
    if (normals) a.nx = ctx->nrm.x(), a.ny = ctx->nrm.y(), a.nz = ctx->nrm.z();
    a.n = n;
    a.seed = p->seed;
    a.t = p->distance_threshold;
    a.H = p->n_hypotheses, a.min_inliers = p->min_inliers;
    a.keep_inliers = (flags & ICPK_PLANE_KEEP_INLIERS) != 0, a.select_plane = p->select_plane;
    a.labels = ctx->pl_labels, a.out_index = ctx->pl_oidx, a.E = ctx->pl_E, a.bsum = ctx->pl_bsum;
    a.hyp = reinterpret_cast<PlaneHyp*>(ctx->pl_hyp.get()), a.hyp_idx = ctx->pl_hidx, a.hcount = ctx->pl_hcount;
    a.partial = ctx->pl_partial, a.pcount = ctx->pl_pcount;
    a.model = ctx->pl_model, a.info = ctx->pl_info, a.sums = ctx->pl_sums;
    a.ox = o, a.oy = o + n, a.oz = o + 2 * (size_t)n;
    if (normals) a.onx = o + 3 * (size_t)n, a.ony = o + 4 * (size_t)n, a.onz = o + 5 * (size_t)n;
    int bound = n;  // |E| of the next round, or (before the first) a bound on it
    for (int r = 0; r < p->max_planes; ++r) {
      // (from the second round on `bound` is |E| itself: a round the rule ends at once is not launched)
      if (r > 0 && (bound < 3 || bound < p->min_inliers)) break;
      a.round = r;
      a.m_bound = bound;
      a.counts = ctx->pl_counts + (size_t)r * PL_COUNTS;
      launch_plane_round(a, ctx->stream);
      ICPK_HIP(ctx, hipGetLastError());
      // the one host wait of the round: its count block
      ICPK_HIP(ctx, hipMemcpyAsync(ctx->pl_counts_host, a.counts, PL_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const int* c = ctx->pl_counts_host;
      const int m = c[PL_M], fin = c[PL_FINAL];
      if (m < 0 || m > bound || fin < 0 || fin > m) return fail(ctx, ICPK_E_HIP, "plane segmentation: impossible counts");
      unassigned = m;
      if (!c[PL_ACCEPTED]) break;
      finals[planes++] = fin;
      unassigned = m - fin;
      bound = unassigned;
    }
    a.counts = ctx->pl_counts + (size_t)PL_MAX_PLANES * PL_COUNTS;
    launch_plane_select(a, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
  }
  const int m = selected_count(p, flags, planes, finals, unassigned);
  if (!labels_only) {
    // the new cloud takes the way of icpk_set_*_device, which drops everything derived from the old one (the copies
    // out of pl_out are stream-ordered; nothing writes pl_out before the next segmentation on this stream)
    if (which == 0) {
      rc = set_source_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
    } else {
      rc = set_target_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
      if (!rc && normals) {
        if ((rc = ensure_cloud(ctx, ctx->nrm, m))) return rc;
        const Cloud& c = ctx->nrm;
        float* const planes3[3] = {c.x(), c.y(), c.z()};
        for (int k = 0; k < 3; ++k) {
          if (m > 0)
            ICPK_HIP(ctx, hipMemcpyAsync(planes3[k], o + (3 + k) * (size_t)n, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice,
                                         ctx->stream));
          launch_fill_f32(planes3[k] + m, c.cap - m, 0.f, ctx->stream);
        }
        ICPK_HIP(ctx, hipGetLastError());
        ctx->have_normals = true;
      }
    }
    if (rc) return rc;
  }
  ctx->pl_n_in = n;
  ctx->pl_n_planes = planes;
  ctx->have_pl = true;
  if (n_planes) *n_planes = planes;
  if (n_unassigned) *n_unassigned = unassigned;
  if (n_out) *n_out = m;
  return ICPK_OK;
}

int icpk_get_planes(icpk_ctx* ctx, int32_t* n_in, int32_t* n_planes, int32_t* labels, int32_t* out_index, double* model,
                    int32_t* info, double* sums) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_pl) return fail(ctx, ICPK_E_NOT_SET, "no plane segmentation has run on this context");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->pl_n_in, np = (size_t)ctx->pl_n_planes;
  const struct {
    void* dst;
    const void* src;
    size_t bytes;
  } copies[] = {{labels, ctx->pl_labels.get(), n * sizeof(int32_t)},  {out_index, ctx->pl_oidx.get(), n * sizeof(int32_t)},
                {model, ctx->pl_model.get(), np * 8 * sizeof(double)}, {info, ctx->pl_info.get(), np * 6 * sizeof(int32_t)},
                {sums, ctx->pl_sums.get(), np * 9 * sizeof(double)}};
  bool any = false;
  for (const auto& c : copies)
    if (c.dst && c.bytes) {
      ICPK_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
      any = true;
    }
  if (any) ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_in) *n_in = ctx->pl_n_in;
  if (n_planes) *n_planes = ctx->pl_n_planes;
  return ICPK_OK;
}

int icpk_plane_fit_host(const double sums[9], int32_t count, const float a[3], const double hyp_normal[3], double model[8]) {
  if (!sums || !a || !hyp_normal || !model || count < 1) return ICPK_E_ARG;
  plane_fit(sums, count, a, hyp_normal, model);
  return ICPK_OK;
}

int icpk_segment_planes_host(const float* points, int32_t n, const icpk_plane_params* p, int32_t flags, int32_t* n_planes,
                             int32_t* n_unassigned, int32_t* n_out, int32_t* labels, int32_t* out_index, double* model,
                             int32_t* info, double* sums) {
  if (n_planes) *n_planes = 0;
  if (n_unassigned) *n_unassigned = 0;
  if (n_out) *n_out = 0;
  if (bad_params(p, flags) || n < 0 || (n > 0 && !points)) return ICPK_E_ARG;
  const size_t N = (size_t)n;
  const float *x = points, *y = points + N, *z = points + 2 * N;
  const float t = p->distance_threshold;
  const int H = p->n_hypotheses;
  std::vector<int> label(N, -1), E;
  std::vector<uint8_t> fin(N);
  for (size_t i = 0; i < N; ++i) fin[i] = plane_finite3(x[i], y[i], z[i]);
  std::vector<double> models, all_sums, terms(N * 9);
  std::vector<int> infos;
  int planes = 0, unassigned = 0;
  for (int r = 0; r < p->max_planes; ++r) {
    E.clear();
    for (size_t i = 0; i < N; ++i)
      if (fin[i] && label[i] < 0) E.push_back((int)i);
    const int m = (int)E.size();
    unassigned = m;
    if (m < 3 || m < p->min_inliers) break;
    // the hypotheses and their counts
    int win = -1, win_count = 0, win_idx[3] = {-1, -1, -1};
    PlaneHyp win_hyp = {};
    for (int h = 0; h < H; ++h) {
      uint32_t c[3];
      if (!plane_sample(p->seed, (uint64_t)r * (uint64_t)H + (uint64_t)h, (uint32_t)m, c)) continue;
      float s[3][3];
      for (int k = 0; k < 3; ++k) {
        const size_t i = (size_t)E[c[k]];
        s[k][0] = x[i], s[k][1] = y[i], s[k][2] = z[i];
      }
      const PlaneHyp hyp = plane_hypothesis(s[0], s[1], s[2], t);
      if (!hyp.valid) continue;
      int count = 0;
      for (const int i : E) {
        double e[3];
        count += plane_hyp_inlier(hyp.a, hyp.N, hyp.G, x[(size_t)i], y[(size_t)i], z[(size_t)i], e);
      }
      if (win < 0 || count > win_count) {  // (ties to the lowest h)
        win = h, win_count = count, win_hyp = hyp;
        for (int k = 0; k < 3; ++k) win_idx[k] = E[c[k]];
      }
    }
    if (win < 0 || win_count < 3) break;
    // the refit: the nine sums through the canonical tree over all n points
    for (size_t i = 0; i < N; ++i) {
      double e[3], *row = &terms[i * 9];
      const bool in = fin[i] && label[i] < 0 && plane_hyp_inlier(win_hyp.a, win_hyp.N, win_hyp.G, x[i], y[i], z[i], e);
      if (in) {
        row[0] = e[0], row[1] = e[1], row[2] = e[2];
        row[3] = e[0] * e[0], row[4] = e[0] * e[1], row[5] = e[0] * e[2];
        row[6] = e[1] * e[1], row[7] = e[1] * e[2], row[8] = e[2] * e[2];
      } else {
        for (int s = 0; s < 9; ++s) row[s] = 0.0;
      }
    }
    double S[9], M[8];
    host_canonical(terms, n, S);
    const float a3[3] = {(float)win_hyp.a[0], (float)win_hyp.a[1], (float)win_hyp.a[2]};
    plane_fit(S, win_count, a3, win_hyp.N, M);
    // the final inliers
    int final_count = 0;
    for (const int i : E) final_count += plane_final_inlier(M, x[(size_t)i], y[(size_t)i], z[(size_t)i], t);
    if (final_count < p->min_inliers) break;  // the round writes nothing
    for (const int i : E)
      if (plane_final_inlier(M, x[(size_t)i], y[(size_t)i], z[(size_t)i], t)) label[(size_t)i] = r;
    models.insert(models.end(), M, M + 8);
    all_sums.insert(all_sums.end(), S, S + 9);
    const int row[6] = {win, win_idx[0], win_idx[1], win_idx[2], win_count, final_count};
    infos.insert(infos.end(), row, row + 6);
    ++planes;
    unassigned = m - final_count;
  }
  // selection
  int kept = 0;
  for (size_t i = 0; i < N; ++i) {
    const int lab = label[i];
    const bool keep = (flags & ICPK_PLANE_KEEP_INLIERS) ? lab >= 0 && (p->select_plane < 0 || lab == p->select_plane)
                                                        : lab < 0 && fin[i];
    if (out_index) out_index[i] = keep ? kept : -1;
    kept += keep;
    if (labels) labels[i] = lab;
  }
  for (size_t k = 0; k < models.size(); ++k)
    if (model) model[k] = models[k];
  for (size_t k = 0; k < infos.size(); ++k)
    if (info) info[k] = infos[k];
  for (size_t k = 0; k < all_sums.size(); ++k)
    if (sums) sums[k] = all_sums[k];
  if (n_planes) *n_planes = planes;
  if (n_unassigned) *n_unassigned = unassigned;
  if (n_out) *n_out = kept;
  return ICPK_OK;
}

}  // extern "C"
