// icpk_cluster.cpp -- host side of the DBSCAN clustering (K33; kernels_cluster.hip): icpk_cluster_dbscan labels one of the
// context's clouds over K1d's index of it, selects clusters by size and compacts on the device, and replaces the cloud
// through the path icpk_remove_outliers takes; the record stays on the device for icpk_get_clusters.  icpk_cluster_host
// is THE CLUSTER RULE of include/icpk.h once more as a literal O(n^2) program with a plain union-find, host only.
#include <cmath>
#include <vector>

#include "cluster_rule.h"
#include "icpk_ctx.h"

using namespace icpk;

namespace {

// what both entry points refuse (nullptr: the parameters are good)
const char* bad_params(const icpk_cluster_params* p) {
  if (!p) return "no cluster parameters given";
  if (!(p->eps > 0.f) || !std::isfinite(p->eps)) return "eps must be finite and > 0";
  if (p->min_points < 1) return "min_points must be at least 1";
  if (p->min_size < 0 || p->max_size < 0) return "min_size and max_size must not be negative";
  if (p->max_size != 0 && p->max_size < p->min_size) return "max_size must be 0 or at least min_size";
  if (p->largest_only != 0 && p->largest_only != 1) return "largest_only must be 0 or 1";
  return nullptr;
}

// the record of a call on a cloud of n_in points (the contents of a previous call are given up) and the scratch
int ensure_cluster_buffers(icpk_ctx* ctx, int n_in, bool normals) {
  ctx->have_cl = false;
  const size_t n = n_in < 1 ? 1 : (size_t)n_in;
  int rc = ctx->cl_labels.reserve(ctx, n);
  if (!rc) rc = ctx->cl_core.reserve(ctx, n);
  if (!rc) rc = ctx->cl_count.reserve(ctx, n);
  if (!rc) rc = ctx->cl_nearest.reserve(ctx, n);
  if (!rc) rc = ctx->cl_oidx.reserve(ctx, n);
  if (!rc) rc = ctx->cl_sizes.reserve(ctx, n);
  if (!rc) rc = ctx->cl_first.reserve(ctx, n);
  if (!rc) rc = ctx->cl_parent.reserve(ctx, n);
  if (!rc) rc = ctx->cl_cid.reserve(ctx, n);
  if (!rc) rc = ctx->cl_bsum.reserve(ctx, (n + 1023) / 1024);
  if (!rc) rc = ctx->cl_counts.reserve(ctx, CL_COUNTS);
  if (!rc) rc = ctx->cl_counts_host.reserve(ctx, CL_COUNTS);
  if (!rc) rc = ctx->cl_out.reserve(ctx, (size_t)(normals ? 6 : 3) * n);
  return rc;
}

// the plain union-find of icpk_cluster_host: the root of x, the path halved on the way
int host_find(std::vector<int>& parent, int x) {
  while (parent[(size_t)x] != x) {
    parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
    x = parent[(size_t)x];
  }
  return x;
}

}  // namespace

extern "C" {

int icpk_cluster_dbscan(icpk_ctx* ctx, int32_t which, const icpk_cluster_params* p, int32_t flags, int32_t* n_clusters,
                        int32_t* n_noise, int32_t* n_out) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (flags & ~ICPK_CLUSTER_LABELS_ONLY) return fail(ctx, ICPK_E_ARG, "unknown cluster flag");
  if (const char* why = bad_params(p)) return fail(ctx, ICPK_E_ARG, why);
  if (which == 0 ? !ctx->have_src : !ctx->have_tgt)
    return fail(ctx, ICPK_E_NOT_SET, which == 0 ? "source cloud not set" : "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (which == 0)
    if (int ru = ensure_unpacked(ctx)) return ru;  // (the call reads the working source)
  const Cloud& in = which == 0 ? ctx->src : ctx->tgt;
  const int n = in.n;
  const bool labels_only = (flags & ICPK_CLUSTER_LABELS_ONLY) != 0;
  const bool normals = which == 1 && ctx->have_normals && !labels_only;
  int rc = ensure_cluster_buffers(ctx, n, normals);
  if (rc) return rc;
  int counts[CL_COUNTS] = {};
  float* o = nullptr;
  if (n > 0) {
    // the index: the target's own (built here if it has none yet, and then valid for the alignment that follows), or
    // one of the working source in aux_grid (the target's have_grid state is not touched)
    GridView v;
    if ((rc = which == 1 ? index_target(ctx, &v) : index_aux(ctx, ctx->src, &v))) return rc;
    ICPK_HIP(ctx, hipMemsetAsync(ctx->cl_counts, 0, CL_COUNTS * sizeof(int), ctx->stream));
    o = ctx->cl_out;
    ClusterArgs a{};
    a.index = v;
    a.x = in.x(), a.y = in.y(), a.z = in.z();
    if (normals) a.nx = ctx->nrm.x(), a.ny = ctx->nrm.y(), a.nz = ctx->nrm.z();
    a.n = n;
    a.eps = p->eps;
    a.min_points = p->min_points, a.min_size = p->min_size, a.max_size = p->max_size, a.largest_only = p->largest_only;
    a.labels = ctx->cl_labels, a.core = ctx->cl_core, a.count = ctx->cl_count, a.nearest = ctx->cl_nearest;
    a.out_index = ctx->cl_oidx, a.sizes = ctx->cl_sizes, a.first = ctx->cl_first;
    a.parent = ctx->cl_parent, a.cid = ctx->cl_cid, a.bsum = ctx->cl_bsum, a.counts = ctx->cl_counts;
    a.ox = o, a.oy = o + n, a.oz = o + 2 * (size_t)n;
    if (normals) a.onx = o + 3 * (size_t)n, a.ony = o + 4 * (size_t)n, a.onz = o + 5 * (size_t)n;
    launch_cluster_dbscan(a, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    // the one host wait of the call: the counts
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->cl_counts_host, ctx->cl_counts, CL_COUNTS * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < CL_COUNTS; ++k) counts[k] = ctx->cl_counts_host[k];
    if (counts[CL_ERROR] != 0) return fail(ctx, ICPK_E_HIP, "clustering: a union-find step bound was passed");
    for (int k : {CL_N_CLUSTERS, CL_N_NOISE, CL_N_OUT, CL_N_DROPPED})
      if (counts[k] < 0 || counts[k] > n) return fail(ctx, ICPK_E_HIP, "clustering: impossible counts");
  }
  const int m = counts[CL_N_OUT];
  if (!labels_only) {
    // the new cloud takes the way of icpk_set_*_device, which drops everything derived from the old one (the copies
    // out of cl_out are stream-ordered; nothing writes cl_out before the next clustering on this stream)
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
  ctx->cl_n_in = n;
  ctx->cl_n_clusters = counts[CL_N_CLUSTERS];
  ctx->have_cl = true;
  if (n_clusters) *n_clusters = counts[CL_N_CLUSTERS];
  if (n_noise) *n_noise = counts[CL_N_NOISE];
  if (n_out) *n_out = m;
  return ICPK_OK;
}

int icpk_get_clusters(icpk_ctx* ctx, int32_t* n_in, int32_t* n_clusters, int32_t* labels, uint8_t* core, int32_t* count,
                      int32_t* nearest_core, int32_t* out_index, int32_t* sizes, int32_t* first) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_cl) return fail(ctx, ICPK_E_NOT_SET, "no clustering has run on this context");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->cl_n_in, nc = (size_t)ctx->cl_n_clusters;
  const struct {
    void* dst;
    const void* src;
    size_t bytes;
  } copies[] = {{labels, ctx->cl_labels.get(), n * sizeof(int32_t)},     {core, ctx->cl_core.get(), n},
                {count, ctx->cl_count.get(), n * sizeof(int32_t)},       {nearest_core, ctx->cl_nearest.get(), n * sizeof(int32_t)},
                {out_index, ctx->cl_oidx.get(), n * sizeof(int32_t)},    {sizes, ctx->cl_sizes.get(), nc * sizeof(int32_t)},
                {first, ctx->cl_first.get(), nc * sizeof(int32_t)}};
  bool any = false;
  for (const auto& c : copies)
    if (c.dst && c.bytes) {
      ICPK_HIP(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
      any = true;
    }
  if (any) ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_in) *n_in = ctx->cl_n_in;
  if (n_clusters) *n_clusters = ctx->cl_n_clusters;
  return ICPK_OK;
}

int icpk_cluster_host(const float* points, int32_t n, const icpk_cluster_params* p, int32_t* n_clusters, int32_t* n_noise,
                      int32_t* n_out, int32_t* labels, uint8_t* core, int32_t* count, int32_t* nearest_core,
                      int32_t* out_index, int32_t* sizes, int32_t* first) {
  if (n_clusters) *n_clusters = 0;
  if (n_noise) *n_noise = 0;
  if (n_out) *n_out = 0;
  if (bad_params(p) || n < 0 || (n > 0 && !points)) return ICPK_E_ARG;
  const size_t N = (size_t)n;
  const float *x = points, *y = points + N, *z = points + 2 * N;
  const float eps = p->eps;
  std::vector<uint8_t> fin(N), is_core(N);
  std::vector<int> m(N, 0), parent(N), nearest(N, -1), label(N, -1);
  for (size_t i = 0; i < N; ++i) fin[i] = cluster_finite3(x[i], y[i], z[i]);
  // count and core
  for (size_t i = 0; i < N; ++i) {
    if (fin[i])
      for (size_t j = 0; j < N; ++j) m[i] += fin[j] && cluster_dist(x[i], y[i], z[i], x[j], y[j], z[j]) <= eps;
    is_core[i] = m[i] >= p->min_points;
    parent[i] = (int)i;
  }
  // components of the core points (the smaller root stays a root), and every border point's partner
  for (size_t i = 0; i < N; ++i) {
    if (!fin[i]) continue;
    unsigned long long best = CLUSTER_NO_KEY;
    for (size_t j = 0; j < N; ++j) {
      if (!is_core[j]) continue;
      const float d = cluster_dist(x[i], y[i], z[i], x[j], y[j], z[j]);
      if (!(d <= eps)) continue;
      if (is_core[i]) {
        const int a = host_find(parent, (int)i), b = host_find(parent, (int)j);
        if (a != b) parent[(size_t)(a > b ? a : b)] = a > b ? b : a;
      } else {
        const unsigned long long key = cluster_key(d, (int)j);
        best = key < best ? key : best;
      }
    }
    nearest[i] = is_core[i] ? (int)i : best == CLUSTER_NO_KEY ? -1 : (int)(unsigned)best;
  }
  // clusters by ascending representative, labels, sizes
  std::vector<int> id(N, -1), size, rep;
  for (size_t i = 0; i < N; ++i)
    if (is_core[i] && host_find(parent, (int)i) == (int)i) {
      id[i] = (int)rep.size();
      rep.push_back((int)i);
      size.push_back(0);
    }
  int noise = 0;
  for (size_t i = 0; i < N; ++i) {
    if (nearest[i] < 0) {
      ++noise;
      continue;
    }
    label[i] = id[(size_t)host_find(parent, nearest[i])];
    ++size[(size_t)label[i]];
  }
  int largest = -1;
  unsigned long long largest_key = 0;
  for (size_t c = 0; c < rep.size(); ++c) {
    const unsigned long long key = cluster_size_key(size[c], (int)c);
    if (key > largest_key) largest_key = key, largest = (int)c;
  }
  // selection
  int kept = 0;
  for (size_t i = 0; i < N; ++i) {
    const int lab = label[i];
    const bool keep = cluster_keeps(lab, lab >= 0 ? size[(size_t)lab] : 0, p->min_size, p->max_size, p->largest_only, largest);
    if (out_index) out_index[i] = keep ? kept : -1;
    kept += keep;
    if (labels) labels[i] = lab;
    if (core) core[i] = is_core[i];
    if (count) count[i] = m[i];
    if (nearest_core) nearest_core[i] = nearest[i];
  }
  for (size_t c = 0; c < rep.size(); ++c) {
    if (sizes) sizes[c] = size[c];
    if (first) first[c] = rep[c];
  }
  if (n_clusters) *n_clusters = (int32_t)rep.size();
  if (n_noise) *n_noise = noise;
  if (n_out) *n_out = kept;
  return ICPK_OK;
}

}  // extern "C"
