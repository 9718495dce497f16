// icpk_esdf.cpp -- host side of K31 (kernels_esdf.hip): the exact Euclidean distance map of the TSDF volume.  The map's
// own state behind ctx->esdf (a snapshot, like the ray-cast maps: icpk_tsdf.cpp drops it where the volume is replaced,
// cleared, set or shifted), the refusals, the radius, the launches, the downloads and the query of host points; and the
// two host-only entry points, which run the same rule (esdf_rule.h) over host arrays.  The rules are written out in
// include/icpk.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

struct icpk_esdf_state {
  bool have = false;
  icpk_esdf_params p{};
  int R = 0;
  int dims[3] = {0, 0, 0};  // of the volume the map was computed from (the same while `have`: what changes them drops it)
  float voxel = 0.f;
  long long n = 0;
  DevBuf<uint8_t> cls;
  DevBuf<int32_t> plane[2];  // [0] holds q after a compute
  DevBuf<int> slots;         // 4 x TSDF_MAX_BLOCKS
  DevBuf<long long> counts;  // 4
  PinnedBuf<long long> counts_host;
  // the staging of icpk_esdf_get / _get_box and of icpk_esdf_query
  DevBuf<int32_t> box_sq;
  DevBuf<uint8_t> box_cls;
  DevBuf<float> box_dist, query_in, query_out;
};

void icpk_esdf_free(icpk_ctx* ctx) {
  delete ctx->esdf;  // (its buffers free themselves)
  ctx->esdf = nullptr;
}

void icpk_esdf_drop(icpk_ctx* ctx) {
  if (ctx->esdf) ctx->esdf->have = false;
}

namespace {

constexpr int32_t ESDF_MAX_QUERY = 1 << 24;

// nullptr: fine, and *R is rule 0's radius; else what is wrong
const char* check_esdf(const icpk_esdf_params& p, float voxel, int* R) {
  if (p.min_weight < 1 || p.min_weight > 65535) return "min_weight outside 1 .. 65535";
  if (!std::isfinite(p.max_distance) || !(p.max_distance > 0.f)) return "max_distance must be finite and > 0";
  if (p.flags & ~ICPK_ESDF_UNKNOWN_OCCUPIED) return "unknown ESDF flag";
  const double r = std::floor((double)p.max_distance / (double)voxel);
  if (!(r >= 1.0 && r <= (double)ICPK_ESDF_MAX_RADIUS)) return "max_distance / voxel outside 1 .. ICPK_ESDF_MAX_RADIUS";
  *R = (int)r;
  return nullptr;
}

// the map a context holds, or ICPK_E_NOT_SET with the reason
int current_map(icpk_ctx* ctx, icpk_esdf_state** out) {
  if (!ctx->tsdf) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!ctx->esdf || !ctx->esdf->have) return fail(ctx, ICPK_E_NOT_SET, "no distance map (icpk_esdf_compute)");
  *out = ctx->esdf;
  return ICPK_OK;
}

// fn(begin, end) over [0, n) on up to 16 threads (the passes of icpk_esdf_host: every entry is written by one call)
template <class Fn>
void parallel_ranges(long long n, Fn fn) {
  const long long want = std::min<long long>(std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency())), n / 8192 + 1);
  if (want <= 1) return fn(0LL, n);
  std::vector<std::thread> pool;
  const long long per = (n + want - 1) / want;
  for (long long b = 0; b < n; b += per) pool.emplace_back(fn, b, std::min(n, b + per));
  for (std::thread& t : pool) t.join();
}

}  // namespace

extern "C" {

void icpk_default_esdf_params(icpk_esdf_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_weight = 1;
  p->max_distance = 2.0f;
  p->flags = 0;
}

int icpk_esdf_compute(icpk_ctx* ctx, const icpk_esdf_params* params, int64_t counts[4]) {
  if (!ctx) return ICPK_E_ARG;
  TsdfVolumeView vol;
  if (int rc = tsdf_volume_view(ctx, &vol)) return rc;
  icpk_esdf_params p;
  icpk_default_esdf_params(&p);
  if (params) p = *params;
  int R = 0;
  if (const char* why = check_esdf(p, vol.p.voxel, &R)) return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->esdf) ctx->esdf = new icpk_esdf_state();
  icpk_esdf_state* m = ctx->esdf;
  const long long n = (long long)vol.p.dims[0] * vol.p.dims[1] * vol.p.dims[2];
  bool grown = false;
  int rc = m->cls.reserve(ctx, (size_t)n, &grown);
  if (!rc) rc = m->plane[0].reserve(ctx, (size_t)n, &grown);
  if (!rc) rc = m->plane[1].reserve(ctx, (size_t)n, &grown);
  if (!rc) rc = m->slots.reserve(ctx, 4 * (size_t)TSDF_MAX_BLOCKS);
  if (!rc) rc = m->counts.reserve(ctx, 4);
  if (!rc) rc = m->counts_host.reserve(ctx, 4);
  if (rc) {
    if (grown) m->have = false;  // (the planes of the map that was are gone)
    return rc;
  }
  m->have = false;
  EsdfArgs a{};
  a.tsdf = vol.tsdf, a.weight = vol.weight;
  a.cls = m->cls, a.plane[0] = m->plane[0], a.plane[1] = m->plane[1];
  for (int k = 0; k < 3; ++k) a.dims[k] = m->dims[k] = vol.p.dims[k];
  a.n = n, a.chunk = tsdf_chunk(n);
  a.min_weight = p.min_weight, a.flags = p.flags, a.R = R;
  a.slots = m->slots;
  launch_esdf_compute(a, tsdf_blocks(n), m->counts, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  m->p = p, m->R = R, m->voxel = vol.p.voxel, m->n = n;
  m->have = true;
  if (!counts) return ICPK_OK;  // (nothing is asked: the call does not wait)
  ICPK_HIP(ctx, hipMemcpyAsync(m->counts_host, m->counts, 4 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) counts[k] = m->counts_host[k];
  return ICPK_OK;
}

int icpk_esdf_get_box(icpk_ctx* ctx, const int32_t lo[3], const int32_t hi[3], int32_t* sq, uint8_t* cls, float* dist) {
  if (!ctx) return ICPK_E_ARG;
  icpk_esdf_state* m = nullptr;
  if (int rc = current_map(ctx, &m)) return rc;
  if (!lo || !hi) return fail(ctx, ICPK_E_ARG, "lo or hi is NULL");
  EsdfBoxArgs a{};
  a.box.m = 1;
  for (int k = 0; k < 3; ++k) {
    if (lo[k] < 0 || hi[k] > m->dims[k] || lo[k] >= hi[k]) return fail(ctx, ICPK_E_ARG, "the box is empty or out of bounds");
    a.box.dims[k] = m->dims[k], a.box.lo[k] = lo[k], a.box.size[k] = hi[k] - lo[k];
    a.box.m *= a.box.size[k];  // (<= n <= 2^30)
  }
  if (!sq && !cls && !dist) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t count = (size_t)a.box.m;
  if (sq)
    if (int rc = m->box_sq.reserve(ctx, count)) return rc;
  if (cls)
    if (int rc = m->box_cls.reserve(ctx, count)) return rc;
  if (dist)
    if (int rc = m->box_dist.reserve(ctx, count)) return rc;
  a.sq = m->plane[0], a.cls = m->cls, a.R = m->R, a.voxel = m->voxel;
  launch_esdf_box(a, sq ? m->box_sq.get() : nullptr, cls ? m->box_cls.get() : nullptr, dist ? m->box_dist.get() : nullptr, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  if (sq) ICPK_HIP(ctx, hipMemcpyAsync(sq, m->box_sq, count * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (cls) ICPK_HIP(ctx, hipMemcpyAsync(cls, m->box_cls, count, hipMemcpyDeviceToHost, ctx->stream));
  if (dist) ICPK_HIP(ctx, hipMemcpyAsync(dist, m->box_dist, count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_esdf_get(icpk_ctx* ctx, int32_t* sq, uint8_t* cls, float* dist) {
  if (!ctx) return ICPK_E_ARG;
  icpk_esdf_state* m = nullptr;
  if (int rc = current_map(ctx, &m)) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)m->n;
  // (the two stored planes where they lie; m(q) is not stored: it goes through the box staging)
  if (sq) ICPK_HIP(ctx, hipMemcpyAsync(sq, m->plane[0], n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (cls) ICPK_HIP(ctx, hipMemcpyAsync(cls, m->cls, n, hipMemcpyDeviceToHost, ctx->stream));
  if (dist) {
    const int32_t lo[3] = {0, 0, 0};
    return icpk_esdf_get_box(ctx, lo, m->dims, nullptr, nullptr, dist);  // (it waits for the stream: the copies above too)
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_esdf_query(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, float* dist, float* gx, float* gy,
                    float* gz, uint8_t* status) {
  if (!ctx) return ICPK_E_ARG;
  icpk_esdf_state* m = nullptr;
  if (int rc = current_map(ctx, &m)) return rc;
  if (n < 0 || n > ESDF_MAX_QUERY) return fail(ctx, ICPK_E_ARG, "n outside 0 .. 2^24");
  if (n > 0 && (!x || !y || !z)) return fail(ctx, ICPK_E_ARG, "a coordinate array is NULL");
  if (n == 0) return ICPK_OK;
  TsdfVolumeView vol;
  if (int rc = tsdf_volume_view(ctx, &vol)) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t count = (size_t)n;
  if (int rc = m->query_in.reserve(ctx, 3 * count)) return rc;
  if (int rc = m->query_out.reserve(ctx, 5 * count)) return rc;
  const float* const in[3] = {x, y, z};
  for (int k = 0; k < 3; ++k)
    ICPK_HIP(ctx, hipMemcpyAsync(m->query_in + (size_t)k * count, in[k], count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  EsdfMap map{};
  map.sq = m->plane[0], map.cls = m->cls;
  for (int k = 0; k < 3; ++k) map.dims[k] = m->dims[k], map.origin[k] = vol.p.origin[k];  // (the CURRENT origin)
  map.voxel = m->voxel, map.R = m->R;
  launch_esdf_query(map, m->query_in, n, m->query_out, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  std::vector<float> back(5 * count);  // one copy brings the five arrays back
  ICPK_HIP(ctx, hipMemcpyAsync(back.data(), m->query_out, 5 * count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float* const out[4] = {dist, gx, gy, gz};
  for (int k = 0; k < 4; ++k)
    if (out[k]) std::memcpy(out[k], back.data() + (size_t)k * count, count * sizeof(float));
  if (status) {
    const int32_t* st = reinterpret_cast<const int32_t*>(back.data() + 4 * count);
    for (size_t i = 0; i < count; ++i) status[i] = (uint8_t)st[i];
  }
  return ICPK_OK;
}

int icpk_esdf_release(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->esdf) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  icpk_esdf_free(ctx);
  return ICPK_OK;
}

int icpk_esdf_host(const icpk_tsdf_params* params, const icpk_esdf_params* esdf, const float* tsdf, const uint16_t* weight,
                   int32_t* sq, uint8_t* cls, float* dist, int64_t counts[4]) {
  if (!params || !esdf || !tsdf || !weight) return ICPK_E_ARG;
  int R = 0;
  if (tsdf_check_volume(*params) || check_esdf(*esdf, params->voxel, &R)) return ICPK_E_ARG;
  const int* dims = params->dims;
  const long long dx = dims[0], dxy = dx * dims[1], n = dxy * dims[2];
  const int cap = esdf_cap(R), flags = esdf->flags, min_weight = esdf->min_weight;
  std::vector<uint8_t> classes((size_t)n);
  std::vector<int32_t> a((size_t)n), b((size_t)n);
  int64_t count[4] = {0, 0, 0, 0};
  for (long long at = 0; at < n; ++at) {
    const int c = esdf_class(tsdf[at], weight[at], min_weight);
    classes[(size_t)at] = (uint8_t)c;
    count[c] += 1;
    a[(size_t)at] = esdf_seed(esdf_obstacle(c, flags), cap);
  }
  // the three passes of the rule, a voxel at a time as the kernels take them: a -> b -> a -> b
  const long long strides[3] = {1, dx, dxy};
  for (int axis = 0; axis < 3; ++axis) {
    const int32_t* in = (axis == 1 ? b : a).data();
    int32_t* out = (axis == 1 ? a : b).data();
    const long long stride = strides[axis];
    const int len = dims[axis];
    parallel_ranges(n, [=](long long begin, long long end) {
      for (long long at = begin; at < end; ++at) {
        const int j = (int)(axis == 0 ? at % dx : axis == 1 ? at % dxy / dx : at / dxy);
        const int32_t* line = in + at;
        out[at] = esdf_line_min<1>(line[0], j, len, [=](int d) { return line[(long long)d * stride]; });
      }
    });
  }
  for (long long at = 0; at < n; ++at) {
    const int q = esdf_finish(b[(size_t)at], cap);
    count[3] += q == ESDF_FAR || q == -ESDF_FAR;
    if (sq) sq[at] = q;
    if (cls) cls[at] = classes[(size_t)at];
    if (dist) dist[at] = esdf_metric(q, R, params->voxel);
  }
  if (counts)
    for (int k = 0; k < 4; ++k) counts[k] = count[k];
  return ICPK_OK;
}

int icpk_esdf_query_host(const icpk_tsdf_params* params, const icpk_esdf_params* esdf, const int32_t* sq, const uint8_t* cls,
                         const float* x, const float* y, const float* z, int32_t n, float* dist, float* gx, float* gy, float* gz,
                         uint8_t* status) {
  if (!params || !esdf || !sq || !cls || n < 0 || n > ESDF_MAX_QUERY) return ICPK_E_ARG;
  if (n > 0 && (!x || !y || !z)) return ICPK_E_ARG;
  EsdfMap map{};
  if (tsdf_check_volume(*params) || check_esdf(*esdf, params->voxel, &map.R)) return ICPK_E_ARG;
  map.sq = sq, map.cls = cls;
  for (int k = 0; k < 3; ++k) map.dims[k] = params->dims[k], map.origin[k] = params->origin[k];
  map.voxel = params->voxel;
  for (int32_t i = 0; i < n; ++i) {
    const float p[3] = {x[i], y[i], z[i]};
    float d, g[3];
    const int st = esdf_query(map, p, &d, g);
    if (dist) dist[i] = d;
    if (gx) gx[i] = g[0];
    if (gy) gy[i] = g[1];
    if (gz) gz[i] = g[2];
    if (status) status[i] = (uint8_t)st;
  }
  return ICPK_OK;
}

}  // extern "C"
