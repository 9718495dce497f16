// icpk_map.cpp -- host side of the voxel certainty map (map.hpp, map.cpp; icpk_map_* in include/icpk.h).
//
// The grid (uint8 certainty), the slots (int32: (list index << 1) | list, -1 = empty) and the two point lists live in
// HBM next to the context's clouds.  An update is 12 launches (kernels_map.hip) and ONE host wait, for the number of
// points it appended; the lists grow on the device with capacity doubling.  The host keeps the list lengths.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "icpk.h"
#include "icpk_ctx.h"
#include "icpk_internal.h"
#include "solve_impl.h"

using namespace icpk;

namespace {

// three planes of stride() floats in one device buffer (x | y | z)
struct Planes {
  DevBuf<float> mem;
  int stride() const { return (int)(mem.capacity() / 3); }
  float* plane(int k) const { return mem + (size_t)k * stride(); }
  int reserve(icpk_ctx* ctx, int n) { return mem.reserve(ctx, (size_t)3 * n); }  // (contents lost when it grows)
};

}  // namespace

struct icpk_map_state {
  DevBuf<uint8_t> cert;  // MAP_CELLS, world[x][y][z]
  DevBuf<int> slot;      // MAP_CELLS
  Planes list[2];        // the two point lists, list_n[k] points each
  int list_n[2] = {0, 0};
  DevBuf<int> scratch;  // MapBuffers of up to scratch_cap batch elements
  int scratch_cap = 0;
  MapBuffers b{};       // (views into scratch)
  DevBuf<int> idx;      // uploaded index list
  Planes batch;         // uploaded points / query points / rejected positions
  Planes pos;           // the positions of every association sweep (icpk_align_to_map)
  DevBuf<Rt> motion;
  DevBuf<int> qout;  // icpk_map_query: certainty and slot per point
  PinnedBuf<int> total_host;
  DevBuf<unsigned> mask;  // K9's occupancy mask (MAP_MASK_WORDS) ...
  bool mask_valid = false;
  unsigned mask_version = 0;  // ... built from the slots of this map version
  DevBuf<nn_key_t> nnkey;  // icpk_map_nearest: K9's keys per query
  // K9's distance bound holds while every filled slot names a point inside its voxel's cell: true until
  // icpk_map_set_points replaces a point list that slots filled by ADD_ASSOCIATED name (never in the reference's flow,
  // where the list is assigned only at the seed); a reset restores it
  bool points_named = false;  // ADD_ASSOCIATED has filled a slot since the last reset
  bool cells_exact = true;
};

namespace {

int ensure_map(icpk_ctx* ctx) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->map) return ICPK_OK;
  icpk_map_state* m = new icpk_map_state();
  ctx->map = m;
  int rc = m->cert.reserve(ctx, MAP_CELLS);
  if (!rc) rc = m->slot.reserve(ctx, MAP_CELLS);
  if (!rc) rc = m->total_host.reserve(ctx, 1);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemsetAsync(m->cert, 0, (size_t)MAP_CELLS, ctx->stream);  // map.cpp:26
  if (!rc && e == hipSuccess) e = hipMemsetAsync(m->slot, 0xff, (size_t)MAP_CELLS * sizeof(int), ctx->stream);  // map.cpp:27
  if (e != hipSuccess) rc = hip_failure(ctx, "map set-up", e);
  if (rc) icpk_map_free(ctx);  // (no half-built map is left behind)
  return rc;
}

// room for `need` entries in a list, its first list_n entries kept (capacity doubling)
int ensure_list(icpk_ctx* ctx, int list, int need) {
  icpk_map_state* m = ctx->map;
  Planes& L = m->list[list];
  if (need <= L.stride()) return ICPK_OK;
  int cap = L.stride() * 2;
  if (cap < need) cap = need;
  if (cap < 1024) cap = 1024;
  Planes grown;
  if (int rc = grown.reserve(ctx, cap)) return rc;
  const int n = m->list_n[list];
  if (n > 0)
    for (int k = 0; k < 3; ++k)
      ICPK_HIP(ctx, hipMemcpyAsync(grown.plane(k), L.plane(k), (size_t)n * sizeof(float), hipMemcpyDeviceToDevice,
                                   ctx->stream));
  if (L.mem) ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::swap(L, grown);
  ICPK_HIP(ctx, grown.mem.release());  // (the old list)
  return ICPK_OK;
}

int ensure_scratch(icpk_ctx* ctx, int n) {
  icpk_map_state* m = ctx->map;
  if (n <= m->scratch_cap) return ICPK_OK;
  int cap = m->scratch_cap * 2;
  if (cap < n) cap = n;
  const size_t tiles = (size_t)(cap + MAP_TILE - 1) / MAP_TILE;
  const size_t ints = (size_t)6 * cap + (size_t)MAP_RADIX * tiles + (tiles + 1) + 1;
  m->scratch_cap = 0;
  if (int rc = m->scratch.reserve(ctx, ints)) return rc;
  int* p = m->scratch;
  m->b.key = p;
  m->b.ka = p + (size_t)cap;
  m->b.kb = p + (size_t)2 * cap;
  m->b.va = p + (size_t)3 * cap;
  m->b.vb = p + (size_t)4 * cap;
  m->b.flag = p + (size_t)5 * cap;
  m->b.hist = p + (size_t)6 * cap;
  m->b.tcount = m->b.hist + (size_t)MAP_RADIX * tiles;
  m->b.total = m->b.tcount + tiles + 1;
  m->scratch_cap = cap;
  return ICPK_OK;
}

int list_of_rule(int rule) { return rule == ICPK_MAP_ADD_ASSOCIATED ? ICPK_MAP_POINTS : ICPK_MAP_KEYPOINTS; }

// the batch through `rule`; one host wait for the number of appended points
int run_update(icpk_ctx* ctx, int rule, const MapPoints& p, int delta) {
  icpk_map_state* m = ctx->map;
  if (p.n <= 0) return ICPK_OK;
  ++ctx->map_version;
  const int list = list_of_rule(rule);
  const int old = m->list_n[list];
  if ((long long)old + p.n > (1ll << 30)) return fail(ctx, ICPK_E_ARG, "map list would exceed 2^30 entries");
  int rc = ensure_list(ctx, list, old + p.n);
  if (rc) return rc;
  rc = ensure_scratch(ctx, p.n);
  if (rc) return rc;
  const Planes& L = m->list[list];
  launch_map_update(p, rule, delta, old, list, L.plane(0), L.plane(1), L.plane(2), m->cert, m->slot, m->b, ctx->stream);
  if (list == ICPK_MAP_POINTS) m->points_named = true;  // (possibly: a superset is safe)
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(m->total_host, m->b.total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  m->list_n[list] = old + *m->total_host;
  return ICPK_OK;
}

// the context's source (working copy) or target as update input
int cloud_of(icpk_ctx* ctx, int from, const Cloud** c) {
  if (from == ICPK_MAP_FROM_SOURCE) {
    if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
    if (int rc = ensure_unpacked(ctx)) return rc;
    *c = &ctx->src;
    return ICPK_OK;
  }
  if (from == ICPK_MAP_FROM_TARGET) {
    if (!ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
    *c = &ctx->tgt;
    return ICPK_OK;
  }
  return fail(ctx, ICPK_E_ARG, "bad map source (ICPK_MAP_FROM_*)");
}

bool bad_rule(int rule, int delta) {
  return rule < ICPK_MAP_ADD_CLOUD || rule > ICPK_MAP_ADD_UNASSOCIATED || delta < 1 || delta > 255;
}

int upload_points(icpk_ctx* ctx, const float* x, const float* y, const float* z, int n) {
  icpk_map_state* m = ctx->map;
  int rc = m->batch.reserve(ctx, n);
  if (rc) return rc;
  const float* src[3] = {x, y, z};
  for (int k = 0; k < 3; ++k)
    ICPK_HIP(ctx, hipMemcpyAsync(m->batch.plane(k), src[k], (size_t)n * sizeof(float), hipMemcpyHostToDevice,
                                 ctx->stream));
  return ICPK_OK;
}

// the motion the loop of the last icpk_align applied after each completed iteration (reference flavour R^-1 and
// -offset, icp.cpp:235-245; Kabsch the step itself), on the device; *niter = their number.  The sweeps ran at
// P_0 .. P_niter.
int upload_motion(icpk_ctx* ctx, const icpk_params* p, int* niter_out) {
  icpk_map_state* m = ctx->map;
  const int niter = (int)(ctx->trace_R.size() / 9);
  std::vector<Rt> mo((size_t)(niter > 0 ? niter : 1));
  for (int s = 0; s < niter; ++s) {
    const float* R = ctx->trace_R.data() + 9 * (size_t)s;
    const float* t = ctx->trace_t.data() + 3 * (size_t)s;
    if (p->solve == ICPK_SOLVE_REFERENCE) {
      invert3f(R, mo[(size_t)s].R);
      for (int k = 0; k < 3; ++k) mo[(size_t)s].t[k] = -t[k];
    } else {
      std::memcpy(mo[(size_t)s].R, R, sizeof(mo[(size_t)s].R));
      std::memcpy(mo[(size_t)s].t, t, sizeof(mo[(size_t)s].t));
    }
  }
  if (int rc = m->motion.reserve(ctx, niter)) return rc;
  if (niter > 0)
    ICPK_HIP(ctx, hipMemcpyAsync(m->motion, mo.data(), (size_t)niter * sizeof(Rt), hipMemcpyHostToDevice, ctx->stream));
  *niter_out = niter;
  return ICPK_OK;
}

// K9's occupancy mask, rebuilt from the slots if the map has changed since it was built
int ensure_mask(icpk_ctx* ctx) {
  icpk_map_state* m = ctx->map;
  if (int rc = m->mask.reserve(ctx, MAP_MASK_WORDS)) return rc;
  if (m->mask_valid && m->mask_version == ctx->map_version) return ICPK_OK;
  launch_map_mask(m->slot, m->mask, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  m->mask_valid = true;
  m->mask_version = ctx->map_version;
  return ICPK_OK;
}

MapNnArgs nn_args(icpk_ctx* ctx, const float* x, const float* y, const float* z, int n, nn_key_t* best,
                  const int* stop) {
  icpk_map_state* m = ctx->map;
  MapNnArgs a{};
  a.qx = x;
  a.qy = y;
  a.qz = z;
  a.nq = n;
  a.slot = m->slot;
  a.mask = m->mask;
  a.cells_exact = m->cells_exact ? 1 : 0;
  a.l0x = m->list[0].plane(0), a.l0y = m->list[0].plane(1), a.l0z = m->list[0].plane(2), a.n0 = m->list_n[0];
  a.l1x = m->list[1].plane(0), a.l1y = m->list[1].plane(1), a.l1z = m->list[1].plane(2), a.n1 = m->list_n[1];
  a.best = best;
  a.stop = stop;
  return a;
}

}  // namespace

bool icpk_map_lookup_current(const icpk_ctx* ctx) {
  return ctx->map && ctx->have_tgt && ctx->tgt_lookup && ctx->tgt_lookup_version == ctx->map_version &&
         ctx->tgt.n == ctx->map->list_n[0] + ctx->map->list_n[1] + 1;
}

int icpk_map_nn_sweep(icpk_ctx* ctx) {
  int rc = ensure_mask(ctx);
  if (rc) return rc;
  launch_map_nn(nn_args(ctx, ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->src.n, ctx->best, ctx->stop), ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

void icpk_map_free(icpk_ctx* ctx) {
  icpk_map_state* m = ctx ? ctx->map : nullptr;
  if (!m) return;
  ++ctx->map_version;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete m;  // (its buffers free themselves)
  ctx->map = nullptr;
}

extern "C" {

int icpk_map_reset(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  const bool fresh = ctx->map == nullptr;
  int rc = ensure_map(ctx);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  if (!fresh) {
    ICPK_HIP(ctx, hipMemsetAsync(m->cert, 0, (size_t)MAP_CELLS, ctx->stream));
    ICPK_HIP(ctx, hipMemsetAsync(m->slot, 0xff, (size_t)MAP_CELLS * sizeof(int), ctx->stream));
  }
  m->list_n[0] = m->list_n[1] = 0;
  m->points_named = false;
  m->cells_exact = true;
  ++ctx->map_version;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_map_release(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  icpk_map_free(ctx);
  return ICPK_OK;
}

int icpk_map_update(icpk_ctx* ctx, int32_t rule, int32_t from, const int32_t* indices, int32_t n, int32_t delta) {
  if (!ctx) return ICPK_E_ARG;
  if (bad_rule(rule, delta)) return fail(ctx, ICPK_E_ARG, "bad map rule or delta (1 <= d <= 255)");
  if (indices && n < 0) return fail(ctx, ICPK_E_ARG, "negative index count");
  int rc = ensure_map(ctx);
  if (rc) return rc;
  const Cloud* c = nullptr;
  rc = cloud_of(ctx, from, &c);
  if (rc) return rc;
  MapPoints p{c->x(), c->y(), c->z(), nullptr, c->n};
  if (indices) {
    for (int32_t k = 0; k < n; ++k)
      if (indices[k] < 0 || indices[k] >= c->n) return fail(ctx, ICPK_E_ARG, "map index outside the cloud");
    icpk_map_state* m = ctx->map;
    rc = m->idx.reserve(ctx, n);
    if (rc) return rc;
    if (n > 0)
      ICPK_HIP(ctx, hipMemcpyAsync(m->idx, indices, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    p.idx = m->idx;
    p.n = n;
  }
  return run_update(ctx, rule, p, delta);
}

int icpk_map_update_points(icpk_ctx* ctx, int32_t rule, const float* x, const float* y, const float* z, int32_t n,
                           int32_t delta) {
  if (!ctx) return ICPK_E_ARG;
  if (bad_rule(rule, delta)) return fail(ctx, ICPK_E_ARG, "bad map rule or delta (1 <= d <= 255)");
  if (n < 0 || (n > 0 && (!x || !y || !z))) return fail(ctx, ICPK_E_ARG, "bad point arrays");
  int rc = ensure_map(ctx);
  if (rc) return rc;
  if (n == 0) return ICPK_OK;
  rc = upload_points(ctx, x, y, z, n);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  MapPoints p{m->batch.plane(0), m->batch.plane(1), m->batch.plane(2), nullptr,
              n};
  return run_update(ctx, rule, p, delta);
}

int icpk_map_set_points(icpk_ctx* ctx, int32_t from) {
  if (!ctx) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc) return rc;
  const Cloud* c = nullptr;
  rc = cloud_of(ctx, from, &c);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  ++ctx->map_version;
  if (m->points_named) m->cells_exact = false;
  m->list_n[ICPK_MAP_POINTS] = 0;  // (nothing of the old list survives the assignment)
  rc = ensure_list(ctx, ICPK_MAP_POINTS, c->n);
  if (rc) return rc;
  const float* src[3] = {c->x(), c->y(), c->z()};
  if (c->n > 0)
    for (int k = 0; k < 3; ++k)
      ICPK_HIP(ctx, hipMemcpyAsync(m->list[ICPK_MAP_POINTS].plane(k), src[k], (size_t)c->n * sizeof(float),
                                   hipMemcpyDeviceToDevice, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  m->list_n[ICPK_MAP_POINTS] = c->n;
  return ICPK_OK;
}

int32_t icpk_map_size(icpk_ctx* ctx, int32_t list) {
  if (!ctx || (list != ICPK_MAP_KEYPOINTS && list != ICPK_MAP_POINTS)) return ICPK_E_ARG;
  return ctx->map ? ctx->map->list_n[list] : 0;
}

int icpk_map_get_list(icpk_ctx* ctx, int32_t list, float* x, float* y, float* z) {
  if (!ctx || (list != ICPK_MAP_KEYPOINTS && list != ICPK_MAP_POINTS)) return ICPK_E_ARG;
  if (!ctx->map || ctx->map->list_n[list] == 0) return ICPK_OK;
  if (!x || !y || !z) return ICPK_E_ARG;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  icpk_map_state* m = ctx->map;
  float* dst[3] = {x, y, z};
  for (int k = 0; k < 3; ++k)
    ICPK_HIP(ctx, hipMemcpyAsync(dst[k], m->list[list].plane(k), (size_t)m->list_n[list] * sizeof(float),
                                 hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_map_get_certainty(icpk_ctx* ctx, uint8_t* out) {
  if (!ctx || !out) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc) return rc;
  ICPK_HIP(ctx, hipMemcpyAsync(out, ctx->map->cert, (size_t)MAP_CELLS, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_map_query(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, uint8_t* cert_out,
                   uint8_t* occupied_out, int32_t* slot_list_out, int32_t* slot_index_out) {
  if (!ctx || n < 0 || (n > 0 && (!x || !y || !z))) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc || n == 0) return rc;
  rc = upload_points(ctx, x, y, z, n);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  rc = m->qout.reserve(ctx, 2 * (size_t)n);
  if (rc) return rc;
  launch_map_query(m->batch.plane(0), m->batch.plane(1), m->batch.plane(2), n,
                   m->cert, m->slot, m->qout, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  std::vector<int> out((size_t)2 * n);
  ICPK_HIP(ctx, hipMemcpyAsync(out.data(), m->qout, out.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int32_t i = 0; i < n; ++i) {
    const int c = out[(size_t)i], s = out[(size_t)n + i];
    if (cert_out) cert_out[i] = (uint8_t)c;
    if (occupied_out) occupied_out[i] = c >= ICPK_MAP_MAX_CONFIDENCE ? 1 : 0;  // map.cpp:443
    if (slot_list_out) slot_list_out[i] = s < 0 ? -1 : (s & 1);
    if (slot_index_out) slot_index_out[i] = s < 0 ? -1 : (s >> 1);
  }
  return ICPK_OK;
}

int icpk_map_list_to_target(icpk_ctx* ctx, int32_t list) {
  if (!ctx || (list != ICPK_MAP_KEYPOINTS && list != ICPK_MAP_POINTS)) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  const Planes& L = m->list[list];
  return icpk_set_target_device(ctx, L.plane(0), L.plane(1), L.plane(2), m->list_n[list]);
}

void icpk_map_voxel(const float p[3], int32_t v[3]) {
  const float c = 10.0f / (float)MAP_DIM;  // map.cpp:58
  for (int k = 0; k < 3; ++k) {
    const float q = p[k] / c;
    // int(q) as the reference's x86 build converts (cvttss2si: truncation, INT_MIN for NaN, +-inf, |q| >= 2^31), then
    // the clamp of map.cpp:65-82: whatever is negative, NaN or out of range lands in 0 (as kernels_map.hip's map_axis)
    const int i = (q >= 0.f && q < 2147483648.f) ? (int)q : 0;
    v[k] = i >= MAP_DIM ? MAP_DIM - 1 : i;
  }
}

int icpk_align_to_map(icpk_ctx* ctx, const icpk_params* p, int32_t delta, float T_out[16], icpk_stats* stats) {
  reset_outputs(T_out, stats);
  if (!ctx || !p || !T_out) return ICPK_E_ARG;
  if (delta < 1 || delta > 255) return fail(ctx, ICPK_E_ARG, "bad delta (1 <= d <= 255)");
  if (p->solve != ICPK_SOLVE_REFERENCE && p->solve != ICPK_SOLVE_KABSCH)
    return fail(ctx, ICPK_E_ARG, "icpk_align_to_map: reference or Kabsch flavour (the map has no normals)");
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  int rc = ensure_map(ctx);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  if (m->list_n[ICPK_MAP_KEYPOINTS] == 0) {  // icp.cpp:490-491, :622-638, map.cpp:124-126
    rc = icpk_reset_source(ctx);
    if (rc) return rc;
    clear_trace(ctx);
    if (stats) stats->status = ICPK_W_EMPTY_MAP;
    return ICPK_W_EMPTY_MAP;
  }
  rc = icpk_map_list_to_target(ctx, ICPK_MAP_KEYPOINTS);
  if (rc) return rc;
  icpk_stats st;
  const int status = icpk_align(ctx, p, T_out, &st);
  if (stats) *stats = st;
  if (status < 0) return status;
  const int ns = ctx->src0.n;
  if (st.final_pairs <= 0 || ns <= 0) return status;  // map.cpp:124-126: no associations, no update

  int niter = 0;
  rc = upload_motion(ctx, p, &niter);
  if (rc) return rc;
  const int nsw = niter + 1;
  const long long total_pos = (long long)ns * nsw;
  if (total_pos > (1ll << 30)) return fail(ctx, ICPK_E_ARG, "too many sweep positions");
  const int mpos = (int)total_pos;
  rc = ensure_scratch(ctx, mpos);
  if (!rc) rc = m->pos.reserve(ctx, mpos);
  if (!rc) rc = m->batch.reserve(ctx, mpos);
  if (rc) return rc;
  launch_map_rejected(ctx->src0.x(), ctx->src0.y(), ctx->src0.z(), ns, m->motion, nsw, m->pos.plane(0),
                      m->pos.plane(1), m->pos.plane(2), ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(),
                      ctx->tgt.n, p->max_nn_dist, m->batch.plane(0), m->batch.plane(1),
                      m->batch.plane(2), m->b, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(m->total_host, m->b.total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int nrej = *m->total_host;
  MapPoints rej{m->batch.plane(0), m->batch.plane(1), m->batch.plane(2), nullptr,
                nrej};
  rc = run_update(ctx, ICPK_MAP_ADD_UNASSOCIATED, rej, delta);  // icp.cpp:271
  return rc ? rc : status;
}

int icpk_map_nearest(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, float* dist_out,
                     int32_t* list_out, int32_t* index_out) {
  if (!ctx || n < 0 || (n > 0 && (!x || !y || !z))) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc || n == 0) return rc;
  rc = upload_points(ctx, x, y, z, n);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  rc = m->nnkey.reserve(ctx, n);
  if (!rc) rc = ensure_mask(ctx);
  if (rc) return rc;
  launch_map_nn(nn_args(ctx, m->batch.plane(0), m->batch.plane(1),
                        m->batch.plane(2), n, m->nnkey, nullptr),
                ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  std::vector<nn_key_t> keys((size_t)n);
  ICPK_HIP(ctx, hipMemcpyAsync(keys.data(), m->nnkey, keys.size() * sizeof(nn_key_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const unsigned n0 = (unsigned)m->list_n[0], n1 = (unsigned)m->list_n[1];
  for (int32_t i = 0; i < n; ++i) {
    const unsigned t = (unsigned)keys[(size_t)i], db = (unsigned)(keys[(size_t)i] >> 32);
    float d;
    std::memcpy(&d, &db, sizeof(d));
    int32_t lst, idx;
    if (t < n0) {
      lst = ICPK_MAP_KEYPOINTS, idx = (int32_t)t;
    } else if (t < n0 + n1) {
      lst = ICPK_MAP_POINTS, idx = (int32_t)(t - n0);
    } else {  // the zero point: an empty voxel won (d < 0.75), or nothing did (d = 0.75 exactly)
      lst = d < ICPK_MAX_NN_DISTANCE ? ICPK_MAP_NN_EMPTY : ICPK_MAP_NN_NONE, idx = -1;
    }
    if (dist_out) dist_out[i] = d;
    if (list_out) list_out[i] = lst;
    if (index_out) index_out[i] = idx;
  }
  return ICPK_OK;
}

int icpk_map_lookup_to_target(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  int rc = ensure_map(ctx);
  if (rc) return rc;
  icpk_map_state* m = ctx->map;
  const int n0 = m->list_n[0], n1 = m->list_n[1];
  if ((long long)n0 + n1 + 1 > (1ll << 31) - 1) return fail(ctx, ICPK_E_ARG, "map lists too long for a target");
  rc = ensure_cloud(ctx, ctx->tgt, n0 + n1 + 1);
  if (rc) return rc;
  Cloud& c = ctx->tgt;
  float* dst[3] = {c.x(), c.y(), c.z()};
  for (int k = 0; k < 3; ++k) {
    if (n0 > 0)
      ICPK_HIP(ctx, hipMemcpyAsync(dst[k], m->list[0].plane(k), (size_t)n0 * sizeof(float),
                                   hipMemcpyDeviceToDevice, ctx->stream));
    if (n1 > 0)
      ICPK_HIP(ctx, hipMemcpyAsync(dst[k] + n0, m->list[1].plane(k), (size_t)n1 * sizeof(float),
                                   hipMemcpyDeviceToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemsetAsync(dst[k] + n0 + n1, 0, sizeof(float), ctx->stream));  // the zero point
  }
  rc = pad_target(ctx);
  if (rc) return rc;
  target_changed(ctx, false);
  ctx->tgt_lookup = true;
  ctx->tgt_lookup_version = ctx->map_version;
  return ICPK_OK;
}

int icpk_align_to_map_dense(icpk_ctx* ctx, const icpk_params* p, int32_t delta, float T_out[16], icpk_stats* stats) {
  reset_outputs(T_out, stats);
  if (!ctx || !p || !T_out) return ICPK_E_ARG;
  if (delta < 0 || delta > 255) return fail(ctx, ICPK_E_ARG, "bad delta (0 <= d <= 255)");
  if (p->solve != ICPK_SOLVE_REFERENCE && p->solve != ICPK_SOLVE_KABSCH)
    return fail(ctx, ICPK_E_ARG, "icpk_align_to_map_dense: reference or Kabsch flavour (the map has no normals)");
  if (!(p->max_nn_dist <= ICPK_MAX_NN_DISTANCE)) return fail(ctx, ICPK_E_ARG, "max_nn_dist above 0.75");
  if (!ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  int rc = icpk_map_lookup_to_target(ctx);
  if (rc) return rc;
  icpk_params q = *p;
  q.nn_mode = ICPK_NN_MAP;
  icpk_stats st;
  const int status = icpk_align(ctx, &q, T_out, &st);
  if (stats) *stats = st;
  if (status < 0 || delta == 0) return status;
  const int ns = ctx->src0.n;
  if (ns <= 0) return status;
  // the accepted data points of the last sweep (icp.cpp:254 then :269, map.cpp:88-119), at the positions that sweep
  // saw: replayed from the uploaded source by the loop's own motions (after a min_pairs fallback the working source has
  // moved on by the fallback motion)
  icpk_map_state* m = ctx->map;
  int niter = 0;
  rc = upload_motion(ctx, p, &niter);
  if (rc) return rc;
  const int nsw = niter + 1;
  const long long total_pos = (long long)ns * nsw;
  if (total_pos > (1ll << 30)) return fail(ctx, ICPK_E_ARG, "too many sweep positions");
  rc = ensure_scratch(ctx, ns);
  if (!rc) rc = m->pos.reserve(ctx, (int)total_pos);
  if (!rc) rc = m->batch.reserve(ctx, ns);
  if (rc) return rc;
  launch_map_poses(ctx->src0.x(), ctx->src0.y(), ctx->src0.z(), ns, m->motion, nsw, m->pos.plane(0),
                   m->pos.plane(1), m->pos.plane(2), ctx->stream);
  const size_t last = (size_t)niter * ns;
  launch_map_accepted(m->pos.plane(0) + last, m->pos.plane(1) + last, m->pos.plane(2) + last, ns, ctx->best,
                      p->max_nn_dist, m->batch.plane(0), m->batch.plane(1),
                      m->batch.plane(2), m->b, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(m->total_host, m->b.total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MapPoints acc{m->batch.plane(0), m->batch.plane(1), m->batch.plane(2),
                nullptr, *m->total_host};
  rc = run_update(ctx, ICPK_MAP_ADD_ASSOCIATED, acc, delta);
  return rc ? rc : status;
}

}  // extern "C"
