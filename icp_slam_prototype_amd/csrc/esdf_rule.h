// esdf_rule.h -- the distance rule and the query rule of the Euclidean distance map of the TSDF volume (K31);
// include/icpk.h writes them out ("THE DISTANCE RULE", "THE QUERY RULE").  Header-inline and __host__ __device__:
// kernels_esdf.hip runs it per voxel and per query point on the device, icpk_esdf.cpp runs it over host arrays
// (icpk_esdf_host, icpk_esdf_query_host), compiled with -ffp-contract=off on both sides.  Integers only up to the metric
// value m(q); from there float32, +, -, *, / and sqrt in the order written, no libm: the same bits wherever those five
// are correctly rounded.  The query is made of the ray rule's cell, corner order and trilinear value and of K29's
// gradient of that interpolant (tsdf_rule.h).
#pragma once
#include "tsdf_rule.h"

namespace icpk {

enum { ESDF_UNKNOWN = 0, ESDF_FREE = 1, ESDF_OCCUPIED = 2 };  // rule 1's classes
enum { ESDF_UNKNOWN_OCCUPIED = 1 };                           // ICPK_ESDF_UNKNOWN_OCCUPIED
enum { ESDF_MAX_RADIUS = 1024, ESDF_FAR = 0x7fffffff };       // ICPK_ESDF_MAX_RADIUS, ICPK_ESDF_FAR
enum { ESDF_Q_FAR = 1, ESDF_Q_UNKNOWN = 2, ESDF_Q_OUTSIDE = 0x80 };  // the query's status bits

// rule 1: the class of a voxel with value f and weight w (the surface rule's sign convention: !(f < 0) is free)
ICPK_HD int esdf_class(float f, int w, int min_weight) { return w < min_weight ? ESDF_UNKNOWN : f < 0.f ? ESDF_OCCUPIED : ESDF_FREE; }

// rule 2: whether a voxel of that class belongs to the obstacle set O
ICPK_HD bool esdf_obstacle(int cls, int flags) { return (flags & ESDF_UNKNOWN_OCCUPIED) ? cls != ESDF_FREE : cls == ESDF_OCCUPIED; }

// Rule 3 runs on ONE signed plane s: s(v) < 0 for v in O, s(v) > 0 otherwise, and |s(v)| the squared distance found so
// far -- along the axes passed -- from v to the nearest voxel on the OTHER side, capped at cap = R^2 + 1 (the seed: no
// axis passed, nothing found).  Both distance transforms of the rule live in it: the one a voxel of O takes part in has
// its sites outside O, where it reads 0, and the other one the other way round.
ICPK_HD int esdf_cap(int R) { return R * R + 1; }  // (R <= 1024: 2^20 + 1)
ICPK_HD int esdf_seed(bool obstacle, int cap) { return obstacle ? -cap : cap; }

// what the voxel with plane value s offers a target on the side `target_in_O`, before the squared offset is added: a
// voxel of the other side is a site (0), a voxel of the target's own side is |s| away from one
ICPK_HD int esdf_offer(int s, bool target_in_O) {
  const bool in_O = s < 0;
  return in_O != target_in_O ? 0 : in_O ? -s : s;
}

// One pass for one target voxel with plane value `own`: j its index along the pass's axis, len the axis' length, at(d)
// the plane value of the voxel d steps along the axis (called only for 0 <= j + d < len).  The result is
// +-min over d of offer(j + d) + d^2, d = 0 being |own| <= cap.  The search goes outwards and stops at the first d with
// d^2 >= best: every candidate from there on is >= d^2.  That also bounds it by R, since best <= cap = R^2 + 1 <
// (R + 1)^2.  STEP offsets are taken between two looks at the bound (more candidates never change a minimum);
// candidates past the line's ends are skipped.
template <int STEP, class At>
ICPK_HD int esdf_line_min(int own, int j, int len, At at) {
  const bool in_O = own < 0;
  int best = in_O ? -own : own;
  for (int d = 1; d * d < best; d += STEP) {
#pragma unroll
    for (int u = 0; u < STEP; ++u) {
      const int e = d + u, e2 = e * e;  // (e < R + 1 + STEP and an offer <= cap: the sum fits an int)
      if (j - e >= 0) {
        const int c = esdf_offer(at(-e), in_O) + e2;
        best = c < best ? c : best;
      }
      if (j + e < len) {
        const int c = esdf_offer(at(e), in_O) + e2;
        best = c < best ? c : best;
      }
    }
  }
  return in_O ? -best : best;
}

// rule 3's end: the plane value after the last pass becomes q
ICPK_HD int esdf_finish(int s, int cap) { return s <= -cap ? -ESDF_FAR : s >= cap ? ESDF_FAR : s; }

// rule 4: the metric distance of q
ICPK_HD float esdf_metric(int q, int R, float voxel) {
  const int mag = q < 0 ? -q : q;  // (q is never INT32_MIN)
  const float s = mag == ESDF_FAR ? (float)(R + 1) : __builtin_sqrtf((float)mag);
  const float m = (s - 0.5f) * voxel;
  return q < 0 ? -m : m;
}

// the map as the query reads it
struct EsdfMap {
  const int32_t* sq;
  const uint8_t* cls;
  int dims[3];
  float voxel;
  float origin[3];  // the volume's CURRENT origin (K23)
  int R;
};

// THE QUERY RULE for the world point p: dist, the gradient g and the status
ICPK_HD int esdf_query(const EsdfMap& m, const float p[3], float* dist, float g[3]) {
  TsdfPlanes v{};  // (the cell reads its geometry alone)
#pragma unroll
  for (int a = 0; a < 3; ++a) v.dims[a] = m.dims[a], v.origin[a] = m.origin[a];
  v.voxel = m.voxel;
  TsdfCell cell;
  *dist = 0.f, g[0] = g[1] = g[2] = 0.f;
  if (!tsdf_cell(v, p, &cell)) return ESDF_Q_OUTSIDE;
  float e[8];
  int status = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const long long at = tsdf_corner(v, cell, k);
    const int q = m.sq[at];
    e[k] = esdf_metric(q, m.R, m.voxel);
    if (q == ESDF_FAR || q == -ESDF_FAR) status |= ESDF_Q_FAR;
    if (m.cls[at] == ESDF_UNKNOWN) status |= ESDF_Q_UNKNOWN;
  }
  *dist = tsdf_trilerp(e, cell.w);
  float gr[3];
  sdf_gradient(e, cell.w, gr);
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = gr[a] / m.voxel;
  return status;
}

}  // namespace icpk
