// sdf_track_rule.h -- the SDF tracking rule (K29) for one source pixel; include/icpk.h writes it out ("THE SDF TRACKING
// RULE").  Header-inline and __host__ __device__: kernels_sdf_track.hip runs it per pixel of a pyramid level on the
// device, icpk_sdf_track.cpp runs it over host arrays (icpk_sdf_pixels), compiled with -ffp-contract=off on both sides.
// It is made of the projective rule's vertex, pose rounding, proj_move and cross normal (projective_rule.h) and of the
// ray rule's cell and trilinear sample (tsdf_rule.h); what it adds is the gradient of that interpolant inside the cell.
// float32 only up to the accepted pixel, +, -, *, / and sqrt in the order written, no libm: the same bits wherever
// those five are correctly rounded.  The terms of an accepted pixel are K5's, in double.
#pragma once
#include "projective_rule.h"
#include "tsdf_rule.h"

namespace icpk {

// the codes of a rejected pixel (ICPK_SDF_* of include/icpk.h)
enum { SDF_NO_DEPTH = -1, SDF_OUTSIDE = -2, SDF_UNKNOWN = -3, SDF_TOO_FAR = -4, SDF_NO_GRADIENT = -5, SDF_NO_NORMAL = -6,
       SDF_NORMAL = -7 };

struct SdfGate {
  float trunc, max_abs_tsdf, min_normal_cos;
};

// what an accepted pixel hands to the terms: the world point, the unit gradient and the distance D = fl(f trunc)
struct SdfHit {
  float p[3], n[3], D;
};

// (rule 6's sdf_gradient: tsdf_rule.h holds it, beside tsdf_trilerp, for THE QUERY RULE of esdf_rule.h too)

// Rules 1 - 8 for source pixel (r, c) of depth d: the linear index of its cell's lowest corner (>= 0, and *out filled),
// or its code.  No index into the planes is formed before tsdf_cell's range test has passed on all three axes; the
// largest one read is at + 1 + dims_x (1 + dims_y), the cell's far corner.
template <bool WITH_NORMAL>
ICPK_HD int sdf_pixel(const ProjLevel& lv, const TsdfPlanes& vol, const ProjPose& E, const SdfGate& g, int r, int c,
                      uint16_t d, SdfHit* out) {
  if (d == 0) return SDF_NO_DEPTH;
  float v[3];  // (the projective rule's step 2)
  v[2] = (float)d / 5000.0f;
  v[0] = ((float)c - lv.cx) * v[2] / lv.fx;
  v[1] = ((float)r - lv.cx) * v[2] / lv.fx;
  proj_move(E.R, E.t, v, out->p);
  TsdfCell cell;
  if (!tsdf_cell(vol, out->p, &cell)) return SDF_OUTSIDE;
  if (!tsdf_cell_known(vol, cell)) return SDF_UNKNOWN;
  float e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = vol.tsdf[tsdf_corner(vol, cell, k)];
  const float f = tsdf_trilerp(e, cell.w);
  out->D = f * g.trunc;
  if (!(__builtin_fabsf(f) < g.max_abs_tsdf)) return SDF_TOO_FAR;
  float gr[3];
  sdf_gradient(e, cell.w, gr);
  const float len = __builtin_sqrtf((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
  if (!(len > 0.f)) return SDF_NO_GRADIENT;
  out->n[0] = gr[0] / len, out->n[1] = gr[1] / len, out->n[2] = gr[2] / len;
  if (WITH_NORMAL) {  // (the projective rule's step 8 with n in place of the view's normal)
    float s[3];
    if (!proj_cross_normal(lv, r, c, s)) return SDF_NO_NORMAL;
    if ((s[0] * v[0] + s[1] * v[1]) + s[2] * v[2] > 0.f) s[0] = -s[0], s[1] = -s[1], s[2] = -s[2];
    float w3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w3[k] = (E.R[3 * k] * s[0] + E.R[3 * k + 1] * s[1]) + E.R[3 * k + 2] * s[2];
    const float cosv = (w3[0] * out->n[0] + w3[1] * out->n[1]) + w3[2] * out->n[2];
    if (!(cosv >= g.min_normal_cos)) return SDF_NORMAL;
  }
  return (int)cell.at;  // (< the volume's voxels <= 2^30)
}

// rule 8: K5's 28 terms of an accepted pixel, ICPK_NP2L layout, added to v: J = [p x n ; n], r = D
ICPK_HD void sdf_add_terms(const SdfHit& h, double (&v)[28]) {
  const double p0 = h.p[0], p1 = h.p[1], p2 = h.p[2];
  const double n0 = h.n[0], n1 = h.n[1], n2 = h.n[2];
  double J[6];
  J[0] = p1 * n2 - p2 * n1;
  J[1] = p2 * n0 - p0 * n2;
  J[2] = p0 * n1 - p1 * n0;
  J[3] = n0;
  J[4] = n1;
  J[5] = n2;
  const double r = (double)h.D;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[k++] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[21 + a] += J[a] * r;
  v[27] += (double)__builtin_fabsf(h.D);
}

}  // namespace icpk
