// frame_view_rule.h -- the frame view rule (K28) for one pixel of a pyramid level; include/icpk.h writes it out ("THE
// FRAME VIEW RULE").  Header-inline and __host__ __device__: kernels_frame_view.hip runs it per pixel of every level of
// the resident pyramid, icpk_frame_view.cpp runs it over a host image (icpk_frame_view_pixels), compiled with
// -ffp-contract=off on both sides.  It is the projective rule's own arithmetic -- the vertex of its step 2, the cross
// normal and the flip of its step 8, proj_move -- so that a pixel seen through the pose the view was built at lands on
// the view's own point bit for bit.
#pragma once
#include "projective_rule.h"

namespace icpk {

enum { FRAME_VIEW_HOLE = 0, FRAME_VIEW_NO_NORMAL = 1, FRAME_VIEW_LISTED = 2 };

// Pixel (r, c) of the level at the pose P (rounded to float once): out[0 .. 7] = x, y, z, nx, ny, nz, depth, intensity.
// Everything is 0 unless the pixel is listed; `intensity` is the level's value at the pixel (0 without a pyramid of them).
ICPK_HD int frame_view_pixel(const ProjLevel& lv, const ProjPose& P, int r, int c, float intensity, float out[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = 0.f;
  const uint16_t d = lv.depth[r * lv.cols + c];
  if (d == 0) return FRAME_VIEW_HOLE;
  float v[3];
  v[2] = (float)d / 5000.0f;
  v[0] = ((float)c - lv.cx) * v[2] / lv.fx;
  v[1] = ((float)r - lv.cx) * v[2] / lv.fx;
  float s[3];
  if (!proj_cross_normal(lv, r, c, s)) return FRAME_VIEW_NO_NORMAL;
  if ((s[0] * v[0] + s[1] * v[1]) + s[2] * v[2] > 0.f) s[0] = -s[0], s[1] = -s[1], s[2] = -s[2];
  proj_move(P.R, P.t, v, out);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 + k] = (P.R[3 * k] * s[0] + P.R[3 * k + 1] * s[1]) + P.R[3 * k + 2] * s[2];
  out[6] = v[2];
  out[7] = intensity;
  return FRAME_VIEW_LISTED;
}

}  // namespace icpk
