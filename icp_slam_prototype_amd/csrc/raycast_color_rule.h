// raycast_color_rule.h -- the view gradient rule (K26) for one pixel of a ray-cast view; include/icpk.h writes it out
// ("THE VIEW GRADIENT RULE").  Header-inline and __host__ __device__: kernels_raycast_color.hip runs it per view pixel
// on the device, icpk_raycast_color.cpp over host planes (icpk_raycast_color_gradients_host), compiled with
// -ffp-contract=off on both sides.  It is K17's gradient rule with the neighbourhood replaced by the 3 x 3 window of
// the view: the sums are integers, the solve is float64 with K14's adjugate, one rounded operation per symbol.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef ICPK_HD
#define ICPK_HD __host__ __device__ inline
#endif
#else
#ifndef ICPK_HD
#define ICPK_HD inline
#endif
#endif
#include <stdint.h>

namespace icpk {

constexpr int RAY_COLOR_SUMS = 10;  // m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2 (K17's ten words)

// the eight planes of a view, rows x cols floats each
struct RayColorView {
  const float *x, *y, *z, *nx, *ny, *nz, *depth, *intensity;
  int rows, cols;
};

// nn in float64 lies in [1 - 2^-10, 1 + 2^-10] (false for NaN)
ICPK_HD bool ray_color_usable(double n0, double n1, double n2) {
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
  return nn >= 1.0 - 0x1p-10 && nn <= 1.0 + 0x1p-10;
}

// The ten words of hit pixel (r, c) (depth > 0 is the caller's test).  No index outside the view is formed.
ICPK_HD void ray_color_sums(const RayColorView& v, int r, int c, float radius, long long S[RAY_COLOR_SUMS]) {
  const int j = r * v.cols + c;
  const float px = v.x[j], py = v.y[j], pz = v.z[j];
  const double n0 = v.nx[j], n1 = v.ny[j], n2 = v.nz[j];
  const double Ij = v.intensity[j];
  const bool usable = ray_color_usable(n0, n1, n2);
  const double rd = (double)radius;
  for (int k = 0; k < RAY_COLOR_SUMS; ++k) S[k] = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int rr = r + dy, cc = c + dx;
      if (rr < 0 || rr >= v.rows || cc < 0 || cc >= v.cols) continue;
      const int q = rr * v.cols + cc;
      if (!(v.depth[q] > 0.f)) continue;
      const float qx = v.x[q], qy = v.y[q], qz = v.z[q];
      const float f0 = qx - px, f1 = qy - py, f2 = qz - pz;
      const float d = __builtin_sqrtf((f0 * f0 + f1 * f1) + f2 * f2);
      if (!(d <= radius)) continue;  // (NaN compares false)
      S[0] += 1;
      if (!usable) continue;
      const double e0 = (double)qx - (double)px, e1 = (double)qy - (double)py, e2 = (double)qz - (double)pz;
      const double h = (e0 * n0 + e1 * n1) + e2 * n2;
      const double u0 = e0 - h * n0, u1 = e1 - h * n1, u2 = e2 - h * n2;
      const long long q0 = (long long)__builtin_rint((u0 / rd) * 32768.0);
      const long long q1 = (long long)__builtin_rint((u1 / rd) * 32768.0);
      const long long q2 = (long long)__builtin_rint((u2 / rd) * 32768.0);
      const long long dc = (long long)__builtin_rint(((double)v.intensity[q] - Ij) * 32768.0);
      S[1] += q0 * q0, S[2] += q0 * q1, S[3] += q0 * q2, S[4] += q1 * q1, S[5] += q1 * q2, S[6] += q2 * q2;
      S[7] += q0 * dc, S[8] += q1 * dc, S[9] += q2 * dc;
    }
}

// K17's solve of the ten words with the pixel's normal: the gradient, or (0, 0, 0)
ICPK_HD void ray_color_solve(const long long S[RAY_COLOR_SUMS], float nx, float ny, float nz, float radius,
                             int min_neighbors, float g[3]) {
  const long long m = S[0];
  const double n0 = nx, n1 = ny, n2 = nz;
  const bool usable = ray_color_usable(n0, n1, n2);
  const double w = (double)m * 32768.0, w2 = w * w;
  const double H00 = (double)S[1] + (w2 * n0) * n0;
  const double H01 = (double)S[2] + (w2 * n0) * n1;
  const double H02 = (double)S[3] + (w2 * n0) * n2;
  const double H11 = (double)S[4] + (w2 * n1) * n1;
  const double H12 = (double)S[5] + (w2 * n1) * n2;
  const double H22 = (double)S[6] + (w2 * n2) * n2;
  const double T0 = (double)S[7], T1 = (double)S[8], T2 = (double)S[9];
  const double K00 = H11 * H22 - H12 * H12;
  const double K01 = H02 * H12 - H01 * H22;
  const double K02 = H01 * H12 - H02 * H11;
  const double K11 = H00 * H22 - H02 * H02;
  const double K12 = H01 * H02 - H00 * H12;
  const double K22 = H00 * H11 - H01 * H01;
  const double det = (H00 * K00 + H01 * K01) + H02 * K02;
  const double inv = 1.0 / det;
  const double rd = (double)radius;
  const float g0 = (float)((((K00 * T0 + K01 * T1) + K02 * T2) * inv) / rd);
  const float g1 = (float)((((K01 * T0 + K11 * T1) + K12 * T2) * inv) / rd);
  const float g2 = (float)((((K02 * T0 + K12 * T1) + K22 * T2) * inv) / rd);
  const bool ok = m >= (long long)min_neighbors && usable && det > 0.0 && det < __builtin_inf() &&
                  __builtin_isfinite(g0) && __builtin_isfinite(g1) && __builtin_isfinite(g2);
  g[0] = ok ? g0 : 0.f, g[1] = ok ? g1 : 0.f, g[2] = ok ? g2 : 0.f;
}

// One view pixel: its ten words (all zero for a non-hit) and its gradient ((0, 0, 0) for a non-hit)
ICPK_HD void ray_color_pixel(const RayColorView& v, int r, int c, float radius, int min_neighbors,
                             long long S[RAY_COLOR_SUMS], float g[3]) {
  const int j = r * v.cols + c;
  if (!(v.depth[j] > 0.f)) {
    for (int k = 0; k < RAY_COLOR_SUMS; ++k) S[k] = 0;
    g[0] = g[1] = g[2] = 0.f;
    return;
  }
  ray_color_sums(v, r, c, radius, S);
  ray_color_solve(S, v.nx[j], v.ny[j], v.nz[j], radius, min_neighbors, g);
}

}  // namespace icpk
