// projective_rule.h -- the projective rule (K25) for one source pixel; include/icpk.h writes it out ("THE PROJECTIVE
// RULE").  Header-inline and __host__ __device__: kernels_projective.hip runs it per pixel of a pyramid level on the
// device, icpk_projective.cpp runs it over host images (icpk_projective_pixels), compiled with -ffp-contract=off on
// both sides.  float32 only up to the pair, +, -, *, / and sqrt in the order written, no libm: the same bits wherever
// those five are correctly rounded.  The terms of an accepted pair are K5's, in double.
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

// the codes of a pixel without a pair (ICPK_PROJ_* of include/icpk.h)
enum { PROJ_NO_DEPTH = -1, PROJ_BEHIND = -2, PROJ_OUTSIDE = -3, PROJ_NO_MODEL = -4, PROJ_TOO_FAR = -5,
       PROJ_NO_NORMAL = -6, PROJ_NORMAL = -7 };

// the level: its own shape and the intrinsics it is seen through (fx / 2^l, cx / 2^l)
struct ProjLevel {
  const uint16_t* depth;
  int rows, cols;
  float fx, cx;
};

// the view: seven planes of the last ray cast, its camera, and its pose inverted (world -> view camera)
struct ProjView {
  const float *x, *y, *z, *nx, *ny, *nz, *depth;
  int rows, cols;
  float fx, cx;
  float Q[9], s[3];
};

// the estimate rounded to float once, and the gates
struct ProjPose {
  float R[9], t[3];
};
struct ProjGate {
  float max_dist, min_normal_cos;
};

// what an accepted pixel hands to the terms
struct ProjPair {
  float p[3], m[3], n[3], dist;
};

// the nine R and three t of a camera-to-world pose (double[16]) rounded to float once
ICPK_HD void proj_round_pose(const double pose[16], float R[9], float t[3]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (float)pose[4 * r + c];
    t[r] = (float)pose[4 * r + 3];
  }
}

// R v + t in the form of integration rule 2
ICPK_HD void proj_move(const float R[9], const float t[3], const float v[3], float out[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = ((R[3 * a] * v[0] + R[3 * a + 1] * v[1]) + R[3 * a + 2] * v[2]) + t[a];
}

// K4's ICPK_NORMALS_CROSS normal of pixel (r, c): false when it is zero
ICPK_HD bool proj_cross_normal(const ProjLevel& lv, int r, int c, float n[3]) {
  if (!(r > 0 && r < lv.rows - 1 && c > 0 && c < lv.cols - 1)) return false;
  const uint16_t dE = lv.depth[r * lv.cols + c + 1], dW = lv.depth[r * lv.cols + c - 1];
  const uint16_t dS = lv.depth[(r + 1) * lv.cols + c], dN = lv.depth[(r - 1) * lv.cols + c];
  if (!(dE && dW && dS && dN)) return false;
  const float fx = lv.fx, cx = lv.cx;
  const float zE = ((float)dE) / 5000.0f, zW = ((float)dW) / 5000.0f;
  const float zS = ((float)dS) / 5000.0f, zN = ((float)dN) / 5000.0f;
  const float xE = ((float)(c + 1) - cx) * zE / fx, yE = ((float)r - cx) * zE / fx;
  const float xW = ((float)(c - 1) - cx) * zW / fx, yW = ((float)r - cx) * zW / fx;
  const float xS = ((float)c - cx) * zS / fx, yS = ((float)(r + 1) - cx) * zS / fx;
  const float xN = ((float)c - cx) * zN / fx, yN = ((float)(r - 1) - cx) * zN / fx;
  const float ax = xE - xW, ay = yE - yW, az = zE - zW;
  const float bx = xS - xN, by = yS - yN, bz = zS - zN;
  const float m0 = ay * bz, m1 = az * by, m2 = az * bx, m3 = ax * bz, m4 = ax * by, m5 = ay * bx;
  const float vx = m0 - m1, vy = m2 - m3, vz = m4 - m5;
  const float s0 = vx * vx, s1 = vy * vy, s2 = vz * vz;
  const float l = __builtin_sqrtf((s0 + s1) + s2);
  if (!(l > 0.f)) return false;
  n[0] = vx / l, n[1] = vy / l, n[2] = vz / l;
  return true;
}

// Rules 1 - 8 for source pixel (r, c) of depth d: the view pixel j >= 0 it pairs with (and *out filled), or its code.
// No index into the view is formed before the range test of rule 5 has passed.
template <bool WITH_NORMAL>
ICPK_HD int proj_pixel(const ProjLevel& lv, const ProjView& vw, const ProjPose& E, const ProjGate& g, int r, int c,
                       uint16_t d, ProjPair* out) {
  if (d == 0) return PROJ_NO_DEPTH;
  float v[3];
  v[2] = (float)d / 5000.0f;
  v[0] = ((float)c - lv.cx) * v[2] / lv.fx;
  v[1] = ((float)r - lv.cx) * v[2] / lv.fx;
  proj_move(E.R, E.t, v, out->p);
  float q[3];
  proj_move(vw.Q, vw.s, out->p, q);
  if (!(q[2] > 0.f)) return PROJ_BEHIND;
  const float u = (q[0] * vw.fx) / q[2] + vw.cx;
  const float w = (q[1] * vw.fx) / q[2] + vw.cx;
  const float a = u + 0.5f, b = w + 0.5f;
  if (!(a >= 0.f && a < (float)vw.cols && b >= 0.f && b < (float)vw.rows)) return PROJ_OUTSIDE;
  const int j = (int)b * vw.cols + (int)a;
  if (!(vw.depth[j] > 0.f)) return PROJ_NO_MODEL;
  out->m[0] = vw.x[j], out->m[1] = vw.y[j], out->m[2] = vw.z[j];
  const float e0 = out->p[0] - out->m[0], e1 = out->p[1] - out->m[1], e2 = out->p[2] - out->m[2];
  out->dist = __builtin_sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
  if (!(out->dist < g.max_dist)) return PROJ_TOO_FAR;
  out->n[0] = vw.nx[j], out->n[1] = vw.ny[j], out->n[2] = vw.nz[j];
  if (WITH_NORMAL) {
    float s[3];
    if (!proj_cross_normal(lv, r, c, s)) return PROJ_NO_NORMAL;
    if ((s[0] * v[0] + s[1] * v[1]) + s[2] * v[2] > 0.f) s[0] = -s[0], s[1] = -s[1], s[2] = -s[2];
    float w3[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w3[k] = (E.R[3 * k] * s[0] + E.R[3 * k + 1] * s[1]) + E.R[3 * k + 2] * s[2];
    const float cosv = (w3[0] * out->n[0] + w3[1] * out->n[1]) + w3[2] * out->n[2];
    if (!(cosv >= g.min_normal_cos)) return PROJ_NORMAL;
  }
  return j;
}

// rule 9: K5's 28 terms of an accepted pair, ICPK_NP2L layout, added to v
ICPK_HD void proj_add_terms(const ProjPair& pr, double (&v)[28]) {
  const double p0 = pr.p[0], p1 = pr.p[1], p2 = pr.p[2];
  const double q0 = pr.m[0], q1 = pr.m[1], q2 = pr.m[2];
  const double n0 = pr.n[0], n1 = pr.n[1], n2 = pr.n[2];
  double J[6];
  J[0] = p1 * n2 - p2 * n1;
  J[1] = p2 * n0 - p0 * n2;
  J[2] = p0 * n1 - p1 * n0;
  J[3] = n0;
  J[4] = n1;
  J[5] = n2;
  const double r = ((p0 - q0) * n0 + (p1 - q1) * n1) + (p2 - q2) * n2;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[k++] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) v[21 + a] += J[a] * r;
  v[27] += (double)pr.dist;
}

// what the coloured rule 9 (K26) reads beside the pair: the view's gradient and intensity at j, the level's at i
struct ProjColor {
  float g[3], It, Is;
};

// rule 9 of the coloured path: K17's joint terms of an accepted pair, ICPK_NP2L layout, added to v.  lg = 1, lc = 0
// adds proj_add_terms' values bit for bit (x + 0.0 == x for every x a sum that started at +0.0 can hold).
ICPK_HD void proj_add_terms_colored(const ProjPair& pr, const ProjColor& pc, double lg, double lc, double (&v)[28]) {
  const double p0 = pr.p[0], p1 = pr.p[1], p2 = pr.p[2];
  const double n0 = pr.n[0], n1 = pr.n[1], n2 = pr.n[2];
  const double g0 = pc.g[0], g1 = pc.g[1], g2 = pc.g[2];
  const double e0 = p0 - (double)pr.m[0], e1 = p1 - (double)pr.m[1], e2 = p2 - (double)pr.m[2];
  const double h = (e0 * n0 + e1 * n1) + e2 * n2;
  double G[6], C[6];
  G[0] = p1 * n2 - p2 * n1;
  G[1] = p2 * n0 - p0 * n2;
  G[2] = p0 * n1 - p1 * n0;
  G[3] = n0;
  G[4] = n1;
  G[5] = n2;
  const double u0 = e0 - h * n0, u1 = e1 - h * n1, u2 = e2 - h * n2;
  const double rc = ((double)pc.It + ((g0 * u0 + g1 * u1) + g2 * u2)) - (double)pc.Is;
  const double gn = (g0 * n0 + g1 * n1) + g2 * n2;
  const double M0 = g0 - gn * n0, M1 = g1 - gn * n1, M2 = g2 - gn * n2;
  C[0] = p1 * M2 - p2 * M1;
  C[1] = p2 * M0 - p0 * M2;
  C[2] = p0 * M1 - p1 * M0;
  C[3] = M0;
  C[4] = M1;
  C[5] = M2;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) v[k++] += lg * (G[a] * G[b]) + lc * (C[a] * C[b]);
#pragma unroll
  for (int a = 0; a < 6; ++a) v[21 + a] += lg * (G[a] * h) + lc * (C[a] * rc);
  v[27] += (double)pr.dist;
}

// the loop's update E' = dT E in double (rows of [R | t], 12 entries): 3-term products
ICPK_HD void proj_compose(const double dR[9], const double dt[3], const double E[12], double out[12]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      out[4 * r + c] = (dR[3 * r] * E[c] + dR[3 * r + 1] * E[4 + c]) + dR[3 * r + 2] * E[8 + c];
    out[4 * r + 3] = ((dR[3 * r] * E[3] + dR[3 * r + 1] * E[7]) + dR[3 * r + 2] * E[11]) + dt[r];
  }
}

}  // namespace icpk
