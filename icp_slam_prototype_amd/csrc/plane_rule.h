// plane_rule.h -- K34: THE PLANE RULE (include/icpk.h) stated once for the kernels (kernels_plane.hip) and the host-only
// icpk_segment_planes_host / icpk_plane_fit_host (icpk_plane.cpp): the draws, the hypothesis plane, the two inlier tests,
// the Jacobi eigen-solve and the refit.  Everything is float64 in the written association; the library is built with
// -ffp-contract=off, so nothing is fused, and nothing of libm but sqrt is called: host and device round alike.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icpk {

constexpr int PLANE_DRAWS = 16;          // draws a hypothesis may use up for its three distinct points
constexpr int PLANE_JACOBI_SWEEPS = 32;  // the fixed bound of the eigen-solve (a sweep is the three rotations)
constexpr double PLANE_LINE_RATIO = 1.0 / 1048576.0;  // 2^-20: l1 <= this * l2 means the inliers lie on a line

// (x - x is 0 for a finite x and NaN otherwise: grid_walk.h's finite3)
__host__ __device__ inline bool plane_finite3(float x, float y, float z) { return ((x - x) + (y - y)) + (z - z) == 0.f; }
__host__ __device__ inline bool plane_finite(double x) { return x - x == 0.0; }

// icpk_set_subsample's finaliser, as K16's draw uses it
__host__ __device__ inline uint64_t plane_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw d of hypothesis g = r * H + h: a position in the list E of m points
__host__ __device__ inline uint32_t plane_draw(uint64_t seed, uint64_t g, int d, uint32_t m) {
  const uint64_t z = plane_mix(seed + (g + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)d * 0xD1B54A32D192ED03ull);
  return (uint32_t)(z >> 32) % m;
}

// the first three distinct positions among the PLANE_DRAWS draws, in draw order; false: fewer than three (m >= 1)
__host__ __device__ inline bool plane_sample(uint64_t seed, uint64_t g, uint32_t m, uint32_t c[3]) {
  int have = 0;
  for (int d = 0; d < PLANE_DRAWS && have < 3; ++d) {
    const uint32_t v = plane_draw(seed, g, d, m);
    bool seen = false;
    for (int k = 0; k < have; ++k) seen = seen || c[k] == v;
    if (!seen) c[have++] = v;
  }
  return have == 3;
}

// a hypothesis as the count launch reads it: 64 bytes at a wave-uniform address
struct PlaneHyp {
  double a[3];  // the first sample, widened
  double N[3];  // (b - a) x (c - a), not normalised
  double G;     // t^2 |N|^2: a point is an inlier iff (N . (p - a))^2 <= G
  int valid;    // |N|^2 > 0 and G finite
  int pad;
};
static_assert(sizeof(PlaneHyp) == 64, "one hypothesis is 64 bytes");

__host__ __device__ inline double plane_len2(const double N[3]) { return (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]; }

__host__ __device__ inline PlaneHyp plane_hypothesis(const float a[3], const float b[3], const float c[3], float t) {
  PlaneHyp h;
  double u[3], v[3];
  for (int k = 0; k < 3; ++k) {
    h.a[k] = (double)a[k];
    u[k] = (double)b[k] - (double)a[k];
    v[k] = (double)c[k] - (double)a[k];
  }
  h.N[0] = u[1] * v[2] - u[2] * v[1];
  h.N[1] = u[2] * v[0] - u[0] * v[2];
  h.N[2] = u[0] * v[1] - u[1] * v[0];
  const double L2 = plane_len2(h.N);
  h.G = ((double)t * (double)t) * L2;
  h.valid = L2 > 0.0 && plane_finite(h.G);
  h.pad = 0;
  return h;
}

// the count's test of a finite point against a hypothesis: e = p - a, s = N . e, s^2 <= G; e is handed back for the sums
__host__ __device__ inline bool plane_hyp_inlier(const double a[3], const double N[3], double G, float px, float py, float pz,
                                                 double e[3]) {
  e[0] = (double)px - a[0];
  e[1] = (double)py - a[1];
  e[2] = (double)pz - a[2];
  const double s = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2];
  return s * s <= G;
}

// the final test against a plane's record (model[0..2] the normal, model[4..6] the centre)
__host__ __device__ inline bool plane_final_inlier(const double model[8], float px, float py, float pz, float t) {
  const double s = (model[0] * ((double)px - model[4]) + model[1] * ((double)py - model[5])) + model[2] * ((double)pz - model[6]);
  return __builtin_fabs(s) <= (double)t;
}

// the sign convention: the component of largest magnitude is positive, the lowest axis on a tie
__host__ __device__ __forceinline__ void plane_orient(double n[3]) {
  const double m0 = __builtin_fabs(n[0]), m1 = __builtin_fabs(n[1]), m2 = __builtin_fabs(n[2]);
  double lead = n[0], big = m0;  // (selects, no indexed access: the fit kernel keeps everything in registers)
  if (m1 > big) lead = n[1], big = m1;
  if (m2 > big) lead = n[2], big = m2;
  if (lead < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
}

// One rotation of the cyclic Jacobi on the symmetric A (full storage) in the plane (p, q), r the third axis; V takes the
// rotation's columns.  An entry that is exactly 0 is left alone.
__host__ __device__ __forceinline__ void plane_rotate(double A[3][3], double V[3][3], int p, int q, int r) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double root = __builtin_sqrt(theta * theta + 1.0);
  const double t = theta < 0.0 ? -1.0 / (root - theta) : 1.0 / (root + theta);
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
  const double s = t * c;
  const double tap = t * apq;
  A[p][p] = A[p][p] - tap;
  A[q][q] = A[q][q] + tap;
  A[p][q] = 0.0;
  A[q][p] = 0.0;
  const double arp = A[r][p], arq = A[r][q];
  const double nrp = c * arp - s * arq, nrq = s * arp + c * arq;
  A[r][p] = nrp, A[p][r] = nrp;
  A[r][q] = nrq, A[q][r] = nrq;
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

// The eigenvalues l[0] <= l[1] <= l[2] of the symmetric matrix (c00, c01, c02, c11, c12, c22) and the eigenvector e0 of
// l[0], normalised once more: sweeps of (0,1), (0,2), (1,2) until every off-diagonal entry is exactly 0, or the bound
__host__ __device__ __forceinline__ void plane_eigen(const double C[6], double l[3], double e0[3]) {
  double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < PLANE_JACOBI_SWEEPS; ++sweep) {
    if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
    plane_rotate(A, V, 0, 1, 2);
    plane_rotate(A, V, 0, 2, 1);
    plane_rotate(A, V, 1, 2, 0);
  }
  const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
  // the least (the lowest axis on a tie), the greatest of the other two (the higher axis on a tie), the one left over --
  // by selects, no indexed access
  int i0 = 0;
  double lo = d0;
  if (d1 < lo) i0 = 1, lo = d1;
  if (d2 < lo) i0 = 2, lo = d2;
  const double x = i0 == 0 ? d1 : d0, y = i0 == 2 ? d1 : d2;  // the other two, in axis order
  l[0] = lo, l[1] = y >= x ? x : y, l[2] = y >= x ? y : x;
  const double v[3] = {i0 == 0 ? V[0][0] : i0 == 1 ? V[0][1] : V[0][2], i0 == 0 ? V[1][0] : i0 == 1 ? V[1][1] : V[1][2],
                       i0 == 0 ? V[2][0] : i0 == 1 ? V[2][1] : V[2][2]};
  const double len = __builtin_sqrt(plane_len2(v));
  for (int k = 0; k < 3; ++k) e0[k] = v[k] / len;
}

// The refit.  sums: e0 e1 e2 e0e0 e0e1 e0e2 e1e1 e1e2 e2e2 over the count inliers, e relative to the sample a; N the
// hypothesis' normal, not normalised.  model: normal (3), d, centre (3), l0 / (l0 + l1 + l2).  Returns 1 if the record
// is the fit, 0 if it fell back to the hypothesis (curvature 0 then).
__host__ __device__ inline int plane_fit(const double sums[9], int count, const float a[3], const double N[3], double model[8]) {
  const double k = (double)count;
  const double mu[3] = {sums[0] / k, sums[1] / k, sums[2] / k};
  const double C[6] = {sums[3] - sums[0] * sums[0] / k, sums[4] - sums[0] * sums[1] / k, sums[5] - sums[0] * sums[2] / k,
                       sums[6] - sums[1] * sums[1] / k, sums[7] - sums[1] * sums[2] / k, sums[8] - sums[2] * sums[2] / k};
  double l[3], n[3];
  plane_eigen(C, l, n);
  plane_orient(n);
  double centre[3] = {(double)a[0] + mu[0], (double)a[1] + mu[1], (double)a[2] + mu[2]};
  double curvature = l[0] / ((l[0] + l[1]) + l[2]);
  bool fit = count > 0 && !(l[1] <= PLANE_LINE_RATIO * l[2]) && plane_finite(curvature);
  for (int j = 0; j < 3; ++j) fit = fit && plane_finite(n[j]) && plane_finite(centre[j]) && plane_finite(l[j]);
  if (!fit) {
    const double len = __builtin_sqrt(plane_len2(N));
    for (int j = 0; j < 3; ++j) n[j] = N[j] / len, centre[j] = (double)a[j];
    plane_orient(n);
    curvature = 0.0;
  }
  for (int j = 0; j < 3; ++j) model[j] = n[j], model[4 + j] = centre[j];
  model[3] = -((n[0] * centre[0] + n[1] * centre[1]) + n[2] * centre[2]);
  model[7] = curvature;
  return fit ? 1 : 0;
}

}  // namespace icpk
