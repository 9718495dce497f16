// tests/cpp/plane_host_main.cpp -- DIAGNOSTIC (build.program("plane_host_sanitized")): icpk_segment_planes_host and
// icpk_plane_fit_host in a program of its own so that the host code (icpk_plane.cpp and so csrc/plane_rule.h) can run
// under -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.  Every array is
// allocated at exactly the size the header asks for -- the points 3 n floats, the per-point outputs n entries, model,
// info and sums 8, 6 and 9 entries per plane (n_planes learnt from a first call with the arrays NULL) -- so a read or
// write past any of them is caught.  What the rule promises of its outputs is checked.  Exit status 0 and
// "plane host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

// returns 0, or the check that failed
static int run_case(const std::vector<float>& pts, int n, const icpk_plane_params& p, int32_t flags, int* planes_out) {
  int32_t np = -1, un = -1, kept = -1;
  if (icpk_segment_planes_host(n ? pts.data() : nullptr, n, &p, flags, &np, &un, &kept, nullptr, nullptr, nullptr, nullptr,
                               nullptr) != ICPK_OK)
    return 1;
  if (np < 0 || np > p.max_planes || un < 0 || un > n || kept < 0 || kept > n) return 2;
  const size_t N = (size_t)n, NP = (size_t)np;
  std::vector<int32_t> labels(N, -7), oidx(N, -7), info(6 * NP, -7);
  std::vector<double> model(8 * NP, -7.0), sums(9 * NP, -7.0);
  int32_t np2 = -1, un2 = -1, kept2 = -1;
  if (icpk_segment_planes_host(n ? pts.data() : nullptr, n, &p, flags, &np2, &un2, &kept2, labels.data(), oidx.data(),
                               model.data(), info.data(), sums.data()) != ICPK_OK)
    return 3;
  if (np2 != np || un2 != un || kept2 != kept) return 4;
  const float* x = pts.data();
  const float *y = x + N, *z = x + 2 * N;
  std::vector<int32_t> members(NP, 0);
  int n_un = 0, n_kept = 0;
  for (size_t i = 0; i < N; ++i) {
    const bool fin = std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i]);
    const int32_t lab = labels[i];
    if (lab < -1 || lab >= np || (!fin && lab != -1)) return 5;
    if (lab >= 0) ++members[(size_t)lab];
    n_un += fin && lab < 0;
    const bool want = (flags & ICPK_PLANE_KEEP_INLIERS) ? lab >= 0 && (p.select_plane < 0 || lab == p.select_plane) : fin && lab < 0;
    if ((oidx[i] >= 0) != want) return 6;
    if (oidx[i] >= 0 && oidx[i] != n_kept) return 7;  // input order
    n_kept += oidx[i] >= 0;
    if (lab >= 0) {  // a labelled point lies within t of its plane
      const double* m = &model[8 * (size_t)lab];
      const double s = (m[0] * ((double)x[i] - m[4]) + m[1] * ((double)y[i] - m[5])) + m[2] * ((double)z[i] - m[6]);
      if (!(std::fabs(s) <= (double)p.distance_threshold)) return 8;
    }
  }
  if (n_un != un || n_kept != kept) return 9;
  for (size_t k = 0; k < NP; ++k) {
    const double* m = &model[8 * k];
    const int32_t* f = &info[6 * k];
    if (std::fabs(std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) - 1.0) > 1e-14) return 10;
    if (m[3] != -((m[0] * m[4] + m[1] * m[5]) + m[2] * m[6])) return 11;
    if (f[0] < 0 || f[0] >= p.n_hypotheses || f[4] < 3 || f[5] != members[k] || f[5] < p.min_inliers) return 12;
    for (int j = 1; j <= 3; ++j)
      if (f[j] < 0 || f[j] >= n || (labels[(size_t)f[j]] >= 0 && labels[(size_t)f[j]] < (int32_t)k)) return 13;
    if (f[1] == f[2] || f[1] == f[3] || f[2] == f[3]) return 14;
    // the refit alone gives the record's plane again (the hypothesis' normal is read by the fallback only)
    const float a[3] = {x[(size_t)f[1]], y[(size_t)f[1]], z[(size_t)f[1]]};
    double again[8];
    if (icpk_plane_fit_host(&sums[9 * k], f[4], a, m, again) != ICPK_OK) return 15;
    for (int j = 0; j < 8 && m[7] != 0.0; ++j)  // (curvature 0: the record may be the fallback)
      if (!(again[j] == m[j])) return 16;
  }
  *planes_out = np;
  return 0;
}

int main() {
  const int sizes[] = {0, 1, 2, 3, 63, 64, 65, 257, 700, 1500};
  for (const int n : sizes) {
    uint32_t s = 31u + (uint32_t)n * 977u;
    std::vector<float> pts(3 * (size_t)n);
    // two thirds of the points near the plane z = 0.3 x - 0.2 y + 1, one sixth near x = 2, the rest anywhere
    for (int i = 0; i < n; ++i) {
      const float u = 4.f * unit(s) - 2.f, v = 4.f * unit(s) - 2.f, w = 0.004f * (unit(s) - 0.5f);
      float* q[3] = {&pts[(size_t)i], &pts[(size_t)n + i], &pts[2 * (size_t)n + i]};
      if (i % 6 < 4)
        *q[0] = u, *q[1] = v, *q[2] = 0.3f * u - 0.2f * v + 1.f + w;
      else if (i % 6 == 4)
        *q[0] = 2.f + w, *q[1] = u, *q[2] = v;
      else
        *q[0] = u, *q[1] = v, *q[2] = 4.f * unit(s) - 2.f;
    }
    if (n > 40) {
      pts[(size_t)n + 17] = std::nanf("");
      pts[23] = std::numeric_limits<float>::infinity();
      pts[2 * (size_t)n + 31] = -std::numeric_limits<float>::infinity();
    }
    const struct {
      icpk_plane_params p;
      int32_t flags;
    } settings[] = {{{1, 0.01f, 64, 4, 3, -1, 0}, 0},
                    {{2, 0.01f, 1, 1, 3, -1, 0}, ICPK_PLANE_KEEP_INLIERS},
                    {{3, 0.02f, 33, 16, 20, 1, 0}, ICPK_PLANE_KEEP_INLIERS},
                    {{4, 1e-6f, 16, 2, 3, -1, 0}, ICPK_PLANE_LABELS_ONLY},
                    {{5, 100.f, 8, 3, 3, 15, 0}, ICPK_PLANE_KEEP_INLIERS | ICPK_PLANE_LABELS_ONLY},
                    {{6, 0.01f, 128, 4, 100000, -1, 0}, 0}};
    for (const auto& c : settings) {
      int planes = -1;
      if (const int rc = run_case(pts, n, c.p, c.flags, &planes)) {
        std::fprintf(stderr, "plane host: n %d t %g hypotheses %d failed check %d\n", n, (double)c.p.distance_threshold,
                     c.p.n_hypotheses, rc);
        return 1;
      }
      std::printf("n %d t %g hypotheses %d min_inliers %d: %d planes\n", n, (double)c.p.distance_threshold, c.p.n_hypotheses,
                  c.p.min_inliers, planes);
    }
  }
  // the largest setting the header allows: 65536 hypotheses, 16 rounds
  {
    const int n = 40;
    std::vector<float> pts(3 * (size_t)n);
    uint32_t s = 7u;
    for (float& v : pts) v = unit(s);
    const icpk_plane_params p{9, 0.05f, ICPK_PLANE_MAX_HYPOTHESES, ICPK_PLANE_MAX_PLANES, 3, -1, 0};
    int planes = -1;
    if (const int rc = run_case(pts, n, p, 0, &planes)) {
      std::fprintf(stderr, "plane host: the largest setting failed check %d\n", rc);
      return 1;
    }
    std::printf("n %d, %d hypotheses, %d rounds: %d planes\n", n, p.n_hypotheses, p.max_planes, planes);
  }
  // the refusals: nothing is read or written
  const icpk_plane_params good{0, 0.01f, 16, 2, 3, -1, 0};
  const float one[3] = {0.f, 0.f, 0.f};
  const float inf = std::numeric_limits<float>::infinity();
  const icpk_plane_params bad[] = {{0, 0.f, 16, 2, 3, -1, 0},     {0, -1.f, 16, 2, 3, -1, 0},    {0, std::nanf(""), 16, 2, 3, -1, 0},
                                   {0, inf, 16, 2, 3, -1, 0},     {0, 0.01f, 0, 2, 3, -1, 0},    {0, 0.01f, 65537, 2, 3, -1, 0},
                                   {0, 0.01f, 16, 0, 3, -1, 0},   {0, 0.01f, 16, 17, 3, -1, 0},  {0, 0.01f, 16, 2, 2, -1, 0},
                                   {0, 0.01f, 16, 2, 3, -2, 0},   {0, 0.01f, 16, 2, 3, 16, 0}};
  int32_t np = 5;
  for (const auto& p : bad)
    if (icpk_segment_planes_host(one, 1, &p, ICPK_PLANE_KEEP_INLIERS, &np, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 nullptr) != ICPK_E_ARG || np != 0) {
      std::fprintf(stderr, "plane host: a bad setting was accepted\n");
      return 1;
    }
  const icpk_plane_params sel{0, 0.01f, 16, 2, 3, 0, 0};
  const double nine[9] = {}, three[3] = {0.0, 0.0, 1.0};
  double eight[8];
  if (icpk_segment_planes_host(one, 1, &sel, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_segment_planes_host(one, 1, &good, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_segment_planes_host(one, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_segment_planes_host(one, -1, &good, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_segment_planes_host(nullptr, 1, &good, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_plane_fit_host(nine, 0, one, three, eight) != ICPK_E_ARG || icpk_plane_fit_host(nullptr, 3, one, three, eight) != ICPK_E_ARG ||
      icpk_plane_fit_host(nine, 3, one, three, nullptr) != ICPK_E_ARG) {
    std::fprintf(stderr, "plane host: a bad call was accepted\n");
    return 1;
  }
  // the fallback of the refit: three identical inliers give the hypothesis' plane
  if (icpk_plane_fit_host(nine, 3, one, three, eight) != ICPK_OK || eight[2] != 1.0 || eight[7] != 0.0) {
    std::fprintf(stderr, "plane host: the refit's fallback\n");
    return 1;
  }
  icpk_plane_params d;
  icpk_default_plane_params(&d);
  icpk_default_plane_params(nullptr);
  if (d.seed != 0 || d.distance_threshold != 0.01f || d.n_hypotheses != 256 || d.max_planes != 4 || d.min_inliers != 1000 ||
      d.select_plane != -1 || d.reserved != 0)
    return 1;
  std::printf("plane host: ok\n");
  return 0;
}
