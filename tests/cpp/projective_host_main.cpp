// tests/cpp/projective_host_main.cpp -- DIAGNOSTIC (build.program("projective_host_sanitized")): icpk_projective_pixels over
// the shapes of the cases of tests/projective_cases.py, in a program of its own so that the host code (icpk_projective.cpp
// and so csrc/projective_rule.h) can run under -fsanitize=address,undefined without anything being loaded into an
// interpreter.  No GPU.  Every array is allocated at exactly the size the header asks for -- the level rows_s x cols_s,
// each of the seven planes rows_v x cols_v, the outputs `count` entries and count x 28 terms -- so a read or write past
// any of them is caught; what the rule promises of its outputs is checked on every pixel.  Exit status 0 and
// "projective host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void pose_of(double yaw_deg, double tx, double ty, double tz, double P[16]) {
  const double a = yaw_deg * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a);
  const double R[16] = {c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz, 0, 0, 0, 1};
  for (int k = 0; k < 16; ++k) P[k] = R[k];
}

struct Case {
  int rows_s, cols_s, rows_v, cols_v, level;
  double yaw;     // of the estimate
  int holes;      // per cent of holes in the frame and in the view
  float max_dist, min_cos;
};

// returns 0, or the check that failed; *pairs_out: the pairs of the whole image
static int run(const Case& k, int* pairs_out) {
  const size_t ns = (size_t)k.rows_s * k.cols_s, nv = (size_t)k.rows_v * k.cols_v;
  uint32_t s = 25u + (uint32_t)(ns % 97);
  std::vector<uint16_t> level(ns);
  for (auto& d : level) d = (int)((lcg(s) >> 8) % 100) < k.holes ? 0 : (uint16_t)(9800 + (lcg(s) >> 8) % 400);  // about 2 m
  // the view: a plane at z = 2 seen from the origin through fx_v = cols_v, cx_v = (cols_v - 1) / 2, with holes
  const float fx_v = (float)k.cols_v, cx_v = (float)(k.cols_v - 1) * 0.5f;
  std::vector<std::vector<float>> plane(7, std::vector<float>(nv, 0.f));
  for (int r = 0; r < k.rows_v; ++r)
    for (int c = 0; c < k.cols_v; ++c) {
      const size_t j = (size_t)r * k.cols_v + c;
      if ((int)((lcg(s) >> 8) % 100) < k.holes) continue;
      plane[0][j] = ((float)c - cx_v) * 2.f / fx_v, plane[1][j] = ((float)r - cx_v) * 2.f / fx_v, plane[2][j] = 2.f;
      plane[5][j] = -1.f, plane[6][j] = 2.f;
    }
  const float* view[7];
  for (int a = 0; a < 7; ++a) view[a] = plane[a].data();
  double E[16], V[16];
  pose_of(k.yaw, 0.01, -0.02, 0.03, E);
  pose_of(0.0, 0.0, 0.0, 0.0, V);
  icpk_projective_params p;
  icpk_default_projective_params(&p);
  p.level = k.level;
  // level-0 intrinsics that make the level's field of view the view's
  p.fx = (float)k.cols_s * (float)(1 << k.level), p.cx = (float)(k.cols_s - 1) * 0.5f * (float)(1 << k.level);
  p.max_dist = k.max_dist, p.min_normal_cos = k.min_cos;
  // the whole image, then windows of it: exactly-sized outputs each time
  std::vector<int32_t> pixel(ns, 12345);
  std::vector<float> dist(ns, -1.f);
  std::vector<double> terms(ns * 28, -1.0);
  const int pairs = icpk_projective_pixels(&p, E, level.data(), k.rows_s, k.cols_s, view, k.rows_v, k.cols_v, fx_v, cx_v, V, 0,
                                           (int32_t)ns, pixel.data(), dist.data(), terms.data());
  if (pairs < 0) return 1;
  int counted = 0;
  for (size_t i = 0; i < ns; ++i) {
    const int32_t j = pixel[i];
    if (j >= 0) {
      ++counted;
      if ((size_t)j >= nv || !(plane[6][(size_t)j] > 0.f) || !(dist[i] < k.max_dist) || !(dist[i] >= 0.f)) return 2;
      if (terms[i * 28 + 27] != (double)dist[i]) return 3;
    } else {
      if (j < ICPK_PROJ_NORMAL || dist[i] != 0.f) return 4;
      for (int t = 0; t < 28; ++t)
        if (terms[i * 28 + t] != 0.0) return 5;
      if ((level[i] == 0) != (j == ICPK_PROJ_NO_DEPTH)) return 6;
      if (!(k.min_cos > -1.f) && (j == ICPK_PROJ_NO_NORMAL || j == ICPK_PROJ_NORMAL)) return 7;
    }
  }
  if (counted != pairs) return 8;
  for (size_t first : {(size_t)0, ns / 3, ns - 1}) {
    const size_t count = first + 5 <= ns ? 5 : ns - first;
    std::vector<int32_t> wp(count, 777);
    std::vector<float> wd(count, -1.f);
    std::vector<double> wt(count * 28, -1.0);
    if (icpk_projective_pixels(&p, E, level.data(), k.rows_s, k.cols_s, view, k.rows_v, k.cols_v, fx_v, cx_v, V, (int64_t)first,
                               (int32_t)count, wp.data(), wd.data(), first ? wt.data() : nullptr) < 0)
      return 9;
    for (size_t e = 0; e < count; ++e) {
      if (wp[e] != pixel[first + e] || wd[e] != dist[first + e]) return 10;
      for (int t = 0; first && t < 28; ++t)
        if (wt[e * 28 + t] != terms[(first + e) * 28 + t]) return 11;
    }
  }
  *pairs_out = pairs;
  return 0;
}

int main() {
  const Case cases[] = {
      {120, 160, 120, 160, 0, 2.0, 0, 0.5f, -2.f},   // the room's shapes
      {60, 80, 120, 160, 1, 2.0, 0, 0.5f, -2.f},     // level 1 against the full view
      {48, 64, 48, 64, 0, 180.0, 0, 0.5f, -2.f},     // every pixel behind the view
      {120, 160, 120, 160, 0, 30.0, 0, 0.5f, -2.f},  // many outside
      {120, 160, 120, 160, 0, 1.0, 30, 0.5f, -2.f},  // holes in the frame and in the view
      {120, 160, 120, 160, 0, 2.0, 0, 0.02f, -2.f},  // a tight gate
      {120, 160, 120, 160, 0, 2.0, 5, 0.5f, 0.9f},   // the normal gate: the four neighbours are read
      {1, 1, 120, 160, 0, 0.0, 0, 0.5f, 0.9f},
      {7, 9, 120, 160, 0, 3.0, 0, 0.5f, 0.9f},
      {17, 19, 120, 160, 0, 3.0, 10, 0.5f, -2.f},
      {3, 3, 1, 1, 0, 0.0, 0, 0.5f, 0.9f},           // a view of one pixel
      {260, 260, 48, 64, 0, 1.0, 0, 0.5f, -2.f},
  };
  int n = 0, total = 0;
  for (const Case& k : cases) {
    int pairs = 0;
    const int rc = run(k, &pairs);
    if (rc) {
      std::fprintf(stderr, "case %d (%d x %d against %d x %d) failed at check %d\n", n, k.rows_s, k.cols_s, k.rows_v, k.cols_v, rc);
      return 1;
    }
    if (n == 2 && pairs != 0) return 2;  // all BEHIND
    if (n == 0 && pairs < 6) return 2;
    total += pairs;
    ++n;
  }
  // the refusals touch nothing
  uint16_t px[1] = {10000};
  float one[1] = {0.f};
  const float* view[7] = {one, one, one, one, one, one, one};
  double I[16];
  pose_of(0, 0, 0, 0, I);
  int32_t pix[1] = {7};
  float d[1] = {7.f};
  icpk_projective_params p;
  icpk_default_projective_params(&p);
  if (icpk_projective_pixels(&p, I, px, 1, 1, view, 1, 1, 1.f, 0.f, I, 0, 1, pix, d, nullptr) < 0 || pix[0] == 7) return 3;
  pix[0] = 7, d[0] = 7.f;
  icpk_projective_params bad = p;
  bad.max_dist = 0.f;
  if (icpk_projective_pixels(&bad, I, px, 1, 1, view, 1, 1, 1.f, 0.f, I, 0, 1, pix, d, nullptr) != ICPK_E_ARG) return 4;
  bad = p, bad.max_iterations = 65;
  if (icpk_projective_pixels(&bad, I, px, 1, 1, view, 1, 1, 1.f, 0.f, I, 0, 1, pix, d, nullptr) != ICPK_E_ARG) return 4;
  if (icpk_projective_pixels(&p, nullptr, px, 1, 1, view, 1, 1, 1.f, 0.f, I, 0, 1, pix, d, nullptr) != ICPK_E_ARG ||
      icpk_projective_pixels(&p, I, px, 1, 1, view, 1, 1, 1.f, 0.f, I, 1, 1, pix, d, nullptr) != ICPK_E_ARG ||
      icpk_projective_pixels(&p, I, px, 1, 1, view, 1, 1, 0.f, 0.f, I, 0, 1, pix, d, nullptr) != ICPK_E_ARG || pix[0] != 7 || d[0] != 7.f)
    return 5;
  std::printf("projective host: ok (%d cases, %d pairs)\n", n, total);
  return 0;
}
