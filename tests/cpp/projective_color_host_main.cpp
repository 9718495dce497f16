// tests/cpp/projective_color_host_main.cpp -- DIAGNOSTIC (build.program("projective_color_host_sanitized")): the three
// host-only functions of K26 -- icpk_intensity_pyramid_host, icpk_raycast_color_gradients_host and
// icpk_projective_pixels_colored -- in a program of its own, so that the host code (icpk_pyramid.cpp,
// icpk_raycast_color.cpp, icpk_projective.cpp and so csrc/pyramid_rule.h, raycast_color_rule.h, projective_rule.h) can
// run under -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.  Every array is
// allocated at exactly the size the header asks for, so a read or write past any of them is caught; windows at the
// start, inside and at the last pixel; the refusals.  Exit status 0 and "projective colour host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)((lcg(s) >> 8) & 0xffff) / 65535.0f; }

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      return __LINE__;                                               \
    }                                                                \
  } while (0)

// the intensity pyramid of a rows x cols image with holes, every level into a buffer of exactly its size
static int pyramid(int rows, int cols, int levels, int K) {
  const size_t n = (size_t)rows * cols;
  uint32_t s = 26u + (uint32_t)(n % 89);
  std::vector<uint16_t> depth(n);
  std::vector<float> inten(n);
  for (size_t i = 0; i < n; ++i) {
    depth[i] = (lcg(s) >> 8) % 10 == 0 ? 0 : (uint16_t)(5000 + (lcg(s) >> 8) % 80);
    inten[i] = unit(s);
  }
  inten[0] = 1.f, inten[n - 1] = 0.f;
  icpk_pyramid_params p;
  icpk_default_pyramid_params(&p);
  p.levels = levels, p.range_cutoff = K;
  int r = rows, c = cols;
  for (int l = 0; l < levels; ++l) {
    std::vector<float> out((size_t)r * c, -1.f);
    std::vector<uint16_t> mask((size_t)r * c);
    CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, l, out.data()) == ICPK_OK);
    CHECK(icpk_depth_pyramid_host(&p, depth.data(), rows, cols, l, mask.data()) == ICPK_OK);
    for (size_t i = 0; i < out.size(); ++i) {
      CHECK(out[i] >= 0.f && out[i] <= 1.f);
      CHECK(l == 0 || mask[i] != 0 || out[i] == 0.f);
    }
    r = (r + 1) / 2, c = (c + 1) / 2;
  }
  std::vector<float> out(n);
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, levels, out.data()) == ICPK_E_ARG);
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, -1, out.data()) == ICPK_E_ARG);
  CHECK(icpk_intensity_pyramid_host(&p, nullptr, inten.data(), rows, cols, 0, out.data()) == ICPK_E_ARG);
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), nullptr, rows, cols, 0, out.data()) == ICPK_E_ARG);
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, 0, nullptr) == ICPK_E_ARG);
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), 0, cols, 0, out.data()) == ICPK_E_ARG);
  inten[n / 2] = 1.5f;
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, 0, out.data()) == ICPK_E_ARG);
  inten[n / 2] = NAN;
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, 0, out.data()) == ICPK_E_ARG);
  // level 0 in place
  inten[n / 2] = 0.5f;
  CHECK(icpk_intensity_pyramid_host(&p, depth.data(), inten.data(), rows, cols, 0, inten.data()) == ICPK_OK);
  return 0;
}

// A view of rows x cols: a slanted plane with holes, some zero normals and a NaN point; eight planes of exactly
// rows x cols floats.
struct View {
  int rows, cols;
  std::vector<std::vector<float>> plane;
  const float* ptr[8];
  View(int r, int c, int holes) : rows(r), cols(c), plane(8, std::vector<float>((size_t)r * c, 0.f)) {
    uint32_t s = 7u + (uint32_t)(r * 131 + c);
    const float nl = std::sqrt(0.02f * 0.02f + 0.01f * 0.01f + 1.f);
    for (int y = 0; y < r; ++y)
      for (int x = 0; x < c; ++x) {
        const size_t j = (size_t)y * c + x;
        if ((int)((lcg(s) >> 8) % 100) < holes) continue;
        const float z = 1.f + 0.02f * x + 0.01f * y;
        plane[0][j] = 0.03f * x, plane[1][j] = 0.03f * y, plane[2][j] = z, plane[6][j] = z;
        if ((lcg(s) >> 8) % 17 != 0) plane[3][j] = -0.02f / nl, plane[4][j] = -0.01f / nl, plane[5][j] = 1.f / nl;
        plane[7][j] = unit(s);
      }
    if (r * c > 20) plane[0][(size_t)r * c / 2] = NAN;
    for (int a = 0; a < 8; ++a) ptr[a] = plane[a].data();
  }
};

static int gradients(int rows, int cols, int holes, float radius, int min_nb, std::vector<float>* keep) {
  View v(rows, cols, holes);
  const int64_t n = (int64_t)rows * cols;
  std::vector<int64_t> S((size_t)n * 10, -7);
  std::vector<float> g((size_t)n * 3, -7.f);
  const int with = icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, min_nb, 0, (int32_t)n, S.data(), g.data());
  CHECK(with >= 0);
  int counted = 0;
  for (int64_t i = 0; i < n; ++i) {
    const bool hit = v.plane[6][(size_t)i] > 0.f;
    const bool any = g[3 * i] != 0.f || g[3 * i + 1] != 0.f || g[3 * i + 2] != 0.f;
    counted += any;
    CHECK(S[10 * i] >= 0 && S[10 * i] <= 9 && (hit || (S[10 * i] == 0 && !any)));
    CHECK(!any || S[10 * i] >= min_nb);
    CHECK(std::isfinite(g[3 * i]) && std::isfinite(g[3 * i + 1]) && std::isfinite(g[3 * i + 2]));
  }
  CHECK(counted == with);
  // windows at the start, inside and at the last pixel: exactly-sized outputs each time
  const int64_t wins[4][2] = {{0, 1}, {n / 3, n / 4 + 1}, {n - 1, 1}, {n, 0}};
  for (const auto& w : wins) {
    const int64_t first = w[0], count = first + w[1] > n ? n - first : w[1];
    std::vector<int64_t> Sw((size_t)count * 10);
    std::vector<float> gw((size_t)count * 3);
    CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, min_nb, first, (int32_t)count, count ? Sw.data() : nullptr,
                                            count ? gw.data() : nullptr) >= 0);
    CHECK(count == 0 || std::memcmp(Sw.data(), S.data() + 10 * first, (size_t)count * 80) == 0);
    CHECK(count == 0 || std::memcmp(gw.data(), g.data() + 3 * first, (size_t)count * 12) == 0);
  }
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, min_nb, 0, (int32_t)n, nullptr, nullptr) == with);
  CHECK(icpk_raycast_color_gradients_host(nullptr, rows, cols, radius, min_nb, 0, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, 0.f, min_nb, 0, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, NAN, min_nb, 0, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, 0, 0, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, min_nb, -1, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows, cols, radius, min_nb, n, 1, S.data(), g.data()) == ICPK_E_ARG);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, 0, cols, radius, min_nb, 0, 0, S.data(), g.data()) == ICPK_E_ARG);
  const float* seven[8];
  for (int a = 0; a < 8; ++a) seven[a] = a == 7 ? nullptr : v.ptr[a];
  CHECK(icpk_raycast_color_gradients_host(seven, rows, cols, radius, min_nb, 0, 1, S.data(), g.data()) == ICPK_E_ARG);
  if (keep) *keep = g;
  return 0;
}

// the joint terms over a level of rows_s x cols_s against a view of rows_v x cols_v with its gradients
static int joint(int rows_s, int cols_s, int rows_v, int cols_v, int level, float lambda) {
  View v(rows_v, cols_v, 10);
  if (rows_v * cols_v > 20) v.plane[0][(size_t)rows_v * cols_v / 2] = 0.03f * (cols_v / 2);  // (finite points for the pairs)
  const size_t ns = (size_t)rows_s * cols_s, nv = (size_t)rows_v * cols_v;
  std::vector<float> gi((size_t)nv * 3);
  CHECK(icpk_raycast_color_gradients_host(v.ptr, rows_v, cols_v, 0.08f, 3, 0, (int32_t)nv, nullptr, gi.data()) >= 0);
  std::vector<std::vector<float>> grad(3, std::vector<float>(nv));
  for (size_t j = 0; j < nv; ++j)
    for (int a = 0; a < 3; ++a) grad[a][j] = gi[3 * j + a];
  const float* gp[3] = {grad[0].data(), grad[1].data(), grad[2].data()};
  uint32_t s = 99u + (uint32_t)ns;
  std::vector<uint16_t> depth(ns);
  std::vector<float> inten(ns);
  for (size_t i = 0; i < ns; ++i) {
    depth[i] = (lcg(s) >> 8) % 10 == 0 ? 0 : (uint16_t)(5200 + (lcg(s) >> 8) % 300);
    inten[i] = unit(s);
  }
  icpk_projective_params p;
  icpk_default_projective_params(&p);
  p.level = level;
  p.fx = 30.f * (float)(1 << level), p.cx = 0.f;
  icpk_projective_color_params c;
  icpk_default_projective_color_params(&c);
  c.lambda_geometric = lambda;
  const double I[16] = {1, 0, 0, 0.01, 0, 1, 0, -0.01, 0, 0, 1, 0.02, 0, 0, 0, 1};
  const double V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const float fx_v = 33.f, cx_v = 0.f;
  std::vector<int32_t> pixel(ns), pg(ns);
  std::vector<float> dist(ns), dg(ns);
  std::vector<double> terms(ns * 28), tg(ns * 28);
  const int pairs = icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0,
                                                   (int32_t)ns, pixel.data(), dist.data(), terms.data(), inten.data(), v.ptr[7], gp, &c);
  CHECK(pairs >= 0);
  CHECK(icpk_projective_pixels(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, (int32_t)ns, pg.data(),
                               dg.data(), tg.data()) == pairs);
  CHECK(std::memcmp(pixel.data(), pg.data(), ns * 4) == 0 && std::memcmp(dist.data(), dg.data(), ns * 4) == 0);
  if (lambda == 1.f) CHECK(std::memcmp(terms.data(), tg.data(), ns * 28 * 8) == 0);
  for (size_t i = 0; i < ns; ++i)
    for (int k = 0; k < 28; ++k) CHECK(std::isfinite(terms[i * 28 + k]) && (pixel[i] >= 0 || terms[i * 28 + k] == 0.0));
  // windows
  const int64_t n = (int64_t)ns;
  const int64_t wins[3][2] = {{0, 1}, {n / 2, n / 3 + 1}, {n - 1, 1}};
  for (const auto& w : wins) {
    const int64_t first = w[0], count = first + w[1] > n ? n - first : w[1];
    std::vector<int32_t> pw((size_t)count);
    std::vector<float> dw((size_t)count);
    std::vector<double> tw((size_t)count * 28);
    CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, first,
                                         (int32_t)count, pw.data(), dw.data(), tw.data(), inten.data(), v.ptr[7], gp, &c) >= 0);
    CHECK(std::memcmp(pw.data(), pixel.data() + first, (size_t)count * 4) == 0);
    CHECK(std::memcmp(tw.data(), terms.data() + 28 * first, (size_t)count * 28 * 8) == 0);
  }
  // the refusals
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, nullptr, v.ptr[7], gp, &c) == ICPK_E_ARG);
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), nullptr, gp, &c) == ICPK_E_ARG);
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), v.ptr[7], nullptr, &c) == ICPK_E_ARG);
  icpk_projective_color_params bad = c;
  bad.lambda_geometric = 1.5f;
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), v.ptr[7], gp, &bad) == ICPK_E_ARG);
  bad.lambda_geometric = NAN;
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), v.ptr[7], gp, &bad) == ICPK_E_ARG);
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, n, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), v.ptr[7], gp, &c) == ICPK_E_ARG);
  CHECK(icpk_projective_pixels_colored(&p, I, depth.data(), rows_s, cols_s, v.ptr, rows_v, cols_v, fx_v, cx_v, V, 0, 1, pixel.data(),
                                       dist.data(), nullptr, inten.data(), v.ptr[7], gp, nullptr) >= 0);  // (NULL: the defaults)
  return pairs > 0 || ns < 4 ? 0 : __LINE__;
}

int main() {
  const int shapes[6][2] = {{1, 1}, {1, 40}, {40, 1}, {3, 3}, {17, 65}, {68, 260}};
  for (const auto& sh : shapes)
    for (int K : {1, 91})
      if (int rc = pyramid(sh[0], sh[1], sh[0] * sh[1] > 100 ? 8 : 3, K)) return std::fprintf(stderr, "pyramid %d x %d failed\n", sh[0], sh[1]), rc;
  const int views[6][2] = {{1, 1}, {1, 5}, {7, 9}, {17, 65}, {48, 64}, {120, 160}};
  for (const auto& sh : views) {
    if (int rc = gradients(sh[0], sh[1], 15, 0.08f, 3, nullptr)) return std::fprintf(stderr, "gradients %d x %d failed\n", sh[0], sh[1]), rc;
    if (int rc = gradients(sh[0], sh[1], 0, 1e-4f, 1, nullptr)) return rc;  // only the centre counts
    if (int rc = gradients(sh[0], sh[1], 30, 1.0f, 9, nullptr)) return rc;
  }
  const int joints[5][5] = {{1, 1, 7, 9, 0}, {7, 9, 17, 19, 0}, {17, 19, 48, 64, 1}, {60, 80, 120, 160, 1}, {260, 260, 48, 64, 0}};
  for (const auto& j : joints)
    for (float lambda : {0.f, 0.5f, 0.968f, 1.f})
      if (int rc = joint(j[0], j[1], j[2], j[3], j[4], lambda)) return std::fprintf(stderr, "joint %d x %d failed\n", j[0], j[1]), rc;
  std::printf("projective colour host: ok\n");
  return 0;
}
