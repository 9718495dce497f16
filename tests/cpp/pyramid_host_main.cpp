// tests/cpp/pyramid_host_main.cpp -- DIAGNOSTIC (build.program("pyramid_host_sanitized")): icpk_depth_pyramid_host over the
// shapes of the host and tile cases, in a program of its own so that the host code can run under
// -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.  Every image is allocated
// at exactly the size the header asks for -- the input rows x cols, the output its level's (rows + 1) / 2 by
// (cols + 1) / 2, level by level -- so a read or write past either is caught; the rule's consequences are checked on
// every level.  Exit status 0 and "pyramid host: ok" when everything held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int run(int rows, int cols, int levels, int K, int kind) {
  icpk_pyramid_params p{levels, K};
  std::vector<uint16_t> in((size_t)rows * cols);
  uint32_t s = 24u + (uint32_t)kind;
  for (size_t i = 0; i < in.size(); ++i) {
    const uint32_t r = lcg(s) >> 8;
    switch (kind) {
      case 0: in[i] = (uint16_t)(5000 + r % 81); break;                          // a noisy plane
      case 1: in[i] = r % 10 < 3 ? (uint16_t)(5000 + (r >> 4) % 81) : 0; break;  // 30 % valid
      case 2: in[i] = 65535; break;                                              // the upper end
      case 3: in[i] = 1; break;
      default: in[i] = (uint16_t)(r % 65536); break;                             // everything, steps everywhere
    }
  }
  const std::vector<uint16_t> keep = in;
  std::vector<uint16_t> below = in;
  int r0 = rows, c0 = cols;
  for (int l = 0; l < levels; ++l) {
    const int r1 = l ? (r0 + 1) / 2 : rows, c1 = l ? (c0 + 1) / 2 : cols;
    std::vector<uint16_t> out((size_t)r1 * c1, 7);  // exactly the level's size
    if (icpk_depth_pyramid_host(&p, in.data(), rows, cols, l, out.data()) != ICPK_OK) return 1;
    if (in != keep) return 2;  // the input is read only
    if (l == 0) {
      if (out != keep) return 3;
    } else {
      for (int y = 0; y < r1; ++y)
        for (int x = 0; x < c1; ++x) {
          const int a = below[(size_t)(2 * y) * c0 + 2 * x], b = out[(size_t)y * c1 + x];
          if ((a != 0) != (b != 0) || std::abs(a - b) > K - 1) return 4;
          if ((kind == 2 || kind == 3 || K == 1) && a != b) return 5;
        }
    }
    below = out;
    r0 = r1;
    c0 = c1;
  }
  return 0;
}

int main() {
  const int shapes[][2] = {{120, 160}, {37, 53}, {1, 1}, {1, 40}, {40, 1}, {2, 2}, {3, 3}, {21, 70}, {30, 70},
                           {16, 64}, {17, 65}, {65, 131}, {68, 260}};
  int n = 0;
  for (const auto& sh : shapes)
    for (int kind = 0; kind < 5; ++kind)
      for (int levels : {1, 2, 3, 4, 8}) {
        const int K = kind == 2 ? 65536 : kind == 4 ? 1 + (n % 3) * 700 : 91;
        const int rc = run(sh[0], sh[1], levels, K, kind);
        if (rc) {
          std::fprintf(stderr, "case %d x %d kind %d levels %d K %d failed at check %d\n", sh[0], sh[1], kind, levels, K, rc);
          return 1;
        }
        ++n;
      }
  if (run(480, 640, 3, 91, 0) || run(480, 640, 8, 65536, 4)) return 2;
  // in place: level 1 over the image it is made from, and level 0 onto itself
  {
    std::vector<uint16_t> a((size_t)37 * 53), want((size_t)19 * 27);
    uint32_t s = 5u;
    for (auto& v : a) v = (uint16_t)(4000 + (lcg(s) >> 8) % 200);
    if (icpk_depth_pyramid_host(nullptr, a.data(), 37, 53, 1, want.data()) != ICPK_OK) return 3;
    const std::vector<uint16_t> keep = a;
    if (icpk_depth_pyramid_host(nullptr, a.data(), 37, 53, 0, a.data()) != ICPK_OK || a != keep) return 3;
    if (icpk_depth_pyramid_host(nullptr, a.data(), 37, 53, 1, a.data()) != ICPK_OK) return 3;
    for (size_t i = 0; i < a.size(); ++i)
      if (a[i] != (i < want.size() ? want[i] : keep[i])) return 3;
  }
  // the refusals touch nothing
  uint16_t px[1] = {900}, o[1] = {7};
  icpk_pyramid_params bad{0, 91};
  if (icpk_depth_pyramid_host(&bad, px, 1, 1, 0, o) != ICPK_E_ARG) return 4;
  bad = {9, 91};
  if (icpk_depth_pyramid_host(&bad, px, 1, 1, 0, o) != ICPK_E_ARG) return 4;
  bad = {3, 0};
  if (icpk_depth_pyramid_host(&bad, px, 1, 1, 0, o) != ICPK_E_ARG) return 4;
  bad = {3, 65537};
  if (icpk_depth_pyramid_host(&bad, px, 1, 1, 0, o) != ICPK_E_ARG) return 4;
  if (icpk_depth_pyramid_host(nullptr, nullptr, 1, 1, 0, o) != ICPK_E_ARG || icpk_depth_pyramid_host(nullptr, px, 0, 1, 0, o) != ICPK_E_ARG ||
      icpk_depth_pyramid_host(nullptr, px, 1, 1, 3, o) != ICPK_E_ARG || icpk_depth_pyramid_host(nullptr, px, 1, 1, -1, o) != ICPK_E_ARG ||
      icpk_depth_pyramid_host(nullptr, px, 1, 1, 0, nullptr) != ICPK_E_ARG || o[0] != 7)
    return 5;
  std::printf("pyramid host: ok (%d pyramids)\n", n + 2);
  return 0;
}
