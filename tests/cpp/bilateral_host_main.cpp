// tests/cpp/bilateral_host_main.cpp -- DIAGNOSTIC (build.program("bilateral_host_sanitized")): icpk_bilateral_tables and
// icpk_bilateral_host over the shapes of the host cases, in a program of its own so that the host code can run under
// -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.  The arrays are exactly as
// large as the header says they must be, so a read or write past them is caught; the rule's invariants are checked on
// every image.  Exit status 0 and "bilateral host: ok" when everything held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int run(int rows, int cols, int radius, float sigma_space, float sigma_range, int cutoff, int kind, bool in_place) {
  icpk_bilateral_params p{radius, sigma_space, sigma_range, cutoff};
  int32_t K = 0;
  if (icpk_bilateral_tables(&p, nullptr, nullptr, &K) != ICPK_OK) return 1;
  std::vector<uint16_t> ws((size_t)(2 * radius + 1) * (2 * radius + 1)), wr((size_t)K);
  if (icpk_bilateral_tables(&p, ws.data(), wr.data(), nullptr) != ICPK_OK) return 2;
  if (ws[ws.size() / 2] != 4096 || wr[0] != 4096) return 3;
  std::vector<uint16_t> in((size_t)rows * cols), out((size_t)rows * cols, 7);
  uint32_t s = 22u + (uint32_t)kind;
  for (size_t i = 0; i < in.size(); ++i) {
    const uint32_t r = lcg(s) >> 8;
    switch (kind) {
      case 0: in[i] = (uint16_t)(5000 + r % 81); break;                                     // a noisy plane
      case 1: in[i] = r % 10 < 3 ? (uint16_t)(5000 + (r >> 4) % 81) : 0; break;             // 30 % valid
      case 2: in[i] = 65535; break;                                                         // the accumulator's upper end
      case 3: in[i] = 1; break;
      default: in[i] = (uint16_t)(r % 65536); break;                                        // everything, steps everywhere
    }
  }
  const std::vector<uint16_t> keep = in;
  uint16_t* dst = in_place ? in.data() : out.data();
  if (icpk_bilateral_host(&p, in.data(), rows, cols, dst) != ICPK_OK) return 4;
  for (size_t i = 0; i < keep.size(); ++i) {
    const int a = keep[i], b = dst[i];
    if ((a != 0) != (b != 0) || std::abs(a - b) > K - 1) return 5;
    if ((kind == 2 || kind == 3) && a != b) return 6;
  }
  return 0;
}

int main() {
  const int shapes[][2] = {{120, 160}, {37, 53}, {1, 1}, {1, 40}, {40, 1}, {16, 64}, {17, 65}};
  int n = 0;
  for (const auto& sh : shapes)
    for (int kind = 0; kind < 5; ++kind)
      for (int radius : {1, 3, 6}) {
        const int rc = run(sh[0], sh[1], radius, 2.0f, 30.0f, 0, kind, (n & 1) != 0);
        if (rc) {
          std::fprintf(stderr, "case %d x %d kind %d radius %d failed at check %d\n", sh[0], sh[1], kind, radius, rc);
          return 1;
        }
        ++n;
      }
  if (run(40, 70, 3, 2.0f, 1365.0f, 0, 4, false) || run(40, 70, 3, 2.0f, 30.0f, 1, 0, true) ||
      run(40, 70, 6, 0.5f, 0.25f, 4096, 4, false))
    return 2;
  // the refusals touch nothing
  icpk_bilateral_params bad{0, 2.0f, 30.0f, 0};
  uint16_t px[1] = {900}, o[1] = {7};
  if (icpk_bilateral_host(&bad, px, 1, 1, o) != ICPK_E_ARG || o[0] != 7) return 3;
  bad = {3, 2.0f, 1365.4f, 0};
  if (icpk_bilateral_tables(&bad, nullptr, nullptr, nullptr) != ICPK_E_ARG) return 4;
  if (icpk_bilateral_host(nullptr, nullptr, 1, 1, o) != ICPK_E_ARG || icpk_bilateral_host(nullptr, px, 0, 1, o) != ICPK_E_ARG)
    return 5;
  std::printf("bilateral host: ok (%d images)\n", n + 3);
  return 0;
}
