// bilateral_rule.h -- the bilateral rule (K22) for one pixel; include/icpk.h writes it out ("THE BILATERAL RULE").
// Header-inline and __host__ __device__: kernels_bilateral.hip runs it per output pixel on the device over an LDS tile,
// icpk_bilateral.cpp runs it over the host image (icpk_bilateral_host).  Integers only: the result is a function of
// the image and the two tables alone, whatever the order of the taps and whoever computes it.
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

// floor(n / m) for m > 0 and a quotient of small magnitude (here |n / m| < 4096): a float estimate, corrected in
// integers until 0 <= n - q m < m.  The estimate is off by a few units at the most, so the loops run once or twice;
// the result does not depend on how the float division rounds.
ICPK_HD int bilateral_floor_div(int64_t n, int64_t m) {
  int q = (int)((float)n / (float)m);
  int64_t r = n - (int64_t)q * m;
  while (r < 0) {
    --q;
    r += m;
  }
  while (r >= m) {
    ++q;
    r -= m;
  }
  return q;
}

// One output pixel.  tap(dy, dx): the depth at that offset from the pixel, 0 for a position outside the image (which
// the rule skips as it skips a hole); ws: (2 radius + 1)^2 spatial weights, row-major; wr: K range weights.
// With D = sum W (d_q - d_p), S_wd = d_p S_w + D, so floor((2 S_wd + S_w) / (2 S_w)) = d_p + floor((2 D + S_w) / (2 S_w)):
// |W (d_q - d_p)| < 2^24 * 2^12 and 169 of them stay below 2^44.
template <class Tap>
ICPK_HD uint16_t bilateral_pixel(int radius, int K, const uint16_t* ws, const uint16_t* wr, Tap tap) {
  const int dp = tap(0, 0);
  if (dp == 0) return 0;  // holes are not filled
  uint32_t sw = 0;
  int64_t sd = 0;
  const uint16_t* w = ws;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx, ++w) {
      const int dq = tap(dy, dx);
      const int diff = dq - dp, k = diff < 0 ? -diff : diff;
      if (dq == 0 || k >= K) continue;  // (wr is read only below K)
      const int32_t W = (int32_t)*w * (int32_t)wr[k];  // <= 2^24
      sw += (uint32_t)W;
      sd += (int64_t)W * diff;
    }
  // the centre always contributes: sw >= 2^24
  return (uint16_t)(dp + bilateral_floor_div(2 * sd + (int64_t)sw, 2 * (int64_t)sw));
}

}  // namespace icpk
