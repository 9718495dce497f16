// pyramid_rule.h -- the pyramid rule (K24) for one pixel; include/icpk.h writes it out ("THE PYRAMID RULE").
// Header-inline and __host__ __device__: kernels_pyramid.hip runs it per output pixel on the device over LDS windows,
// icpk_pyramid.cpp runs it over host images (icpk_depth_pyramid_host).  Integers only: the result is a function of the
// image and K alone, whatever the order of the taps and whoever computes it.
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

// rows or columns of the level above one of n
ICPK_HD int pyramid_half(int n) { return (n + 1) / 2; }

// floor(n / m) for m > 0: C's division truncates towards zero
ICPK_HD int pyramid_floor_div(int n, int m) {
  const int q = n / m;
  return n - q * m < 0 ? q - 1 : q;
}

// One pixel of level l + 1.  tap(dy, dx): the depth of level l at that offset from the centre pixel (2 r, 2 c), 0 for a
// position outside the image (which the rule skips as it skips a hole).  K: 1 .. 65536.
// S <= 16 and |D| <= 16 * 65535, so 2 D + S stays far inside an int.
template <class Tap>
ICPK_HD uint16_t pyramid_pixel(int K, Tap tap) {
  const int dc = tap(0, 0);
  if (dc == 0) return 0;  // the mask is the mask below, subsampled
  int S = 0, D = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int dq = tap(dy, dx);
      const int diff = dq - dc, k = diff < 0 ? -diff : diff;
      if (dq == 0 || k >= K) continue;
      const int w = (2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx));  // 1, 2 or 4
      S += w;
      D += w * diff;
    }
  // the centre always counts: S >= 4
  return (uint16_t)(dc + pyramid_floor_div(2 * D + S, 2 * S));
}

// THE INTENSITY PYRAMID RULE (K26) for one pixel of level l + 1.  dtap as above; itap(dy, dx): the intensity of level l
// at that offset, asked for only where the depth tap counts (so never outside the image).  The taps that count and
// their weights are pyramid_pixel's; integers up to the one final division.  |c_q| <= 2^15 and S <= 16: N fits an int.
template <class DTap, class ITap>
ICPK_HD float pyramid_intensity_pixel(int K, DTap dtap, ITap itap) {
  const int dc = dtap(0, 0);
  if (dc == 0) return 0.f;  // the mask is the depth level's
  int S = 0, N = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int dq = dtap(dy, dx);
      const int diff = dq - dc, k = diff < 0 ? -diff : diff;
      if (dq == 0 || k >= K) continue;
      const int w = (2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx));
      S += w;
      N += w * (int)__builtin_rint((double)itap(dy, dx) * 32768.0);
    }
  return (float)((double)N / ((double)S * 32768.0));
}

}  // namespace icpk
