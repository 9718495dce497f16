// icpk_pyramid.cpp -- K24, the host-only half of the depth pyramid (include/icpk.h, THE PYRAMID RULE): the defaults,
// the parameter check, and the rule over a host image through the header the kernel includes.  The entry points that
// use the device are in icpk_frontend.cpp, next to the image buffers and the back-projection they share with K4 and K22.
#include <cstring>
#include <vector>

#include "icpk.h"
#include "pyramid_rule.h"

extern "C" {

void icpk_default_pyramid_params(icpk_pyramid_params* p) {
  if (!p) return;
  p->levels = 3;
  p->range_cutoff = 91;
}

int icpk_depth_pyramid_host(const icpk_pyramid_params* params, const uint16_t* depth_in, int32_t rows, int32_t cols,
                            int32_t level, uint16_t* out) {
  if (!depth_in || !out || rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  icpk_pyramid_params p;
  if (params)
    p = *params;
  else
    icpk_default_pyramid_params(&p);
  if (p.levels < 1 || p.levels > ICPK_PYRAMID_MAX_LEVELS || p.range_cutoff < 1 || p.range_cutoff > 65536 || level < 0 ||
      level >= p.levels)
    return ICPK_E_ARG;
  if (level == 0) {
    if (out != depth_in) std::memmove(out, depth_in, (size_t)rows * cols * sizeof(uint16_t));
    return ICPK_OK;
  }
  // every level on the way is a buffer of exactly its size; the last one is the caller's
  std::vector<uint16_t> a, b;
  const uint16_t* src = depth_in;
  if (out == depth_in) {  // level 1 would be written over the pixels it still has to read
    a.assign(depth_in, depth_in + (size_t)rows * cols);
    src = a.data();
  }
  int r0 = rows, c0 = cols;
  for (int l = 1; l <= level; ++l) {
    const int r1 = icpk::pyramid_half(r0), c1 = icpk::pyramid_half(c0);
    uint16_t* dst = out;
    if (l < level) {
      b.assign((size_t)r1 * c1, 0);
      dst = b.data();
    }
    const int K = p.range_cutoff;
    for (int y = 0; y < r1; ++y)
      for (int x = 0; x < c1; ++x)
        dst[(size_t)y * c1 + x] = icpk::pyramid_pixel(K, [=](int dy, int dx) {
          const int v = 2 * y + dy, u = 2 * x + dx;
          return v >= 0 && v < r0 && u >= 0 && u < c0 ? (int)src[(size_t)v * c0 + u] : 0;
        });
    a.swap(b);
    src = a.data();
    r0 = r1;
    c0 = c1;
  }
  return ICPK_OK;
}

int icpk_intensity_pyramid_host(const icpk_pyramid_params* params, const uint16_t* depth_in, const float* intensity_in,
                                int32_t rows, int32_t cols, int32_t level, float* out) {
  if (!depth_in || !intensity_in || !out || rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  icpk_pyramid_params p;
  if (params)
    p = *params;
  else
    icpk_default_pyramid_params(&p);
  if (p.levels < 1 || p.levels > ICPK_PYRAMID_MAX_LEVELS || p.range_cutoff < 1 || p.range_cutoff > 65536 || level < 0 ||
      level >= p.levels)
    return ICPK_E_ARG;
  const size_t npix = (size_t)rows * cols;
  for (size_t i = 0; i < npix; ++i)
    if (!(intensity_in[i] >= 0.f && intensity_in[i] <= 1.f)) return ICPK_E_ARG;
  if (level == 0) {
    if (out != intensity_in) std::memmove(out, intensity_in, npix * sizeof(float));
    return ICPK_OK;
  }
  // both pyramids level by level, every level a buffer of exactly its size; the last intensity level is the caller's
  std::vector<uint16_t> d0(depth_in, depth_in + npix), d1;
  std::vector<float> i0(intensity_in, intensity_in + npix), i1;
  int r0 = rows, c0 = cols;
  const int K = p.range_cutoff;
  for (int l = 1; l <= level; ++l) {
    const int r1 = icpk::pyramid_half(r0), c1 = icpk::pyramid_half(c0);
    float* dst = out;
    if (l < level) {
      i1.assign((size_t)r1 * c1, 0.f);
      dst = i1.data();
      d1.assign((size_t)r1 * c1, 0);
    }
    const uint16_t* ds = d0.data();
    const float* is = i0.data();
    for (int y = 0; y < r1; ++y)
      for (int x = 0; x < c1; ++x) {
        auto dtap = [=](int dy, int dx) {
          const int v = 2 * y + dy, u = 2 * x + dx;
          return v >= 0 && v < r0 && u >= 0 && u < c0 ? (int)ds[(size_t)v * c0 + u] : 0;
        };
        dst[(size_t)y * c1 + x] =
            icpk::pyramid_intensity_pixel(K, dtap, [=](int dy, int dx) { return is[(size_t)(2 * y + dy) * c0 + (2 * x + dx)]; });
        if (l < level) d1[(size_t)y * c1 + x] = icpk::pyramid_pixel(K, dtap);
      }
    if (l < level) {
      d0.swap(d1);
      i0.swap(i1);
    }
    r0 = r1;
    c0 = c1;
  }
  return ICPK_OK;
}

}  // extern "C"
