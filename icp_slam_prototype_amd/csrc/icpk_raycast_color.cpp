// icpk_raycast_color.cpp -- K26, the host-only half of the view's colour gradients (include/icpk.h, THE VIEW GRADIENT
// RULE): the rule over eight host planes through the header the kernel includes.  It needs no context and no device and
// refers to nothing else of the library; the entry points that use the device are in icpk_tsdf.cpp, next to the maps.
#include <cmath>

#include "icpk.h"
#include "raycast_color_rule.h"

extern "C" {

int icpk_raycast_color_gradients_host(const float* const view[8], int32_t rows, int32_t cols, float radius,
                                      int32_t min_neighbors, int64_t first, int32_t count, int64_t* sums, float* g) {
  if (!view || rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28) || first < 0 || count < 0) return ICPK_E_ARG;
  for (int k = 0; k < 8; ++k)
    if (!view[k]) return ICPK_E_ARG;
  if (!(std::isfinite(radius) && radius > 0.f) || min_neighbors < 1) return ICPK_E_ARG;
  if (first + count > (int64_t)rows * cols) return ICPK_E_ARG;
  const icpk::RayColorView v{view[0], view[1], view[2], view[3], view[4], view[5], view[6], view[7], rows, cols};
  int with_gradient = 0;
  for (int32_t e = 0; e < count; ++e) {
    const int64_t i = first + e;
    long long S[icpk::RAY_COLOR_SUMS];
    float ge[3];
    icpk::ray_color_pixel(v, (int)(i / cols), (int)(i % cols), radius, min_neighbors, S, ge);
    if (sums)
      for (int k = 0; k < icpk::RAY_COLOR_SUMS; ++k) sums[(size_t)e * icpk::RAY_COLOR_SUMS + k] = S[k];
    if (g) g[3 * (size_t)e] = ge[0], g[3 * (size_t)e + 1] = ge[1], g[3 * (size_t)e + 2] = ge[2];
    with_gradient += ge[0] != 0.f || ge[1] != 0.f || ge[2] != 0.f;
  }
  return with_gradient;
}

}  // extern "C"
