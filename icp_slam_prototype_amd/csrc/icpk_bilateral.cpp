// icpk_bilateral.cpp -- K22, the host-only half of the bilateral filter (include/icpk.h, THE BILATERAL RULE): the
// parameter check, the two tables, and the rule over a host image through the header the kernel includes.  The
// entry points that use the device are in icpk_frontend.cpp, next to the image buffers they share with K4 and K6.
#include <cmath>
#include <vector>

#include "bilateral_rule.h"
#include "icpk.h"

extern "C" {

void icpk_default_bilateral_params(icpk_bilateral_params* p) {
  if (!p) return;
  p->radius = 3;
  p->sigma_space = 2.0f;
  p->sigma_range = 30.0f;
  p->range_cutoff = 0;
}

int icpk_bilateral_tables(const icpk_bilateral_params* params, uint16_t* ws, uint16_t* wr, int32_t* K) {
  icpk_bilateral_params p;
  if (params)
    p = *params;
  else
    icpk_default_bilateral_params(&p);
  if (p.radius < 1 || p.radius > ICPK_BILATERAL_MAX_RADIUS || !std::isfinite(p.sigma_space) || !(p.sigma_space > 0.f) ||
      !std::isfinite(p.sigma_range) || !(p.sigma_range > 0.f) || p.range_cutoff < 0 ||
      p.range_cutoff > ICPK_BILATERAL_MAX_RANGE)
    return ICPK_E_ARG;
  const double ss = p.sigma_space, sr = p.sigma_range;
  const double k_auto = std::floor(3.0 * sr) + 1.0;
  if (p.range_cutoff == 0 && k_auto > (double)ICPK_BILATERAL_MAX_RANGE) return ICPK_E_ARG;  // (refused, not clamped)
  const int k_count = p.range_cutoff ? p.range_cutoff : (int)k_auto;
  if (K) *K = k_count;
  if (ws)
    for (int dy = -p.radius; dy <= p.radius; ++dy)
      for (int dx = -p.radius; dx <= p.radius; ++dx)
        *ws++ = (uint16_t)(int)std::floor(4096.0 * std::exp(-(double)(dx * dx + dy * dy) / (2.0 * ss * ss)) + 0.5);
  if (wr)
    for (int k = 0; k < k_count; ++k)
      wr[k] = (uint16_t)(int)std::floor(4096.0 * std::exp(-((double)k * k) / (2.0 * sr * sr)) + 0.5);
  return ICPK_OK;
}

int icpk_bilateral_host(const icpk_bilateral_params* params, const uint16_t* depth_in, int32_t rows, int32_t cols,
                        uint16_t* depth_out) {
  if (!depth_in || !depth_out || rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28)) return ICPK_E_ARG;
  icpk_bilateral_params p;
  if (params)
    p = *params;
  else
    icpk_default_bilateral_params(&p);
  constexpr int side_max = 2 * ICPK_BILATERAL_MAX_RADIUS + 1;
  uint16_t ws[side_max * side_max];
  std::vector<uint16_t> wr(ICPK_BILATERAL_MAX_RANGE);
  int32_t K = 0;
  const int rc = icpk_bilateral_tables(&p, ws, wr.data(), &K);
  if (rc) return rc;
  std::vector<uint16_t> copy;
  if (depth_out == depth_in) {  // every output pixel reads its neighbours' INPUT
    copy.assign(depth_in, depth_in + (size_t)rows * cols);
    depth_in = copy.data();
  }
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      depth_out[(size_t)y * cols + x] = icpk::bilateral_pixel(p.radius, K, ws, wr.data(), [=](int dy, int dx) {
        const int v = y + dy, u = x + dx;
        return v >= 0 && v < rows && u >= 0 && u < cols ? (int)depth_in[(size_t)v * cols + u] : 0;
      });
  return ICPK_OK;
}

}  // extern "C"
