// kernels_bilateral.hip -- K22: the exact bilateral filter of a uint16 depth image (include/icpk.h, THE BILATERAL
// RULE; the rule itself is csrc/bilateral_rule.h, shared with the host function).
// One 256-thread workgroup = a 64 x 16 tile of output pixels (K6's geometry).  It stages the tile plus a halo of
// `radius` pixels, the spatial table and the K range weights into LDS; every tap then reads LDS only.  Out-of-image
// positions are staged as 0, which the rule skips as it skips a hole.  One thread owns an output pixel from its first
// tap to its store; no atomic, nothing shared is written after the one barrier.
#include "bilateral_rule.h"
#include "icpk.h"
#include "icpk_internal.h"

namespace icpk {

constexpr int BL_TW = 64, BL_TH = 16;
constexpr int BL_IW = BL_TW + 2 * ICPK_BILATERAL_MAX_RADIUS, BL_IH = BL_TH + 2 * ICPK_BILATERAL_MAX_RADIUS;  // 76 x 28
constexpr int BL_WS = (2 * ICPK_BILATERAL_MAX_RADIUS + 1) * (2 * ICPK_BILATERAL_MAX_RADIUS + 1);              // 169

// tables: (2 radius + 1)^2 spatial weights, then K range weights
__global__ __launch_bounds__(256) void depth_bilateral_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                              int rows, int cols, int radius, int K,
                                                              const uint16_t* __restrict__ tables) {
  __shared__ uint16_t tile[BL_IH][BL_IW];
  __shared__ uint16_t ws[BL_WS];
  __shared__ uint16_t wr[ICPK_BILATERAL_MAX_RANGE];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * BL_TW, y0 = blockIdx.y * BL_TH;
  const int side = 2 * radius + 1, iw = BL_TW + 2 * radius, ih = BL_TH + 2 * radius;
  for (int p = t; p < ih * BL_IW; p += 256) {
    const int r = p / BL_IW, c = p % BL_IW;
    if (c < iw) {
      const int y = y0 - radius + r, x = x0 - radius + c;
      unsigned v = 0u;
      if (y >= 0 && y < rows && x >= 0 && x < cols) v = in[(size_t)y * cols + x];
      tile[r][c] = (uint16_t)v;
    }
  }
  for (int p = t; p < side * side; p += 256) ws[p] = tables[p];
  for (int p = t; p < K; p += 256) wr[p] = tables[side * side + p];
  __syncthreads();
  for (int p = t; p < BL_TW * BL_TH; p += 256) {
    const int r = p / BL_TW, c = p % BL_TW;
    const int y = y0 + r, x = x0 + c;
    if (y < rows && x < cols) {
      const uint16_t* centre = &tile[r + radius][c + radius];  // every tap stays inside the staged ih x iw window
      out[(size_t)y * cols + x] =
          bilateral_pixel(radius, K, ws, wr, [centre](int dy, int dx) { return (int)centre[dy * BL_IW + dx]; });
    }
  }
}

void launch_depth_bilateral(const uint16_t* in, uint16_t* out, int rows, int cols, int radius, int K,
                            const uint16_t* tables, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(depth_bilateral_kernel, dim3((cols + BL_TW - 1) / BL_TW, (rows + BL_TH - 1) / BL_TH), dim3(256), 0,
                     s, in, out, rows, cols, radius, K, tables);
}

}  // namespace icpk
