// kernels_raycast_color.hip -- K26: the colour gradients of the ray-cast view (include/icpk.h, THE VIEW GRADIENT RULE;
// the rule itself is csrc/raycast_color_rule.h, shared with the host function).
// One thread per view pixel, a 64 x 4 tile per 256-thread workgroup.  The 3 x 3 window of the five planes the rule
// needs (x, y, z, depth, intensity) is read straight from memory: a wave's nine taps of a plane are three runs of 66
// consecutive floats that its own lanes and the rows above and below share through the cache, so an LDS tile would add
// a barrier and 5 x 66 x 6 words of LDS to save loads that already hit.  Integers per pixel, one writer per word; no
// atomic.  It runs once per ray cast.
#include "icpk.h"
#include "icpk_internal.h"
#include "raycast_color_rule.h"

namespace icpk {

static_assert(RAY_COLOR_SUMS == COLOR_SUMS, "the view's ten words are K17's");

constexpr int RC_TW = 64, RC_TH = 4;

__global__ __launch_bounds__(256) void raycast_color_gradients_kernel(const float* __restrict__ maps, int rows, int cols,
                                                                      float radius, int min_neighbors,
                                                                      float* __restrict__ grad,
                                                                      long long* __restrict__ sums, int tiles_x) {
  const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
  const int c = bx * RC_TW + (int)(threadIdx.x % RC_TW), r = by * RC_TH + (int)(threadIdx.x / RC_TW);
  if (r >= rows || c >= cols) return;
  const size_t n = (size_t)rows * cols;
  const RayColorView v{maps, maps + n, maps + 2 * n, maps + 3 * n, maps + 4 * n, maps + 5 * n, maps + 6 * n, maps + 7 * n,
                       rows, cols};
  long long S[RAY_COLOR_SUMS];
  float g[3];
  ray_color_pixel(v, r, c, radius, min_neighbors, S, g);
  const size_t j = (size_t)r * cols + c;
  grad[j] = g[0], grad[n + j] = g[1], grad[2 * n + j] = g[2];
  if (sums) {
#pragma unroll
    for (int k = 0; k < RAY_COLOR_SUMS; ++k) sums[j * RAY_COLOR_SUMS + k] = S[k];
  }
}

void launch_raycast_color_gradients(const float* maps, int rows, int cols, float radius, int min_neighbors, float* grad,
                                    long long* sums, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  const int tiles_x = (cols + RC_TW - 1) / RC_TW, tiles_y = (rows + RC_TH - 1) / RC_TH;
  hipLaunchKernelGGL(raycast_color_gradients_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(256), 0, s, maps, rows,
                     cols, radius, min_neighbors, grad, sums, tiles_x);
}

}  // namespace icpk
