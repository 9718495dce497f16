// kernels_pyramid_color.hip -- K26: one level of the intensity pyramid beside the depth pyramid (include/icpk.h, THE
// INTENSITY PYRAMID RULE; the rule itself is csrc/pyramid_rule.h, shared with the host function).
// One 256-thread workgroup = a 32 x 8 tile of level l + 1 over the 64 x 16 block of level l under it.  It stages the
// 65 x 17 windows of the depth and of the intensity of level l (the block plus the row above and the column to the
// left; out-of-image positions as depth 0, which the rule skips as it skips a hole), then one thread computes and
// stores one output pixel.  One level per launch: the launch runs once per frame, a level is a sixteenth of a
// millisecond of work, and a second stage would keep a float window of level l + 1 in LDS for 64 of 256 threads.
// Every LDS word is written once, before the barrier its readers wait at; no atomic.
#include "icpk.h"
#include "icpk_internal.h"
#include "pyramid_rule.h"

namespace icpk {

constexpr int PC_TW = 32, PC_TH = 8;                      // the tile of level l + 1
constexpr int PC_WW = 2 * PC_TW + 1, PC_WH = 2 * PC_TH + 1;  // 65 x 17: the window of level l
constexpr int PC_WP = PC_WW + 1;                          // row pitch

__global__ __launch_bounds__(256) void intensity_pyramid_kernel(const uint16_t* __restrict__ depth,
                                                                const float* __restrict__ inten, int rows, int cols,
                                                                float* __restrict__ out, int K, int tiles_x) {
  __shared__ uint16_t wd[PC_WH][PC_WP];
  __shared__ float wi[PC_WH][PC_WP];
  const int t = threadIdx.x;
  const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
  const int rows1 = pyramid_half(rows), cols1 = pyramid_half(cols);
  const int c1 = bx * PC_TW, r1 = by * PC_TH;   // this workgroup's first pixel of level l + 1
  const int x0 = 2 * c1 - 1, y0 = 2 * r1 - 1;  // the window of level l starts here
  for (int p = t; p < PC_WH * PC_WP; p += 256) {
    const int r = p / PC_WP, c = p % PC_WP;
    if (c < PC_WW) {
      const int y = y0 + r, x = x0 + c;
      unsigned d = 0u;
      float v = 0.f;
      if (y >= 0 && y < rows && x >= 0 && x < cols) {
        d = depth[(size_t)y * cols + x];
        v = inten[(size_t)y * cols + x];
      }
      wd[r][c] = (uint16_t)d;
      wi[r][c] = v;
    }
  }
  __syncthreads();
  // tile position (tr, tc) is pixel (r1 + tr, c1 + tc) of level l + 1, centred on window position (2 tr + 1, 2 tc + 1):
  // its taps read rows 2 tr .. 2 tr + 2 <= 16 and columns 2 tc .. 2 tc + 2 <= 64
  const int tr = t / PC_TW, tc = t % PC_TW;
  const int r = r1 + tr, c = c1 + tc;
  if (r >= rows1 || c >= cols1) return;
  const uint16_t* dcen = &wd[2 * tr + 1][2 * tc + 1];
  const float* icen = &wi[2 * tr + 1][2 * tc + 1];
  out[(size_t)r * cols1 + c] = pyramid_intensity_pixel(
      K, [dcen](int dy, int dx) { return (int)dcen[dy * PC_WP + dx]; }, [icen](int dy, int dx) { return icen[dy * PC_WP + dx]; });
}

void launch_intensity_pyramid(const uint16_t* depth, const float* inten, int rows, int cols, float* out, int K,
                              hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  const int rows1 = pyramid_half(rows), cols1 = pyramid_half(cols);
  const int tiles_x = (cols1 + PC_TW - 1) / PC_TW, tiles_y = (rows1 + PC_TH - 1) / PC_TH;
  hipLaunchKernelGGL(intensity_pyramid_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(256), 0, s, depth, inten,
                     rows, cols, out, K, tiles_x);
}

}  // namespace icpk
