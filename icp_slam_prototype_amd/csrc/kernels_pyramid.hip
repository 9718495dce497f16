// kernels_pyramid.hip -- K24: two levels of the depth pyramid from one read of the level below (include/icpk.h, THE
// PYRAMID RULE; the rule itself is csrc/pyramid_rule.h, shared with the host function).
// One 256-thread workgroup = a 16 x 4 tile of level l + 2, which is the 32 x 8 tile of level l + 1 and the 64 x 16
// block of level l under it.  It stages the 67 x 19 window of level l (the block plus a halo of 3; out-of-image
// positions as 0, which the rule skips as it skips a hole), computes the 33 x 9 window of level l + 1 (its tile plus
// the row above and the column to the left, 0 outside the level) into LDS and stores the 32 x 8 pixels it owns; after
// the second barrier 64 of its threads compute and store the 16 x 4 pixels of level l + 2.  out2 == nullptr: the
// second stage is off and the grid covers level l + 1 by its 32 x 8 tiles.  One thread writes an output pixel, and
// every LDS word is written once, before the barrier its readers wait at; no atomic.
#include "icpk.h"
#include "icpk_internal.h"
#include "pyramid_rule.h"

namespace icpk {

constexpr int PY_T2W = 16, PY_T2H = 4;                          // the tile of level l + 2
constexpr int PY_W1W = 2 * PY_T2W + 1, PY_W1H = 2 * PY_T2H + 1;  // 33 x 9: the window of level l + 1
constexpr int PY_W0W = 2 * PY_W1W + 1, PY_W0H = 2 * PY_W1H + 1;  // 67 x 19: the window of level l
constexpr int PY_W0P = PY_W0W + 1, PY_W1P = PY_W1W + 1;          // row pitches (even: rows stay word aligned)

__global__ __launch_bounds__(256) void depth_pyramid_kernel(const uint16_t* __restrict__ in, int rows, int cols,
                                                            uint16_t* __restrict__ out1, uint16_t* __restrict__ out2,
                                                            int K, int tiles_x) {
  __shared__ uint16_t w0[PY_W0H][PY_W0P];
  __shared__ uint16_t w1[PY_W1H][PY_W1P];
  const int t = threadIdx.x;
  const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x;
  const int rows1 = pyramid_half(rows), cols1 = pyramid_half(cols);
  const int c1 = bx * (2 * PY_T2W), r1 = by * (2 * PY_T2H);  // this workgroup's first pixel of level l + 1
  const int x0 = 2 * c1 - 3, y0 = 2 * r1 - 3;                // the window of level l starts here
  for (int p = t; p < PY_W0H * PY_W0P; p += 256) {
    const int r = p / PY_W0P, c = p % PY_W0P;
    if (c < PY_W0W) {
      const int y = y0 + r, x = x0 + c;
      unsigned v = 0u;
      if (y >= 0 && y < rows && x >= 0 && x < cols) v = in[(size_t)y * cols + x];
      w0[r][c] = (uint16_t)v;
    }
  }
  __syncthreads();
  // window position (wr, wc) is pixel (r1 - 1 + wr, c1 - 1 + wc) of level l + 1, centred on window position
  // (2 wr + 1, 2 wc + 1) of level l: its taps read rows 2 wr .. 2 wr + 2 <= 18 and columns 2 wc .. 2 wc + 2 <= 66
  for (int p = t; p < PY_W1H * PY_W1W; p += 256) {
    const int wr = p / PY_W1W, wc = p % PY_W1W;
    const int r = r1 - 1 + wr, c = c1 - 1 + wc;
    const bool inside = r >= 0 && r < rows1 && c >= 0 && c < cols1;
    uint16_t v = 0;
    if (inside) {
      const uint16_t* centre = &w0[2 * wr + 1][2 * wc + 1];
      v = pyramid_pixel(K, [centre](int dy, int dx) { return (int)centre[dy * PY_W0P + dx]; });
      if (wr >= 1 && wc >= 1) out1[(size_t)r * cols1 + c] = v;  // (row 0 and column 0 belong to the neighbours)
    }
    w1[wr][wc] = v;
  }
  if (!out2) return;  // (the whole workgroup: out2 is a launch argument)
  __syncthreads();
  if (t < PY_T2W * PY_T2H) {
    const int r = t / PY_T2W, c = t % PY_T2W;
    const int R = by * PY_T2H + r, C = bx * PY_T2W + c;
    const int rows2 = pyramid_half(rows1), cols2 = pyramid_half(cols1);
    if (R < rows2 && C < cols2) {
      // pixel (2 R, 2 C) of level l + 1 is window position (2 r + 1, 2 c + 1): taps stay inside 9 x 33
      const uint16_t* centre = &w1[2 * r + 1][2 * c + 1];
      out2[(size_t)R * cols2 + C] = pyramid_pixel(K, [centre](int dy, int dx) { return (int)centre[dy * PY_W1P + dx]; });
    }
  }
}

void launch_depth_pyramid(const uint16_t* in, int rows, int cols, uint16_t* out1, uint16_t* out2, int K, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  const int rows1 = pyramid_half(rows), cols1 = pyramid_half(cols);
  // the grid covers the deepest level written: every pixel of level l + 1 lies under one of its tiles
  const int tw = out2 ? PY_T2W : 2 * PY_T2W, th = out2 ? PY_T2H : 2 * PY_T2H;
  const int ow = out2 ? pyramid_half(cols1) : cols1, oh = out2 ? pyramid_half(rows1) : rows1;
  const int tiles_x = (ow + tw - 1) / tw, tiles_y = (oh + th - 1) / th;
  hipLaunchKernelGGL(depth_pyramid_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(256), 0, s, in, rows, cols,
                     out1, out2, K, tiles_x);
}

}  // namespace icpk
