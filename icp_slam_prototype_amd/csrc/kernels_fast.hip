// kernels_fast.hip -- K8: FAST key points of a colour frame (SLAM.cpp:255-256: cv::cvtColor BGR -> GRAY, then
// cv::FAST(grayscale, keypoints, 60, true, TYPE_7_12)) and their back-projection (pointcloud.cpp:60-98) on the device.
//
// The contract is OpenCV 3.2's scalar FAST_t<patternSize> (features2d/src/fast.cpp) as include/icpk.h restates it:
// grey conversion, quick test on the wrapped circle table, arc test, cornerScore, 3 x 3 strict non-maximum suppression,
// row-major order.  Everything is integer work.
//   fast_tile     one 64 x 16 output tile per workgroup: the tile and a 4-pixel halo into LDS (BGR -> grey on the
//                 way), corner flag and score for the tile and a 1-pixel ring, suppression, and per (row, tile column)
//                 the ballot of kept pixels and its popcount                                          1 launch
//   fast_scan     exclusive scan of the counts in row-major (y, tile column) order, one workgroup     1 launch
//   fast_scatter  (x, y, response) of every kept pixel at its rank: row-major order                   1 launch
//   fast_cloud    the detected list back-projected from a depth image, posed, compacted in list order
//                 into the context's source / target planes, padded; the count to a mapped word       1 launch
#include "block_scan.h"
#include "icpk.h"
#include "icpk_internal.h"

namespace icpk {

constexpr int FT_W = 64, FT_H = 16;                                 // output tile
constexpr int FT_HALO = 4;                                          // circle radius 3 + the suppression ring
constexpr int FT_LW = FT_W + 2 * FT_HALO, FT_LH = FT_H + 2 * FT_HALO;  // grey tile in LDS
constexpr int FT_SW = FT_W + 2, FT_SH = FT_H + 2;                   // scores: tile + 1-pixel ring
constexpr int FT_THREADS = 256;                                     // 4 wave64; wave w owns output rows w, w + 4, ...
constexpr int FT_SCAN_THREADS = 1024;
constexpr int FT_CLOUD_THREADS = 1024;

// OpenCV's makeOffsets order, (dx, dy)
__constant__ signed char FAST_DX16[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__constant__ signed char FAST_DY16[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
__constant__ signed char FAST_DX12[12] = {0, 1, 2, 2, 2, 1, 0, -1, -2, -2, -2, -1};
__constant__ signed char FAST_DY12[12] = {2, 2, 1, 0, -1, -2, -2, -2, -1, 0, 1, 2};

// cv::cvtColor(CV_BGR2GRAY), 8-bit fixed point (yuv_shift = 14)
__device__ __forceinline__ int bgr_gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

__device__ __forceinline__ int fast_class(int x, int v, int t) { return x < v - t ? 1 : (x > v + t ? 2 : 0); }

// P consecutive circle positions (circularly) form a run of K + 1 set bits in m?  (FAST_t's scan of k = 0 .. P + K
// over the wrapped table finds exactly the circular runs of more than K)
template <int P>
__device__ __forceinline__ bool has_arc(unsigned m) {
  constexpr int K = P / 2;
  const unsigned e = m | (m << P);
  unsigned r = e;
#pragma unroll
  for (int i = 1; i <= K; ++i) r &= e >> i;
  return (r & ((1u << P) - 1u)) != 0u;
}

// FAST_t + cornerScore at grey position (ly, lx) of the LDS tile: -1 = no corner, else the score (0 .. 254)
template <int P>
__device__ int fast_score(const uint8_t (*g)[FT_LW], int ly, int lx, int t) {
  constexpr int K = P / 2;
  const int v = g[ly][lx];
  int c[P];
#pragma unroll
  for (int k = 0; k < P; ++k)
    c[k] = P == 16 ? g[ly + FAST_DY16[k]][lx + FAST_DX16[k]] : g[ly + FAST_DY12[k]][lx + FAST_DX12[k]];
  // the quick test, same index pairs of the wrapped table for every pattern size (pixel[k] = pixel[k - P])
  int d = fast_class(c[0], v, t) | fast_class(c[8 % P], v, t);
  if (d == 0) return -1;
  d &= fast_class(c[2], v, t) | fast_class(c[10 % P], v, t);
  d &= fast_class(c[4], v, t) | fast_class(c[12 % P], v, t);
  d &= fast_class(c[6], v, t) | fast_class(c[14 % P], v, t);
  if (d == 0) return -1;
  d &= fast_class(c[1], v, t) | fast_class(c[9 % P], v, t);
  d &= fast_class(c[3], v, t) | fast_class(c[11 % P], v, t);
  d &= fast_class(c[5], v, t) | fast_class(c[13 % P], v, t);
  d &= fast_class(c[7], v, t) | fast_class(c[15 % P], v, t);
  unsigned dark = 0u, bright = 0u;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    dark |= (unsigned)(c[k] < v - t) << k;
    bright |= (unsigned)(c[k] > v + t) << k;
  }
  const bool corner = ((d & 1) && has_arc<P>(dark)) || ((d & 2) && has_arc<P>(bright));
  if (!corner) return -1;
  // cornerScore<P>: M - 1, M = max over the P arcs of K + 1 pixels of max(min(v - x), min(x - v))
  int M = 0;
#pragma unroll
  for (int s = 0; s < P; ++s) {
    int mn = 255, mx = -255;
#pragma unroll
    for (int j = 0; j <= K; ++j) {
      const int dd = v - c[(s + j) % P];
      mn = min(mn, dd);
      mx = max(mx, dd);
    }
    M = max(M, max(mn, -mx));
  }
  return M - 1;
}

template <int P>
__global__ __launch_bounds__(FT_THREADS) void fast_tile_kernel(const uint8_t* __restrict__ img, int rows, int cols,
                                                               int channels, int t, int nonmax, int ntx,
                                                               unsigned long long* __restrict__ masks,
                                                               int* __restrict__ counts, uint8_t* __restrict__ score) {
  __shared__ uint8_t g[FT_LH][FT_LW];
  __shared__ int sc[FT_SH][FT_SW];  // corner ? 0x100 | score : 0
  const int x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H;
  for (int i = threadIdx.x; i < FT_LH * FT_LW; i += FT_THREADS) {
    const int ly = i / FT_LW, lx = i - ly * FT_LW;
    const int gy = y0 - FT_HALO + ly, gx = x0 - FT_HALO + lx;
    int v = 0;  // (outside the image: never read by a candidate, whose circle lies inside)
    if (gy >= 0 && gy < rows && gx >= 0 && gx < cols) {
      const size_t p = (size_t)gy * cols + gx;
      v = channels == 3 ? bgr_gray(img[3 * p], img[3 * p + 1], img[3 * p + 2]) : img[p];
    }
    g[ly][lx] = (uint8_t)v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < FT_SH * FT_SW; i += FT_THREADS) {
    const int sy = i / FT_SW, sx = i - sy * FT_SW;
    const int gy = y0 - 1 + sy, gx = x0 - 1 + sx;
    int s = 0;
    if (gy >= 3 && gy <= rows - 4 && gx >= 3 && gx <= cols - 4) {
      const int r = fast_score<P>(g, sy + FT_HALO - 1, sx + FT_HALO - 1, t);
      s = r < 0 ? 0 : (0x100 | r);
    }
    sc[sy][sx] = s;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < FT_H / (FT_THREADS / 64); ++k) {
    const int ty = wave + k * (FT_THREADS / 64);
    const int gy = y0 + ty, gx = x0 + lane;
    const int s = sc[ty + 1][lane + 1];
    bool kept = s != 0;
    if (kept && nonmax) {
      const int v = s & 0xff;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
          if (dy != 1 || dx != 1) kept = kept && v > (sc[ty + dy][lane + dx] & 0xff);
    }
    const unsigned long long m = __ballot(kept);
    if (gy < rows) {
      if (kept) score[(size_t)gy * cols + gx] = (uint8_t)(s & 0xff);
      if (lane == 0) {
        masks[(size_t)gy * ntx + blockIdx.x] = m;
        counts[(size_t)gy * ntx + blockIdx.x] = __popcll(m);
      }
    }
  }
}

// exclusive scan in place of m ints by one workgroup, one contiguous run per lane; *total = the sum
__global__ __launch_bounds__(FT_SCAN_THREADS) void fast_scan_kernel(int* __restrict__ a, int m, int* __restrict__ total) {
  const int sum = scan_runs<FT_SCAN_THREADS>(a, m);
  if (threadIdx.x == 0) *total = sum;
}

// one wave per (row, tile column): the kept pixels of its mask at offset + rank among them
__global__ __launch_bounds__(FT_THREADS) void fast_scatter_kernel(const unsigned long long* __restrict__ masks,
                                                                  const int* __restrict__ offs, int m, int ntx, int cols,
                                                                  const uint8_t* __restrict__ score, int nonmax,
                                                                  float* __restrict__ kp, float* __restrict__ resp) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * (FT_THREADS / 64) + (threadIdx.x >> 6);
  if (e >= m) return;
  const unsigned long long mask = masks[e];
  if (!((mask >> lane) & 1ull)) return;
  const int y = e / ntx, x = (e - y * ntx) * FT_W + lane;
  const int r = offs[e] + __popcll(mask & ((1ull << lane) - 1ull));
  kp[2 * r] = (float)x;
  kp[2 * r + 1] = (float)y;
  resp[r] = nonmax ? (float)score[(size_t)y * cols + x] : 0.f;  // (OpenCV scores only under suppression)
}

__global__ __launch_bounds__(256) void bgr_gray_kernel(const uint8_t* __restrict__ bgr, int n, uint8_t* __restrict__ out) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = (uint8_t)bgr_gray(bgr[3 * (size_t)i], bgr[3 * (size_t)i + 1], bgr[3 * (size_t)i + 2]);
}

// icpk_backproject_keypoints (pointcloud.cpp:60-98) on the detected list, then p <- fl32(fl32(R p) + t) with K3's
// arithmetic, compacted in list order by ONE workgroup (a frame has a few thousand key points): x / y / z and the
// working copy x2 / y2 / z2 (or null), padded with `pad` up to the next multiple of NN_TILE.  The count goes to *n_dev
// and, after every store, to the mapped word *n_host (or null).  map (or null, K32): per key point its rank in the cloud,
// -1 where it was dropped.
__global__ __launch_bounds__(FT_CLOUD_THREADS) void fast_cloud_kernel(
    const float* __restrict__ kp, int n, const uint16_t* __restrict__ depth, int rows, int cols, float fx, float cx,
    const Rt rt, float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, float* __restrict__ x2,
    float* __restrict__ y2, float* __restrict__ z2, float pad, int* __restrict__ n_dev, int* __restrict__ n_host,
    int* __restrict__ map) {
  __shared__ int wcnt[FT_CLOUD_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int off = 0;
  for (int base = 0; base < n; base += FT_CLOUD_THREADS) {
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    if (i < n) {
      const float fxp = kp[2 * i], fyp = kp[2 * i + 1];
      if (fxp > -1.f && fxp < (float)cols + 1.f && fyp > -1.f && fyp < (float)rows + 1.f) {
        const int xi = __float2int_rn(fxp), yi = __float2int_rn(fyp);  // cvRound: to nearest, ties to even
        if (xi >= 0 && xi < cols && yi >= 0 && yi < rows) {
          const uint16_t d = depth[(size_t)yi * cols + xi];
          if (d != 0) {  // pointcloud.cpp:67-70
            const float pz = __fdiv_rn((float)d, 5000.0f);                                // :86
            const float px = __fdiv_rn(__fmul_rn(__fsub_rn((float)xi, cx), pz), fx);    // :87
            const float py = __fdiv_rn(__fmul_rn(__fsub_rn((float)yi, cx), pz), fx);    // :88 (CX, FX)
            const double dx = px, dy = py, dz = pz;
            vx = __fadd_rn((float)__builtin_fma((double)rt.R[2], dz, __builtin_fma((double)rt.R[1], dy, (double)rt.R[0] * dx)), rt.t[0]);
            vy = __fadd_rn((float)__builtin_fma((double)rt.R[5], dz, __builtin_fma((double)rt.R[4], dy, (double)rt.R[3] * dx)), rt.t[1]);
            vz = __fadd_rn((float)__builtin_fma((double)rt.R[8], dz, __builtin_fma((double)rt.R[7], dy, (double)rt.R[6] * dx)), rt.t[2]);
            keep = true;
          }
        }
      }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FT_CLOUD_THREADS / 64; ++w) {
      before += w < wave ? wcnt[w] : 0;
      total += wcnt[w];
    }
    if (keep) {
      const int r = off + before + __popcll(mask & ((1ull << lane) - 1ull));
      x[r] = vx;
      y[r] = vy;
      z[r] = vz;
      if (x2) {
        x2[r] = vx;
        y2[r] = vy;
        z2[r] = vz;
      }
      if (map) map[i] = r;
    } else if (map && i < n) {
      map[i] = -1;
    }
    off += total;
    __syncthreads();  // (wcnt is rewritten by the next chunk)
  }
  const int padded = ((off < 1 ? 1 : off) + NN_TILE - 1) / NN_TILE * NN_TILE;
  for (int i = off + (int)threadIdx.x; i < padded; i += FT_CLOUD_THREADS) {
    x[i] = y[i] = z[i] = pad;
    if (x2) x2[i] = y2[i] = z2[i] = pad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *n_dev = off;
    if (n_host) {
      __threadfence_system();
      __hip_atomic_store(n_host, off, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

int fast_tiles_x(int cols) { return (cols + FT_W - 1) / FT_W; }

void launch_fast_detect(const uint8_t* img, int rows, int cols, int channels, int threshold, int nonmax, int pattern,
                        unsigned long long* masks, int* counts, uint8_t* score, int* total, float* kp, float* resp,
                        hipStream_t s) {
  const int ntx = fast_tiles_x(cols), nty = (rows + FT_H - 1) / FT_H;
  const int m = rows * ntx;
  if (pattern == 16)
    hipLaunchKernelGGL(fast_tile_kernel<16>, dim3(ntx, nty), dim3(FT_THREADS), 0, s, img, rows, cols, channels, threshold,
                       nonmax, ntx, masks, counts, score);
  else
    hipLaunchKernelGGL(fast_tile_kernel<12>, dim3(ntx, nty), dim3(FT_THREADS), 0, s, img, rows, cols, channels, threshold,
                       nonmax, ntx, masks, counts, score);
  hipLaunchKernelGGL(fast_scan_kernel, dim3(1), dim3(FT_SCAN_THREADS), 0, s, counts, m, total);
  hipLaunchKernelGGL(fast_scatter_kernel, dim3((m + FT_THREADS / 64 - 1) / (FT_THREADS / 64)), dim3(FT_THREADS), 0, s, masks,
                     counts, m, ntx, cols, score, nonmax, kp, resp);
}

void launch_bgr_to_gray(const uint8_t* bgr, int n, uint8_t* out, hipStream_t s) {
  if (n <= 0) return;
  int blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(bgr_gray_kernel, dim3(blocks), dim3(256), 0, s, bgr, n, out);
}

void launch_fast_cloud(const float* kp, int n, const uint16_t* depth, int rows, int cols, float fx, float cx, const Rt& rt,
                       float* x, float* y, float* z, float* x2, float* y2, float* z2, float pad, int* n_dev, int* n_host,
                       int* map, hipStream_t s) {
  hipLaunchKernelGGL(fast_cloud_kernel, dim3(1), dim3(FT_CLOUD_THREADS), 0, s, kp, n, depth, rows, cols, fx, cx, rt, x, y, z,
                     x2, y2, z2, pad, n_dev, n_host, map);
}

}  // namespace icpk
