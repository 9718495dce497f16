// brief_rule.h -- K32: THE BRIEF RULE of include/icpk.h, stated once for the kernels (kernels_brief.hip) and for the
// host-only entry points (icpk_brief.cpp).  Integers only: no libm, no float arithmetic.  The two committed tables are
// brief_table.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "brief_table.h"

namespace icpk {

constexpr int BRIEF_B = 15;        // the reach: a key point is described iff B <= x < cols - B and B <= y < rows - B
constexpr int BRIEF_R2 = 225;      // the moments' disc, x^2 + y^2 <= 225
constexpr int BRIEF_BINS = 32;     // orientation bins of 11.25 degrees
constexpr int BRIEF_TESTS = 256;
constexpr int BRIEF_WORDS = 8;     // bit t is bit t & 31 of word t >> 5
constexpr int BRIEF_BOX = 2;       // S(q): the 5 x 5 box around q
constexpr int BRIEF_OFF = 13;      // |offset coordinate| <= 13: offset + box = the reach
constexpr int BRIEF_GW = 2 * BRIEF_B + 1;    // 31: the grey window around a key point
constexpr int BRIEF_SW = 2 * BRIEF_OFF + 1;  // 27: the box sums an offset can name
constexpr int BRIEF_NONE = 257;    // H2 without a second valid descriptor; more than any distance
static_assert(BRIEF_OFF + BRIEF_BOX == BRIEF_B, "offset + box = the reach");

// K8's grey: cv::cvtColor(CV_BGR2GRAY), 8-bit fixed point (yuv_shift = 14)
__host__ __device__ inline int brief_gray(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }

__host__ __device__ inline int brief_pixel(const uint8_t* img, int cols, int channels, int x, int y) {
  const size_t p = (size_t)y * cols + x;
  return channels == 3 ? brief_gray(img[3 * p], img[3 * p + 1], img[3 * p + 2]) : img[p];
}

// the pixel of key point coordinate f (K8's are whole numbers; any other is rounded to nearest, ties to even, as
// icpk_backproject_keypoints does), or -1 when it is not in [lo, hi) -- NaN and infinities included
__host__ __device__ inline int brief_coord(float f, int lo, int hi) {
  if (!(f > (float)lo - 1.f && f < (float)hi + 1.f)) return -1;
#if defined(__HIP_DEVICE_COMPILE__)
  const int v = __float2int_rn(f);
#else
  const int v = (int)__builtin_rintf(f);
#endif
  return v >= lo && v < hi ? v : -1;
}

// The bin of the direction (m10, m01): the multiple of 11.25 degrees nearest to it.  Bin k is the arc (b_{k-1}, b_k] of
// the boundaries b_j = (j + 1/2) 11.25 degrees taken as the committed integer directions: a direction exactly on b_j is
// in bin j (the lower one; for b_31 that is bin 31).  The direction is turned by quarter turns into x > 0, y >= 0; there
// the bin is the number of boundaries it lies strictly past, by the sign of an int64 cross product.
__host__ __device__ inline int brief_bin(int32_t m10, int32_t m01) {
  if (m10 == 0 && m01 == 0) return 0;
  long long x, y;
  int q;
  if (m10 > 0 && m01 >= 0) q = 0, x = m10, y = m01;
  else if (m10 <= 0 && m01 > 0) q = 1, x = m01, y = -(long long)m10;
  else if (m10 < 0 && m01 <= 0) q = 2, x = -(long long)m10, y = -(long long)m01;
  else q = 3, x = -(long long)m01, y = m10;
  int c = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) c += ((long long)BRIEF_BOUNDARY[j][0] * y - (long long)BRIEF_BOUNDARY[j][1] * x) > 0 ? 1 : 0;
  return (8 * q + c) & 31;
}

// the Hamming distance of two descriptors
__host__ __device__ inline int brief_hamming(const uint32_t* a, const uint32_t* b) {
  int h = 0;
#pragma unroll
  for (int w = 0; w < BRIEF_WORDS; ++w) h += __builtin_popcount(a[w] ^ b[w]);
  return h;
}

// The running best of a brute-force scan in ascending j: (H, j) least lexicographically and H2, the least distance to
// any other descriptor.  merge() folds in the record of a later run of j's.
struct BriefBest {
  int H = BRIEF_NONE, j = -1, H2 = BRIEF_NONE;
  __host__ __device__ void take(int h, int at) {
    if (h < H) H2 = H, H = h, j = at;
    else if (h < H2) H2 = h;
  }
  __host__ __device__ void merge(const BriefBest& o) {
    if (o.j < 0) return;
    if (o.H < H) {
      H2 = H < o.H2 ? H : o.H2;
      H = o.H, j = o.j;
    } else {
      if (o.H < H2) H2 = o.H;
    }
  }
};

// conditions 1 and 2 of THE MATCH RULE
__host__ __device__ inline bool brief_keep(const BriefBest& b, int max_hamming, int ratio_num, int ratio_den) {
  if (b.j < 0 || b.H > max_hamming) return false;
  if (ratio_num > 0 && !((long long)b.H * ratio_den < (long long)b.H2 * ratio_num)) return false;
  return true;
}

}  // namespace icpk
