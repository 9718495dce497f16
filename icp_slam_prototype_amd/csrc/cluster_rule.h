// cluster_rule.h -- K33: the parts of THE CLUSTER RULE (include/icpk.h) that the kernels (kernels_cluster.hip) and the
// host-only icpk_cluster_host (icpk_cluster.cpp) share: the pair distance, the finiteness test, the border point's key
// and the selection predicate.  What a kernel or the host loop concludes from them is its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace icpk {

constexpr unsigned long long CLUSTER_NO_KEY = ~0ull;  // no core neighbour

// nn_device.h's pair_dist, callable from the host as well: float differences, the float64 sum of squares (the products
// are exact, every fma rounds once), narrowed, correctly rounded float sqrt.  Symmetric: the differences only change sign
__host__ __device__ inline float cluster_dist(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = qx - tx;
  const float dy = qy - ty;
  const float dz = qz - tz;
  const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
  const double s = __builtin_fma(ddz, ddz, __builtin_fma(ddy, ddy, ddx * ddx));
  return __builtin_sqrtf((float)s);
}

// (x - x is 0 for a finite x and NaN otherwise: grid_walk.h's finite3)
__host__ __device__ inline bool cluster_finite3(float x, float y, float z) { return ((x - x) + (y - y)) + (z - z) == 0.f; }

__host__ __device__ inline uint32_t cluster_float_bits(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(d);
#else
  return __builtin_bit_cast(uint32_t, d);
#endif
}

// the key a border point minimises over its core neighbours j: (d, j) lexicographically -- distances are non-negative
// floats, so the bit pattern orders like the value
__host__ __device__ inline unsigned long long cluster_key(float d, int j) {
  return ((unsigned long long)cluster_float_bits(d) << 32) | (unsigned)j;
}

// the key of a cluster in the search for the largest: greatest size, ties to the lower label
__host__ __device__ inline unsigned long long cluster_size_key(int size, int label) {
  return ((unsigned long long)(unsigned)size << 32) | (unsigned)~label;
}

// Selection: the point of label `label` in a cluster of `size` members (core and border) is kept
__host__ __device__ inline bool cluster_keeps(int label, int size, int min_size, int max_size, int largest_only, int largest) {
  if (label < 0) return false;
  if (size < min_size || (max_size != 0 && size > max_size)) return false;
  return !largest_only || label == largest;
}

}  // namespace icpk
