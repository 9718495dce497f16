// map_device.h -- the voxel rule of the certainty map (map.cpp:55-85), shared by kernels_map.hip (K7) and
// kernels_map_nn.hip (K9).
#pragma once
#include "icpk_internal.h"

namespace icpk {

constexpr float MAP_C = 10.0f / (float)MAP_DIM;  // map.hpp:17 CELL_PHYSICAL_HEIGHT as float(...) (map.cpp:58)

// map.cpp:60-82 for one axis: int(p / c) with the x86 conversion (cvttss2si: NaN, +-inf and |q| >= 2^31 give INT_MIN,
// which the clamp sends to 0 -- v_cvt_i32_f32 would saturate +1e10 to INT_MAX and land in voxel 299), clamped to
// [0, 299].  The division is correctly rounded (v_div_scale / v_div_fmas / v_div_fixup, no bare v_rcp_f32).
__device__ __forceinline__ int map_axis(float p) {
  const float q = __fdiv_rn(p, MAP_C);
  return (q >= 0.f && q < 2147483648.f) ? min((int)q, MAP_DIM - 1) : 0;
}

__device__ __forceinline__ int map_key_of(float x, float y, float z) {
  return (map_axis(x) * MAP_DIM + map_axis(y)) * MAP_DIM + map_axis(z);  // world[x][y][z]
}

}  // namespace icpk
