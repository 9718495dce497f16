// kernels_sdf_track.hip -- K29: depth frames tracked directly against the TSDF (include/icpk.h, THE SDF TRACKING RULE).
//
// One iteration is two launches.  sdf_reduce_kernel walks the pixels of a pyramid level in the canonical geometry
// (red_blocks(npix) workgroups of RED_THREADS, thread g takes pixels g, g + 256 B, ...): each pixel is back-projected,
// moved by the state's pose and looked up in the volume where it lands (sdf_track_rule.h) -- eight distances and eight
// weights of one cell, no view, no pair, no search; an accepted pixel adds K5's 28 terms with n = grad D / |grad D| and
// r = D to the lane's double accumulators, which end in block_partials.  The step is K25's proj_step_kernel, unchanged,
// on a state block of this family's own.  No atomic, and no word travels between workgroups of one launch.  Once the
// state says done the launch returns at once.
//
// The gathers: neighbouring pixels land in neighbouring cells, so a wave's sixteen loads touch a few rows of the planes.
// The two corners of an x-pair are adjacent, but `at` is any voxel, so a pair is 4-byte aligned only (2-byte for the
// weights): they are loaded as singles, in plain C++.
#include "icpk.h"
#include "icpk_internal.h"
#include "pair_reduce.h"
#include "sdf_track_rule.h"

namespace icpk {

namespace {

__device__ __forceinline__ ProjPose sdf_pose(const ProjState* __restrict__ st) {
  ProjPose E;
#pragma unroll
  for (int k = 0; k < 9; ++k) E.R[k] = st->R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) E.t[k] = st->t[k];
  return E;
}

}  // namespace

// WITH_NORMAL: rule 7 is on (four more depth loads per surviving pixel); the default path is compiled without it.
template <bool WITH_NORMAL>
__global__ __launch_bounds__(RED_THREADS) void sdf_reduce_kernel(const SdfArgs a) {
  if (a.st->done) return;  // (uniform)
  const int npix = a.rows * a.cols;
  const int P = (int)gridDim.x * RED_THREADS;
  int i = (int)blockIdx.x * RED_THREADS + (int)threadIdx.x;
  // a lane's first depth is asked for before the pose is read: two cold round trips side by side
  uint16_t d_next = i < npix ? a.depth[i] : (uint16_t)0;
  const ProjLevel lv{a.depth, a.rows, a.cols, a.fx, a.cx};
  const ProjPose E = sdf_pose(a.st);
  const SdfGate g{a.trunc, a.max_abs_tsdf, a.min_normal_cos};
  double v[NP2L];
#pragma unroll
  for (int s = 0; s < NP2L; ++s) v[s] = 0.0;
  int cnt = 0;
  for (; i < npix; i += P) {
    const uint16_t d = d_next;
    if (i + P < npix) d_next = a.depth[i + P];  // the NEXT pixel is on its way while this one is consumed
    const int r = i / a.cols, c = i - r * a.cols;
    SdfHit h;
    if (sdf_pixel<WITH_NORMAL>(lv, a.vol, E, g, r, c, d, &h) >= 0) {
      sdf_add_terms(h, v);
      ++cnt;
    }
  }
  block_partials<NP2L>(v, cnt, a.partial + blockIdx.x, RED_MAX_BLOCKS, a.pcount + blockIdx.x);
}

void launch_sdf_reduce(const SdfArgs& a, hipStream_t s) {
  const int B = red_blocks(a.rows * a.cols);
  if (a.min_normal_cos > -1.f)
    hipLaunchKernelGGL(sdf_reduce_kernel<true>, dim3(B), dim3(RED_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(sdf_reduce_kernel<false>, dim3(B), dim3(RED_THREADS), 0, s, a);
}

// rules 1 - 7 per pixel, one thread each: icpk_sdf_associate
template <bool WITH_NORMAL>
__global__ __launch_bounds__(RED_THREADS) void sdf_associate_kernel(const SdfArgs a, int32_t* __restrict__ cell,
                                                                    float* __restrict__ value) {
  const int npix = a.rows * a.cols;
  const int i = (int)blockIdx.x * RED_THREADS + (int)threadIdx.x;
  if (i >= npix) return;
  const ProjLevel lv{a.depth, a.rows, a.cols, a.fx, a.cx};
  const ProjPose E = sdf_pose(a.st);
  const SdfGate g{a.trunc, a.max_abs_tsdf, a.min_normal_cos};
  const int r = i / a.cols, c = i - r * a.cols;
  SdfHit h;
  const int at = sdf_pixel<WITH_NORMAL>(lv, a.vol, E, g, r, c, a.depth[i], &h);
  cell[i] = at;
  value[i] = at >= 0 ? h.D : 0.f;
}

void launch_sdf_associate(const SdfArgs& a, int32_t* cell, float* value, hipStream_t s) {
  const int B = (a.rows * a.cols + RED_THREADS - 1) / RED_THREADS;
  if (a.min_normal_cos > -1.f)
    hipLaunchKernelGGL(sdf_associate_kernel<true>, dim3(B), dim3(RED_THREADS), 0, s, a, cell, value);
  else
    hipLaunchKernelGGL(sdf_associate_kernel<false>, dim3(B), dim3(RED_THREADS), 0, s, a, cell, value);
}

}  // namespace icpk
