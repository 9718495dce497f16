// kernels_frame_view.hip -- K28: the frame view (include/icpk.h, THE FRAME VIEW RULE; frame_view_rule.h).
//
// ONE launch covers every level of the resident pyramid: the levels' pixels are cut into workgroups of
// FRAME_VIEW_THREADS, level l owns the workgroups block0[l] .. block0[l + 1) of the grid, and a workgroup finds its
// level by walking that table (at most FRAME_VIEW_MAX_LEVELS uniform comparisons).  One thread owns one pixel: it
// reads the pixel's depth and, for an interior pixel, its four neighbours (2 bytes each, neighbouring lanes share
// them through the cache), the intensity where the pyramid carries one, and writes the pixel's eight floats -- a wave
// writes 256 contiguous bytes of each plane.  No atomic and no word between workgroups.  The two counts of a
// workgroup go through a workgroup sum into its own two slots; frame_view_sum_kernel, one workgroup per level, adds
// a level's slots into that level's two totals, as tsdf_integrate_kernel's n_updated is counted.
#include "frame_view_rule.h"
#include "icpk_internal.h"

namespace icpk {

namespace {

// the sum of v over the workgroup's four waves, in every thread; one barrier on the caller's own four words
__device__ __forceinline__ int frame_view_block_sum(int v, int* lds4) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

}  // namespace

static_assert(FRAME_VIEW_THREADS == 256, "frame_view_block_sum adds four waves");

__global__ __launch_bounds__(FRAME_VIEW_THREADS) void frame_view_kernel(const FrameViewArgs a) {
  int l = 0;
  while (l + 1 < a.levels && (int)blockIdx.x >= a.block0[l + 1]) ++l;  // (uniform)
  const FrameViewLevel& L = a.level[l];
  const int npix = L.rows * L.cols;
  const int i = ((int)blockIdx.x - a.block0[l]) * FRAME_VIEW_THREADS + (int)threadIdx.x;
  int listed = 0, no_normal = 0;
  if (i < npix) {
    const ProjLevel lv{L.depth, L.rows, L.cols, L.fx, L.cx};
    ProjPose P;
#pragma unroll
    for (int k = 0; k < 9; ++k) P.R[k] = a.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) P.t[k] = a.t[k];
    const int r = i / L.cols, c = i - r * L.cols;
    float out[8];
    const int what = frame_view_pixel(lv, P, r, c, L.inten ? L.inten[i] : 0.f, out);
    listed = what == FRAME_VIEW_LISTED, no_normal = what == FRAME_VIEW_NO_NORMAL;
#pragma unroll
    for (int k = 0; k < 8; ++k) L.planes[(size_t)k * npix + i] = out[k];
  }
  __shared__ int lds4[2][4];
  const int nl = frame_view_block_sum(listed, lds4[0]);
  const int nn = frame_view_block_sum(no_normal, lds4[1]);
  if (threadIdx.x == 0) a.slots[2 * blockIdx.x] = nl, a.slots[2 * blockIdx.x + 1] = nn;
}

// one workgroup per level: totals[2 l] = the listed pixels of level l, totals[2 l + 1] = those without a normal
__global__ __launch_bounds__(FRAME_VIEW_THREADS) void frame_view_sum_kernel(const FrameViewArgs a, int* __restrict__ totals) {
  const int l = blockIdx.x;
  int nl = 0, nn = 0;
  for (int b = a.block0[l] + (int)threadIdx.x; b < a.block0[l + 1]; b += FRAME_VIEW_THREADS)
    nl += a.slots[2 * b], nn += a.slots[2 * b + 1];
  __shared__ int lds4[2][4];
  nl = frame_view_block_sum(nl, lds4[0]);
  nn = frame_view_block_sum(nn, lds4[1]);
  if (threadIdx.x == 0) totals[2 * l] = nl, totals[2 * l + 1] = nn;
}

void launch_frame_view(const FrameViewArgs& a, int* totals, hipStream_t s) {
  hipLaunchKernelGGL(frame_view_kernel, dim3(a.block0[a.levels]), dim3(FRAME_VIEW_THREADS), 0, s, a);
  hipLaunchKernelGGL(frame_view_sum_kernel, dim3(a.levels), dim3(FRAME_VIEW_THREADS), 0, s, a, totals);
}

}  // namespace icpk
