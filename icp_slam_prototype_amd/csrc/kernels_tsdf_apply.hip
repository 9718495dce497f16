// kernels_tsdf_apply.hip -- K30: several signed frame updates in one pass over the TSDF volume.  K19's geometry (the
// volume as a line of voxels, x fastest, cut into chunks of a multiple of TSDF_THREADS, a wave on 64 consecutive
// voxels) and K19's ownership: a voxel belongs to one thread, which takes the ops in the order listed with the voxel's
// tsdf, weight and intensity in registers.  Each plane is read at most once per voxel -- at the first op that produces
// a sample there -- and written at most once, and only where some op wrote: apart from the frames, the volume crosses
// memory once per call, not once per op.  The op table lies in the kernel-argument segment and is indexed by the loop
// counter, which is uniform.  No atomic of any kind: the per-op counts go from a ballot into the wave's own LDS word
// for the op, the four waves' words into the workgroup's slot, and a second kernel sums the slots.
#include "block_scan.h"
#include "icpk_internal.h"
#include "tsdf_rule.h"

namespace icpk {

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_apply_kernel(const TsdfApplyArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const unsigned dx = (unsigned)a.fr.dims[0], dxy = dx * (unsigned)a.fr.dims[1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ int counts[TSDF_THREADS / 64][TSDF_MAX_OPS];  // [wave][op]: written by that wave's lane 0 alone
  if (lane < TSDF_MAX_OPS) counts[wave][lane] = 0;
  __syncthreads();
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    const bool valid = at < end;  // (no early exit: the ballots below are the whole wave's)
    int c[3] = {0, 0, 0};
    if (valid) {  // (at < n <= 2^30: 32-bit divisions)
      const unsigned k = (unsigned)at / dxy, rem = (unsigned)at - k * dxy, j = rem / dx;
      c[0] = (int)(rem - j * dx), c[1] = (int)j, c[2] = (int)k;
    }
    float tv = 0.f, ci = 0.f;
    int w = 0;
    bool loaded = false, dirty = false;
    for (int op = 0; op < a.n_ops; ++op) {  // (uniform: the table is read by scalar loads)
      bool wrote = false;
      if (valid) {
        TsdfFrame fr = a.fr;
#pragma unroll
        for (int q = 0; q < 9; ++q) fr.R[q] = a.ops[op].R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) fr.t[q] = a.ops[op].t[q];
        const long long image = (long long)a.ops[op].frame * a.npix;  // (frame < n_frames: inside the stack)
        float f;
        int pix;
        if (tsdf_sample(fr, c[0], c[1], c[2], a.depth + image, &f, &pix)) {
          if (!loaded) {  // (the first hit: the voxel's state comes in, once)
            tv = a.tsdf[at], w = a.weight[at];
            if (a.intensity) ci = a.intensity[at];
            loaded = true;
          }
          const float sample_c = a.intensity ? a.intensity_image[image + pix] : 0.f;
          wrote = tsdf_state_apply(a.ops[op].sign, a.fr.max_weight, f, sample_c, a.intensity != nullptr, &tv, &w, &ci);
          dirty = dirty || wrote;
        }
      }
      const unsigned long long hit = __ballot(wrote);
      if (lane == 0) counts[wave][op] += __popcll(hit);
    }
    if (dirty) {  // (valid: only a valid voxel is written)
      a.tsdf[at] = tv, a.weight[at] = (uint16_t)w;
      if (a.intensity) a.intensity[at] = ci;
    }
  }
  __syncthreads();
  if (threadIdx.x < TSDF_MAX_OPS) {
    int total = 0;
#pragma unroll
    for (int v = 0; v < TSDF_THREADS / 64; ++v) total += counts[v][threadIdx.x];
    a.slots[(size_t)blockIdx.x * TSDF_MAX_OPS + threadIdx.x] = total;  // (ops past n_ops: 0)
  }
}

// out[op] = the sum of op's column of the nblocks slots; one workgroup per op.  A thread's share is at most 32 chunks
// of at most 2^17 voxels: below 2^31
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_apply_sum_kernel(const int* __restrict__ slots, int nblocks,
                                                                       long long* __restrict__ out) {
  int v = 0;
  for (int i = threadIdx.x; i < nblocks; i += TSDF_THREADS) v += slots[(size_t)i * TSDF_MAX_OPS + blockIdx.x];
  const long long total = block_total<TSDF_THREADS>((long long)v);
  if (threadIdx.x == 0) out[blockIdx.x] = total;
}

void launch_tsdf_apply(const TsdfApplyArgs& a, int nblocks, long long* n_updated, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_apply_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_apply_sum_kernel, dim3(a.n_ops), dim3(TSDF_THREADS), 0, s, a.slots, nblocks, n_updated);
}

}  // namespace icpk
