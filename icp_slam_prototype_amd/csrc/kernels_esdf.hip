// kernels_esdf.hip -- K31: the exact Euclidean distance map of the TSDF volume (the distance rule and the query rule of
// esdf_rule.h).  K19's geometry throughout: the volume is a line of n voxels, x fastest, cut into chunks of a multiple
// of TSDF_THREADS; a thread owns one voxel, a wave 64 consecutive ones.
//
// One classification pass (tsdf and weight in, the class byte out) and three separable passes, along x, y, then z, over
// ONE signed int32 plane that carries both distance transforms of the rule (esdf_rule.h, rule 3): 4 bytes per voxel in
// and out per pass where the issue's two seed planes would move 8.  The x pass reads its seeds from the class bytes, so
// no seed plane is ever written; the z pass writes q.
//
// A lane searches its line outwards, offset by offset, and stops as soon as the squared offset reaches what it has
// found: the cost follows the distance found, not R, and the radius needs no window -- the bound implies it.  Lanes are
// along x in all three passes: at every offset a wave reads 64 consecutive words (bytes in the x pass), 256 contiguous
// bytes, whatever the axis.  Nothing is staged: a line of any length goes through the same loop, the neighbours come
// from L2 / Infinity Cache, and there is no halo, no segment and no dependence on how the volume is cut into chunks.
// Integers only; no atomic; a voxel is written by its owner alone: the same bytes on every run.  The counts go through
// block totals into per-chunk slots, summed by a second kernel, as K30's do.
#include "block_scan.h"
#include "esdf_rule.h"
#include "icpk_internal.h"

namespace icpk {

namespace {

// (idx < 2^30: 32-bit divisions)
__device__ __forceinline__ void esdf_split(unsigned idx, unsigned dx, unsigned dxy, int c[3]) {
  const unsigned k = idx / dxy, rem = idx - k * dxy, j = rem / dx;
  c[0] = (int)(rem - j * dx), c[1] = (int)j, c[2] = (int)k;
}

}  // namespace

__global__ __launch_bounds__(TSDF_THREADS) void esdf_classify_kernel(const EsdfArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  int count[3] = {0, 0, 0};
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    if (at >= end) continue;
    const int cls = esdf_class(a.tsdf[at], a.weight[at], a.min_weight);
    a.cls[at] = (uint8_t)cls;
#pragma unroll
    for (int k = 0; k < 3; ++k) count[k] += cls == k;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int total = block_total<TSDF_THREADS>(count[k]);
    if (threadIdx.x == 0) a.slots[k * TSDF_MAX_BLOCKS + blockIdx.x] = total;
  }
}

// the pass along AXIS: x from the class bytes into plane[0], y from plane[0] into plane[1], z from plane[1] into
// plane[0], finished to q, with the chunk's FAR voxels counted
template <int AXIS>
__global__ __launch_bounds__(TSDF_THREADS) void esdf_pass_kernel(const EsdfArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const unsigned dx = (unsigned)a.dims[0], dxy = dx * (unsigned)a.dims[1];
  const long long stride = AXIS == 0 ? 1 : AXIS == 1 ? (long long)dx : (long long)dxy;
  const int len = a.dims[AXIS], cap = esdf_cap(a.R), flags = a.flags;
  const int32_t* __restrict__ in = AXIS == 1 ? a.plane[0] : a.plane[1];
  int32_t* __restrict__ out = AXIS == 1 ? a.plane[1] : a.plane[0];
  int far = 0;
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    if (at >= end) continue;
    int c[3];
    esdf_split((unsigned)at, dx, dxy, c);
    const int j = c[AXIS];  // (0 <= j + d < len keeps at + d stride inside the volume)
    int s;
    if (AXIS == 0) {
      const uint8_t* __restrict__ row = a.cls + at;
      const auto seed = [=](int d) { return esdf_seed(esdf_obstacle(row[d], flags), cap); };
      s = esdf_line_min<ESDF_STEP>(seed(0), j, len, seed);
    } else {
      const int32_t* __restrict__ line = in + at;
      s = esdf_line_min<ESDF_STEP>(line[0], j, len, [=](int d) { return line[(long long)d * stride]; });
    }
    if (AXIS == 2) {
      s = esdf_finish(s, cap);
      far += s == ESDF_FAR || s == -ESDF_FAR;
    }
    out[at] = s;
  }
  if (AXIS == 2) {
    const int total = block_total<TSDF_THREADS>(far);
    if (threadIdx.x == 0) a.slots[3 * TSDF_MAX_BLOCKS + blockIdx.x] = total;
  }
}

// out[k] = the sum of row k of the slots; one workgroup per count.  A thread's share is at most 32 chunks of at most
// 2^17 voxels: below 2^31
__global__ __launch_bounds__(TSDF_THREADS) void esdf_sum_kernel(const int* __restrict__ slots, int nblocks,
                                                                 long long* __restrict__ out) {
  int v = 0;
  for (int i = threadIdx.x; i < nblocks; i += TSDF_THREADS) v += slots[blockIdx.x * TSDF_MAX_BLOCKS + i];
  const long long total = block_total<TSDF_THREADS>((long long)v);
  if (threadIdx.x == 0) out[blockIdx.x] = total;
}

__global__ __launch_bounds__(TSDF_THREADS) void esdf_box_kernel(const EsdfBoxArgs a, int32_t* __restrict__ sq_out,
                                                                 uint8_t* __restrict__ cls_out, float* __restrict__ dist_out) {
  const long long e = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (e >= a.box.m) return;
  const long long sxy = (long long)a.box.size[0] * a.box.size[1];
  const long long k = e / sxy, rem = e - k * sxy, j = rem / a.box.size[0], i = rem - j * a.box.size[0];
  const long long at = (a.box.lo[0] + i) + (long long)a.box.dims[0] * ((a.box.lo[1] + j) + (long long)a.box.dims[1] * (a.box.lo[2] + k));
  const int q = a.sq[at];
  if (sq_out) sq_out[e] = q;
  if (cls_out) cls_out[e] = a.cls[at];
  if (dist_out) dist_out[e] = esdf_metric(q, a.R, a.voxel);
}

__global__ __launch_bounds__(TSDF_THREADS) void esdf_query_kernel(const EsdfMap m, const float* __restrict__ xyz, int n,
                                                                   float* __restrict__ out) {
  const int i = blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[i], xyz[(size_t)n + i], xyz[2 * (size_t)n + i]};
  float dist, g[3];
  const int status = esdf_query(m, p, &dist, g);
  out[i] = dist;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[(size_t)(1 + a) * n + i] = g[a];
  reinterpret_cast<int*>(out)[4 * (size_t)n + i] = status;
}

void launch_esdf_compute(const EsdfArgs& a, int nblocks, long long* counts, hipStream_t s) {
  hipLaunchKernelGGL(esdf_classify_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(esdf_pass_kernel<0>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(esdf_pass_kernel<1>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(esdf_pass_kernel<2>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(esdf_sum_kernel, dim3(4), dim3(TSDF_THREADS), 0, s, a.slots, nblocks, counts);
}

void launch_esdf_box(const EsdfBoxArgs& a, int32_t* sq_out, uint8_t* cls_out, float* dist_out, hipStream_t s) {
  const int nblocks = (int)((a.box.m + TSDF_THREADS - 1) / TSDF_THREADS);
  hipLaunchKernelGGL(esdf_box_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a, sq_out, cls_out, dist_out);
}

void launch_esdf_query(const EsdfMap& m, const float* xyz, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(esdf_query_kernel, dim3((n + TSDF_THREADS - 1) / TSDF_THREADS), dim3(TSDF_THREADS), 0, s, m, xyz, n, out);
}

}  // namespace icpk
