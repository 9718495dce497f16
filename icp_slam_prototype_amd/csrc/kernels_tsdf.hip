// kernels_tsdf.hip -- K19, K20, K21: the dense TSDF volume.  Integration of one posed depth frame (one thread per voxel,
// the rule of tsdf_rule.h from the voxel's own indices) and extraction of the zero crossings as an ordered point list with
// normals (count / scan / scatter, as K4 compacts an image).  A voxel is owned by one thread: no atomic of any kind,
// the same bytes on every run.  K20 casts one ray per pixel through the volume (the ray rule of tsdf_rule.h) into eight
// image planes, a pixel owned by one thread, and compacts their valid pixels into a list with K19's scan.  K21 extracts
// a triangle mesh (the mesh rule of tsdf_rule.h): K19's count / scan / scatter for the vertices and for the triangles.
// K23 moves the volume by whole voxels into a second set of planes (the shift rule of tsdf_rule.h), lists the crossings
// such a move would lose with K19's three passes, and packs a sub-box of a plane for download.
//
// Both walks share one geometry: the volume is a line of n = dx dy dz voxels in linear order (x fastest), cut into at
// most TSDF_MAX_BLOCKS contiguous chunks of a multiple of TSDF_THREADS voxels, one workgroup per chunk, which it
// sweeps TSDF_THREADS voxels at a time.  A wave therefore reads and writes 64 consecutive voxels: 256 contiguous bytes
// of the tsdf plane, 128 of the weight plane.
#include "block_scan.h"
#include "icpk_internal.h"
#include "tsdf_rule.h"

namespace icpk {

namespace {

struct VoxelIndex {
  unsigned dx, dxy;
  __device__ __forceinline__ void split(unsigned idx, int c[3]) const {  // (idx < 2^30: 32-bit divisions)
    const unsigned k = idx / dxy, rem = idx - k * dxy, j = rem / dx;
    c[0] = (int)(rem - j * dx), c[1] = (int)j, c[2] = (int)k;
  }
};

// the sum of v over the workgroup, in every thread (integers: the order does not matter).  One barrier, on the caller's
// own four words of LDS: the count kernels below call it once per sum, at their end, and never again on the same words,
// so they do not pay for block_scan.h's barrier in front of the store
__device__ __forceinline__ int block_sum(int v, int* lds4) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

}  // namespace

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(const TsdfIntegrateArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.fr.dims[0], (unsigned)a.fr.dims[0] * (unsigned)a.fr.dims[1]};
  int written = 0;
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    if (at >= end) continue;
    int c[3];
    vi.split((unsigned)at, c);
    float f;
    int pix;
    if (!tsdf_sample(a.fr, c[0], c[1], c[2], a.depth, &f, &pix)) continue;  // (nothing of the volume read or written)
    const int w = a.weight[at];
    a.tsdf[at] = tsdf_blend(a.tsdf[at], w, f);
    if (a.intensity) a.intensity[at] = tsdf_blend(a.intensity[at], w, a.intensity_image[pix]);
    a.weight[at] = (uint16_t)(w + 1 < a.fr.max_weight ? w + 1 : a.fr.max_weight);
    written += 1;
  }
  __shared__ int lds4[4];
  const int total = block_sum(written, lds4);
  if (threadIdx.x == 0) a.slots[blockIdx.x] = total;
}

// out[0] = the sum of the nslots block slots (one workgroup)
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_sum_slots_kernel(const int* __restrict__ slots, int nslots,
                                                                       long long* __restrict__ out) {
  int v = 0;
  for (int i = threadIdx.x; i < nslots; i += TSDF_THREADS) v += slots[i];
  __shared__ int lds4[4];
  const int total = block_sum(v, lds4);
  if (threadIdx.x == 0) out[0] = total;
}

// the statuses of voxel `at`'s three crossings (TSDF_NO_CROSSING where the voxel itself is below min_weight).  LEAVING
// (K23): as the leaving list sees them -- the crossings the shift keeps are no crossings
template <bool LEAVING>
__device__ __forceinline__ void crossing_statuses(const TsdfPlanes& v, const TsdfKeep& keep, const VoxelIndex& vi,
                                                  long long at, bool valid, int c[3], float& fv, int st[3]) {
  st[0] = st[1] = st[2] = TSDF_NO_CROSSING;
  if (!valid || (int)v.weight[at] < v.min_weight) return;
  vi.split((unsigned)at, c);
  fv = v.tsdf[at];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    st[axis] = tsdf_crossing(v, c, at, fv, axis, nullptr);
    if (LEAVING) st[axis] = tsdf_leaving_status(keep, c, axis, st[axis]);
  }
}

// pass 1: per chunk, the crossings that will be listed and those dropped for want of a normal
template <bool LEAVING>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_count_kernel(const TsdfExtractArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.v.dims[0], (unsigned)a.v.dims[0] * (unsigned)a.v.dims[1]};
  int listed = 0, dropped = 0;
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    int c[3] = {0, 0, 0}, st[3];
    float fv = 0.f;
    crossing_statuses<LEAVING>(a.v, a.keep, vi, at, at < end, c, fv, st);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      listed += st[axis] == TSDF_CROSSING;
      dropped += st[axis] == TSDF_NO_NORMAL;
    }
  }
  __shared__ int lds4[2][4];
  const int nl = block_sum(listed, lds4[0]);
  const int nd = block_sum(dropped, lds4[1]);
  if (threadIdx.x == 0) {
    a.counts[blockIdx.x] = nl;
    a.dropped[blockIdx.x] = nd;
  }
}

// pass 2 (one workgroup): offsets[b] = the crossings listed by the chunks before b, offsets[nblocks] = totals[0] =
// their number; totals[1] = the sum of `extra` (the dropped ones), or untouched where extra is null.  64-bit: 3 x 2^30
// crossings do not fit an int, while a round sums 256 chunks of at most 3 x 2^17 each, and a thread's share of
// `extra` is at most 32 such chunks: both below 2^31
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_scan_kernel(const int* __restrict__ counts,
                                                                  const int* __restrict__ extra, int nblocks,
                                                                  long long* __restrict__ offsets,
                                                                  long long* __restrict__ totals) {
  const long long listed = scan_rounds<TSDF_THREADS>(counts, offsets, nblocks);
  long long ne = 0;
  if (extra) {  // (uniform)
    int mine = 0;
    for (int i = threadIdx.x; i < nblocks; i += TSDF_THREADS) mine += extra[i];
    ne = block_total<TSDF_THREADS>((long long)mine);
  }
  if (threadIdx.x == 0) {
    offsets[nblocks] = listed;
    totals[0] = listed;
    if (extra) totals[1] = ne;
  }
}

// pass 3: the chunk's crossings again, each to its place: the chunk's offset, then voxel order, then axis order
template <bool LEAVING>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_scatter_kernel(const TsdfExtractArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.v.dims[0], (unsigned)a.v.dims[0] * (unsigned)a.v.dims[1]};
  if (a.offsets[blockIdx.x + 1] == a.offsets[blockIdx.x]) return;  // (uniform: nothing of this chunk is listed)
  long long run = a.offsets[blockIdx.x];
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    int c[3] = {0, 0, 0}, st[3];
    float fv = 0.f;
    crossing_statuses<LEAVING>(a.v, a.keep, vi, at, at < end, c, fv, st);
    const int mine = (st[0] == TSDF_CROSSING) + (st[1] == TSDF_CROSSING) + (st[2] == TSDF_CROSSING);
    int round_total;
    long long pos = run + block_excl_scan<TSDF_THREADS>(mine, &round_total);
    for (int axis = 0; axis < 3; ++axis) {
      if (st[axis] != TSDF_CROSSING) continue;
      TsdfCrossing cr;
      tsdf_crossing(a.v, c, at, fv, axis, &cr);  // (again, now with its outputs: crossings are few)
      if (pos < a.capacity) {                    // (always: the capacity is the scan's total)
        a.x[pos] = cr.p[0], a.y[pos] = cr.p[1], a.z[pos] = cr.p[2];
        a.nx[pos] = cr.n[0], a.ny[pos] = cr.n[1], a.nz[pos] = cr.n[2];
        a.intensity[pos] = cr.intensity;
        a.voxel_index[pos] = (int)at;
        a.axis[pos] = (uint8_t)axis;
      }
      pos += 1;
    }
    run += round_total;
  }
}

// ---- K23: the shift ----
// The new voxel (i, j, k) takes the old voxel (i + s_x, j + s_y, k + s_z), or the fresh state where that one is out of
// bounds.  Out of place: a thread owns TSDF_SHIFT_RUN consecutive destination voxels of the linear order (the run
// starts at a multiple of 4, so that its stores are one aligned 16-byte word to the float planes and one 8-byte word to
// the weights) and writes them once; no atomic, no LDS.  Where the run lies in one row and so do its four sources, they
// are four consecutive words s_x + dx (s_y + dy s_z) further on: one load, misaligned by s_x mod 4 words, which the
// hardware takes.  Elsewhere (a row's ends, the slab that comes in fresh, the volume's last voxels) voxel by voxel.
struct __attribute__((packed, aligned(4))) F4u {  // four floats wherever a float may lie
  float v[4];
};
struct __attribute__((packed, aligned(2))) H4u {  // four weights wherever a weight may lie
  uint16_t v[4];
};

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_shift_kernel(const TsdfShiftArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const int dx = a.dims[0], dy = a.dims[1], dz = a.dims[2];
  const VoxelIndex vi{(unsigned)dx, (unsigned)dx * (unsigned)dy};
  const long long delta = a.s[0] + (long long)dx * (a.s[1] + (long long)dy * a.s[2]);
  for (long long base = begin; base < end; base += TSDF_THREADS * TSDF_SHIFT_RUN) {
    const long long at = base + (long long)threadIdx.x * TSDF_SHIFT_RUN;  // (a multiple of 4: chunks are multiples of 256)
    if (at >= end) continue;
    int c[3];
    vi.split((unsigned)at, c);
    float f[TSDF_SHIFT_RUN], ci[TSDF_SHIFT_RUN];
    uint16_t w[TSDF_SHIFT_RUN];
    const int sy = c[1] + a.s[1], sz = c[2] + a.s[2], sx = c[0] + a.s[0];  // (|s| <= dims: no overflow)
    const bool row = c[0] + TSDF_SHIFT_RUN <= dx && sy >= 0 && sy < dy && sz >= 0 && sz < dz;
    if (row && sx >= 0 && sx + TSDF_SHIFT_RUN <= dx) {
      // (one row of the destination, one row of the source, all of it in bounds: at + delta .. + 3 are its indices)
      const F4u ff = *reinterpret_cast<const F4u*>(a.tsdf_in + (at + delta));
      const H4u ww = *reinterpret_cast<const H4u*>(a.weight_in + (at + delta));
#pragma unroll
      for (int q = 0; q < TSDF_SHIFT_RUN; ++q) f[q] = ff.v[q], w[q] = ww.v[q], ci[q] = 0.f;
      if (a.intensity_in) {
        const F4u cc = *reinterpret_cast<const F4u*>(a.intensity_in + (at + delta));
#pragma unroll
        for (int q = 0; q < TSDF_SHIFT_RUN; ++q) ci[q] = cc.v[q];
      }
    } else {
#pragma unroll
      for (int q = 0; q < TSDF_SHIFT_RUN; ++q) {
        f[q] = 0.f, w[q] = 0, ci[q] = 0.f;
        if (at + q >= end) continue;
        int cq[3];
        vi.split((unsigned)(at + q), cq);
        const int qx = cq[0] + a.s[0], qy = cq[1] + a.s[1], qz = cq[2] + a.s[2];
        if (qx < 0 || qx >= dx || qy < 0 || qy >= dy || qz < 0 || qz >= dz) continue;  // (fresh)
        const long long from = qx + (long long)dx * (qy + (long long)dy * qz);          // (in bounds: < n)
        f[q] = a.tsdf_in[from], w[q] = a.weight_in[from];
        if (a.intensity_in) ci[q] = a.intensity_in[from];
      }
    }
    if (at + TSDF_SHIFT_RUN <= end) {
      *reinterpret_cast<float4*>(a.tsdf_out + at) = make_float4(f[0], f[1], f[2], f[3]);
      *reinterpret_cast<ushort4*>(a.weight_out + at) = make_ushort4(w[0], w[1], w[2], w[3]);
      if (a.intensity_out) *reinterpret_cast<float4*>(a.intensity_out + at) = make_float4(ci[0], ci[1], ci[2], ci[3]);
    } else {  // (the volume's last one to three voxels)
      for (int q = 0; at + q < end; ++q) {
        a.tsdf_out[at + q] = f[q], a.weight_out[at + q] = w[q];
        if (a.intensity_out) a.intensity_out[at + q] = ci[q];
      }
    }
  }
}

// one thread per voxel of the box: x fastest, so a wave reads runs of a row and writes 64 consecutive entries
inline int tsdf_box_blocks(long long m) { return (int)((m + TSDF_THREADS - 1) / TSDF_THREADS); }
template <class T>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_box_kernel(const TsdfBoxArgs a, const T* __restrict__ plane,
                                                                 T* __restrict__ out) {
  const long long e = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (e >= a.m) return;
  const long long sxy = (long long)a.size[0] * a.size[1];
  const long long k = e / sxy, rem = e - k * sxy, j = rem / a.size[0], i = rem - j * a.size[0];
  out[e] = plane[(a.lo[0] + i) + (long long)a.dims[0] * ((a.lo[1] + j) + (long long)a.dims[1] * (a.lo[2] + k))];
}

// ---- K20: the ray cast ----
// One thread owns one pixel and writes only that pixel's eight words.  A wave is an 8 x 8 quarter of the workgroup's
// tile, so that neighbouring rays read neighbouring cells; the cell gathers are left to L2 / Infinity Cache.  The march
// is tsdf_raycast_pixel: a lane whose ray has ended idles until its wave's last ray has.
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_raycast_kernel(const TsdfRaycastArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ty = (wave >> 1) * 8 + (lane >> 3), tx = (wave & 1) * 8 + (lane & 7);
  const long long npix = (long long)a.r.rows * a.r.cols;
  int hits = 0, dropped = 0;
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int row = (t / a.tiles_x) * TSDF_RAY_TILE + ty, col = (t % a.tiles_x) * TSDF_RAY_TILE + tx;
    if (row >= a.r.rows || col >= a.r.cols) continue;
    float out[8];
    const int st = tsdf_raycast_pixel(a.v, a.r, row, col, out);
    const long long pix = (long long)row * a.r.cols + col;
#pragma unroll
    for (int k = 0; k < 8; ++k) a.maps[k * npix + pix] = out[k];
    hits += st == TSDF_RAY_HIT;
    dropped += st == TSDF_RAY_NO_NORMAL;
  }
  __shared__ int lds4[2][4];
  const int nh = block_sum(hits, lds4[0]);
  const int nd = block_sum(dropped, lds4[1]);
  if (threadIdx.x == 0) {
    a.hits[blockIdx.x] = nh;
    a.dropped[blockIdx.x] = nd;
  }
}

// the hand-over's pass 1: the valid pixels of chunk blockIdx.x
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_ray_count_kernel(const TsdfRayCompactArgs a) {
  const int pix = blockIdx.x * TSDF_THREADS + threadIdx.x;
  const int mine = pix < a.npix && a.maps[6LL * a.npix + pix] > 0.f;
  __shared__ int lds4[4];
  const int total = block_sum(mine, lds4);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

// pass 3: every valid pixel to its place, the chunk's offset plus its rank among the chunk's valid pixels
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_ray_scatter_kernel(const TsdfRayCompactArgs a) {
  const int pix = blockIdx.x * TSDF_THREADS + threadIdx.x;
  const int mine = pix < a.npix && a.maps[6LL * a.npix + pix] > 0.f;
  int total;
  const long long pos = a.offsets[blockIdx.x] + block_excl_scan<TSDF_THREADS>(mine, &total);
  if (!mine || pos >= a.capacity) return;  // (pos < capacity always: the capacity is the scan's total)
#pragma unroll
  for (int k = 0; k < 7; ++k) a.list[k * a.capacity + pos] = a.maps[(long long)(k < 6 ? k : 7) * a.npix + pix];
}

// ---- K21: the triangle mesh ----
// K19's chunk geometry and its count / scan / scatter, twice over: once for the vertices a voxel owns (the crossings on
// its seven edges), once for the triangles of the cell it is the lower corner of.  Both are a function of the voxel's
// own neighbourhood (tsdf_mesh_voxel), so the count pass and the two scatters agree without talking to each other.

// pass 1: per chunk, the listed vertices, those among them without a normal, and the triangles
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_mesh_count_kernel(const TsdfMeshArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.v.dims[0], (unsigned)a.v.dims[0] * (unsigned)a.v.dims[1]};
  int nv = 0, nt = 0, nn = 0;
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    if (at >= end) continue;
    int c[3];
    vi.split((unsigned)at, c);
    TsdfMeshVoxel mv;
    tsdf_mesh_voxel(a.v, c, at, true, &mv);
    nt += mv.triangles;
    for (int m = 1; m < 8; ++m) {
      if (!((mv.vertices >> (m - 1)) & 1)) continue;
      nv += 1;
      nn += !tsdf_mesh_vertex(a.v, c, at, m, nullptr);
    }
  }
  __shared__ int lds4[3][4];
  const int tv = block_sum(nv, lds4[0]);
  const int tt = block_sum(nt, lds4[1]);
  const int tn = block_sum(nn, lds4[2]);
  if (threadIdx.x == 0) {
    a.vcounts[blockIdx.x] = tv;
    a.tcounts[blockIdx.x] = tt;
    a.nonormal[blockIdx.x] = tn;
  }
}

// pass 3a: the chunk's vertices again, each to its place (the chunk's offset, then voxel order, then edge type), with
// its key next to it
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_mesh_vertex_kernel(const TsdfMeshArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.v.dims[0], (unsigned)a.v.dims[0] * (unsigned)a.v.dims[1]};
  if (a.voffsets[blockIdx.x + 1] == a.voffsets[blockIdx.x]) return;  // (uniform: the chunk owns no vertex)
  long long run = a.voffsets[blockIdx.x];
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    int c[3] = {0, 0, 0};
    TsdfMeshVoxel mv{0, 0, 0};
    if (at < end) {
      vi.split((unsigned)at, c);
      tsdf_mesh_voxel(a.v, c, at, true, &mv);
    }
    int round_total;
    long long pos = run + block_excl_scan<TSDF_THREADS>((int)__popc((unsigned)mv.vertices), &round_total);
    for (int m = 1; m < 8; ++m) {
      if (!((mv.vertices >> (m - 1)) & 1)) continue;
      TsdfMeshVertex vx;
      tsdf_mesh_vertex(a.v, c, at, m, &vx);
      if (pos < a.vcapacity) {  // (always: the capacity is the scan's total)
        a.x[pos] = vx.p[0], a.y[pos] = vx.p[1], a.z[pos] = vx.p[2];
        a.nx[pos] = vx.n[0], a.ny[pos] = vx.n[1], a.nz[pos] = vx.n[2];
        a.intensity[pos] = vx.intensity;
        a.voxel_index[pos] = (int)at;
        a.edge[pos] = (uint8_t)m;
      }
      pos += 1;
    }
    run += round_total;
  }
}

// the place of vertex (voxel, m) in the list: a binary search over the vertices of the voxel's chunk, which are sorted
// by (voxel, m).  -1 if it is not there (never: a triangle's cell is known, so its vertices are listed)
__device__ __forceinline__ int mesh_find_vertex(const TsdfMeshArgs& a, long long voxel, int m) {
  const long long ch = voxel / a.chunk;  // (voxel < n: ch < nblocks)
  long long lo = a.voffsets[ch];
  const long long last = a.voffsets[ch + 1];
  long long hi = last < a.vcapacity ? last : a.vcapacity;
  const long long key = voxel * 8 + m;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    const long long k = (long long)a.voxel_index[mid] * 8 + a.edge[mid];
    if (k < key) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= last || lo >= a.vcapacity) return -1;
  return (long long)a.voxel_index[lo] * 8 + a.edge[lo] == key ? (int)lo : -1;
}

// pass 3b (after 3a on the same stream): the chunk's triangles, cell by cell, tetrahedron by tetrahedron, in the
// table's order
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_mesh_triangle_kernel(const TsdfMeshArgs a) {
  const long long begin = (long long)blockIdx.x * a.chunk;
  const long long end = begin + a.chunk < a.n ? begin + a.chunk : a.n;
  const VoxelIndex vi{(unsigned)a.v.dims[0], (unsigned)a.v.dims[0] * (unsigned)a.v.dims[1]};
  if (a.toffsets[blockIdx.x + 1] == a.toffsets[blockIdx.x]) return;  // (uniform: no triangle in this chunk)
  long long run = a.toffsets[blockIdx.x];
  for (long long base = begin; base < end; base += TSDF_THREADS) {
    const long long at = base + threadIdx.x;
    TsdfMeshVoxel mv{0, 0, 0};
    if (at < end) {
      int c[3];
      vi.split((unsigned)at, c);
      tsdf_mesh_voxel(a.v, c, at, false, &mv);
    }
    int round_total;
    long long pos = run + block_excl_scan<TSDF_THREADS>(mv.triangles, &round_total);
    if (mv.triangles > 0) {
      for (int tet = 0; tet < 6; ++tet) {
        int vc[4];
        tsdf_tet_corners(tet, vc);
        const int cs = tsdf_tet_case(mv.signs, vc);
        const unsigned code = tsdf_case_table(cs);
        const int ntri = tsdf_case_triangles(cs);
        for (int tri = 0; tri < ntri; ++tri) {
          int idx[3];
          for (int k = 0; k < 3; ++k) {
            int corner, m;
            tsdf_triangle_edge(vc, tsdf_tet_odd(tet), code, tri, k, &corner, &m);
            idx[k] = mesh_find_vertex(a, at + tsdf_mask_offset(a.v, corner), m);  // (a corner of cell V: in range)
          }
          if (pos < a.tcapacity) {  // (always: the capacity is the scan's total)
            a.triangles[3 * pos] = idx[0], a.triangles[3 * pos + 1] = idx[1], a.triangles[3 * pos + 2] = idx[2];
          }
          pos += 1;
        }
      }
    }
    run += round_total;
  }
}

void launch_tsdf_mesh_count(const TsdfMeshArgs& a, int nblocks, long long* totals, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  // totals[0] = vertices, [1] = those without a normal; totals[2] = triangles
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.vcounts, a.nonormal, nblocks, a.voffsets, totals);
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.tcounts, (const int*)nullptr, nblocks,
                     a.toffsets, totals + 2);
}

void launch_tsdf_mesh_scatter(const TsdfMeshArgs& a, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_mesh_vertex_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_mesh_triangle_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
}

void launch_tsdf_integrate(const TsdfIntegrateArgs& a, int nblocks, long long* n_updated, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_sum_slots_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.slots, nblocks, n_updated);
}

void launch_tsdf_count(const TsdfExtractArgs& a, int nblocks, long long* totals, hipStream_t s) {
  if (a.leaving) hipLaunchKernelGGL(tsdf_count_kernel<true>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  else hipLaunchKernelGGL(tsdf_count_kernel<false>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.counts, a.dropped, nblocks, a.offsets, totals);
}

void launch_tsdf_scatter(const TsdfExtractArgs& a, int nblocks, hipStream_t s) {
  if (a.leaving) hipLaunchKernelGGL(tsdf_scatter_kernel<true>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  else hipLaunchKernelGGL(tsdf_scatter_kernel<false>, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
}

void launch_tsdf_shift(const TsdfShiftArgs& a, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_shift_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
}

void launch_tsdf_box(const TsdfBoxArgs& a, const float* plane, float* out, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_box_kernel<float>, dim3(tsdf_box_blocks(a.m)), dim3(TSDF_THREADS), 0, s, a, plane, out);
}

void launch_tsdf_box(const TsdfBoxArgs& a, const uint16_t* plane, uint16_t* out, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_box_kernel<uint16_t>, dim3(tsdf_box_blocks(a.m)), dim3(TSDF_THREADS), 0, s, a, plane, out);
}

void launch_tsdf_raycast(const TsdfRaycastArgs& a, int nblocks, long long* totals, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_raycast_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_sum_slots_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.hits, nblocks, totals);
  hipLaunchKernelGGL(tsdf_sum_slots_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.dropped, nblocks, totals + 1);
}

void launch_tsdf_ray_count(const TsdfRayCompactArgs& a, long long* totals, hipStream_t s) {
  const int nblocks = tsdf_ray_chunks(a.npix);
  hipLaunchKernelGGL(tsdf_ray_count_kernel, dim3(nblocks), dim3(TSDF_THREADS), 0, s, a);
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_THREADS), 0, s, a.counts, (const int*)nullptr, nblocks, a.offsets,
                     totals);
}

void launch_tsdf_ray_scatter(const TsdfRayCompactArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(tsdf_ray_scatter_kernel, dim3(tsdf_ray_chunks(a.npix)), dim3(TSDF_THREADS), 0, s, a);
}

}  // namespace icpk
