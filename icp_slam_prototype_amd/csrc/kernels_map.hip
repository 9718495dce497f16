// kernels_map.hip -- the voxel certainty map of the reference (map.hpp, map.cpp) on the device.
//
// An update applies one of three per-point rules (map.cpp:88-119, :122-206, :220-269; see ICPK_MAP_* in icpk.h) to a
// batch of points, and must leave grid, slots and lists as the sequential loop over the batch would.  The rules are
// monotone in the certainty, so what k hits on one voxel do depends only on (cert0, d, k): the final certainty and the
// hit j that fills an empty slot have closed forms (map_segment below).  The batch is therefore ordered by voxel
// (stable: hits of one voxel stay in input order), every run of equal voxels is settled by its last element, and the
// points that fill a slot are appended in INPUT order by an exclusive scan of their flags:
//   K_key      voxel key per point + the tile histogram of the first radix digit         1 launch
//   radix sort 25-bit keys, 3 passes of 9 bits (LSD, stable): scan, scatter, histogram   8 launches
//   K_seg      per run of one voxel: binary search for its head, closed forms, flag      1 launch
//   scan       per-tile flag counts -> list positions                                    1 launch
//   K_append   list entries and slots of the flagged points                              1 launch
// Nothing is O(n^2), no lane walks the batch, and no per-voxel scratch needs clearing: the only state outside the
// batch-sized buffers is the grid and the slots themselves.
// Tiles are 1024 items (16 wave64), one per lane.  The rank of an item among the items of its tile with the same
// digit comes from 9 ballots (the lanes of a wave whose digit equals this lane's) and per-wave digit counts in LDS.
#include "block_scan.h"
#include "icpk.h"
#include "icpk_internal.h"
#include "map_device.h"
#include "nn_device.h"

namespace icpk {

constexpr int MAP_WAVES = MAP_TILE / 64;

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// The lanes of this wave holding the same digit as this lane (valid lanes only); the lowest of them records the group
// size in wcnt[wave][digit].  wcnt must be zero on entry and is complete after the caller's __syncthreads().
__device__ __forceinline__ unsigned long long tile_match(unsigned digit, bool valid, int (*wcnt)[MAP_RADIX]) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < MAP_RADIX_BITS; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  if (valid && (m & lanes_below()) == 0) wcnt[threadIdx.x >> 6][digit] = __popcll(m);
  return m;
}

__device__ __forceinline__ void zero_wcnt(int (*wcnt)[MAP_RADIX]) {
  int* w = &wcnt[0][0];
  for (int k = threadIdx.x; k < MAP_WAVES * MAP_RADIX; k += MAP_TILE) w[k] = 0;
  __syncthreads();
}

// digit counts of this tile, digit-major: hist[digit * ntiles + tile] (what the scan turns into scatter bases)
__device__ __forceinline__ void tile_hist(unsigned digit, bool valid, int* __restrict__ hist, int ntiles) {
  __shared__ int wcnt[MAP_WAVES][MAP_RADIX];
  zero_wcnt(wcnt);
  tile_match(digit, valid, wcnt);
  __syncthreads();
  for (int d = threadIdx.x; d < MAP_RADIX; d += MAP_TILE) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < MAP_WAVES; ++w) s += wcnt[w][d];
    hist[d * ntiles + blockIdx.x] = s;
  }
}

// K_key: voxel key of batch element i (point idx[i] of the planes, or point i), the first digit's histogram, and the
// flags / per-tile flag counts of K_seg cleared
__global__ __launch_bounds__(MAP_TILE) void map_key_kernel(const MapPoints p, int* __restrict__ key,
                                                          int* __restrict__ hist, int ntiles, int* __restrict__ flag,
                                                          int* __restrict__ tcount) {
  const int i = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool valid = i < p.n;
  int k = 0;
  if (valid) {
    const int j = p.idx ? p.idx[i] : i;
    k = map_key_of(p.x[j], p.y[j], p.z[j]);
    key[i] = k;
    flag[i] = 0;
  }
  if (threadIdx.x == 0) tcount[blockIdx.x] = 0;
  tile_hist((unsigned)k & (MAP_RADIX - 1), valid, hist, ntiles);
}

__global__ __launch_bounds__(MAP_TILE) void map_hist_kernel(const int* __restrict__ keys, int n, int shift,
                                                           int* __restrict__ hist, int ntiles) {
  const int i = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool valid = i < n;
  tile_hist(valid ? ((unsigned)keys[i] >> shift) & (MAP_RADIX - 1) : 0u, valid, hist, ntiles);
}

// exclusive scan in place of m ints by one workgroup, one contiguous run per lane; *total (if given) = the sum
__global__ __launch_bounds__(MAP_TILE) void map_scan_kernel(int* __restrict__ a, int m, int* __restrict__ total) {
  const int sum = scan_runs<MAP_TILE>(a, m);
  if (threadIdx.x == 0 && total) *total = sum;
}

// one stable radix pass: item i of tile t with digit d goes to base[d][t] + (items of tile t with digit d before it)
__global__ __launch_bounds__(MAP_TILE) void map_scatter_kernel(const int* __restrict__ kin, const int* __restrict__ vin,
                                                              int n, int shift, const int* __restrict__ base,
                                                              int ntiles, int* __restrict__ kout,
                                                              int* __restrict__ vout) {
  __shared__ int wcnt[MAP_WAVES][MAP_RADIX];
  const int i = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool valid = i < n;
  const int k = valid ? kin[i] : 0;
  const unsigned d = ((unsigned)k >> shift) & (MAP_RADIX - 1);
  zero_wcnt(wcnt);
  const unsigned long long m = tile_match(d, valid, wcnt);
  __syncthreads();
  if (!valid) return;
  const int wave = threadIdx.x >> 6;
  int r = base[d * ntiles + blockIdx.x] + __popcll(m & lanes_below());
  for (int w = 0; w < wave; ++w) r += wcnt[w][d];
  kout[r] = k;
  vout[r] = vin ? vin[i] : i;
}

// Closed forms of k hits on one voxel with certainty c0 and delta d (1 <= d <= 255): the final certainty and the hit
// j (1-based) at which the rule fills an empty slot (j > k: it does not).
//   ADD_CLOUD:        cert_j = min(255, c0 + j d);  fills at the first j with cert_j >= 180
//   ADD_ASSOCIATED:   hit j saturates (255, fill) iff c0 + (j - 1) d > 255 - d, i.e. c0 + j d > 255
//   ADD_UNASSOCIATED: hit j saturates (255, fill) iff c0 + (j - 1) d >= 180 - d, i.e. c0 + j d >= 180
// Every later hit keeps 255 and meets a filled slot.
__device__ __forceinline__ void map_segment(int rule, int c0, int d, int k, int& final_cert, int& j) {
  const long long reach = (long long)c0 + (long long)k * d;
  if (rule == ICPK_MAP_ADD_ASSOCIATED) {
    j = (255 - c0) / d + 1;
    final_cert = k >= j ? 255 : (int)reach;
  } else {
    j = c0 + d >= ICPK_MAP_MAX_CONFIDENCE ? 1 : (ICPK_MAP_MAX_CONFIDENCE - c0 + d - 1) / d;
    if (rule == ICPK_MAP_ADD_CLOUD)
      final_cert = reach > 255 ? 255 : (int)reach;
    else
      final_cert = k >= j ? 255 : (int)reach;
  }
}

// K_seg: the last element of every run of equal keys settles its voxel (the only lane that touches it)
__global__ __launch_bounds__(256) void map_segment_kernel(const int* __restrict__ skey, const int* __restrict__ sval,
                                                          int n, int rule, int d, uint8_t* __restrict__ cert,
                                                          const int* __restrict__ slot, int* __restrict__ flag,
                                                          int* __restrict__ tcount) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n) return;
  const int k = skey[s];
  if (s + 1 < n && skey[s + 1] == k) return;
  int lo = 0, hi = s;  // first position holding k: skey[hi] == k throughout
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (skey[mid] < k)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int hits = s - lo + 1;
  int fin, j;
  map_segment(rule, (int)cert[k], d, hits, fin, j);
  cert[k] = (uint8_t)fin;
  if (slot[k] < 0 && j <= hits) {
    const int i = sval[lo + j - 1];  // the j-th hit in input order
    flag[i] = 1;
    atomicAdd(&tcount[i / MAP_TILE], 1);
  }
}

// K_append: flagged element i -> list position old_len + (flagged elements before i); its slot records it
__global__ __launch_bounds__(MAP_TILE) void map_append_kernel(const MapPoints p, const int* __restrict__ key,
                                                             const int* __restrict__ flag, const int* __restrict__ toff,
                                                             int old_len, int list, float* __restrict__ lx,
                                                             float* __restrict__ ly, float* __restrict__ lz,
                                                             int* __restrict__ slot) {
  __shared__ int wc[MAP_WAVES];
  const int i = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool f = i < p.n && flag[i] != 0;
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wc[wave] = __popcll(m);
  __syncthreads();
  if (!f) return;
  int r = toff[blockIdx.x] + __popcll(m & lanes_below());
  for (int w = 0; w < wave; ++w) r += wc[w];
  const int pos = old_len + r;
  const int j = p.idx ? p.idx[i] : i;
  lx[pos] = p.x[j];
  ly[pos] = p.y[j];
  lz[pos] = p.z[j];
  slot[key[i]] = (pos << 1) | list;
}

void launch_map_update(const MapPoints& p, int rule, int delta, int old_len, int list, float* lx, float* ly, float* lz,
                       uint8_t* cert, int* slot, const MapBuffers& b, hipStream_t s) {
  if (p.n <= 0) return;
  const int n = p.n, ntiles = (n + MAP_TILE - 1) / MAP_TILE;
  hipLaunchKernelGGL(map_key_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, p, b.key, b.hist, ntiles, b.flag, b.tcount);
  const int* kin = b.key;
  const int* vin = nullptr;  // pass 0: the identity
  int* kout = b.ka;
  int* vout = b.va;
  for (int pass = 0; pass < MAP_PASSES; ++pass) {
    const int shift = pass * MAP_RADIX_BITS;
    if (pass > 0)
      hipLaunchKernelGGL(map_hist_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, kin, n, shift, b.hist, ntiles);
    hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(MAP_TILE), 0, s, b.hist, MAP_RADIX * ntiles, (int*)nullptr);
    hipLaunchKernelGGL(map_scatter_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, kin, vin, n, shift, b.hist, ntiles, kout,
                       vout);
    kin = kout;
    vin = vout;
    kout = (kout == b.ka) ? b.kb : b.ka;
    vout = (vout == b.va) ? b.vb : b.va;
  }
  hipLaunchKernelGGL(map_segment_kernel, dim3((n + 255) / 256), dim3(256), 0, s, kin, vin, n, rule, delta, cert, slot,
                     b.flag, b.tcount);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(MAP_TILE), 0, s, b.tcount, ntiles, b.total);
  hipLaunchKernelGGL(map_append_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, p, b.key, b.flag, b.tcount, old_len, list,
                     lx, ly, lz, slot);
}

// ---- queries ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_query_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ z, int n,
                                                        const uint8_t* __restrict__ cert,
                                                        const int* __restrict__ slot, int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = map_key_of(x[i], y[i], z[i]);
  out[i] = (int)cert[k];
  out[n + i] = slot[k];
}

void launch_map_query(const float* x, const float* y, const float* z, int n, const uint8_t* cert, const int* slot,
                      int* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(map_query_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, z, n, cert, slot, out);
}

// ---- icpk_align_to_map: the rejected key points of every association sweep -------------------------------------
// The loop of icpk_align ran sweeps 0 .. nsw-1 over positions P_0 = the posed source, P_{s+1} = motion_s(P_s), with
// motion_s the transform the loop applied after sweep s.  The positions are rebuilt with the loop's arithmetic
// (kernels_transform.hip: p' = fl32(fl32(R p) + t)); a position is rejected iff its nearest map key point is not
// closer than max_dist (icp.cpp:503, the acceptance of the loop's reduction); the rejected positions are compacted in
// (sweep, query) order -- the order `nonAssociations` grows in (icp.cpp:507-509).
__device__ __forceinline__ float map_rot_row(float r0, float r1, float r2, float x, float y, float z) {
  return (float)__builtin_fma((double)r2, (double)z, __builtin_fma((double)r1, (double)y, (double)r0 * (double)x));
}

__global__ __launch_bounds__(256) void map_poses_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ z, int ns,
                                                        const Rt* __restrict__ motion, int nsw, float* __restrict__ px,
                                                        float* __restrict__ py, float* __restrict__ pz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  float X = x[i], Y = y[i], Z = z[i];
  for (int s = 0; s < nsw; ++s) {
    px[(size_t)s * ns + i] = X;
    py[(size_t)s * ns + i] = Y;
    pz[(size_t)s * ns + i] = Z;
    if (s + 1 < nsw) {
      const Rt& m = motion[s];
      const float nx = map_rot_row(m.R[0], m.R[1], m.R[2], X, Y, Z) + m.t[0];
      const float ny = map_rot_row(m.R[3], m.R[4], m.R[5], X, Y, Z) + m.t[1];
      const float nz = map_rot_row(m.R[6], m.R[7], m.R[8], X, Y, Z) + m.t[2];
      X = nx;
      Y = ny;
      Z = nz;
    }
  }
}

// flag[g] = position g rejected; tcount[tile] = rejected positions of the tile.  The scan over the map key points is
// the exact pair distance of icp.cpp:606-620 (nn_device.h); only the minimum matters here, not which point attains it.
__global__ __launch_bounds__(MAP_TILE) void map_reject_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pz, int m,
                                                             const float* __restrict__ tx, const float* __restrict__ ty,
                                                             const float* __restrict__ tz, int nt, float max_dist,
                                                             int* __restrict__ flag, int* __restrict__ tcount) {
  __shared__ int wc[MAP_WAVES];
  const int g = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool valid = g < m;
  const float qx = valid ? px[g] : 0.f, qy = valid ? py[g] : 0.f, qz = valid ? pz[g] : 0.f;
  float best = __builtin_inff();
  for (int j = 0; j < nt; ++j) {
    const float d = pair_dist(qx, qy, qz, tx[j], ty[j], tz[j]);
    best = d < best ? d : best;
  }
  const bool rej = valid && !(best < max_dist);
  if (valid) flag[g] = rej ? 1 : 0;
  const unsigned long long b = __ballot(rej);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < MAP_WAVES; ++w) s += wc[w];
    tcount[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(MAP_TILE) void map_compact_kernel(const float* __restrict__ px, const float* __restrict__ py,
                                                              const float* __restrict__ pz, int m,
                                                              const int* __restrict__ flag,
                                                              const int* __restrict__ toff, float* __restrict__ ox,
                                                              float* __restrict__ oy, float* __restrict__ oz) {
  __shared__ int wc[MAP_WAVES];
  const int g = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool f = g < m && flag[g] != 0;
  const unsigned long long b = __ballot(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wc[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int r = toff[blockIdx.x] + __popcll(b & lanes_below());
  for (int w = 0; w < wave; ++w) r += wc[w];
  ox[r] = px[g];
  oy[r] = py[g];
  oz[r] = pz[g];
}

void launch_map_rejected(const float* x, const float* y, const float* z, int ns, const Rt* motion, int nsw, float* px,
                         float* py, float* pz, const float* tx, const float* ty, const float* tz, int nt,
                         float max_dist, float* ox, float* oy, float* oz, const MapBuffers& b, hipStream_t s) {
  const int m = ns * nsw;
  if (m <= 0) return;
  const int ntiles = (m + MAP_TILE - 1) / MAP_TILE;
  hipLaunchKernelGGL(map_poses_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, x, y, z, ns, motion, nsw, px, py, pz);
  hipLaunchKernelGGL(map_reject_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, px, py, pz, m, tx, ty, tz, nt, max_dist,
                     b.flag, b.tcount);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(MAP_TILE), 0, s, b.tcount, ntiles, b.total);
  hipLaunchKernelGGL(map_compact_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, px, py, pz, m, b.flag, b.tcount, ox, oy, oz);
}

// ---- icpk_align_to_map_dense: the accepted positions of the last sweep ------------------------------------------
__global__ __launch_bounds__(MAP_TILE) void map_accept_kernel(const nn_key_t* __restrict__ best, int n, float max_dist,
                                                             int* __restrict__ flag, int* __restrict__ tcount) {
  __shared__ int wc[MAP_WAVES];
  const int g = blockIdx.x * MAP_TILE + threadIdx.x;
  const bool acc = g < n && __uint_as_float((unsigned)(best[g] >> 32)) < max_dist;  // icp.cpp:363
  if (g < n) flag[g] = acc ? 1 : 0;
  const unsigned long long b = __ballot(acc);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < MAP_WAVES; ++w) s += wc[w];
    tcount[blockIdx.x] = s;
  }
}

void launch_map_poses(const float* x, const float* y, const float* z, int ns, const Rt* motion, int nsw, float* px,
                      float* py, float* pz, hipStream_t s) {
  if (ns <= 0 || nsw <= 0) return;
  hipLaunchKernelGGL(map_poses_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, x, y, z, ns, motion, nsw, px, py, pz);
}

void launch_map_accepted(const float* px, const float* py, const float* pz, int n, const nn_key_t* best,
                         float max_dist, float* ox, float* oy, float* oz, const MapBuffers& b, hipStream_t s) {
  if (n <= 0) return;
  const int ntiles = (n + MAP_TILE - 1) / MAP_TILE;
  hipLaunchKernelGGL(map_accept_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, best, n, max_dist, b.flag, b.tcount);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(MAP_TILE), 0, s, b.tcount, ntiles, b.total);
  hipLaunchKernelGGL(map_compact_kernel, dim3(ntiles), dim3(MAP_TILE), 0, s, px, py, pz, n, b.flag, b.tcount, ox, oy, oz);
}

}  // namespace icpk
