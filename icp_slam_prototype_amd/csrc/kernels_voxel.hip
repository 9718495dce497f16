// kernels_voxel.hip -- K11: voxel-grid downsampling of one cloud (icpk_voxel_downsample; the rule is spelled out in
// include/icpk.h and restated in tests/voxel_model.py).
//
// A sparse, unbounded set of voxels is mapped to dense output slots without a sort:
//   1. voxel_insert_kernel   one lane per point: the voxel's packed key goes into an open-addressing table in HBM
//                            (64-bit compare-and-swap on the key word, linear probing); the slot collects the lowest
//                            member index (atomicMax of its complement), the member count and, for the centroid mode,
//                            the fixed-point sums.  Consecutive lanes of a wave that fall into the same voxel -- a wall
//                            puts hundreds of neighbouring pixels into one -- are summed through the cross-lane network
//                            first, and only the first lane of such a run goes to memory.
//   2. voxel_first_kernel    per point: the lowest member index of its voxel; per 1024 points: how many are that
//                            lowest member themselves (the voxel's representative)
//      voxel_scan_kernel     exclusive scan of those block counts (one workgroup); the total is n_out
//   3. voxel_emit_kernel     the representatives' rank in input order is the output position: points, normals and
//                            the groups are written there
//      voxel_resolve_kernel  every other point looks its output position up at its representative
// Every atomic is an integer operation, so nothing depends on the order in which members arrive: the outputs are the
// same bits on every run, and the bits of the CPU model.  All words of one slot share one 64-byte line.
#include "block_scan.h"
#include "icpk_internal.h"

namespace icpk {

static_assert(sizeof(VoxelSlot) == 64, "one slot, one 64-byte line");

namespace {

constexpr double VOXEL_LIMIT = 1048576.0;           // 2^20: a point further out on any axis is dropped
constexpr unsigned long long VOXEL_RADIX = 2097153;  // 2^21 + 1 biased coordinates per axis; RADIX^3 < 2^64 - 1
constexpr double VOXEL_FIX = 1073741824.0;           // 2^30: the fixed point of the centroid's sums
constexpr unsigned long long VOXEL_NO_KEY = ~0ull;   // a lane without a voxel (dropped point, or past the cloud's end)
constexpr unsigned VOXEL_INV = 0x7fffffffu;          // VoxelSlot::inv_first = VOXEL_INV - index

// u = p / L and v = floor(u) per axis; false: the point is dropped
__device__ __forceinline__ bool voxel_of(float px, float py, float pz, double L, double u[3], double v[3]) {
  const float p[3] = {px, py, pz};
  bool ok = true;
  for (int c = 0; c < 3; ++c) {
    u[c] = (double)p[c] / L;
    v[c] = __builtin_floor(u[c]);
    ok = ok && __builtin_isfinite(p[c]) && __builtin_fabs(v[c]) <= VOXEL_LIMIT;  // (a NaN v compares false)
  }
  return ok;
}

__device__ __forceinline__ unsigned long long voxel_key(const double v[3]) {
  const unsigned long long bx = (unsigned long long)((long long)v[0] + 1048576), by = (unsigned long long)((long long)v[1] + 1048576),
                           bz = (unsigned long long)((long long)v[2] + 1048576);
  return (bx * VOXEL_RADIX + by) * VOXEL_RADIX + bz + 1;  // (0 is the empty slot)
}

__device__ __forceinline__ unsigned voxel_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

__device__ __forceinline__ long long voxel_fix(double f) { return (long long)__builtin_rint(f * VOXEL_FIX); }

}  // namespace

__global__ __launch_bounds__(256) void voxel_insert_kernel(const VoxelArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < a.n;
  unsigned long long key = VOXEL_NO_KEY;
  long long q[6] = {0, 0, 0, 0, 0, 0};
  if (in) {
    double u[3], v[3];
    if (voxel_of(a.x[i], a.y[i], a.z[i], a.leaf, u, v)) {
      key = voxel_key(v);
      if (a.centroid) {
        for (int c = 0; c < 3; ++c) q[c] = voxel_fix(u[c] - v[c]);
        if (a.nx) {
          q[3] = voxel_fix((double)a.nx[i]);
          q[4] = voxel_fix((double)a.ny[i]);
          q[5] = voxel_fix((double)a.nz[i]);
        }
      }
    } else {
      atomicAdd(&a.counts[1], 1);  // (one add per wave: the compiler counts the active lanes)
    }
  }
  // runs of consecutive lanes with one key: [head, next) of this lane's run
  const unsigned long long prev = __shfl_up(key, 1);
  const unsigned long long heads = __ballot(lane == 0 || key != prev);
  const int head = 63 - __clzll(heads & (~0ull >> (63 - lane)));
  const unsigned long long rest = head == 63 ? 0ull : heads >> (head + 1);
  const int next = rest ? head + __ffsll((long long)rest) : 64;
  if (a.centroid) {  // the run's sums end up in its first lane
    const int nq = a.nx ? 6 : 3;
    for (int d = 1; d < 64; d <<= 1)
      for (int c = 0; c < nq; ++c) {
        const long long t = __shfl_down(q[c], d);
        if (lane + d < next) q[c] += t;
      }
  }
  int slot = -1;
  if (lane == head && key != VOXEL_NO_KEY) {
    unsigned s = voxel_hash(key) & a.mask;
    for (unsigned probe = 0; probe <= a.mask; ++probe, s = (s + 1) & a.mask) {  // (capacity >= 2 n: an empty slot is near)
      VoxelSlot* e = a.table + s;
      unsigned long long k = __hip_atomic_load(&e->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (k == 0) {
        k = atomicCAS(&e->key, 0ull, key);
        if (k == 0) k = key;
      }
      if (k != key) continue;
      slot = (int)s;
      atomicMax(&e->inv_first, VOXEL_INV - (unsigned)i);
      atomicAdd(&e->count, next - head);
      if (a.centroid) {
        const int nq = a.nx ? 6 : 3;
        for (int c = 0; c < nq; ++c) atomicAdd(reinterpret_cast<unsigned long long*>(&e->sum[c]), (unsigned long long)q[c]);
      }
      break;
    }
  }
  slot = __shfl(slot, head);
  if (in) a.slot_of[i] = slot;
}

// out_of_point[i] := the lowest member index of i's voxel (-1: dropped); bsum[block] := representatives among the
// block's 1024 points
__global__ __launch_bounds__(256) void voxel_first_kernel(const VoxelArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    const int s = a.slot_of[i];
    const int first = s < 0 ? -1 : (int)(VOXEL_INV - a.table[s].inv_first);
    a.out_of_point[i] = first;
    mine += first == i;
  }
  const int total = block_total<256>(mine);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

// bsum[nb] -> its exclusive scan in place; counts[0] := the total
__global__ __launch_bounds__(256) void voxel_scan_kernel(int* __restrict__ bsum, int nb, int* __restrict__ counts) {
  const int total = scan_rounds<256>(bsum, bsum, nb);
  if (threadIdx.x == 0) counts[0] = total;
}

__global__ __launch_bounds__(256) void voxel_emit_kernel(const VoxelArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int first[4];
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    first[k] = i < a.n ? a.out_of_point[i] : -1;
    mine += first[k] == i;  // (i >= 0: a dropped point never counts)
  }
  int total;
  int pos = a.bsum[blockIdx.x] + block_excl_scan<256>(mine, &total);
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    if (first[k] != i) {
      if (first[k] >= 0) a.out_of_point[i] = -2 - first[k];  // (voxel_resolve_kernel looks it up at the representative)
      continue;
    }
    const int o = pos++;
    const VoxelSlot* e = a.table + a.slot_of[i];
    const int m = e->count;
    a.out_of_point[i] = o;
    a.first_index[o] = i;
    a.count[o] = m;
    const float px = a.x[i], py = a.y[i], pz = a.z[i];
    if (!a.centroid) {
      a.ox[o] = px, a.oy[o] = py, a.oz[o] = pz;
      if (a.nx) a.onx[o] = a.nx[i], a.ony[o] = a.ny[i], a.onz[o] = a.nz[i];
      continue;
    }
    double u[3], v[3], r[3];
    voxel_of(px, py, pz, a.leaf, u, v);
    for (int c = 0; c < 3; ++c) r[c] = (v[c] + ((double)e->sum[c] / (double)m) / VOXEL_FIX) * a.leaf;
    a.ox[o] = (float)r[0], a.oy[o] = (float)r[1], a.oz[o] = (float)r[2];
    if (a.nx) {
      const double Nx = (double)e->sum[3], Ny = (double)e->sum[4], Nz = (double)e->sum[5];
      const double g = __builtin_sqrt(Nx * Nx + Ny * Ny + Nz * Nz);
      a.onx[o] = g == 0.0 ? 0.f : (float)(Nx / g);
      a.ony[o] = g == 0.0 ? 0.f : (float)(Ny / g);
      a.onz[o] = g == 0.0 ? 0.f : (float)(Nz / g);
    }
  }
}

__global__ __launch_bounds__(256) void voxel_resolve_kernel(int* __restrict__ out_of_point, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = out_of_point[i];
  if (v <= -2) out_of_point[i] = out_of_point[-2 - v];  // (a representative's entry is >= 0 and not written here)
}

void launch_voxel_downsample(const VoxelArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const int nb = (a.n + 1023) / 1024;
  hipLaunchKernelGGL(voxel_insert_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(voxel_first_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(voxel_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts);
  hipLaunchKernelGGL(voxel_emit_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(voxel_resolve_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a.out_of_point, a.n);
}

}  // namespace icpk
