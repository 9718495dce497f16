// kernels_map_nn.hip -- K9: the reference's mapped nearest-neighbour lookup (icp.cpp:371-486 getNearestMappedPoint /
// processVoxel) over the device certainty map (see ICPK_MAP_NN_* in icpk.h for the contract).
//
// One wave per query.  The walk visits the centre voxel, then cube shells r = 1 .. 43 in the reference's block order;
// inside a shell a candidate replaces the best only if it is strictly closer, so the shell's outcome is the minimum
// over (distance bits, rank in the shell's visit order) -- order-free, which lets 64 lanes split the shell.  Every
// lane keeps its own minimum key; one 64-bit wave minimum per shell, then the (wave-uniform) stop test of :393.
//
// Exact shortcuts (the result is the sequential walk's, bit for bit):
//   * a voxel can hold only points inside its own cell, widened to infinity on the clamping faces (index 0: NaN, huge
//     and negative coordinates land there; index 299: everything >= 299 c).  A voxel whose cell is not closer than the
//     current best cannot win and is not read; a shell whose six face slabs are all out of reach is skipped whole.
//     (Not after icpk_map_set_points has replaced a point list that filled slots name: MapNnArgs::cells_exact.)
//   * a bit per 4^3 brick (occupancy mask, rebuilt from the slots after every map change): empty bricks are not read.
//   * empty voxels yield the zero point (:477 compares a uchar with -1: always true).  They can win only if the query
//     lies within 0.75 m of the origin; such queries walk every voxel without the shortcuts above.
#include "icpk.h"
#include "icpk_internal.h"
#include "map_device.h"
#include "nn_device.h"

namespace icpk {

namespace {

constexpr int MNN_WAVES = 4;                 // queries per 256-thread workgroup
constexpr int MAP_MAX_RADIUS = 44;           // int(float(1.5) / float(10 / 300)): radii 1 .. 43 (icp.cpp:380)
constexpr float MNN_START = 0.75f;           // MAX_NN_COLOR_DISTANCE: the starting shortest distance
constexpr float MNN_STOP = 0.2f;             // MIN_NN_COLOR_DISTANCE
constexpr float MNN_SLACK = 1e-4f;           // metres added to a cell's extent (float rounding of p / c)
constexpr float MNN_LB_REL = 1.0f + 1e-5f;   // relative slack of the squared lower bound

// the coordinates a point stored in voxel index i may have along one axis
__device__ __forceinline__ float cell_lo(int i) { return i == 0 ? -__builtin_inff() : (float)i * MAP_C - MNN_SLACK; }
__device__ __forceinline__ float cell_hi(int i) {
  return (i == 0 || i == MAP_DIM - 1) ? __builtin_inff() : (float)(i + 1) * MAP_C + MNN_SLACK;
}
__device__ __forceinline__ float cell_gap(float q, int i) {
  return __builtin_fmaxf(__builtin_fmaxf(cell_lo(i) - q, q - cell_hi(i)), 0.f);
}

struct Walker {
  MapNnArgs a;
  float qx, qy, qz, d0;
  bool zmode;  // the zero point can win: read every voxel
  bool bound;  // stored points lie in their voxels' cells: the distance bound may skip voxels
  float lim2;  // a cell farther than sqrt(lim2) cannot beat the current best
  float shortest;
  unsigned long long bk;  // this lane's best (distance bits, rank) of the shell
  unsigned bt;            // ... and its target index

  // processVoxel (:476-486) at flat offset f = voxel (X, Y, Z), rank k of the shell
  __device__ __forceinline__ void visit(int f, int X, int Y, int Z, unsigned k) {
    if (!zmode) {
      if (bound) {
        const float gx = cell_gap(qx, X), gy = cell_gap(qy, Y), gz = cell_gap(qz, Z);
        if (__builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx)) > lim2) return;
      }
      const int b = ((X >> 2) * MAP_BRICKS + (Y >> 2)) * MAP_BRICKS + (Z >> 2);
      if (((a.mask[b >> 5] >> (b & 31)) & 1u) == 0u) return;
    }
    const int s = a.slot[f];
    const int li = s >> 1;
    float d = d0;
    unsigned t = a.n0 + a.n1;  // the zero point
    if (s >= 0 && (s & 1) == 0 && li < a.n0) {
      d = pair_dist(qx, qy, qz, a.l0x[li], a.l0y[li], a.l0z[li]);
      t = (unsigned)li;
    } else if (s >= 0 && (s & 1) == 1 && li < a.n1) {
      d = pair_dist(qx, qy, qz, a.l1x[li], a.l1y[li], a.l1z[li]);
      t = (unsigned)(a.n0 + li);
    } else if (!zmode) {
      return;  // empty (or names an entry past its list's end): the zero point, out of reach
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | k;
    if (d < shortest && key < bk) {
      bk = key;
      bt = t;
    }
  }
};

// step -> (row, column) of a rows x B block: floor(step / B) by a float reciprocal, corrected (step < 2^16)
__device__ __forceinline__ void split(int step, int B, float inv, int& ia, int& ib) {
  ia = (int)((float)step * inv);
  ib = step - ia * B;
  if (ib >= B) {
    ++ia;
    ib -= B;
  } else if (ib < 0) {
    --ia;
    ib += B;
  }
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(64 * MNN_WAVES) void map_nn_kernel(const MapNnArgs a) {
  if (loop_stopped(a.stop)) return;
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * MNN_WAVES + (threadIdx.x >> 6);
  if (qi >= a.nq) return;  // (wave-uniform)
  Walker w;
  w.a = a;
  w.qx = a.qx[qi];
  w.qy = a.qy[qi];
  w.qz = a.qz[qi];
  w.shortest = MNN_START;
  unsigned tgt = a.n0 + a.n1;
  const bool finite = __builtin_isfinite(w.qx) && __builtin_isfinite(w.qy) && __builtin_isfinite(w.qz);
  if (finite) {  // (a non-finite query is at distance inf or NaN from everything: nothing beats 0.75)
    const int vx = map_axis(w.qx), vy = map_axis(w.qy), vz = map_axis(w.qz);
    w.d0 = pair_dist(w.qx, w.qy, w.qz, 0.f, 0.f, 0.f);
    w.zmode = w.d0 < MNN_START;
    w.bound = !w.zmode && a.cells_exact != 0;
    // centre (:384-388): every lane reads the same voxel
    w.lim2 = MNN_START * MNN_START * MNN_LB_REL;
    w.bk = ~0ull;
    w.bt = tgt;
    w.visit((vx * MAP_DIM + vy) * MAP_DIM + vz, vx, vy, vz, 0u);
    if (w.bk != ~0ull) {
      w.shortest = __uint_as_float((unsigned)(w.bk >> 32));
      tgt = w.bt;
    }
    const bool walk = !(w.shortest < MNN_START);  // :386-388: a hit in the centre voxel ends the search
    for (int r = 1; walk && w.shortest >= MNN_STOP && r < MAP_MAX_RADIUS; ++r) {
      w.lim2 = w.shortest * w.shortest * MNN_LB_REL;
      const bool bx = vx - r >= 0 && vx + r < MAP_DIM, by = vy - r >= 0 && vy + r < MAP_DIM,
                 bz = vz - r >= 0 && vz + r < MAP_DIM;
      if (w.bound) {  // every voxel read in this shell lies in one of its face slabs (z overruns keep x = vx +- r)
        const float inf = __builtin_inff();
        float g = inf;
        if (bx) g = __builtin_fminf(g, __builtin_fminf(cell_gap(w.qx, vx - r), cell_gap(w.qx, vx + r)));
        if (by) g = __builtin_fminf(g, __builtin_fminf(cell_gap(w.qy, vy - r), cell_gap(w.qy, vy + r)));
        if (bz) g = __builtin_fminf(g, __builtin_fminf(cell_gap(w.qz, vz - r), cell_gap(w.qz, vz + r)));
        if (g * g > w.lim2) continue;
      }
      w.bk = ~0ull;
      const int B1 = 2 * r, B3 = 2 * r - 2;
      const unsigned base2 = 2u * B1 * B1, base3 = base2 + 2u * B3 * B1;
      if (bx) {  // block 1 (:393-418): x = vx -+ r, y in [vy - r, vy + r) checked, z in [vz - r, vz + r) NOT checked
        const float inv = 1.0f / (float)B1;
        for (int k = lane; k < 2 * B1 * B1; k += 64) {
          int ia, ib;
          split(k >> 1, B1, inv, ia, ib);
          const int y = vy - r + ia;
          if (y < 0 || y >= MAP_DIM) continue;
          const int z = vz - r + ib;
          int X = (k & 1) ? vx + r : vx - r, Y = y, Z = z;
          // pointLookupTable[x][y][z] with z outside [0, 300) is the flat neighbour ((x * 300 + y) * 300 + z)
          if (Z < 0) {
            Z += MAP_DIM;
            if (--Y < 0) {
              Y = MAP_DIM - 1;
              --X;
            }
          } else if (Z >= MAP_DIM) {
            Z -= MAP_DIM;
            if (++Y >= MAP_DIM) {
              Y = 0;
              ++X;
            }
          }
          if (X < 0 || X >= MAP_DIM) continue;  // beyond the table's ends: unpinned, not read
          w.visit((X * MAP_DIM + Y) * MAP_DIM + Z, X, Y, Z, (unsigned)k);
        }
      }
      if (by && B3 > 0) {  // block 2 (:421-443): x in [vx - r + 1, vx + r - 1), z in [vz - r, vz + r), y = vy -+ r
        const float inv = 1.0f / (float)B1;
        for (int k = lane; k < 2 * B3 * B1; k += 64) {
          int ia, ib;
          split(k >> 1, B1, inv, ia, ib);
          const int x = vx - r + 1 + ia, z = vz - r + ib;
          if (x < 0 || x >= MAP_DIM || z < 0 || z >= MAP_DIM) continue;
          const int y = (k & 1) ? vy + r : vy - r;
          w.visit((x * MAP_DIM + y) * MAP_DIM + z, x, y, z, base2 + (unsigned)k);
        }
      }
      if (bz && B3 > 0) {  // block 3 (:446-467): x in [vx - r + 1, vx + r - 1), y in [vy - r + 1, vy + r - 1), z = vz -+ r
        const float inv = 1.0f / (float)B3;
        for (int k = lane; k < 2 * B3 * B3; k += 64) {
          int ia, ib;
          split(k >> 1, B3, inv, ia, ib);
          const int x = vx - r + 1 + ia, y = vy - r + 1 + ib;
          if (x < 0 || x >= MAP_DIM || y < 0 || y >= MAP_DIM) continue;
          const int z = (k & 1) ? vz + r : vz - r;
          w.visit((x * MAP_DIM + y) * MAP_DIM + z, x, y, z, base3 + (unsigned)k);
        }
      }
      const unsigned long long m = wave_min_u64(w.bk);
      if (m != ~0ull) {  // (only keys below the shell's starting distance were kept)
        const unsigned long long who = __ballot(w.bk == m);
        const int src = __builtin_ctzll(who);
        tgt = __shfl(w.bt, src, 64);
        w.shortest = __uint_as_float((unsigned)(m >> 32));
      }
    }
  }
  if (lane == 0) a.best[qi] = ((unsigned long long)__float_as_uint(w.shortest) << 32) | tgt;
}

// one bit per 4^3 brick: set iff a slot of the brick is filled (a brick row of 4 z is one 16-byte load: 300 % 4 == 0)
__global__ __launch_bounds__(256) void map_mask_kernel(const int* __restrict__ slot, unsigned* __restrict__ mask) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  bool occ = false;
  if (b < MAP_BRICKS * MAP_BRICKS * MAP_BRICKS) {
    const int bx = b / (MAP_BRICKS * MAP_BRICKS), by = (b / MAP_BRICKS) % MAP_BRICKS, bz = b % MAP_BRICKS;
    int all = -1;
#pragma unroll
    for (int dx = 0; dx < 4; ++dx)
#pragma unroll
      for (int dy = 0; dy < 4; ++dy) {
        const int4 v = *reinterpret_cast<const int4*>(slot + ((size_t)(4 * bx + dx) * MAP_DIM + (4 * by + dy)) * MAP_DIM + 4 * bz);
        all &= v.x & v.y & v.z & v.w;
      }
    occ = all != -1;  // (empty slots are -1, filled ones non-negative)
  }
  const unsigned long long m = __ballot(occ);
  const int lane = threadIdx.x & 63;
  if ((lane & 31) == 0 && (b >> 5) < MAP_MASK_WORDS) mask[b >> 5] = (unsigned)(m >> lane);
}

}  // namespace

void launch_map_mask(const int* slot, unsigned* mask, hipStream_t s) {
  const int n = MAP_BRICKS * MAP_BRICKS * MAP_BRICKS;
  hipLaunchKernelGGL(map_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, s, slot, mask);
}

void launch_map_nn(const MapNnArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  hipLaunchKernelGGL(map_nn_kernel, dim3((a.nq + MNN_WAVES - 1) / MNN_WAVES), dim3(64 * MNN_WAVES), 0, s, a);
}

}  // namespace icpk
