// kernels_score.hip -- K15: scoring of candidate poses (icpk_score_poses; the rule is spelled out in include/icpk.h and
// restated in tests/score_model.py).
//
//   1. score_search_kernel  the hot path: ONE launch over the (pose, source point) grid of a chunk of poses
//                           (blockIdx.y = pose).  Every (pose, point) moves its point by the pose -- K3's arithmetic --
//                           and finds its exact nearest target within max_dist by an expanding walk over K1d's index of
//                           the target (kernels_grid.hip: the target sorted by cell, `cell_start`), see below.  No seeds:
//                           a candidate pose may be anywhere.  The result is one 64-bit (distance bits, index) key per
//                           (pose, point), NN_KEY_INIT where the point has no partner.
//   2. score_reduce_kernel  the eleven terms of every inlier through the canonical tree (include/icpk.h, ICPK_RED_*),
//      score_final_kernel   with the canonical geometry PER POSE (blockIdx.y = pose, red_blocks(ns) workgroups each):
//                           per-block partials, then the 256 slots on one workgroup per pose.
// The keys are the interface between the two: the search may deal a point to any number of lanes in any order (its
// result is a minimum over different keys), the sums follow the source's index order whatever the search did.
#include "grid_walk.h"
#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {

// Diagnostic build only (-DICPK_SCORE_COUNT, tools/score_bench.py --count): candidates evaluated and rounds walked,
// added up over all (pose, point) lanes since the last read
#ifdef ICPK_SCORE_COUNT
__device__ unsigned long long score_dbg[2];
extern "C" int icpk_debug_read_score_count(unsigned long long* out) {
  const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(score_dbg), sizeof(score_dbg));
  const unsigned long long zero[2] = {0, 0};
  return rc ? rc : (int)hipMemcpyToSymbol(HIP_SYMBOL(score_dbg), zero, sizeof(zero));
}
#define SCORE_COUNT(k, v) atomicAdd(&score_dbg[k], (unsigned long long)(v))
#else
#define SCORE_COUNT(k, v)
#endif

namespace {

constexpr int SC_S = 8;        // lanes per (pose, point): a cube of 3 cells per axis has 9 (y, z) rows (as K12, K13)
constexpr int SC_BLOCK = 256;
constexpr int SC_UNROLL = 4;   // candidates per lane and round trip
constexpr int SC_MAX_ROUNDS = 256;  // (a guard: a radius that doubles reaches max_dist, a finite float, sooner)

// The exact nearest target with d < max_dist of one moved point, without a seed.
//
// Exactness.  After the cube of radius R has been walked, every target with pair_dist <= R has been seen
// (grid_walk.h).  `best` is the smallest (d, j) key among the targets seen so far that have
// d < max_dist.  Three ways out:
//   best.d <= R         every target that could beat or tie best has d <= best.d <= R and has been seen: best is final.
//   best.d >  R         (a target from a corner of the cube) one more round with R := best.d -- which is < max_dist, so
//                       this is the cube of min(best.d, max_dist) -- sees everything with d <= best.d: final after it.
//   nothing, R >= max_dist   every target with d < max_dist <= R has been seen: the point has no partner.
// Otherwise nothing has been found and R doubles, up to max_dist.  When the cube is the whole grid on all three axes
// every target has been seen and whatever was found is final.
// Cost.  The first radius is one cell edge h: the grid is sized for `ppc` targets per h x h of surface, so where a
// target lies within h -- every point of a pose near the truth -- the walk ends after one round of ~4 ppc candidates,
// whatever max_dist is.  Only a point with nothing near pays for its growing cube (each round at most twice the last).
// Shape.  SC_S adjacent lanes share a (pose, point): the walk of grid_walk.h, the points in the source's order.
__global__ __launch_bounds__(SC_BLOCK) void score_search_kernel(const ScoreArgs a) {
  const int slice = threadIdx.x & (SC_S - 1);
  const int i = (int)((blockIdx.x * (unsigned)SC_BLOCK + threadIdx.x) / SC_S);
  const int pose = blockIdx.y;
  const bool live = i < a.ns;
  float px = live ? a.sx[i] : 0.f, py = live ? a.sy[i] : 0.f, pz = live ? a.sz[i] : 0.f;
  if (a.T) {  // (uniform) p = fl32(fl32(R s) + t): K3's arithmetic
    const float* __restrict__ T = a.T + 16 * (size_t)pose;  // uniform address: scalar loads
    const float sx = px, sy = py, sz = pz;
    px = rot_row(T[0], T[1], T[2], sx, sy, sz) + T[3];
    py = rot_row(T[4], T[5], T[6], sx, sy, sz) + T[7];
    pz = rot_row(T[8], T[9], T[10], sx, sy, sz) + T[11];
  }
  const GridInfo g = *a.index.gi;
  const float max_dist = a.max_dist;
  // a non-finite point never pairs (and its cube would be the whole grid)
  bool active = live && finite3(px, py, pz);
  float R = __builtin_fminf(g.h, max_dist);
  bool last = false;  // this round is the one after a find beyond R
  nn_key_t best = NN_KEY_INIT;
  for (int round = 0; round < SC_MAX_ROUNDS && __builtin_amdgcn_ballot_w64(active) != 0; ++round) {
    // (the rows and candidates by hand, not through grid_walk.h's iterators: with them the fourth load of a batch
    // went behind a branch)
    const Walk w = make_walk(g, px, py, pz, R, active);
    const bool whole = w.whole(g);
    if (active && slice == 0) SCORE_COUNT(1, 1);
    for (int row = slice; row < w.nrows; row += SC_S) {
      const int rz = row / w.nyr, ry = row - rz * w.nyr;
      const int base = ((w.z0 + rz) * g.ny + (w.y0 + ry)) * g.nx;  // cells base + x0 .. base + x1 < ncells, one range
      const int s0 = a.index.cell_start[base + w.x0], s1 = a.index.cell_start[base + w.x1 + 1];  // s1 <= the target's size
      SCORE_COUNT(0, s1 - s0);
      for (int j = s0; j < s1; j += SC_UNROLL) {
        float4 c[SC_UNROLL];
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) c[u] = a.index.t4[min(j + u, s1 - 1)];
#pragma unroll
        for (int u = 0; u < SC_UNROLL; ++u) {
          const float d = pair_dist(px, py, pz, c[u].x, c[u].y, c[u].z);
          // icp.cpp:553 (NaN and inf compare false: a non-finite target never pairs)
          const nn_key_t key = ((nn_key_t)__float_as_uint(d) << 32) | (unsigned)__float_as_int(c[u].w);
          const bool ok = j + u < s1 && d < max_dist;
          best = ok && key < best ? key : best;
        }
      }
    }
#pragma unroll
    for (int m = 1; m < SC_S; m <<= 1) {
      const nn_key_t o = __shfl_xor(best, m, 64);
      best = o < best ? o : best;
    }
    if (active) {
      const float bd = __uint_as_float((unsigned)(best >> 32));
      if (whole || last) {
        active = false;
      } else if (best != NN_KEY_INIT) {
        if (bd <= R) active = false;
        else R = bd, last = true;
      } else if (R >= max_dist) {
        active = false;
      } else {
        R = __builtin_fminf(R * 2.f, max_dist);
      }
    }
  }
  // (a point the guard stopped keeps what its last round found; no float radius gets there)
  if (live && slice == 0) a.keys[(size_t)pose * a.ns + i] = best;
}

// per pose the per-block partials of the eleven sums and the inlier count; `keys` holds an inlier's (d, j) or NN_KEY_INIT
__global__ __launch_bounds__(RED_THREADS) void score_reduce_kernel(const nn_key_t* __restrict__ keys,
                                                                   const float4* __restrict__ o4, int ns,
                                                                   double* __restrict__ partial,
                                                                   int* __restrict__ pcount) {
  const int tid = threadIdx.x, pose = blockIdx.y;
  const int P = gridDim.x * RED_THREADS;
  keys += (size_t)pose * ns;
  partial += (size_t)pose * NSCORE * RED_MAX_BLOCKS;
  pcount += (size_t)pose * RED_MAX_BLOCKS;
  double v[NSCORE];
#pragma unroll
  for (int s = 0; s < NSCORE; ++s) v[s] = 0.0;
  int cnt = 0;
  for (int i = blockIdx.x * RED_THREADS + tid; i < ns; i += P) {
    const nn_key_t key = keys[i];
    if (key == NN_KEY_INIT) continue;  // (not an inlier: +0.0 at its index)
    const double dd = (double)__uint_as_float((unsigned)(key >> 32));
    const float4 q = o4[(unsigned)(key & 0xffffffffu)];
    const double qx = q.x, qy = q.y, qz = q.z;
    v[0] += dd;
    v[1] += dd * dd;
    v[2] += qx; v[3] += qy; v[4] += qz;
    v[5] += qx * qx; v[6] += qx * qy; v[7] += qx * qz;
    v[8] += qy * qy; v[9] += qy * qz;
    v[10] += qz * qz;
    ++cnt;
  }
  block_partials<NSCORE>(v, cnt, partial + blockIdx.x, RED_MAX_BLOCKS, pcount + blockIdx.x);
}

// stage 2, one workgroup per pose: slot b = the sums of block b, +0.0 beyond nblocks, one slot per lane;
// out: per pose NSCORE doubles followed by the count as an int64
__global__ __launch_bounds__(RED_THREADS) void score_final_kernel(const double* __restrict__ partial,
                                                                  const int* __restrict__ pcount, int nblocks,
                                                                  double* __restrict__ out) {
  const int tid = threadIdx.x, pose = blockIdx.x;
  partial += (size_t)pose * NSCORE * RED_MAX_BLOCKS;
  pcount += (size_t)pose * RED_MAX_BLOCKS;
  out += (size_t)pose * (NSCORE + 1);
  double v[NSCORE];
#pragma unroll
  for (int s = 0; s < NSCORE; ++s) v[s] = tid < nblocks ? partial[s * RED_MAX_BLOCKS + tid] : 0.0;
  int cnt = tid < nblocks ? pcount[tid] : 0;
  block_partials<NSCORE>(v, cnt, out, 1, reinterpret_cast<long long*>(out) + NSCORE);
}

}  // namespace

void launch_score_poses(const ScoreArgs& a, int n_poses, hipStream_t s) {
  if (n_poses <= 0) return;
  if (a.ns > 0) {
    const unsigned blocks = (unsigned)(((size_t)a.ns * SC_S + SC_BLOCK - 1) / SC_BLOCK);
    hipLaunchKernelGGL(score_search_kernel, dim3(blocks, n_poses), dim3(SC_BLOCK), 0, s, a);
  }
  const int B = red_blocks(a.ns);  // (ns = 0: one block per pose that adds nothing)
  hipLaunchKernelGGL(score_reduce_kernel, dim3(B, n_poses), dim3(RED_THREADS), 0, s, a.keys, a.o4, a.ns, a.partial,
                     a.pcount);
  hipLaunchKernelGGL(score_final_kernel, dim3(n_poses), dim3(RED_THREADS), 0, s, a.partial, a.pcount, B, a.out);
}

}  // namespace icpk
