// grid_walk.h -- the cube walk over K1d's index of a cloud (kernels_grid.hip: the cloud sorted by cell, `cell_start`),
// shared by the kernels that visit a point's neighbourhood: K12's moments, K13's k-NN and radius count, K15's search,
// K16's two stages and K17's gradient sums.
//
// Exactness.  After the rows of cube_cells(p, r) on all three axes have been walked, every indexed point with
// pair_dist <= r has been met: the cube is a superset of their cells (the proof stands in front of K1d's sweep in
// kernels_grid.hip, "Cells met by the cube"; cube_cells is the same function).  What a kernel concludes from that --
// a radius that grows, a k-th distance -- is its own and stays with it.
// Shape.  S adjacent lanes share a point and deal the (y, z) rows of its cube among themselves; every row is one
// contiguous range of the sorted copy, and consecutive points are neighbours in space (cell order, or a depth
// camera's order), so the lanes of a wave read the same few rows of cells.
// Everything here is __forceinline__ and takes its callables by template parameter: a kernel compiles to one body.
#pragma once
#include "icpk_internal.h"
#include "nn_device.h"

namespace icpk {

// (x - x is 0 for a finite x and NaN otherwise)
__device__ __forceinline__ bool finite3(float x, float y, float z) { return ((x - x) + (y - y)) + (z - z) == 0.f; }

// the sum of v over the S adjacent lanes of a point, on every one of them
template <int S>
__device__ __forceinline__ long long sum_over_point(long long v) {
#pragma unroll
  for (int k = 1; k < S; k <<= 1) v += __shfl_xor(v, k, 64);
  return v;
}

// q = (int64)rint((u / r) * fix), fix a power of two, the quotient taken as the rules say -- by a division -- only
// where that can matter.  t = (u * fl(1 / r)) * fix differs from fl(u / r) * fix by less than 2^-36 at fix = 2^15
// (|u / r| <= 1 + 2^-19 for an accepted neighbour -- K17's figure, the looser of its two users': K12's is 1 + 2^-20,
// and the bound holds with either -- three roundings of 2^-53 each, times 2^15; the scaling is exact),
// so whenever t is further than 2^-30 from a rounding boundary k + 1/2 both round to the same integer, ties included.
__device__ __forceinline__ int quantise(double u, double rd, double inv_r, double fix) {
  double t = (u * inv_r) * fix;
  double k = __builtin_rint(t);
  if (!(__builtin_fabs(t - k) < 0.5 - 0x1p-30)) {
    t = (u / rd) * fix;
    k = __builtin_rint(t);
  }
  return (int)k;
}

// a point's S lanes store its N words side by side: lane k word k, lanes 0 and 1 also words 8 and 9
template <int S, int N>
__device__ __forceinline__ void store_point_words(long long* __restrict__ out, int slice, const long long (&w)[N]) {
  static_assert(S == 8 && N == 10, "the store deals ten words to eight lanes");
  const long long last = w[S + 1];
  long long mine = w[0], late = w[S];
#pragma unroll
  for (int k = 1; k < S; ++k) {
    const long long wk = w[k];  // (read whatever the lane: a select, no indexed copy of w)
    mine = slice == k ? wk : mine;
  }
  late = slice == 1 ? last : late;
  out[slice] = mine;
  if (slice < N - S) out[S + slice] = late;
}

// the cube of point (px, py, pz) and radius r: cells [x0, x1] x [y0, y1] x [z0, z1], nrows (y, z) rows of nyr per z
struct Walk {
  int x0, x1, y0, y1, z0, z1, nyr, nrows;
  // the cube is the whole grid: everything indexed is met
  __device__ __forceinline__ bool whole(const GridInfo& g) const {
    return x0 == 0 && x1 == g.nx - 1 && y0 == 0 && y1 == g.ny - 1 && z0 == 0 && z1 == g.nz - 1;
  }
};
// scan == false: no rows (a lane past the end, or a non-finite point, whose cube would be the whole grid)
__device__ __forceinline__ Walk make_walk(const GridInfo& g, float px, float py, float pz, float r, bool scan) {
  Walk w;
  cube_cells(px, r, g.lo[0], g.inv_hx, g.nx, w.x0, w.x1);
  cube_cells(py, r, g.lo[1], g.inv_h, g.ny, w.y0, w.y1);
  cube_cells(pz, r, g.lo[2], g.inv_h, g.nz, w.z0, w.z1);
  w.nyr = w.y1 - w.y0 + 1;
  w.nrows = scan ? w.nyr * (w.z1 - w.z0 + 1) : 0;  // <= 1024 x 1024 (grid_info_body)
  return w;
}

// row(s0, s1) for every row dealt to lane `slice` of S: its points are [s0, s1) of the sorted copy
template <int S, class Row>
__device__ __forceinline__ void walk_rows(const Walk& w, const GridInfo& g, const int* __restrict__ cell_start, int slice,
                                          Row&& row_fn) {
  for (int row = slice; row < w.nrows; row += S) {
    const int rz = row / w.nyr, ry = row - rz * w.nyr;
    const int base = ((w.z0 + rz) * g.ny + (w.y0 + ry)) * g.nx;  // cells base + x0 .. base + x1 < ncells, one range
    row_fn(cell_start[base + w.x0], cell_start[base + w.x1 + 1]);  // s1 <= the indexed cloud's size
  }
}

// The candidates of those rows, UNROLL per round trip: load(jj) for the whole batch (jj clamped into the row), THEN
// use(candidate, in_range) for each -- in_range false for the clamped repeats past the row's end.
template <int S, int UNROLL, class Load, class Use>
__device__ __forceinline__ void walk_candidates(const Walk& w, const GridInfo& g, const int* __restrict__ cell_start,
                                                int slice, Load&& load, Use&& use) {
  walk_rows<S>(w, g, cell_start, slice, [&](int s0, int s1) {
    for (int j = s0; j < s1; j += UNROLL) {
      decltype(load(0)) c[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) c[u] = load(UNROLL == 1 ? j : min(j + u, s1 - 1));
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) use(c[u], j + u < s1);
    }
  });
}

}  // namespace icpk
