// kernels_filter.hip -- K13: outlier removal on one of the context's clouds (icpk_remove_outliers; the rule is spelled
// out in include/icpk.h and restated in tests/filter_model.py).
//
//   1. knn_mean_kernel       STATISTICAL's hot path: the exact k smallest pair distances of every point over K1d's index
//                            of its own cloud (kernels_grid.hip: the cloud sorted by cell, `cell_start`), see below
//      radius_count_kernel   RADIUS: K12's radius search with a counter instead of ten moments
//   2. filter_sums_kernel    S1 = sum mean_i, S2 = sum mean_i^2 and N through the canonical tree (include/icpk.h,
//      filter_threshold_kernel  ICPK_RED_*): per-block partials, then the 256 slots on one workgroup, whose lane 0 goes
//                            on to mu, sigma and T -- the threshold never visits the host
//   3. filter_flag_kernel    keep flags -> counts per 1024 points; filter_scan_kernel: their exclusive scan, the total is
//      filter_emit_kernel    n_out; then the kept points (and normals) go to their rank in input order
// Nothing here is an atomic on a float and no sum depends on the order in which candidates arrive: a point's k smallest
// distances are selected as 64-bit (distance bits, index) keys, which are all different, and added in ascending order.
#include "block_scan.h"
#include "grid_walk.h"
#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {

namespace {

constexpr int KNN_S = 4;       // lanes per query (they share the rows of the query's cube, as K12's do)
constexpr int KNN_BLOCK = 64;  // one wave per workgroup: its lists are KNN_BLOCK x KCAP keys of LDS (32 KiB at KCAP = 64)
constexpr int KNN_UNROLL = 4;  // candidates per lane and round trip
constexpr int KNN_MAX_ROUNDS = 256;  // (a guard: doubling any float radius reaches +inf, hence the whole grid, sooner)

// The exact k nearest neighbours of a query over the uniform grid.
//
// Exactness.  After the cube of radius R has been walked, every indexed point with pair_dist <= R has been seen
// (grid_walk.h).  So if at least k of the points seen (the query's own index left out) have d <= R, the k smallest keys
// among THOSE are the k smallest of the whole cloud: every point not seen, and every point seen with d > R, is further
// than all of them.  Otherwise R doubles and the scan starts again; when the cube is the whole grid on all three axes
// every point of the cloud has been seen and whatever was found is final -- with fewer than k other finite points,
// all of them (k' = min(k, N - 1)).  A key is (distance bits << 32) | index: distances are non-negative floats, so the
// bit pattern orders like the value, and the index makes every key different, so "the k smallest keys" is one set.
//
// Shape.  Queries are taken in cell order, KNN_S adjacent lanes per query (the walk of grid_walk.h).  Each lane keeps
// the k smallest keys it has met in its own column of an LDS array (unsorted, with the largest remembered: a
// candidate is compared with one register, and only a candidate that enters costs a walk of the column).  At the end
// a key's rank among the keys of the query's KNN_S columns is counted directly -- the keys are different, so the ranks
// are a permutation -- and the k smallest distances go to their places in a second LDS array, from where one lane
// adds them in ascending order.
// The first radius is taken from the cell edge h and k: the grid is sized for `ppc` points per h x h of surface, so a
// ball of radius R holds about pi R^2 ppc / h^2 of them; r0_scale = 2.5 / (pi ppc) aims at 2.5 (k + 1).
template <int KCAP>
__global__ __launch_bounds__(KNN_BLOCK) void knn_mean_kernel(const KnnArgs a) {
  __shared__ nn_key_t list[KCAP][KNN_BLOCK];
  __shared__ unsigned sorted[KNN_BLOCK / KNN_S][KCAP];
  const int lane = threadIdx.x;
  const int slice = lane & (KNN_S - 1);
  const int grp = lane / KNN_S, g0 = grp * KNN_S;
  const int iq = (int)((blockIdx.x * (unsigned)KNN_BLOCK + threadIdx.x) / KNN_S);  // position in cell order
  const bool live = iq < a.nq;
  const float4 p4 = live ? a.q4[iq] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int self = __float_as_int(p4.w);
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const int k = a.k;  // <= KCAP (launch_knn_mean)
  // a non-finite query has no neighbours (and its cube would be the whole grid)
  const bool scan = live && finite3(px, py, pz);
  float R = g.h * __builtin_sqrtf((float)(k + 1) * a.r0_scale);
  bool active = scan;
  int cnt = 0;  // keys in this lane's column
  for (int round = 0; round < KNN_MAX_ROUNDS && __builtin_amdgcn_ballot_w64(active) != 0; ++round) {
    const Walk walk = make_walk(g, px, py, pz, R, active);
    const bool whole = walk.whole(g);
    int within = 0;  // candidates with d <= R met by this lane
    nn_key_t cur_max = 0;
    int max_at = 0;
    if (active) cnt = 0;
    walk_candidates<KNN_S, KNN_UNROLL>(
        walk, g, a.index.cell_start, slice, [&](int jj) { return a.index.t4[jj]; },
        [&](const float4 c, bool in_range) {
          const float d = pair_dist(px, py, pz, c.x, c.y, c.z);
          const int cj = __float_as_int(c.w);
          // a neighbour: a finite point other than the query itself, by index
          const bool nb = in_range && cj != self && finite3(c.x, c.y, c.z);
          const bool in = nb && d <= R;
          within += in;
          if (!(in || (nb && whole))) return;  // (beyond R nothing is final unless this is the whole cloud)
          const nn_key_t key = ((nn_key_t)__float_as_uint(d) << 32) | (unsigned)cj;
          if (cnt < k) {
            list[cnt][lane] = key;
            ++cnt;
          } else if (key < cur_max) {
            list[max_at][lane] = key;
          } else {
            return;
          }
          if (cnt == k) {  // the column is full: its largest key is the one a candidate has to beat
            cur_max = list[0][lane];
            max_at = 0;
            for (int e = 1; e < k; ++e) {
              const nn_key_t v = list[e][lane];
              if (v > cur_max) cur_max = v, max_at = e;
            }
          }
        });
#pragma unroll
    for (int m = 1; m < KNN_S; m <<= 1) within += __shfl_xor(within, m, 64);
    if (active) {
      if (within >= k || whole) active = false;  // the columns hold the k smallest keys (or all there are)
      else R *= 2.f;
    }
  }
  // (a query the guard stopped keeps what its last round found; no float radius gets there)
  __syncthreads();
  if (!scan) cnt = 0;
  int cs[KNN_S], total = 0;
#pragma unroll
  for (int s = 0; s < KNN_S; ++s) {
    cs[s] = __shfl(cnt, g0 + s, 64);
    total += cs[s];
  }
  for (int e = 0; e < cnt; ++e) {
    const nn_key_t key = list[e][lane];
    int rank = 0;
#pragma unroll
    for (int s = 0; s < KNN_S; ++s)
      for (int f = 0; f < cs[s]; ++f) rank += list[f][g0 + s] < key;
    if (rank < k) sorted[grp][rank] = (unsigned)(key >> 32);
  }
  __syncthreads();
  if (!live || slice != 0) return;
  const int kp = total < k ? total : k;  // k' = min(k, N - 1)
  double D = 0.0;
  for (int r = 0; r < kp; ++r) D += (double)__uint_as_float(sorted[grp][r]);
  a.mean[self] = kp > 0 ? D / (double)kp : 0.0;
  a.kth[self] = kp > 0 ? __uint_as_float(sorted[grp][kp - 1]) : 0.f;
}

// ---- RADIUS: K12's neighbourhood, counted -----------------------------------------------------------------------
constexpr int RAD_S = 8;  // lanes per point, as kernels_normals.hip
constexpr int RAD_BLOCK = 256;
constexpr int RAD_UNROLL = 4;

__global__ __launch_bounds__(RAD_BLOCK) void radius_count_kernel(const float4* __restrict__ t4,
                                                                 const int* __restrict__ cell_start,
                                                                 const GridInfo* __restrict__ gi, int n, float r,
                                                                 double* __restrict__ value) {
  const int slice = threadIdx.x & (RAD_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)RAD_BLOCK + threadIdx.x) / RAD_S);  // position in cell order
  const bool live = ip < n;
  const float4 p4 = live ? t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const GridInfo g = *gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const bool scan = live && finite3(px, py, pz);
  const Walk walk = make_walk(g, px, py, pz, r, scan);
  int m = 0;
  walk_candidates<RAD_S, RAD_UNROLL>(
      walk, g, cell_start, slice, [&](int jj) { return t4[jj]; },
      [&](const float4 c, bool in_range) {  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
        m += in_range && pair_dist(px, py, pz, c.x, c.y, c.z) <= r;
      });
#pragma unroll
  for (int s = 1; s < RAD_S; s <<= 1) m += __shfl_xor(m, s, 64);
  if (live && slice == 0) value[__float_as_int(p4.w)] = (double)m;
}

// ---- the canonical tree over mean_i and mean_i^2 (pair_reduce.h's epilogue with two sums) -----------------------
__global__ __launch_bounds__(RED_THREADS) void filter_sums_kernel(const FilterArgs a) {
  const int P = gridDim.x * RED_THREADS;
  double v[2] = {0.0, 0.0};
  int cnt = 0;
  for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < a.n; i += P) {
    const bool fin = finite3(a.x[i], a.y[i], a.z[i]);
    const double m = fin ? a.value[i] : 0.0;  // (a dropped point adds +0.0 at its index)
    v[0] += m;
    v[1] += m * m;
    cnt += fin;
  }
  block_partials<2>(v, cnt, a.partial + blockIdx.x, RED_MAX_BLOCKS, a.pcount + blockIdx.x);
}

// stage 2: slot b = the sums of block b, +0.0 beyond nblocks, one slot per lane; lane 0 goes on to the threshold
__global__ __launch_bounds__(RED_THREADS) void filter_threshold_kernel(const FilterArgs a, int nblocks) {
  const int tid = threadIdx.x;
  const double v[2] = {tid < nblocks ? a.partial[tid] : 0.0, tid < nblocks ? a.partial[RED_MAX_BLOCKS + tid] : 0.0};
  const BlockTotals<2> t = block_tree<2>(v, tid < nblocks ? a.pcount[tid] : 0);
  if (tid != 0) return;
  const double S1 = t.sum(0), S2 = t.sum(1);
  const int N = (int)t.count();
  const double Nd = (double)N;
  const double mu = N > 0 ? S1 / Nd : 0.0;
  double var = N >= 2 ? (S2 - S1 * S1 / Nd) / (Nd - 1.0) : 0.0;
  var = var > 0.0 ? var : 0.0;  // (NaN: 0)
  const double sigma = __builtin_sqrt(var);
  a.summary[0] = Nd;
  a.summary[1] = mu;
  a.summary[2] = sigma;
  a.summary[3] = mu + (double)a.std_ratio * sigma;
}

// ---- order-preserving compaction (count per block, scan, emit by rank: block_scan.h) -----------------------------
__device__ __forceinline__ bool filter_keeps(const FilterArgs& a, int i, double T, bool* dropped) {
  const bool fin = finite3(a.x[i], a.y[i], a.z[i]);
  *dropped = !fin;
  const double v = a.value[i];
  return fin && (a.kind == 0 ? v <= T : v >= (double)a.min_neighbors);
}

// out_index[i] := keep flag; bsum[block] := kept among the block's 1024 points; counts[1] += dropped
__global__ __launch_bounds__(256) void filter_flag_kernel(const FilterArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  const double T = a.kind == 0 ? a.summary[3] : 0.0;
  int mine = 0, gone = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    bool dropped;
    const bool keep = filter_keeps(a, i, T, &dropped);
    a.out_index[i] = keep ? 1 : 0;
    mine += keep;
    gone += dropped;
  }
  const int total = block_total<256>(mine);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
  if (gone) atomicAdd(&a.counts[1], gone);  // (an integer count: the order of arrival does not show)
}

// bsum[nb] -> its exclusive scan in place; counts[0] := the total
__global__ __launch_bounds__(256) void filter_scan_kernel(int* __restrict__ bsum, int nb, int* __restrict__ counts) {
  const int total = scan_rounds<256>(bsum, bsum, nb);
  if (threadIdx.x == 0) counts[0] = total;
}

__global__ __launch_bounds__(256) void filter_emit_kernel(const FilterArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int keep[4];
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    keep[k] = i < a.n ? a.out_index[i] : 0;
    mine += keep[k];
  }
  int total;
  int pos = a.bsum[blockIdx.x] + block_excl_scan<256>(mine, &total);
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    if (!keep[k]) {
      a.out_index[i] = -1;
      continue;
    }
    const int o = pos++;  // o <= i < n
    a.out_index[i] = o;
    a.ox[o] = a.x[i], a.oy[o] = a.y[i], a.oz[o] = a.z[i];
    if (a.nx) a.onx[o] = a.nx[i], a.ony[o] = a.ny[i], a.onz[o] = a.nz[i];
  }
}

}  // namespace

void launch_knn_mean(const KnnArgs& a, hipStream_t s) {
  if (a.nq <= 0 || a.k < 1 || a.k > FILTER_MAX_K) return;
  const unsigned blocks = (unsigned)(((size_t)a.nq * KNN_S + KNN_BLOCK - 1) / KNN_BLOCK);
  // the columns' capacity: the next of 8, 16, 32, 64 (LDS per workgroup 4.5, 9, 18, 36 KiB)
  if (a.k <= 8)
    hipLaunchKernelGGL(knn_mean_kernel<8>, dim3(blocks), dim3(KNN_BLOCK), 0, s, a);
  else if (a.k <= 16)
    hipLaunchKernelGGL(knn_mean_kernel<16>, dim3(blocks), dim3(KNN_BLOCK), 0, s, a);
  else if (a.k <= 32)
    hipLaunchKernelGGL(knn_mean_kernel<32>, dim3(blocks), dim3(KNN_BLOCK), 0, s, a);
  else
    hipLaunchKernelGGL(knn_mean_kernel<64>, dim3(blocks), dim3(KNN_BLOCK), 0, s, a);
}

void launch_radius_count(const GridView& index, int n, float radius, double* value, hipStream_t s) {
  if (n <= 0) return;
  const unsigned blocks = (unsigned)(((size_t)n * RAD_S + RAD_BLOCK - 1) / RAD_BLOCK);
  hipLaunchKernelGGL(radius_count_kernel, dim3(blocks), dim3(RAD_BLOCK), 0, s, index.t4, index.cell_start, index.gi, n,
                     radius, value);
}

void launch_filter_compact(const FilterArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  if (a.kind == 0) {
    const int nblocks = red_blocks(a.n);
    hipLaunchKernelGGL(filter_sums_kernel, dim3(nblocks), dim3(RED_THREADS), 0, s, a);
    hipLaunchKernelGGL(filter_threshold_kernel, dim3(1), dim3(RED_THREADS), 0, s, a, nblocks);
  }
  const int nb = (a.n + 1023) / 1024;
  hipLaunchKernelGGL(filter_flag_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts);
  hipLaunchKernelGGL(filter_emit_kernel, dim3(nb), dim3(256), 0, s, a);
}

}  // namespace icpk
