// kernels_cluster.hip -- K33: DBSCAN clustering of one of the context's clouds (icpk_cluster_dbscan; THE CLUSTER RULE is
// spelled out in include/icpk.h, its shared parts are cluster_rule.h, tests/cluster_model.py restates it).
//
//   1. cluster_count_kernel    m_i over K1d's index of the cloud (K13's radius_count_kernel, written out again so that
//                              kernels_filter.hip generates the code it generates today): count, core, parent[i] = i or -1
//   2. cluster_link_kernel     the same walk again, the hot path: a core point unites itself with every core neighbour of
//                              lower index in a lock-free union-find over parent[] (-1 for a point that is not core); a
//                              finite non-core point takes the least (distance bits, index) key among its core neighbours
//   3. cluster_flatten_kernel  in a launch of its own: every point's root (a border point's is its partner's), the
//                              representatives (core, root == itself) counted per 1024 points; cluster_scan_kernel;
//      cluster_rank_kernel     a representative's rank is its cluster's id: cid, first, sizes := 0
//      cluster_label_kernel    labels, and the sizes by one integer atomicAdd per (wave, label)
//   4. cluster_largest_kernel  (largest_only) one workgroup: the greatest (size, ~label) key
//   5. cluster_flag_kernel / cluster_scan_kernel / cluster_emit_kernel   K13's order-preserving compaction over the
//                              selection predicate
// No atomic on a float anywhere; every atomic is an integer CAS, min or add whose result does not show the order of
// arrival (see the invariants in front of cl_unite).
#include "block_scan.h"
#include "cluster_rule.h"
#include "grid_walk.h"
#include "icpk_internal.h"

namespace icpk {

namespace {

constexpr int CL_S = 8;  // lanes per point, as K12's and K13's radius walk
constexpr int CL_BLOCK = 256;
constexpr int CL_UNROLL = 4;

__global__ __launch_bounds__(CL_BLOCK) void cluster_count_kernel(const ClusterArgs a) {
  const int slice = threadIdx.x & (CL_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)CL_BLOCK + threadIdx.x) / CL_S);  // position in cell order
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const float eps = a.eps;
  const bool scan = live && cluster_finite3(px, py, pz);
  const Walk walk = make_walk(g, px, py, pz, eps, scan);
  int m = 0;
  walk_candidates<CL_S, CL_UNROLL>(
      walk, g, a.index.cell_start, slice, [&](int jj) { return a.index.t4[jj]; },
      [&](const float4 c, bool in_range) {  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
        m += in_range && cluster_dist(px, py, pz, c.x, c.y, c.z) <= eps;
      });
#pragma unroll
  for (int s = 1; s < CL_S; s <<= 1) m += __shfl_xor(m, s, 64);
  if (live && slice == 0) {
    const int i = __float_as_int(p4.w);  // 0 <= i < n: the index holds every point of the cloud once
    a.count[i] = m;
    const bool core = m >= a.min_points;
    a.core[i] = core ? 1 : 0;
    a.parent[i] = core ? i : -1;  // (the forest is over the core points: every other entry says so and stays as it is)
  }
}

// ---- the lock-free union-find over the core points ---------------------------------------------------------------
// Invariants, which hold at every moment of the link launch whatever the schedule:
//   (a) for a core point x, parent[x] <= x, and parent[x] only ever decreases: it starts at x; a hook stores a smaller
//       root into a root; a shortening is an atomic min.  So the forest has no cycle and cl_find descends strictly: at
//       most n steps.  (Any other point's entry is -1 from the count launch on, and nothing reads past it.)
//   (b) parent[x] always names a member of x's component (the hook's target is a point united with x; a shortening
//       stores an ancestor), so a STALE value of parent[x] still names one: no step depends on reading the latest
//       value, and correctness rests on the atomicity of the CAS alone.
//   (c) a point that stopped being a root never becomes one again (a), so the CAS on parent[r] expecting r succeeds
//       only while r is a root; the min never touches a root (it is applied where parent[x] != x was read).
//   (d) a hook puts the larger root under the smaller, so a tree's root is the smallest index in it; when the launch has
//       ended every edge has been united, and the root of a component is its smallest core index whatever the order of
//       arrival: the result is a function of the cloud although the schedule is not.
// Memory.  Every read of parent[] in the link launch is an agent-scope relaxed atomic load and every write an agent-scope
// atomic (CAS, min): nothing depends on a plain load seeing another workgroup's store within the launch.
// Termination.  Nothing waits for another thread.  cl_find and the retry of cl_unite carry a step bound (n + 1) that the
// invariants make unreachable -- find by (a); a failed CAS means the larger root was hooked by somebody else, and the
// next pair of roots has a smaller maximum --; passing it sets the error word (the host answers ICPK_E_HIP) and gives up.
__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x (-1: the bound was passed), halving the path on the way
__device__ __forceinline__ int cl_find(int* __restrict__ parent, int x, int bound, int* __restrict__ err) {
  for (int step = 0; step <= bound; ++step) {
    const int p = cl_load(parent + x);
    if (p == x) return x;
    if (p < 0) break;  // (x is no core point: no caller passes one)
    const int gp = cl_load(parent + p);  // 0 <= gp <= p < x: the parent of a core point is a core point
    if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
  __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return -1;
}

// unites the components of a and b; returns the root they share afterwards (a member of a's component at the least)
__device__ __forceinline__ int cl_unite(int* __restrict__ parent, int a, int b, int bound, int* __restrict__ err) {
  for (int step = 0; step <= bound; ++step) {
    const int ra = cl_find(parent, a, bound, err), rb = cl_find(parent, b, bound, err);
    if (ra < 0 || rb < 0) return a;
    if (ra == rb) return ra;
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    int seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    a = seen, b = lo;  // hi was hooked meanwhile: seen < hi is in its component
  }
  __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return a;
}

__global__ __launch_bounds__(CL_BLOCK) void cluster_link_kernel(const ClusterArgs a) {
  const int slice = threadIdx.x & (CL_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)CL_BLOCK + threadIdx.x) / CL_S);
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const float eps = a.eps;
  const int i = __float_as_int(p4.w);
  const bool scan = live && cluster_finite3(px, py, pz);
  const bool is_core = live && a.core[i] != 0;  // (written by the launch before: a plain load)
  const Walk walk = make_walk(g, px, py, pz, eps, scan);
  int* const err = a.counts + CL_ERROR;
  int mine = i;  // a member of i's component, as far down the tree as this lane knows
  unsigned long long best = CLUSTER_NO_KEY;
  // walk_candidates' round trip with one more stage: the CL_UNROLL candidates of a trip, THEN parent[] of those that are
  // neighbours -- independent loads, all in flight together -- and only then the unites, which are rare: a neighbour
  // whose parent is the root this lane already knows is joined to it already
  walk_rows<CL_S>(walk, g, a.index.cell_start, slice, [&](int s0, int s1) {
    for (int j0 = s0; j0 < s1; j0 += CL_UNROLL) {
      float4 c[CL_UNROLL];
#pragma unroll
      for (int u = 0; u < CL_UNROLL; ++u) c[u] = a.index.t4[min(j0 + u, s1 - 1)];
      float d[CL_UNROLL];
      int pj[CL_UNROLL];
#pragma unroll
      for (int u = 0; u < CL_UNROLL; ++u) {
        d[u] = cluster_dist(px, py, pz, c[u].x, c[u].y, c[u].z);
        const int j = __float_as_int(c[u].w);
        // (a core point acts on the edges to lower indices: each is met from both ends)
        const bool near = j0 + u < s1 && d[u] <= eps && (!is_core || j < i);
        pj[u] = near ? cl_load(a.parent + j) : -1;  // >= 0: j is a core point, and pj a member of its component (b)
      }
#pragma unroll
      for (int u = 0; u < CL_UNROLL; ++u) {
        if (pj[u] < 0) continue;
        if (is_core) {
          if (pj[u] != mine) mine = cl_unite(a.parent, mine, pj[u], a.n, err);
        } else {
          const unsigned long long key = cluster_key(d[u], __float_as_int(c[u].w));
          best = key < best ? key : best;
        }
      }
    }
  });
#pragma unroll
  for (int s = 1; s < CL_S; s <<= 1) {
    const unsigned long long o = __shfl_xor(best, s, 64);
    best = o < best ? o : best;
  }
  if (live && slice == 0) a.nearest[i] = is_core ? i : best == CLUSTER_NO_KEY ? -1 : (int)(unsigned)best;
}

// ---- roots, representatives, labels (launches of their own: plain loads are valid again) -------------------------
__device__ __forceinline__ int cl_find_plain(const int* __restrict__ parent, int x, int bound, int* __restrict__ err) {
  for (int step = 0; step <= bound; ++step) {
    const int p = parent[x];
    if (p == x) return x;
    if (p < 0) break;  // (x is no core point: no caller passes one)
    x = p;
  }
  *err = 3;
  return -1;
}

// labels[i] := the root of i's cluster (-1: noise); bsum[block] := representatives among the block's 1024 points;
// counts[CL_N_NOISE] += noise, counts[CL_N_DROPPED] += non-finite
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const ClusterArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int mine = 0, noise = 0, gone = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    const bool core = a.core[i] != 0;
    const int nc = a.nearest[i];  // i, the partner (a core point), or -1
    const int r = nc >= 0 ? cl_find_plain(a.parent, nc, a.n, a.counts + CL_ERROR) : -1;
    a.labels[i] = r;
    mine += core && r == i;
    noise += r < 0;
    gone += !cluster_finite3(a.x[i], a.y[i], a.z[i]);
  }
  const int total = block_total<256>(mine);
  const int block_noise = block_total<256>(noise), block_gone = block_total<256>(gone);
  if (threadIdx.x != 0) return;
  a.bsum[blockIdx.x] = total;
  if (block_noise) atomicAdd(&a.counts[CL_N_NOISE], block_noise);  // (one add per block; integer counts: the order of
  if (block_gone) atomicAdd(&a.counts[CL_N_DROPPED], block_gone);  //  arrival does not show)
}

// bsum[nb] -> its exclusive scan in place; *total_out := the total
__global__ __launch_bounds__(256) void cluster_scan_kernel(int* __restrict__ bsum, int nb, int* __restrict__ total_out) {
  const int total = scan_rounds<256>(bsum, bsum, nb);
  if (threadIdx.x == 0) *total_out = total;
}

// the cluster id is the rank of the representative: clusters are numbered by ascending representative
__global__ __launch_bounds__(256) void cluster_rank_kernel(const ClusterArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int rep[4];
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    rep[k] = i < a.n && a.core[i] != 0 && a.labels[i] == i;
    mine += rep[k];
  }
  int total;
  int pos = a.bsum[blockIdx.x] + block_excl_scan<256>(mine, &total);
  for (int k = 0; k < 4; ++k) {
    if (!rep[k]) continue;
    const int id = pos++;  // id <= i < n
    a.cid[i0 + k] = id;
    a.first[id] = i0 + k;
    a.sizes[id] = 0;
  }
}

// labels[i]: root -> cluster id; sizes[id] += members, one add per (wave, label)
__global__ __launch_bounds__(256) void cluster_label_kernel(const ClusterArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int lab = -1;
  if (i < a.n) {
    const int r = a.labels[i];  // a representative: 0 <= r < n, cid[r] written by the launch before
    lab = r >= 0 ? a.cid[r] : -1;
    if ((unsigned)lab >= (unsigned)a.counts[CL_N_CLUSTERS]) lab = -1;  // (only after a passed bound: sizes[] stays in range)
    a.labels[i] = lab;
  }
  bool todo = lab >= 0;
  for (int round = 0; round < 64; ++round) {  // (every round retires its leader's label: at most 64)
    const unsigned long long open = __builtin_amdgcn_ballot_w64(todo);
    if (open == 0) break;
    const int leader = __builtin_ctzll(open);
    const int L = __shfl(lab, leader, 64);
    const bool same = todo && lab == L;
    const unsigned long long members = __builtin_amdgcn_ballot_w64(same);
    if (lane == leader) atomicAdd(&a.sizes[L], __builtin_popcountll(members));
    todo = todo && !same;
  }
}

// one workgroup: counts[CL_LARGEST] := the label of the greatest (size, ~label) key, -1 without a cluster
__global__ __launch_bounds__(256) void cluster_largest_kernel(const ClusterArgs a) {
  __shared__ unsigned long long wbest[4];
  const int nc = a.counts[CL_N_CLUSTERS];
  unsigned long long best = 0;  // (a cluster has at least one member: its key is above 2^32)
  for (int c = threadIdx.x; c < nc; c += 256) {
    const unsigned long long key = cluster_size_key(a.sizes[c], c);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
  a.counts[CL_LARGEST] = best == 0 ? -1 : (int)~(unsigned)best;
}

// ---- the selection: K13's order-preserving compaction (count per block, scan, emit by rank: block_scan.h) ---------
// out_index[i] := keep flag; bsum[block] := kept among the block's 1024 points
__global__ __launch_bounds__(256) void cluster_flag_kernel(const ClusterArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  const int largest = a.largest_only ? a.counts[CL_LARGEST] : -1;
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    const int lab = a.labels[i];
    const bool keep = cluster_keeps(lab, lab >= 0 ? a.sizes[lab] : 0, a.min_size, a.max_size, a.largest_only, largest);
    a.out_index[i] = keep ? 1 : 0;
    mine += keep;
  }
  const int total = block_total<256>(mine);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void cluster_emit_kernel(const ClusterArgs a) {
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

void launch_cluster_dbscan(const ClusterArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const unsigned walk_blocks = (unsigned)(((size_t)a.n * CL_S + CL_BLOCK - 1) / CL_BLOCK);
  const int nb = (a.n + 1023) / 1024;
  hipLaunchKernelGGL(cluster_count_kernel, dim3(walk_blocks), dim3(CL_BLOCK), 0, s, a);
  hipLaunchKernelGGL(cluster_link_kernel, dim3(walk_blocks), dim3(CL_BLOCK), 0, s, a);
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts + CL_N_CLUSTERS);
  hipLaunchKernelGGL(cluster_rank_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cluster_label_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
  if (a.largest_only) hipLaunchKernelGGL(cluster_largest_kernel, dim3(1), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cluster_flag_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts + CL_N_OUT);
  hipLaunchKernelGGL(cluster_emit_kernel, dim3(nb), dim3(256), 0, s, a);
}

}  // namespace icpk
