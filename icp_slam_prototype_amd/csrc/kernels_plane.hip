// kernels_plane.hip -- K34: RANSAC plane segmentation of one of the context's clouds (icpk_segment_planes; THE PLANE RULE
// is spelled out in include/icpk.h, stated once in plane_rule.h and restated by tests/plane_model.py).  One round:
//
//   1. plane_list_flag_kernel / plane_scan_kernel / plane_list_emit_kernel   E, the finite points still labelled -1, in
//                              index order as (x, y, z, index bits): block_scan.h's count / scan / emit
//   2. plane_hypotheses_kernel one thread per hypothesis: the draws, the three samples, (a, N, G, valid); count[h] := 0
//   3. plane_score_kernel      the hot path, (points of E) x (hypotheses): a workgroup keeps 256 x PL_PTS points in
//                              registers as doubles and walks a chunk of PL_HCHUNK hypotheses, each read at a
//                              wave-uniform address; per test a ballot and a population count, the wave's count in a
//                              scalar until the hypothesis is done, one integer add per (wave, hypothesis) into LDS and
//                              one per (workgroup, hypothesis) into count[h]
//   4. plane_pick_kernel       one workgroup: the greatest (count << 32) | ~h over the valid h
//   5. plane_moments_kernel    the nine sums of the winner's inliers through the canonical tree over all n points
//      plane_fit_kernel        stage 2 of the tree, then plane_fit on one lane: the plane's record
//   6. plane_final_kernel      the final inliers of E counted (one integer add per workgroup)
//      plane_label_kernel      ... and labelled, if there are min_inliers of them
// and after the last round plane_select_flag_kernel / plane_scan_kernel / plane_select_emit_kernel, K13's order-preserving
// compaction over the selection.  Counts are integers and nothing else is added atomically, so the schedule does not
// show; every loop is bounded and nothing waits on another workgroup.
#include "block_scan.h"
#include "icpk_internal.h"
#include "pair_reduce.h"
#include "plane_rule.h"

namespace icpk {

namespace {

constexpr int PL_PTS = 4;      // points of E a lane of the score launch holds
constexpr int PL_HCHUNK = 64;  // hypotheses a score workgroup walks
constexpr int PL_TILE = 256 * PL_PTS;

// ---- membership ---------------------------------------------------------------------------------------------------
// E of the round: finite and not yet on a plane
__device__ __forceinline__ bool plane_open(const PlaneArgs& a, int i) {
  return a.labels[i] < 0 && plane_finite3(a.x[i], a.y[i], a.z[i]);
}
// the selection: what is left over, or the points of the planes (of one plane)
__device__ __forceinline__ bool plane_selected(const PlaneArgs& a, int i) {
  const int lab = a.labels[i];
  if (a.keep_inliers) return lab >= 0 && (a.select_plane < 0 || lab == a.select_plane);
  return lab < 0 && plane_finite3(a.x[i], a.y[i], a.z[i]);
}

template <bool SELECT>
__device__ __forceinline__ void flag_block(const PlaneArgs& a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= a.n) break;
    mine += SELECT ? plane_selected(a, i) : plane_open(a, i);
  }
  const int total = block_total<256>(mine);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void plane_list_flag_kernel(const PlaneArgs a) { flag_block<false>(a); }
__global__ __launch_bounds__(256) void plane_select_flag_kernel(const PlaneArgs a) { flag_block<true>(a); }

// bsum[nb] -> its exclusive scan in place; *total_out := the total
__global__ __launch_bounds__(256) void plane_scan_kernel(int* __restrict__ bsum, int nb, int* __restrict__ total_out) {
  const int total = scan_rounds<256>(bsum, bsum, nb);
  if (threadIdx.x == 0) *total_out = total;
}

// E[rank] := (x, y, z, index bits) of every open point
__global__ __launch_bounds__(256) void plane_list_emit_kernel(const PlaneArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int keep[4];
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    keep[k] = i < a.n && plane_open(a, i);
    mine += keep[k];
  }
  int total;
  int pos = a.bsum[blockIdx.x] + block_excl_scan<256>(mine, &total);
  for (int k = 0; k < 4; ++k) {
    if (!keep[k]) continue;
    const int i = i0 + k;
    a.E[pos++] = make_float4(a.x[i], a.y[i], a.z[i], __int_as_float(i));  // pos <= i < n
  }
}

// out_index and the selected cloud
__global__ __launch_bounds__(256) void plane_select_emit_kernel(const PlaneArgs a) {
  const int i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  int keep[4];
  int mine = 0;
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    keep[k] = i < a.n && plane_selected(a, i);
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

// ---- hypotheses -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plane_hypotheses_kernel(const PlaneArgs a) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= a.H) return;
  const int m = a.counts[PL_M];  // 0 <= m <= n
  PlaneHyp hyp = {};
  int idx[3] = {-1, -1, -1};
  uint32_t c[3];
  // (a round that ends the call has no valid hypothesis: the pick finds no winner)
  if (m >= 3 && m >= a.min_inliers && plane_sample(a.seed, (uint64_t)a.round * (uint64_t)a.H + (uint64_t)h, (uint32_t)m, c)) {
    float p[3][3];
    for (int k = 0; k < 3; ++k) {
      const float4 e = a.E[c[k]];  // c[k] < m
      p[k][0] = e.x, p[k][1] = e.y, p[k][2] = e.z;
      idx[k] = __float_as_int(e.w);
    }
    hyp = plane_hypothesis(p[0], p[1], p[2], a.t);
  }
  a.hyp[h] = hyp;
  for (int k = 0; k < 3; ++k) a.hyp_idx[3 * h + k] = idx[k];
  a.hcount[h] = 0;
}

// ---- the count --------------------------------------------------------------------------------------------------------
// grid (tiles of E, chunks of hypotheses).  The tile's points stay in registers; a hypothesis is read once per wave at a
// uniform address (scalar loads), and its count leaves the wave as one LDS add
__global__ __launch_bounds__(256) void plane_score_kernel(const PlaneArgs a) {
  __shared__ int lc[PL_HCHUNK];
  const int m = a.counts[PL_M];
  const int base = blockIdx.x * PL_TILE;
  if (base >= m) return;  // (the whole workgroup: the grid is sized by the host's bound on m)
  const int tid = threadIdx.x;
  double px[PL_PTS], py[PL_PTS], pz[PL_PTS];
  bool live[PL_PTS];
#pragma unroll
  for (int k = 0; k < PL_PTS; ++k) {
    const int j = base + k * 256 + tid;
    live[k] = j < m;
    const float4 e = live[k] ? a.E[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    px[k] = (double)e.x, py[k] = (double)e.y, pz[k] = (double)e.z;
  }
  if (tid < PL_HCHUNK) lc[tid] = 0;
  __syncthreads();
  const int h0 = blockIdx.y * PL_HCHUNK;
  const int h1 = min(a.H, h0 + PL_HCHUNK);
  const PlaneHyp* __restrict__ hyp = a.hyp;
  for (int h = h0; h < h1; ++h) {
    if (!hyp[h].valid) continue;  // (uniform)
    const double a0 = hyp[h].a[0], a1 = hyp[h].a[1], a2 = hyp[h].a[2];
    const double N0 = hyp[h].N[0], N1 = hyp[h].N[1], N2 = hyp[h].N[2];
    const double G = hyp[h].G;
    int c = 0;
#pragma unroll
    for (int k = 0; k < PL_PTS; ++k) {
      // plane_hyp_inlier, written out over the registers
      const double e0 = px[k] - a0, e1 = py[k] - a1, e2 = pz[k] - a2;
      const double s = (N0 * e0 + N1 * e1) + N2 * e2;
      c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(live[k] && s * s <= G));
    }
    if ((tid & 63) == 0 && c) atomicAdd(&lc[h - h0], c);
  }
  __syncthreads();
  if (tid < h1 - h0 && lc[tid]) atomicAdd(&a.hcount[h0 + tid], lc[tid]);
}

// one workgroup: counts[PL_WINNER] := the valid h of the greatest count, ties to the lowest h (-1: none, or a count
// below 3); counts[PL_RANSAC] := its count
__global__ __launch_bounds__(256) void plane_pick_kernel(const PlaneArgs a) {
  __shared__ unsigned long long wbest[4];
  unsigned long long best = 0;  // (~h != 0 for h < 2^32 - 1: a valid hypothesis' key is never 0)
  for (int h = threadIdx.x; h < a.H; h += 256) {
    if (!a.hyp[h].valid) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)a.hcount[h] << 32) | (unsigned)~h;
    best = key > best ? key : best;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(best, s, 64);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
  const int cnt = (int)(best >> 32);
  a.counts[PL_WINNER] = best != 0 && cnt >= 3 ? (int)~(unsigned)best : -1;
  a.counts[PL_RANSAC] = cnt;
}

// ---- the refit --------------------------------------------------------------------------------------------------------
// red_blocks(n) workgroups: the per-block partials of the nine sums over the winner's inliers, every point of the cloud
// at its index (a point that is no inlier adds nothing)
__global__ __launch_bounds__(RED_THREADS) void plane_moments_kernel(const PlaneArgs a) {
  const int w = a.counts[PL_WINNER];
  if (w < 0) return;  // (uniform)
  const PlaneHyp hyp = a.hyp[w];
  const int P = gridDim.x * RED_THREADS;
  double v[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) v[s] = 0.0;
  int cnt = 0;
  for (int i = blockIdx.x * RED_THREADS + threadIdx.x; i < a.n; i += P) {
    if (!plane_open(a, i)) continue;
    double e[3];
    if (!plane_hyp_inlier(hyp.a, hyp.N, hyp.G, a.x[i], a.y[i], a.z[i], e)) continue;
    v[0] += e[0], v[1] += e[1], v[2] += e[2];
    v[3] += e[0] * e[0], v[4] += e[0] * e[1], v[5] += e[0] * e[2];
    v[6] += e[1] * e[1], v[7] += e[1] * e[2];
    v[8] += e[2] * e[2];
    ++cnt;
  }
  block_partials<9>(v, cnt, a.partial + blockIdx.x, RED_MAX_BLOCKS, a.pcount + blockIdx.x);
}

// one workgroup: stage 2 of the canonical tree (slot b = the sums of block b, +0.0 beyond nblocks), then the fit on one
// lane; the plane's record goes to slot `round`
__global__ __launch_bounds__(RED_THREADS) void plane_fit_kernel(const PlaneArgs a, int nblocks) {
  const int w = a.counts[PL_WINNER];
  if (w < 0) return;  // (uniform)
  const int tid = threadIdx.x;
  double v[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) v[s] = tid < nblocks ? a.partial[s * RED_MAX_BLOCKS + tid] : 0.0;
  int cnt = tid < nblocks ? a.pcount[tid] : 0;
  const BlockTotals<9> t = block_tree<9>(v, cnt);
  if (tid != 0) return;
  double S[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) S[s] = t.sum(s);
  const int count = (int)t.count();
  const PlaneHyp hyp = a.hyp[w];
  const float a3[3] = {(float)hyp.a[0], (float)hyp.a[1], (float)hyp.a[2]};  // (widened floats: the way back is exact)
  double model[8];
  a.counts[PL_FIT] = plane_fit(S, count, a3, hyp.N, model);
  const int r = a.round;
  for (int k = 0; k < 8; ++k) a.model[8 * r + k] = model[k];
  for (int k = 0; k < 9; ++k) a.sums[9 * r + k] = S[k];
  a.info[6 * r + 0] = w;
  for (int k = 0; k < 3; ++k) a.info[6 * r + 1 + k] = a.hyp_idx[3 * w + k];
  a.info[6 * r + 4] = count;
  a.info[6 * r + 5] = 0;  // (the final count: plane_label_kernel)
}

// ---- the final inliers ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool plane_final_of(const PlaneArgs& a, int m, int j, int* i) {
  if (j >= m) return false;
  const float4 e = a.E[j];
  *i = __float_as_int(e.w);
  double model[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) model[k] = a.model[8 * a.round + k];  // (uniform)
  return plane_final_inlier(model, e.x, e.y, e.z, a.t);
}

__global__ __launch_bounds__(256) void plane_final_kernel(const PlaneArgs a) {
  if (a.counts[PL_WINNER] < 0) return;  // (uniform)
  const int m = a.counts[PL_M];
  int i;
  const int in = plane_final_of(a, m, blockIdx.x * 256 + threadIdx.x, &i);
  const int total = block_total<256>(in);
  if (threadIdx.x == 0 && total) atomicAdd(&a.counts[PL_FINAL], total);  // (an integer: the order of arrival does not show)
}

__global__ __launch_bounds__(256) void plane_label_kernel(const PlaneArgs a) {
  const int final_count = a.counts[PL_FINAL];  // (complete: written by the launch before)
  if (a.counts[PL_WINNER] < 0 || final_count < a.min_inliers) return;  // the round writes nothing
  const int m = a.counts[PL_M];
  int i = 0;
  if (plane_final_of(a, m, blockIdx.x * 256 + threadIdx.x, &i)) a.labels[i] = a.round;  // 0 <= i < n: E holds indices of the cloud
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.counts[PL_ACCEPTED] = 1;
    a.info[6 * a.round + 5] = final_count;
  }
}

}  // namespace

void launch_plane_round(const PlaneArgs& a, hipStream_t s) {
  if (a.n <= 0 || a.H <= 0) return;
  const int nb = (a.n + 1023) / 1024;
  const int bound = a.m_bound < 1 ? 1 : a.m_bound;  // (|E| <= m_bound: the host knows it from the rounds before)
  hipLaunchKernelGGL(plane_list_flag_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(plane_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts + PL_M);
  hipLaunchKernelGGL(plane_list_emit_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(plane_hypotheses_kernel, dim3((a.H + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(plane_score_kernel, dim3((bound + PL_TILE - 1) / PL_TILE, (a.H + PL_HCHUNK - 1) / PL_HCHUNK), dim3(256), 0,
                     s, a);
  hipLaunchKernelGGL(plane_pick_kernel, dim3(1), dim3(256), 0, s, a);
  const int B = red_blocks(a.n);
  hipLaunchKernelGGL(plane_moments_kernel, dim3(B), dim3(RED_THREADS), 0, s, a);
  hipLaunchKernelGGL(plane_fit_kernel, dim3(1), dim3(RED_THREADS), 0, s, a, B);
  hipLaunchKernelGGL(plane_final_kernel, dim3((bound + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(plane_label_kernel, dim3((bound + 255) / 256), dim3(256), 0, s, a);
}

void launch_plane_select(const PlaneArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const int nb = (a.n + 1023) / 1024;
  hipLaunchKernelGGL(plane_select_flag_kernel, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(plane_scan_kernel, dim3(1), dim3(256), 0, s, a.bsum, nb, a.counts + PL_N_OUT);
  hipLaunchKernelGGL(plane_select_emit_kernel, dim3(nb), dim3(256), 0, s, a);
}

}  // namespace icpk
