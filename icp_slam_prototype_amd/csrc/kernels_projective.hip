// kernels_projective.hip -- K25: projective frame-to-model alignment (include/icpk.h, THE PROJECTIVE RULE).
//
// One iteration is two launches.  proj_reduce_kernel walks the pixels of a pyramid level in the canonical geometry
// (red_blocks(npix) workgroups of RED_THREADS, thread g takes pixels g, g + 256 B, ...): each pixel is back-projected,
// moved by the state's pose, projected into the ray-cast view and paired with the view pixel it lands on
// (projective_rule.h); an accepted pair adds K5's 28 terms to the lane's double accumulators, which end in
// block_partials.  Neighbouring source pixels land on neighbouring view pixels, so the seven gathers at j are nearly
// coalesced.  proj_step_kernel, one workgroup, sums the partials through the same tree and runs the loop rule of
// iteration k on one lane: trace entry, exit tests, solve_p2l, E' = dT E.  Nothing is moved and nothing is listed; no
// atomic, and no word travels between workgroups of one launch.  Once the state says done both launches return at once.
#include "icpk.h"
#include "icpk_internal.h"
#include "pair_reduce.h"
#include "projective_rule.h"
#include "solve_impl.h"

namespace icpk {

namespace {

__device__ __forceinline__ ProjView proj_view(const ProjArgs& a) {
  const size_t n = (size_t)a.rows_v * a.cols_v;
  ProjView vw;
  vw.x = a.maps, vw.y = a.maps + n, vw.z = a.maps + 2 * n;
  vw.nx = a.maps + 3 * n, vw.ny = a.maps + 4 * n, vw.nz = a.maps + 5 * n, vw.depth = a.maps + 6 * n;
  vw.rows = a.rows_v, vw.cols = a.cols_v, vw.fx = a.fx_v, vw.cx = a.cx_v;
#pragma unroll
  for (int k = 0; k < 9; ++k) vw.Q[k] = a.Q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) vw.s[k] = a.s[k];
  return vw;
}

__device__ __forceinline__ ProjPose proj_pose(const ProjState* __restrict__ st) {
  ProjPose E;
#pragma unroll
  for (int k = 0; k < 9; ++k) E.R[k] = st->R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) E.t[k] = st->t[k];
  return E;
}

}  // namespace

// WITH_NORMAL: rule 8 is on (four more depth loads per paired pixel); the default path is compiled without it.
// COLORED (K26): rule 9 is K17's joint step -- one more coalesced float per pixel (the level's intensity, prefetched
// with the depth) and four more gathers per pair (the view's intensity and its three gradient planes at j).
template <bool WITH_NORMAL, bool COLORED>
__global__ __launch_bounds__(RED_THREADS) void proj_reduce_kernel(const ProjArgs a) {
  if (a.st->done) return;  // (uniform)
  const int npix = a.rows * a.cols;
  const int P = (int)gridDim.x * RED_THREADS;
  int i = (int)blockIdx.x * RED_THREADS + (int)threadIdx.x;
  // a lane's first depth is asked for before the pose is read: two cold round trips side by side
  uint16_t d_next = i < npix ? a.depth[i] : (uint16_t)0;
  float I_next = COLORED && i < npix ? a.inten[i] : 0.f;
  const size_t nv = (size_t)a.rows_v * a.cols_v;
  const double lg = (double)a.lambda_geometric, lc = 1.0 - lg;
  const ProjLevel lv{a.depth, a.rows, a.cols, a.fx, a.cx};
  const ProjView vw = proj_view(a);
  const ProjPose E = proj_pose(a.st);
  const ProjGate g{a.max_dist, a.min_normal_cos};
  double v[NP2L];
#pragma unroll
  for (int s = 0; s < NP2L; ++s) v[s] = 0.0;
  int cnt = 0;
  for (; i < npix; i += P) {
    const uint16_t d = d_next;
    const float Is = I_next;
    if (i + P < npix) {  // the NEXT pixel is on its way while this one is consumed
      d_next = a.depth[i + P];
      if (COLORED) I_next = a.inten[i + P];
    }
    const int r = i / a.cols, c = i - r * a.cols;
    ProjPair pr;
    const int j = proj_pixel<WITH_NORMAL>(lv, vw, E, g, r, c, d, &pr);
    if (j >= 0) {
      if (COLORED) {
        const ProjColor pc{{a.grad[j], a.grad[nv + j], a.grad[2 * nv + j]}, a.maps[7 * nv + j], Is};
        proj_add_terms_colored(pr, pc, lg, lc, v);
      } else {
        proj_add_terms(pr, v);
      }
      ++cnt;
    }
  }
  block_partials<NP2L>(v, cnt, a.partial + blockIdx.x, RED_MAX_BLOCKS, a.pcount + blockIdx.x);
}

void launch_proj_reduce(const ProjArgs& a, hipStream_t s) {
  const int B = red_blocks(a.rows * a.cols);
  const bool normal = a.min_normal_cos > -1.f;
  void (*kernel)(const ProjArgs) = proj_reduce_kernel<false, false>;
  if (a.grad)  // the coloured step
    kernel = normal ? proj_reduce_kernel<true, true> : proj_reduce_kernel<false, true>;
  else if (normal)
    kernel = proj_reduce_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(RED_THREADS), 0, s, a);
}

// canonical stage 2 (slot b = the sums of block b, +0.0 beyond nblocks, one slot per lane), then the loop rule
__global__ __launch_bounds__(RED_THREADS) void proj_step_kernel(const double* __restrict__ partial,
                                                                const int* __restrict__ pcount, int nblocks,
                                                                ProjBlock* __restrict__ blk, int k, int min_pairs) {
  if (blk->st.done) return;  // (uniform; lane 0 writes it only behind the tree's barrier)
  const int tid = threadIdx.x;
  double v[NP2L];
#pragma unroll
  for (int s = 0; s < NP2L; ++s) v[s] = tid < nblocks ? partial[s * RED_MAX_BLOCKS + tid] : 0.0;
  const int c = tid < nblocks ? pcount[tid] : 0;
  const BlockTotals<NP2L> t = block_tree<NP2L>(v, c);
  if (tid != 0) return;
  ProjState& st = blk->st;
  ProjIter& it = blk->trace[k];
  double sums[NP2L];
#pragma unroll
  for (int s = 0; s < NP2L; ++s) sums[s] = it.sums[s] = t.sum(s);
  const long long count = t.count();
  it.count = count;
  it.pad0 = 0;
  for (int e = 0; e < 12; ++e) it.E[e] = st.E[e];
  double dR[9], dt[3];
  if (count < (long long)min_pairs) {
    it.status = st.status = ICPK_W_TOO_FEW_PAIRS;
    st.done = 1;
  } else if (!solve_p2l(sums, dR, dt)) {
    it.status = st.status = ICPK_W_DEGENERATE;
    st.done = 1;
  } else {
    it.status = ICPK_OK;
    double En[12];
    proj_compose(dR, dt, st.E, En);
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) st.R[3 * r + cc] = (float)En[4 * r + cc];
      st.t[r] = (float)En[4 * r + 3];
    }
    for (int e = 0; e < 12; ++e) st.E[e] = En[e];
    st.iterations += 1;
  }
}

void launch_proj_step(const double* partial, const int* pcount, int nblocks, ProjBlock* blk, int k, int min_pairs,
                      hipStream_t s) {
  hipLaunchKernelGGL(proj_step_kernel, dim3(1), dim3(RED_THREADS), 0, s, partial, pcount, nblocks, blk, k, min_pairs);
}

// rules 1 - 8 per pixel, one thread each: icpk_projective_associate
template <bool WITH_NORMAL>
__global__ __launch_bounds__(RED_THREADS) void proj_associate_kernel(const ProjArgs a, int32_t* __restrict__ pixel,
                                                                     float* __restrict__ dist) {
  const int npix = a.rows * a.cols;
  const int i = (int)blockIdx.x * RED_THREADS + (int)threadIdx.x;
  if (i >= npix) return;
  const ProjLevel lv{a.depth, a.rows, a.cols, a.fx, a.cx};
  const ProjView vw = proj_view(a);
  const ProjPose E = proj_pose(a.st);
  const ProjGate g{a.max_dist, a.min_normal_cos};
  const int r = i / a.cols, c = i - r * a.cols;
  ProjPair pr;
  const int j = proj_pixel<WITH_NORMAL>(lv, vw, E, g, r, c, a.depth[i], &pr);
  pixel[i] = j;
  dist[i] = j >= 0 ? pr.dist : 0.f;
}

void launch_proj_associate(const ProjArgs& a, int32_t* pixel, float* dist, hipStream_t s) {
  const int B = (a.rows * a.cols + RED_THREADS - 1) / RED_THREADS;
  if (a.min_normal_cos > -1.f)
    hipLaunchKernelGGL(proj_associate_kernel<true>, dim3(B), dim3(RED_THREADS), 0, s, a, pixel, dist);
  else
    hipLaunchKernelGGL(proj_associate_kernel<false>, dim3(B), dim3(RED_THREADS), 0, s, a, pixel, dist);
}

}  // namespace icpk
