// kernels_robust.hip -- K10, the selection half of a robust sweep (include/icpk.h, icpk_set_robust): the exact cut
// tau (k-th smallest accepted distance) and median m (ceil(n/2)-th) of the sweep's accepted distances, by a radix
// select over their bit patterns.  Accepted distances are non-negative floats (d < max_dist is false for NaN), so with
// the sign bit cleared their patterns sort as unsigned integers; three passes narrow the buckets of both ranks:
// bits 30..20 (2048 bins), 19..10 (1024), 9..0 (1024).  Per pass a histogram kernel -- LDS integer atomics per block,
// then the block's non-zero bins added into one global histogram with integer atomics (exact: the result does not
// depend on the order blocks arrive in) -- and a one-block scan that finds each rank's bucket, keeps the rank left
// inside it, and clears the histogram for the next pass.  The last scan also computes the scale c.  The weighted
// reduction that follows (kernels_reduce.hip) reads tau and c from the RobustSel state.
// Inside a device loop every launch is a no-op once the loop has exited, as K2's are.
#include "icpk_internal.h"

namespace icpk {

constexpr int SEL_THREADS = 256;
constexpr int SEL_SHIFT[3] = {20, 10, 0};
constexpr int SEL_NBINS[3] = {2048, 1024, 1024};
constexpr unsigned SEL_NONE = 0xffffffffu;  // not accepted: its high bits match no prefix of any pass

__device__ __forceinline__ bool sel_stopped(const LoopState* st) { return st && (st->done | st->stop_after_transform); }

// pass 0 reads the sweep (records of a grid sweep in a device loop, else the keys), decides acceptance and keeps the
// patterns in dsel; passes 1 and 2 read dsel
template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void robust_hist_kernel(const nn_key_t* __restrict__ best,
                                                                  const float4* __restrict__ rec, int nq, float max_dist,
                                                                  const float* __restrict__ nx, const float* __restrict__ ny,
                                                                  const float* __restrict__ nz, unsigned* __restrict__ dsel,
                                                                  const RobustSel* __restrict__ sel, int* __restrict__ hist,
                                                                  const LoopState* __restrict__ st) {
  if (sel_stopped(st)) return;
  constexpr int NB = SEL_NBINS[PASS];
  constexpr int NH = PASS == 0 ? 1 : 2;  // pass 0: both ranks share the (empty) prefix
  __shared__ int h[NH][NB];
  for (int b = threadIdx.x; b < NH * NB; b += SEL_THREADS) (&h[0][0])[b] = 0;
  unsigned pre0 = 0, pre1 = 0;
  bool two = false;
  if constexpr (PASS > 0) {
    pre0 = sel->prefix[0];
    pre1 = sel->prefix[1];
    two = !sel->same;
  }
  __syncthreads();
  const int stride = gridDim.x * SEL_THREADS;
  for (int i = blockIdx.x * SEL_THREADS + threadIdx.x; i < nq; i += stride) {
    if constexpr (PASS == 0) {
      float d;
      int j;
      if (rec) {
        d = rec[2 * (size_t)i].w;
        j = __float_as_int(rec[2 * (size_t)i + 1].w);
      } else {
        const nn_key_t key = best[i];
        d = __uint_as_float((unsigned)(key >> 32));
        j = (int)(unsigned)(key & 0xffffffffu);
      }
      bool acc = d < max_dist;  // icp.cpp:553 (false for NaN)
      if (acc && nx) acc = !(nx[j] == 0.f && ny[j] == 0.f && nz[j] == 0.f);  // K5's acceptance
      const unsigned u = acc ? (__float_as_uint(d) & 0x7fffffffu) : SEL_NONE;
      dsel[i] = u;
      if (acc) atomicAdd(&h[0][u >> SEL_SHIFT[0]], 1);
    } else {
      const unsigned u = dsel[i];
      const unsigned hi = u >> SEL_SHIFT[PASS - 1], bin = (u >> SEL_SHIFT[PASS]) & (NB - 1);
      if (hi == pre0) atomicAdd(&h[0][bin], 1);
      if (two && hi == pre1) atomicAdd(&h[1][bin], 1);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < NH * NB; b += SEL_THREADS) {
    const int v = (&h[0][0])[b];
    if (v) atomicAdd(&hist[(b / NB) * SEL_BINS + b % NB], v);
  }
}

// one block: the bucket of each rank, the rank left inside it; then the histogram is cleared
template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void robust_scan_kernel(RobustSel* __restrict__ sel, int* __restrict__ hist,
                                                                  const RobustCfg cfg, const LoopState* __restrict__ st) {
  if (sel_stopped(st)) return;
  constexpr int NB = SEL_NBINS[PASS], PER = NB / SEL_THREADS;
  __shared__ long long part[SEL_THREADS];
  __shared__ long long total;
  const int t = threadIdx.x;
  long long n = 0, rank[2] = {0, 0};
  unsigned prefix[2] = {0, 0};
  int same = 1;
  if constexpr (PASS > 0) {
    n = sel->n;
    rank[0] = sel->rank[0], rank[1] = sel->rank[1];
    prefix[0] = sel->prefix[0], prefix[1] = sel->prefix[1];
    same = sel->same;
  }
  __syncthreads();  // (every thread has read sel before thread 0 writes it)
  for (int r = 0; r < 2; ++r) {
    const int* hr = hist + ((PASS > 0 && r == 1 && !same) ? SEL_BINS : 0);
    int c[PER];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) s += (c[k] = hr[t * PER + k]);
    // inclusive scan of the threads' sums (Hillis-Steele; integers: exact)
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < SEL_THREADS; off <<= 1) {
      const long long v = t >= off ? part[t - off] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    if (PASS == 0 && r == 0) {
      if (t == SEL_THREADS - 1) total = part[t];
      __syncthreads();
      n = total;
      if (n > 0) {
        long long k = (long long)ceil((double)cfg.trim * (double)n);
        rank[0] = k < 1 ? 1 : (k > n ? n : k);
        rank[1] = (n + 1) / 2;
      }
    }
    const long long before = part[t] - s;
    if (n > 0 && before < rank[r] && rank[r] <= part[t]) {  // the rank falls into this thread's bins
      long long cum = before, below = 0;
      int kb = -1;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        if (kb < 0 && cum + c[k] >= rank[r]) kb = k, below = cum;
        cum += c[k];
      }
      sel->prefix[r] = (PASS == 0 ? 0u : prefix[r] << 10) | (unsigned)(t * PER + kb);
      sel->rank[r] = rank[r] - below;
    }
    __syncthreads();
  }
  for (int b = t; b < NB; b += SEL_THREADS) {
    hist[b] = 0;
    if (PASS > 0) hist[SEL_BINS + b] = 0;
  }
  __syncthreads();
  if (t != 0) return;
  if (n == 0) {
    sel->prefix[0] = sel->prefix[1] = 0u;
    sel->rank[0] = sel->rank[1] = 0;
  }
  if (PASS == 0) sel->n = n;
  sel->same = sel->prefix[0] == sel->prefix[1];
  if (PASS == 2) {
    const float cut = __uint_as_float(sel->prefix[0]), m = __uint_as_float(sel->prefix[1]);
    sel->cut = cut;
    sel->median = m;
    sel->kernel = cfg.kernel;
    sel->c = cfg.scale_mode == 1 ? (double)cfg.scale * 1.4826 * (double)m : (double)cfg.scale;  // ICPK_SCALE_MEDIAN
  }
}

void launch_robust_select(const nn_key_t* best, const float4* rec, int nq, float max_dist, const float* nx,
                          const float* ny, const float* nz, unsigned* dsel, int* hist, RobustSel* sel, const RobustCfg& cfg,
                          const LoopState* st, hipStream_t s) {
  int B = (nq + 8 * SEL_THREADS - 1) / (8 * SEL_THREADS);  // >= 8 distances per lane
  B = B < 1 ? 1 : (B > 256 ? 256 : B);
  hipLaunchKernelGGL(robust_hist_kernel<0>, dim3(B), dim3(SEL_THREADS), 0, s, best, rec, nq, max_dist, nx, ny, nz, dsel,
                     sel, hist, st);
  hipLaunchKernelGGL(robust_scan_kernel<0>, dim3(1), dim3(SEL_THREADS), 0, s, sel, hist, cfg, st);
  hipLaunchKernelGGL(robust_hist_kernel<1>, dim3(B), dim3(SEL_THREADS), 0, s, best, rec, nq, max_dist, nx, ny, nz, dsel,
                     sel, hist, st);
  hipLaunchKernelGGL(robust_scan_kernel<1>, dim3(1), dim3(SEL_THREADS), 0, s, sel, hist, cfg, st);
  hipLaunchKernelGGL(robust_hist_kernel<2>, dim3(B), dim3(SEL_THREADS), 0, s, best, rec, nq, max_dist, nx, ny, nz, dsel,
                     sel, hist, st);
  hipLaunchKernelGGL(robust_scan_kernel<2>, dim3(1), dim3(SEL_THREADS), 0, s, sel, hist, cfg, st);
}

}  // namespace icpk
