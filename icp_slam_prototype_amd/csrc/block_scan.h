// block_scan.h -- the scaffold shared by the order-preserving compactions (count per block, scan the counts, scatter:
// K4, K11, K13, K19-K21, the association split, the map's radix sort and list append, FAST): the rank of a thread
// inside its workgroup, and the exclusive scan of the block counts by one workgroup.  Everything here is
// __forceinline__ and takes the workgroup's size by template parameter: a kernel compiles to one body, as if the
// scaffold were written out in it, and every .hip keeps its own __global__ wrappers.
//
// The barrier contract, the same for every function here: all THREADS threads of the workgroup call it together, and
// it may be called again at once -- in a loop, or twice in a row on different data -- with no barrier from the caller.
// The LDS is block_excl_scan's own (THREADS / 64 words per kernel and value type), and it waits before its store for
// the readers of the call before.  Integers only: the order of a sum does not show.
#pragma once
#include <hip/hip_runtime.h>

namespace icpk {

// the exclusive rank of v among the workgroup's threads (the sum of v over the threads before this one); *total = the
// sum over the workgroup, in every thread.  wave64 inclusive scan, the waves' totals through LDS, the waves before
template <int THREADS, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* total) {
  static_assert(THREADS % 64 == 0 && THREADS >= 64 && THREADS <= 1024, "whole wave64s");
  constexpr int WAVES = THREADS / 64;
  __shared__ T wsum[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();  // (wsum of a previous call has been read)
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  T before = 0, all = 0;
  for (int w = 0; w < wave; ++w) before += wsum[w];
#pragma unroll
  for (int w = 0; w < WAVES; ++w) all += wsum[w];
  *total = all;
  return before + incl - v;
}

// the sum of v over the workgroup, in every thread
template <int THREADS, class T>
__device__ __forceinline__ T block_total(T v) {
  T total;
  block_excl_scan<THREADS>(v, &total);
  return total;
}

// out[i] = in[0] + ... + in[i - 1] for i < m, by one workgroup in rounds of THREADS; returns the sum of all m, in every
// thread.  The carry is an Out (int, or long long where the total outgrows an int; the sum of one round must fit an
// int either way).  in == out is allowed: a thread reads entry i before it writes entry i, and no other thread does
template <int THREADS, class Out>
__device__ __forceinline__ Out scan_rounds(const int* in, Out* out, int m) {
  Out carry = 0;
  for (int base = 0; base < m; base += THREADS) {
    const int i = base + (int)threadIdx.x;
    const int v = i < m ? in[i] : 0;
    int total;
    const int ex = block_excl_scan<THREADS>(v, &total);
    if (i < m) out[i] = carry + ex;
    carry += total;
  }
  return carry;
}

// the same scan in place with one contiguous run per thread, [t * per, (t + 1) * per) for thread t: one round whatever
// m is, for the tables of tens of thousands of entries (the map's digit histogram, FAST's mask words) that would take
// scan_rounds dozens.  Returns the sum, in every thread
template <int THREADS>
__device__ __forceinline__ int scan_runs(int* __restrict__ a, int m) {
  const int per = (m + THREADS - 1) / THREADS;
  const int b = (int)threadIdx.x * per, e = min(b + per, m);  // (b >= m: an empty run)
  int s = 0;
  for (int k = b; k < e; ++k) s += a[k];
  int total;
  int run = block_excl_scan<THREADS>(s, &total);
  for (int k = b; k < e; ++k) {
    const int v = a[k];
    a[k] = run;
    run += v;
  }
  return total;
}

}  // namespace icpk
