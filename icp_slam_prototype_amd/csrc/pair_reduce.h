// pair_reduce.h -- the scaffold shared by the reductions over one sweep's pairs (K2, K5, K14, K17, K15's sums and
// stage 2): the stream of accepted pairs in front of a kernel's per-pair arithmetic and the block epilogue behind it.
// Everything here is __forceinline__ and takes its callables by template parameter: a kernel compiles to one body, as
// if the scaffold were written out in it.
#pragma once
#include "icpk_internal.h"
#include "wave_sum.h"

namespace icpk {

// ---- the block epilogue -------------------------------------------------------------------------------------------
// The canonical tree of include/icpk.h (ICPK_RED_*) over a workgroup of RED_THREADS: the wave64 butterfly (order 32,
// 16, ..., 1) as a reduce-scatter (wave_sum.h), the waves' totals through LDS, then ((w0 + w1) + w2) + w3.
template <int NS>
struct BlockTotals {
  const double (*ws)[NS];
  const int* wc;
  __device__ __forceinline__ double sum(int s) const { return ((ws[0][s] + ws[1][s]) + ws[2][s]) + ws[3][s]; }
  __device__ __forceinline__ long long count() const { return (long long)wc[0] + wc[1] + wc[2] + wc[3]; }
};
struct NoHook {
  __device__ __forceinline__ void operator()(double) const {}
};

// every thread of the workgroup calls it; any thread may then read any total.  The LDS is the function's, one copy per
// kernel and NS, and nothing waits in front of its stores: a kernel that calls it a second time with the same NS
// needs a __syncthreads() before that call, or the second call overwrites totals that are still being read.
// after_butterfly(u[0]): a diagnostic build's stamp between the butterfly and the LDS round
template <int NS, class Hook = NoHook>
__device__ __forceinline__ BlockTotals<NS> block_tree(const double (&v)[NS], int cnt, Hook after_butterfly = {}) {
  __shared__ double ws[RED_THREADS / 64][NS];
  __shared__ int wc[RED_THREADS / 64];
  double u[WaveScatter<NS>::H2];
  wave_reduce_scatter<NS>(v, u, cnt);
  after_butterfly(u[0]);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  wave_scatter_store<NS>(u, lane, ws[wave]);
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  return BlockTotals<NS>{ws, wc};
}

// sum s of the workgroup to sums_dst[s * stride] (thread s), the count to *count_dst (thread NS)
template <int NS, class Count, class Hook = NoHook>
__device__ __forceinline__ void block_partials(const double (&v)[NS], int cnt, double* __restrict__ sums_dst, int stride,
                                               Count* __restrict__ count_dst, Hook after_butterfly = {}) {
  const BlockTotals<NS> t = block_tree<NS>(v, cnt, after_butterfly);
  const int tid = threadIdx.x;
  if (tid < NS) sums_dst[tid * stride] = t.sum(tid);
  if (tid == NS) *count_dst = (Count)t.count();
}

// ---- the pair stream ----------------------------------------------------------------------------------------------
// One accepted pair as a kernel's term sees it: the moved query p = (p0, p1, p2), its index i, the match's index j and
// their distance d.  The match itself comes from the record where there is one (REC) and is gathered only when the
// term asks for it otherwise -- after whatever the term checks first.
template <bool REC>
struct Pair {
  const PairArgs& a;
  int i, j;
  float d, p0, p1, p2;
  float4 r1;  // REC: (match, index bits)
  // O4: take the context's caller-order (x, y, z, 0) points where it has them: one 16-byte gather instead of three
  template <bool O4 = false>
  __device__ __forceinline__ void match(float& q0, float& q1, float& q2) const {
    if constexpr (REC) {
      q0 = r1.x, q1 = r1.y, q2 = r1.z;
    } else {
      if (O4 && a.o4) {  // (uniform)
        const float4 b = a.o4[j];
        q0 = b.x, q1 = b.y, q2 = b.z;
      } else {
        q0 = a.tx[j], q1 = a.ty[j], q2 = a.tz[j];
      }
    }
  }
};

// `block` of `nblocks` workgroups of RED_THREADS: the canonical geometry of the pair (nblocks = red_blocks(nq)), which
// the frame-batch kernel takes from its arguments and not from the grid.
// Use: construct, open(), the kernel's own set-up, for_each(term), block_partials.
struct PairStream {
  const PairArgs& a;
  const int block, P, i_first;
  float4 f0, f1;

  // Records path (a.rec, uniform: behind a grid sweep of the device loop, one coalesced 32-byte record per query, no
  // gather): a lane's first record is asked for BEFORE the loop state is looked at -- two cold round trips side by side
  // instead of one after the other, ~0.7 us of a 5 us kernel; if the loop has ended the loads were for nothing.
  __device__ __forceinline__ PairStream(const PairArgs& args, int block_, int nblocks)
      : a(args), block(block_), P(nblocks * RED_THREADS), i_first(block_ * RED_THREADS + (int)threadIdx.x) {
    f0 = make_float4(0.f, 0.f, 0.f, 0.f), f1 = f0;
    if (a.rec && i_first < a.nq) {
      f0 = a.rec[2 * (size_t)i_first];
      f1 = a.rec[2 * (size_t)i_first + 1];
    }
  }

  // false: the device loop has ended and the launch is a no-op; else this sweep's associations count as consumed
  __device__ __forceinline__ bool open() const {
    if (a.st) {
      if (a.st->done | a.st->stop_after_transform) return false;
      if (block == 0 && threadIdx.x == 0) a.st->sweeps += 1;
    }
    return true;
  }

  // term(const Pair<REC>&) for every pair of this lane with d < max_dist, in index order
  template <class Term>
  __device__ __forceinline__ void for_each(Term&& term) {
    if (a.rec) {
      // the NEXT record is on its way while this one is consumed (a lane has 3-4 of them at Kinect-v2 size, each a
      // chain of record -> gathers -> arithmetic otherwise)
      for (int i = i_first; i < a.nq; i += P) {
        const float4 r0 = f0, r1 = f1;
        if (i + P < a.nq) {
          f0 = a.rec[2 * (size_t)(i + P)];
          f1 = a.rec[2 * (size_t)(i + P) + 1];
        }
        if (r0.w < a.max_dist)  // icp.cpp:553 (false for NaN)
          term(Pair<true>{a, i, __float_as_int(r1.w), r0.w, r0.x, r0.y, r0.z, r1});
      }
    } else {
      for (int i = i_first; i < a.nq; i += P) {
        const nn_key_t key = a.best[i];
        const float d = __uint_as_float((unsigned)(key >> 32));
        const int j = (int)(unsigned)(key & 0xffffffffu);
        if (a.idx_out) {  // (null in the device loop: icpk_get_associations unpacks on demand)
          a.idx_out[i] = j;
          a.dist_out[i] = d;
        }
        if (d < a.max_dist)  // icp.cpp:553 (false for NaN)
          term(Pair<false>{a, i, j, d, a.ax[i], a.ay[i], a.az[i], make_float4(0.f, 0.f, 0.f, 0.f)});
      }
    }
  }
};

}  // namespace icpk
