// kernels_reduce.hip -- K2: masked reduction over the associations of one sweep.
//
// Folds into one pass what the reference does with four O(N) loops:
//   icp.cpp:186-200  association split + N x 3 matrix export
//   icp.cpp:212      M = previousMat.t() * dataMat      (9 sums, M[r][c] = sum b_r a_c)
//   icp.cpp:314-344  calculateOffset                    (3 sums of (float)(a - b))
//   icp.cpp:622-638  meanSquareError                    (1 sum of distances, count)
// plus sum a / sum b (6) for the centred Kabsch flavour (rigid_transform_3D.py:14-20).
//
// Summation order is the canonical tree of include/icpk.h (ICPK_RED_*): double
// accumulators, wave64 xor butterfly via __shfl_xor, fixed wave and block
// order -- no atomics, so results are bit-reproducible and equal to the
// oracle's orc_sums_canonical.
#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {

// Diagnostic build only (-DICPK_RED_STAMPS, tools/stamp_reduce.py): wall_clock64 stamps per block
#ifdef ICPK_RED_STAMPS
__device__ unsigned long long red_dbg[8 * 256];
#define RED_STAMP(k)                                                               \
  do {                                                                             \
    if (threadIdx.x == 0) red_dbg[blockIdx.x * 8 + (k)] = wall_clock64();          \
  } while (0)
extern "C" int icpk_debug_read_red_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(red_dbg), sizeof(red_dbg));
}
#else
#define RED_STAMP(k)
#endif

// NACT: how many of the NSUM sums the consumer needs.  NACT == NSUM_W: the weighted K2 of a robust sweep (K10): every
// sum but the distance sum multiplied by the pair's weight w (RobustWeight of the cut and scale in `sel`), and W and
// the kept count in [19], [20]; the int count stays the accepted pairs'.  icpk_reduce and the Kabsch flavour take
// all 19; the reference flavour's loop step only reads [0..12] (M, mean difference, distance
// sum), so the device loop skips the sums of a and b: a third less butterfly.
// `block` of `nblocks` (the canonical geometry of the pair: nblocks = red_blocks(nq)); shared
// by the single-pair kernel and the frame-batch kernel (blockIdx.y = pair).
template <int NACT>
__device__ __forceinline__ void assoc_reduce_body(const PairArgs& args, const int block, const int nblocks,
                                                  const RobustSel* __restrict__ sel = nullptr) {
  constexpr bool WEIGHTED = NACT == NSUM_W;
  PairStream pairs(args, block, nblocks);
  if (!pairs.open()) return;
  RED_STAMP(0);
  double v[NACT];
#pragma unroll
  for (int s = 0; s < NACT; ++s) v[s] = 0.0;
  int cnt = 0;
  RobustWeight weight{};
  if constexpr (WEIGHTED) weight = RobustWeight{sel->kernel, sel->cut, sel->c};

  // the accumulation of one accepted pair (a = moved query, b = its match, d = their distance)
  pairs.for_each([&](const auto& pr) {
      const float a0 = pr.p0, a1 = pr.p1, a2 = pr.p2, d = pr.d;
      float b0, b1, b2;
      pr.template match<true>(b0, b1, b2);
      if constexpr (WEIGHTED) {
        v[12] += (double)d;
        ++cnt;
        const double w = weight(d);
        if (!(w > 0.0)) return;  // (trimmed or zero weight: not kept, adds nothing)
        // w * x: with w == 1 every term is the plain one, bit for bit
        const double da0 = a0, da1 = a1, da2 = a2, wb0 = w * (double)b0, wb1 = w * (double)b1, wb2 = w * (double)b2;
        v[0] += wb0 * da0; v[1] += wb0 * da1; v[2] += wb0 * da2;
        v[3] += wb1 * da0; v[4] += wb1 * da1; v[5] += wb1 * da2;
        v[6] += wb2 * da0; v[7] += wb2 * da1; v[8] += wb2 * da2;
        v[9] += w * (double)(a0 - b0);
        v[10] += w * (double)(a1 - b1);
        v[11] += w * (double)(a2 - b2);
        v[13] += w * da0; v[14] += w * da1; v[15] += w * da2;
        v[16] += wb0; v[17] += wb1; v[18] += wb2;
        v[19 % NACT] += w;
        v[20 % NACT] += 1.0;
        return;
      }
      const double da0 = a0, da1 = a1, da2 = a2, db0 = b0, db1 = b1, db2 = b2;
      v[0] += db0 * da0; v[1] += db0 * da1; v[2] += db0 * da2;
      v[3] += db1 * da0; v[4] += db1 * da1; v[5] += db1 * da2;
      v[6] += db2 * da0; v[7] += db2 * da1; v[8] += db2 * da2;
      v[9] += (double)(a0 - b0);
      v[10] += (double)(a1 - b1);
      v[11] += (double)(a2 - b2);
      v[12] += (double)d;
      if constexpr (NACT > 13) {
        v[13] += da0; v[14] += da1; v[15] += da2;
        v[16] += db0; v[17] += db1; v[18] += db2;
      }
      ++cnt;
  });

  if (v[12] > -1.0) RED_STAMP(1);  // loads and accumulation done
  block_partials<NACT>(v, cnt, args.partial + block, RED_MAX_BLOCKS, args.pcount + block, [](double u0) {
    if (u0 > -1.0) RED_STAMP(2);  // butterfly done
  });
  RED_STAMP(3);
}

template <int NACT>
__global__ __launch_bounds__(RED_THREADS) void assoc_reduce_kernel(const PairArgs a, const RobustSel* __restrict__ sel) {
  assoc_reduce_body<NACT>(a, blockIdx.x, gridDim.x, sel);
}

// frame-batch mode: blockIdx.y = pair; every pair keeps ITS canonical geometry (its own
// nblocks), so its sums equal those of a single-pair launch bit for bit
template <int NACT>
__global__ __launch_bounds__(RED_THREADS) void assoc_reduce_batch_kernel(const ReduceBatch b, float max_dist) {
  const ReduceArgs& r = b.p[blockIdx.y];
  if ((int)blockIdx.x >= r.nblocks) return;
  const PairArgs a{r.best, r.ax, r.ay, r.az, r.tx, r.ty, r.tz, r.o4, r.rec, r.nq, max_dist, nullptr, nullptr,
                   r.partial, r.pcount, nullptr, r.st};
  assoc_reduce_body<NACT>(a, blockIdx.x, r.nblocks);
}

// K5: normal equations of the linearised point-to-plane step (extension; the
// reference only plans it, TODO:9).  Per accepted pair (dist < max_dist and a
// non-zero target normal n): J = [p x n ; n], r = (p - q).n; 21 upper-triangle
// entries of J J^T, 6 of J r, 1 distance sum -- same canonical tree as K2.
// NS == NP2L_W: the weighted K5 of a robust sweep (K10): the 27 terms multiplied by w, the distance sum unweighted,
// W and the kept count in [28], [29].
template <int NS>
__global__ __launch_bounds__(RED_THREADS) void p2l_reduce_kernel(const PairArgs args, const float* __restrict__ nxp,
                                                                 const float* __restrict__ nyp,
                                                                 const float* __restrict__ nzp,
                                                                 const RobustSel* __restrict__ sel) {
  constexpr bool WEIGHTED = NS == NP2L_W;
  PairStream pairs(args, blockIdx.x, gridDim.x);
  if (!pairs.open()) return;
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  int cnt = 0;
  RobustWeight weight{};
  if constexpr (WEIGHTED) weight = RobustWeight{sel->kernel, sel->cut, sel->c};
  pairs.for_each([&](const auto& pr) {
    const double n0 = nxp[pr.j], n1 = nyp[pr.j], n2 = nzp[pr.j];
    if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) return;
    float b0, b1, b2;
    pr.match(b0, b1, b2);
    const double p0 = pr.p0, p1 = pr.p1, p2 = pr.p2;
    const double q0 = b0, q1 = b1, q2 = b2;
    double J[6];
    J[0] = p1 * n2 - p2 * n1;
    J[1] = p2 * n0 - p0 * n2;
    J[2] = p0 * n1 - p1 * n0;
    J[3] = n0;
    J[4] = n1;
    J[5] = n2;
    const double r = ((p0 - q0) * n0 + (p1 - q1) * n1) + (p2 - q2) * n2;
    v[27] += (double)pr.d;
    ++cnt;
    if constexpr (WEIGHTED) {
      const double w = weight(pr.d);
      if (w > 0.0) {  // w * x: with w == 1 every term is the plain one, bit for bit
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[k++] += w * (J[a] * J[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] += w * (J[a] * r);
        v[28 % NS] += w;
        v[29 % NS] += 1.0;
      }
    } else {
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) v[k++] += J[a] * J[b];
#pragma unroll
      for (int a = 0; a < 6; ++a) v[21 + a] += J[a] * r;
    }
  });
  block_partials<NS>(v, cnt, args.partial + blockIdx.x, RED_MAX_BLOCKS, args.pcount + blockIdx.x);
}

void launch_p2l_reduce(const PairArgs& a, const float* nx, const float* ny, const float* nz, hipStream_t s,
                       const RobustSel* sel) {
  const int B = red_blocks(a.nq);
  if (sel)
    hipLaunchKernelGGL(p2l_reduce_kernel<NP2L_W>, dim3(B), dim3(RED_THREADS), 0, s, a, nx, ny, nz, sel);
  else
    hipLaunchKernelGGL(p2l_reduce_kernel<NP2L>, dim3(B), dim3(RED_THREADS), 0, s, a, nx, ny, nz, nullptr);
  if (a.out) launch_reduce_final(a.partial, a.pcount, B, sel ? NP2L_W : NP2L, a.out, s);
}

void launch_assoc_reduce(const PairArgs& a, int nact, hipStream_t s, const RobustSel* sel) {
  const int B = red_blocks(a.nq);
  if (sel)
    hipLaunchKernelGGL(assoc_reduce_kernel<NSUM_W>, dim3(B), dim3(RED_THREADS), 0, s, a, sel);
  else if (nact == NSUM_REF && !a.out)
    hipLaunchKernelGGL(assoc_reduce_kernel<NSUM_REF>, dim3(B), dim3(RED_THREADS), 0, s, a, nullptr);
  else
    hipLaunchKernelGGL(assoc_reduce_kernel<NSUM>, dim3(B), dim3(RED_THREADS), 0, s, a, nullptr);
  if (a.out) launch_reduce_final(a.partial, a.pcount, B, sel ? NSUM_W : NSUM, a.out, s);
}

void launch_assoc_reduce_batch(const ReduceBatch& b, int count, float max_dist, int nact, hipStream_t s) {
  int bmax = 0;
  for (int k = 0; k < count; ++k) bmax = b.p[k].nblocks > bmax ? b.p[k].nblocks : bmax;
  if (count <= 0 || bmax <= 0) return;
  if (nact == NSUM_REF)
    hipLaunchKernelGGL(assoc_reduce_batch_kernel<NSUM_REF>, dim3(bmax, count), dim3(RED_THREADS), 0, s, b, max_dist);
  else
    hipLaunchKernelGGL(assoc_reduce_batch_kernel<NSUM>, dim3(bmax, count), dim3(RED_THREADS), 0, s, b, max_dist);
}

}  // namespace icpk
