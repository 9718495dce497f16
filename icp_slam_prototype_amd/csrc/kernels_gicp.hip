// kernels_gicp.hip -- K14: normal equations of the plane-to-plane step of Generalized-ICP (extension; the rule is
// spelled out operation by operation in include/icpk.h under ICPK_SOLVE_PLANE_TO_PLANE and restated in
// tests/gicp_model.py).
//
// Per accepted pair (dist < max_dist and a finite, positive determinant) with working source point p, match q, source
// normal a rotated by the pose accumulated so far (m = R_acc a) and target normal b:
//   S = 2 I - (1 - eps)(m m^T + b b^T),  M = S^-1 (adjugate and one determinant),  r = p - q,  J = [-[p]x | I]
// and the 28 sums of ICPK_NP2L's layout -- 21 upper-triangle entries of J^T M J, 6 of J^T M r, 1 distance sum -- through
// the same canonical tree as K2 and K5, so that solve_p2l and the loop step of point-to-plane take them as they are.
// J is never formed: with B = [p]x M (column c = p x M_c) and w = M r,
//   J^T M J = [ rows a: p x B_a | B ]      J^T M r = [ p x w ]
//             [        .        | M ]                [   w   ]
// The scaffold is pair_reduce.h's, as K5's (p2l_reduce_kernel): the pair stream in front, the block epilogue behind.
// The records are in the CALLER's order (kernels_grid.hip, REC), so record i's source normal is normal i: a
// coalesced load, no permutation in between.
// Built with -ffp-contract=off like every exact kernel here: no multiply and add below is fused.
#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {

__global__ __launch_bounds__(RED_THREADS) void gicp_reduce_kernel(const PairArgs args, const GicpArgs g) {
  constexpr int NS = NP2L;
  PairStream pairs(args, blockIdx.x, gridDim.x);
  if (!pairs.open()) return;
  // R_acc: the rotation of the accumulated pose as icpk_align returns it (float), widened
  double R[9];
  if (args.st) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)(float)args.st->Tk[4 * r + c];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)g.R[k];
  }
  const double c1 = 1.0 - (double)g.epsilon;
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  int cnt = 0;
  pairs.for_each([&](const auto& pr) {
    const double a0 = g.snx[pr.i], a1 = g.sny[pr.i], a2 = g.snz[pr.i];
    const double b0 = g.tnx[pr.j], b1 = g.tny[pr.j], b2 = g.tnz[pr.j];
    float q0f, q1f, q2f;
    pr.match(q0f, q1f, q2f);
    const double p0 = pr.p0, p1 = pr.p1, p2 = pr.p2;
    const double m0 = (R[0] * a0 + R[1] * a1) + R[2] * a2;
    const double m1 = (R[3] * a0 + R[4] * a1) + R[5] * a2;
    const double m2 = (R[6] * a0 + R[7] * a1) + R[8] * a2;
    // S = 2 I - c1 (m m^T + b b^T), upper triangle
    const double S00 = 2.0 - c1 * (m0 * m0 + b0 * b0);
    const double S01 = 0.0 - c1 * (m0 * m1 + b0 * b1);
    const double S02 = 0.0 - c1 * (m0 * m2 + b0 * b2);
    const double S11 = 2.0 - c1 * (m1 * m1 + b1 * b1);
    const double S12 = 0.0 - c1 * (m1 * m2 + b1 * b2);
    const double S22 = 2.0 - c1 * (m2 * m2 + b2 * b2);
    // adjugate and determinant
    const double K00 = S11 * S22 - S12 * S12;
    const double K01 = S02 * S12 - S01 * S22;
    const double K02 = S01 * S12 - S02 * S11;
    const double K11 = S00 * S22 - S02 * S02;
    const double K12 = S01 * S02 - S00 * S12;
    const double K22 = S00 * S11 - S01 * S01;
    const double det = (S00 * K00 + S01 * K01) + S02 * K02;
    if (det > 0.0 && det < __builtin_inf()) {  // (false for NaN: only non-unit normals from the host get here)
      const double inv = 1.0 / det;
      const double M00 = K00 * inv, M01 = K01 * inv, M02 = K02 * inv;
      const double M11 = K11 * inv, M12 = K12 * inv, M22 = K22 * inv;
      const double r0 = p0 - (double)q0f, r1 = p1 - (double)q1f, r2 = p2 - (double)q2f;
      const double w0 = (M00 * r0 + M01 * r1) + M02 * r2;
      const double w1 = (M01 * r0 + M11 * r1) + M12 * r2;
      const double w2 = (M02 * r0 + M12 * r1) + M22 * r2;
      // B = [p]x M: column c is p x (column c of M)
      const double B00 = p1 * M02 - p2 * M01, B10 = p2 * M00 - p0 * M02, B20 = p0 * M01 - p1 * M00;
      const double B01 = p1 * M12 - p2 * M11, B11 = p2 * M01 - p0 * M12, B21 = p0 * M11 - p1 * M01;
      const double B02 = p1 * M22 - p2 * M12, B12 = p2 * M02 - p0 * M22, B22 = p0 * M12 - p1 * M02;
      // [p]x M [p]x^T, upper triangle: row a is p x (row a of B)
      v[0] += p1 * B02 - p2 * B01;
      v[1] += p2 * B00 - p0 * B02;
      v[2] += p0 * B01 - p1 * B00;
      v[3] += B00;
      v[4] += B01;
      v[5] += B02;
      v[6] += p2 * B10 - p0 * B12;
      v[7] += p0 * B11 - p1 * B10;
      v[8] += B10;
      v[9] += B11;
      v[10] += B12;
      v[11] += p0 * B21 - p1 * B20;
      v[12] += B20;
      v[13] += B21;
      v[14] += B22;
      v[15] += M00;
      v[16] += M01;
      v[17] += M02;
      v[18] += M11;
      v[19] += M12;
      v[20] += M22;
      v[21] += p1 * w2 - p2 * w1;
      v[22] += p2 * w0 - p0 * w2;
      v[23] += p0 * w1 - p1 * w0;
      v[24] += w0;
      v[25] += w1;
      v[26] += w2;
      v[27] += (double)pr.d;
      ++cnt;
    }
  });
  block_partials<NS>(v, cnt, args.partial + blockIdx.x, RED_MAX_BLOCKS, args.pcount + blockIdx.x);
}

void launch_gicp_reduce(const PairArgs& a, const GicpArgs& g, hipStream_t s) {
  const int B = red_blocks(a.nq);
  hipLaunchKernelGGL(gicp_reduce_kernel, dim3(B), dim3(RED_THREADS), 0, s, a, g);
  if (a.out) launch_reduce_final(a.partial, a.pcount, B, NP2L, a.out, s);
}

}  // namespace icpk
