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
// Same shape as p2l_reduce_kernel (kernels_reduce.hip): 256-thread blocks, the records of a device loop's grid sweep
// with the next record on its way while the normals of the current one are gathered, wave_reduce_scatter, LoopState
// gating.  The records are in the CALLER's order (kernels_grid.hip, REC), so record i's source normal is normal i: a
// coalesced load, no permutation in between.
// Built with -ffp-contract=off like every exact kernel here: no multiply and add below is fused.
#include "icpk_internal.h"
#include "wave_sum.h"

namespace icpk {

__global__ __launch_bounds__(RED_THREADS) void gicp_reduce_kernel(
    const nn_key_t* __restrict__ best, const float* __restrict__ ax, const float* __restrict__ ay,
    const float* __restrict__ az, int nq, const float* __restrict__ tx, const float* __restrict__ ty,
    const float* __restrict__ tz, const GicpArgs g, const float4* __restrict__ rec, float max_dist,
    int32_t* __restrict__ idx_out, float* __restrict__ dist_out, double* __restrict__ partial, int* __restrict__ pcount,
    LoopState* __restrict__ st) {
  constexpr int NS = NP2L;
  const int tid = threadIdx.x;
  const int P = gridDim.x * RED_THREADS;
  // (records path: a lane's first record is asked for before the loop state is looked at, as in p2l_reduce_kernel)
  const int i_first = blockIdx.x * RED_THREADS + tid;
  float4 nx0 = make_float4(0.f, 0.f, 0.f, 0.f), nx1 = nx0;
  if (rec && i_first < nq) {
    nx0 = rec[2 * (size_t)i_first];
    nx1 = rec[2 * (size_t)i_first + 1];
  }
  // R_acc: the rotation of the accumulated pose as icpk_align returns it (float), widened
  double R[9];
  if (st) {
    if (st->done | st->stop_after_transform) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->sweeps += 1;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = (double)(float)st->Tk[4 * r + c];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)g.R[k];
  }
  const double c1 = 1.0 - (double)g.epsilon;
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  int cnt = 0;
  for (int i = i_first; i < nq; i += P) {
    float d, p0f, p1f, p2f, q0f = 0.f, q1f = 0.f, q2f = 0.f;
    int j;
    if (rec) {  // (uniform) behind a grid sweep of the device loop: query, match and distance in one 32-byte record
      const float4 r0 = nx0, r1 = nx1;
      if (i + P < nq) {
        nx0 = rec[2 * (size_t)(i + P)];
        nx1 = rec[2 * (size_t)(i + P) + 1];
      }
      p0f = r0.x, p1f = r0.y, p2f = r0.z, d = r0.w;
      q0f = r1.x, q1f = r1.y, q2f = r1.z, j = __float_as_int(r1.w);
    } else {
      const nn_key_t key = best[i];
      d = __uint_as_float((unsigned)(key >> 32));
      j = (int)(unsigned)(key & 0xffffffffu);
      if (idx_out) {  // (null in the device loop: icpk_get_associations unpacks on demand)
        idx_out[i] = j;
        dist_out[i] = d;
      }
      p0f = ax[i], p1f = ay[i], p2f = az[i];
    }
    if (d < max_dist) {  // icp.cpp:553 (false for NaN)
      const double a0 = g.snx[i], a1 = g.sny[i], a2 = g.snz[i];
      const double b0 = g.tnx[j], b1 = g.tny[j], b2 = g.tnz[j];
      if (!rec) q0f = tx[j], q1f = ty[j], q2f = tz[j];
      const double p0 = p0f, p1 = p1f, p2 = p2f;
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
        v[27] += (double)d;
        ++cnt;
      }
    }
  }
  double u[WaveScatter<NS>::H2];
  wave_reduce_scatter<NS>(v, u, cnt);
  __shared__ double ws[RED_THREADS / 64][NS];
  __shared__ int wc[RED_THREADS / 64];
  const int wave = tid >> 6, lane = tid & 63;
  wave_scatter_store<NS>(u, lane, ws[wave]);
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  if (tid < NS) partial[tid * RED_MAX_BLOCKS + blockIdx.x] = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
  if (tid == NS) pcount[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

void launch_gicp_reduce(const nn_key_t* best, const float* ax, const float* ay, const float* az, int nq, const float* tx,
                        const float* ty, const float* tz, const GicpArgs& g, const float4* rec, float max_dist,
                        int32_t* idx_out, float* dist_out, double* partial, int* pcount, double* out, LoopState* st,
                        hipStream_t s) {
  const int B = red_blocks(nq);
  hipLaunchKernelGGL(gicp_reduce_kernel, dim3(B), dim3(RED_THREADS), 0, s, best, ax, ay, az, nq, tx, ty, tz, g, rec,
                     max_dist, idx_out, dist_out, partial, pcount, st);
  if (out) launch_reduce_final(partial, pcount, B, NP2L, out, s);
}

}  // namespace icpk
