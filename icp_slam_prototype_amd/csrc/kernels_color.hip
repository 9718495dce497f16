// kernels_color.hip -- K17: colored ICP (the rule is spelled out operation by operation in include/icpk.h under
// "colored ICP" and restated in tests/color_model.py).
//
//   1. color_gather_kernel        the target's intensities into cell order, so that a row of cells is one contiguous
//                                 range of them as it is of the points
//   2. color_gradient_sums_kernel K12's radius walk (normals_moments_kernel: the points in cell order, CG_S adjacent lanes
//                                 per point, the (y, z) rows of the cube dealt to them, an xor butterfly over the point's
//                                 lanes) with other sums: per neighbour the offset projected onto the point's tangent
//                                 plane and the intensity difference, both quantised to integers, and the nine sums of
//                                 their products.  Integers, so the sums are the same bits on every run, for every order
//                                 of the cloud, and the bits of the CPU model.
//   3. color_gradient_solve_kernel one lane per point: the 3x3 normal equations with the row that pins the normal
//                                 component, solved by K14's adjugate in float64.
//   4. colored_reduce_kernel      the joint step: gicp_reduce_kernel's shape (256-thread blocks, the records of a device
//                                 loop's grid sweep with the next record on its way, wave_reduce_scatter, LoopState
//                                 gating), point-to-plane's acceptance and geometric terms, and the photometric terms
//                                 beside them in the same 28 sums.
// Built with -ffp-contract=off like every exact kernel here: no multiply and add below is fused.
#include "icpk_internal.h"
#include "nn_device.h"
#include "wave_sum.h"

namespace icpk {

namespace {

constexpr int CG_S = 8;  // lanes per point, as K12
constexpr int CG_BLOCK = 256;
constexpr int CG_UNROLL = 4;
constexpr double CG_FIX = 32768.0;  // F = 2^15

// q = (int64)rint((u / r) * F), K12's way (kernels_normals.hip, quantise): the product with fl(1 / r) differs from the
// rule's quotient by less than 2^-36 after the scaling (|u / r| <= 1 + 2^-19 for an accepted neighbour and a usable
// normal, three roundings of 2^-53 each, times 2^15), so unless it lies within 2^-30 of a rounding boundary both round
// to the same integer; there the division decides.
__device__ __forceinline__ int quantise(double u, double rd, double inv_r) {
  double t = (u * inv_r) * CG_FIX;
  double k = __builtin_rint(t);
  if (!(__builtin_fabs(t - k) < 0.5 - 0x1p-30)) {
    t = (u / rd) * CG_FIX;
    k = __builtin_rint(t);
  }
  return (int)k;
}

__global__ __launch_bounds__(CG_BLOCK) void color_gather_kernel(const float4* __restrict__ t4,
                                                                 const float* __restrict__ col, int n,
                                                                 float* __restrict__ col_sorted) {
  const int ip = blockIdx.x * CG_BLOCK + threadIdx.x;
  if (ip >= n) return;
  const int j = __float_as_int(t4[ip].w);              // 0 <= j < n: the index K1d's sort wrote
  col_sorted[ip] = col[min(max(j, 0), n - 1)];
}

struct ColorSums {
  long long m, s00, s01, s02, s11, s12, s22, t0, t1, t2;
};

__device__ __forceinline__ long long sum_over_point(long long v) {
#pragma unroll
  for (int k = 1; k < CG_S; k <<= 1) v += __shfl_xor(v, k, 64);
  return v;
}

__global__ __launch_bounds__(CG_BLOCK) void color_gradient_sums_kernel(const ColorGradArgs a) {
  const int slice = threadIdx.x & (CG_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)CG_BLOCK + threadIdx.x) / CG_S);  // position in cell order
  const bool live = ip < a.n;
  const float4 p4 = live ? a.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int orig = live ? min(max(__float_as_int(p4.w), 0), a.n - 1) : 0;
  const GridInfo g = *a.gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const float r = a.radius;
  const double rd = (double)r, inv_r = 1.0 / rd;
  const double n0 = live ? (double)a.nx[orig] : 0.0, n1 = live ? (double)a.ny[orig] : 0.0,
               n2 = live ? (double)a.nz[orig] : 0.0;
  const double Ii = live ? (double)a.col_sorted[ip] : 0.0;
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
  const bool usable = nn >= 1.0 - 0x1p-10 && nn <= 1.0 + 0x1p-10;  // (false for NaN)
  // a non-finite point has an empty neighbourhood (and its cube would be the whole grid)
  const bool scan = live && __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz);
  int x0, x1, y0, y1, z0, z1;
  cube_cells(px, r, g.lo[0], g.inv_hx, g.nx, x0, x1);
  cube_cells(py, r, g.lo[1], g.inv_h, g.ny, y0, y1);
  cube_cells(pz, r, g.lo[2], g.inv_h, g.nz, z0, z1);
  const int nyr = y1 - y0 + 1;
  const int nrows = scan ? nyr * (z1 - z0 + 1) : 0;
  ColorSums M{};
  for (int row = slice; row < nrows; row += CG_S) {
    const int rz = row / nyr, ry = row - rz * nyr;
    const int base = ((z0 + rz) * g.ny + (y0 + ry)) * g.nx;  // cells base + x0 .. base + x1 < ncells, one range
    const int s0 = a.cell_start[base + x0], s1 = a.cell_start[base + x1 + 1];  // s1 <= n
    for (int j = s0; j < s1; j += CG_UNROLL) {
      float4 c[CG_UNROLL];
      float ic[CG_UNROLL];
#pragma unroll
      for (int u = 0; u < CG_UNROLL; ++u) {
        const int jj = min(j + u, s1 - 1);
        c[u] = a.t4[jj];
        ic[u] = a.col_sorted[jj];
      }
#pragma unroll
      for (int u = 0; u < CG_UNROLL; ++u) {
        const float d = pair_dist(px, py, pz, c[u].x, c[u].y, c[u].z);
        if (j + u < s1 && d <= r) {  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
          M.m += 1;
          if (usable) {
            const double e0 = (double)c[u].x - (double)px, e1 = (double)c[u].y - (double)py,
                         e2 = (double)c[u].z - (double)pz;
            const double h = (e0 * n0 + e1 * n1) + e2 * n2;
            const int q0 = quantise(e0 - h * n0, rd, inv_r);
            const int q1 = quantise(e1 - h * n1, rd, inv_r);
            const int q2 = quantise(e2 - h * n2, rd, inv_r);
            const int dc = (int)__builtin_rint(((double)ic[u] - Ii) * CG_FIX);
            // |q| <= F + 2^7, |dc| <= F: the products fit 32 bits, the sums of fewer than 2^31 of them 64
            M.s00 += (long long)(q0 * q0);
            M.s01 += (long long)(q0 * q1);
            M.s02 += (long long)(q0 * q2);
            M.s11 += (long long)(q1 * q1);
            M.s12 += (long long)(q1 * q2);
            M.s22 += (long long)(q2 * q2);
            M.t0 += (long long)(q0 * dc);
            M.t1 += (long long)(q1 * dc);
            M.t2 += (long long)(q2 * dc);
          }
        }
      }
    }
  }
  long long w[COLOR_SUMS] = {M.m, M.s00, M.s01, M.s02, M.s11, M.s12, M.s22, M.t0, M.t1, M.t2};
#pragma unroll
  for (int k = 0; k < COLOR_SUMS; ++k) w[k] = sum_over_point(w[k]);
  if (!live) return;
  // the point's lanes store its ten words side by side: lane k word k, lanes 0 and 1 also words 8 and 9
  long long* const out = a.sums + (size_t)orig * COLOR_SUMS;
  long long mine = w[0], late = w[CG_S];
#pragma unroll
  for (int k = 1; k < CG_S; ++k) mine = slice == k ? w[k] : mine;
  late = slice == 1 ? w[CG_S + 1] : late;
  out[slice] = mine;
  if (slice < COLOR_SUMS - CG_S) out[CG_S + slice] = late;
}
static_assert(CG_S == 8 && COLOR_SUMS == 10, "the store above deals ten words to eight lanes");

__global__ __launch_bounds__(CG_BLOCK) void color_gradient_solve_kernel(const ColorGradArgs a) {
  const int i = blockIdx.x * CG_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const long long* const S = a.sums + (size_t)i * COLOR_SUMS;
  const long long m = S[0];
  const double n0 = a.nx[i], n1 = a.ny[i], n2 = a.nz[i];
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
  const bool usable = nn >= 1.0 - 0x1p-10 && nn <= 1.0 + 0x1p-10;
  const double w = (double)m * CG_FIX, w2 = w * w;
  const double H00 = (double)S[1] + (w2 * n0) * n0;
  const double H01 = (double)S[2] + (w2 * n0) * n1;
  const double H02 = (double)S[3] + (w2 * n0) * n2;
  const double H11 = (double)S[4] + (w2 * n1) * n1;
  const double H12 = (double)S[5] + (w2 * n1) * n2;
  const double H22 = (double)S[6] + (w2 * n2) * n2;
  const double T0 = (double)S[7], T1 = (double)S[8], T2 = (double)S[9];
  // adjugate and determinant, K14's association
  const double K00 = H11 * H22 - H12 * H12;
  const double K01 = H02 * H12 - H01 * H22;
  const double K02 = H01 * H12 - H02 * H11;
  const double K11 = H00 * H22 - H02 * H02;
  const double K12 = H01 * H02 - H00 * H12;
  const double K22 = H00 * H11 - H01 * H01;
  const double det = (H00 * K00 + H01 * K01) + H02 * K02;
  const double inv = 1.0 / det;
  const double rd = (double)a.radius;
  const float g0 = (float)((((K00 * T0 + K01 * T1) + K02 * T2) * inv) / rd);
  const float g1 = (float)((((K01 * T0 + K11 * T1) + K12 * T2) * inv) / rd);
  const float g2 = (float)((((K02 * T0 + K12 * T1) + K22 * T2) * inv) / rd);
  const bool ok = m >= (long long)a.min_neighbors && usable && det > 0.0 && det < __builtin_inf() &&
                  __builtin_isfinite(g0) && __builtin_isfinite(g1) && __builtin_isfinite(g2);
  a.gx[i] = ok ? g0 : 0.f;
  a.gy[i] = ok ? g1 : 0.f;
  a.gz[i] = ok ? g2 : 0.f;
}

__global__ __launch_bounds__(RED_THREADS) void colored_reduce_kernel(
    const nn_key_t* __restrict__ best, const float* __restrict__ ax, const float* __restrict__ ay,
    const float* __restrict__ az, int nq, const float* __restrict__ tx, const float* __restrict__ ty,
    const float* __restrict__ tz, const ColoredArgs g, const float4* __restrict__ rec, float max_dist,
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
  if (st) {
    if (st->done | st->stop_after_transform) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st->sweeps += 1;
  }
  const double lg = (double)g.lambda_geometric, lc = 1.0 - lg;
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
      const double n0 = g.tnx[j], n1 = g.tny[j], n2 = g.tnz[j];
      if (!(n0 == 0.0 && n1 == 0.0 && n2 == 0.0)) {
        const double g0 = g.gx[j], g1 = g.gy[j], g2 = g.gz[j];
        const double It = g.tcol[j], Is = g.scol[i];
        if (!rec) q0f = tx[j], q1f = ty[j], q2f = tz[j];
        const double p0 = p0f, p1 = p1f, p2 = p2f;
        const double e0 = p0 - (double)q0f, e1 = p1 - (double)q1f, e2 = p2 - (double)q2f;
        const double h = (e0 * n0 + e1 * n1) + e2 * n2;
        double JG[6], JC[6];
        JG[0] = p1 * n2 - p2 * n1;
        JG[1] = p2 * n0 - p0 * n2;
        JG[2] = p0 * n1 - p1 * n0;
        JG[3] = n0;
        JG[4] = n1;
        JG[5] = n2;
        const double u0 = e0 - h * n0, u1 = e1 - h * n1, u2 = e2 - h * n2;
        const double rc = (It + ((g0 * u0 + g1 * u1) + g2 * u2)) - Is;
        const double gn = (g0 * n0 + g1 * n1) + g2 * n2;
        const double M0 = g0 - gn * n0, M1 = g1 - gn * n1, M2 = g2 - gn * n2;
        JC[0] = p1 * M2 - p2 * M1;
        JC[1] = p2 * M0 - p0 * M2;
        JC[2] = p0 * M1 - p1 * M0;
        JC[3] = M0;
        JC[4] = M1;
        JC[5] = M2;
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[k++] += lg * (JG[a] * JG[b]) + lc * (JC[a] * JC[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] += lg * (JG[a] * h) + lc * (JC[a] * rc);
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

}  // namespace

void launch_color_gradients(const ColorGradArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const unsigned point_blocks = (unsigned)((a.n + CG_BLOCK - 1) / CG_BLOCK);
  const unsigned lanes_blocks = (unsigned)(((size_t)a.n * CG_S + CG_BLOCK - 1) / CG_BLOCK);
  hipLaunchKernelGGL(color_gather_kernel, dim3(point_blocks), dim3(CG_BLOCK), 0, s, a.t4, a.col, a.n, a.col_sorted);
  hipLaunchKernelGGL(color_gradient_sums_kernel, dim3(lanes_blocks), dim3(CG_BLOCK), 0, s, a);
  hipLaunchKernelGGL(color_gradient_solve_kernel, dim3(point_blocks), dim3(CG_BLOCK), 0, s, a);
}

void launch_colored_reduce(const nn_key_t* best, const float* ax, const float* ay, const float* az, int nq,
                           const float* tx, const float* ty, const float* tz, const ColoredArgs& g, const float4* rec,
                           float max_dist, int32_t* idx_out, float* dist_out, double* partial, int* pcount, double* out,
                           LoopState* st, hipStream_t s) {
  const int B = red_blocks(nq);
  hipLaunchKernelGGL(colored_reduce_kernel, dim3(B), dim3(RED_THREADS), 0, s, best, ax, ay, az, nq, tx, ty, tz, g, rec,
                     max_dist, idx_out, dist_out, partial, pcount, st);
  if (out) launch_reduce_final(partial, pcount, B, NP2L, out, s);
}

}  // namespace icpk
