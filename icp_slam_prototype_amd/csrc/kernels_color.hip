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
//   4. colored_reduce_kernel      the joint step on pair_reduce.h's scaffold (as K5 and K14): point-to-plane's
//                                 acceptance and geometric terms, and the photometric terms beside them in the same
//                                 28 sums.
// Built with -ffp-contract=off like every exact kernel here: no multiply and add below is fused.
#include "grid_walk.h"
#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {

namespace {

constexpr int CG_S = 8;  // lanes per point, as K12
constexpr int CG_BLOCK = 256;
constexpr int CG_UNROLL = 4;
constexpr double CG_FIX = 32768.0;  // F = 2^15

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

__global__ __launch_bounds__(CG_BLOCK) void color_gradient_sums_kernel(const ColorGradArgs a) {
  const int slice = threadIdx.x & (CG_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)CG_BLOCK + threadIdx.x) / CG_S);  // position in cell order
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int orig = live ? min(max(__float_as_int(p4.w), 0), a.n - 1) : 0;
  const GridInfo g = *a.index.gi;
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
  const Walk walk = make_walk(g, px, py, pz, r, scan);
  ColorSums M{};
  struct Cand {
    float4 c;
    float ic;
  };
  walk_candidates<CG_S, CG_UNROLL>(
      walk, g, a.index.cell_start, slice, [&](int jj) { return Cand{a.index.t4[jj], a.col_sorted[jj]}; },
      [&](const Cand& k, bool in_range) {
        const float4 c = k.c;
        const float d = pair_dist(px, py, pz, c.x, c.y, c.z);
        if (!(in_range && d <= r)) return;  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
        M.m += 1;
        if (!usable) return;
        const double e0 = (double)c.x - (double)px, e1 = (double)c.y - (double)py, e2 = (double)c.z - (double)pz;
        const double h = (e0 * n0 + e1 * n1) + e2 * n2;
        // (quantise: the product with fl(1 / r) where it provably rounds as the rule's quotient, |u / r| <= 1 + 2^-19)
        const int q0 = quantise(e0 - h * n0, rd, inv_r, CG_FIX);
        const int q1 = quantise(e1 - h * n1, rd, inv_r, CG_FIX);
        const int q2 = quantise(e2 - h * n2, rd, inv_r, CG_FIX);
        const int dc = (int)__builtin_rint(((double)k.ic - Ii) * CG_FIX);
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
      });
  long long w[COLOR_SUMS] = {M.m, M.s00, M.s01, M.s02, M.s11, M.s12, M.s22, M.t0, M.t1, M.t2};
#pragma unroll
  for (int k = 0; k < COLOR_SUMS; ++k) w[k] = sum_over_point<CG_S>(w[k]);
  if (!live) return;
  store_point_words<CG_S>(a.sums + (size_t)orig * COLOR_SUMS, slice, w);
}

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

__global__ __launch_bounds__(RED_THREADS) void colored_reduce_kernel(const PairArgs args, const ColoredArgs g) {
  constexpr int NS = NP2L;
  PairStream pairs(args, blockIdx.x, gridDim.x);
  if (!pairs.open()) return;
  const double lg = (double)g.lambda_geometric, lc = 1.0 - lg;
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  int cnt = 0;
  pairs.for_each([&](const auto& pr) {
    const int i = pr.i, j = pr.j;
    const double n0 = g.tnx[j], n1 = g.tny[j], n2 = g.tnz[j];
    if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) return;
    const double g0 = g.gx[j], g1 = g.gy[j], g2 = g.gz[j];
    const double It = g.tcol[j], Is = g.scol[i];
    float q0f, q1f, q2f;
    pr.match(q0f, q1f, q2f);
    const double p0 = pr.p0, p1 = pr.p1, p2 = pr.p2;
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
    v[27] += (double)pr.d;
    ++cnt;
  });
  block_partials<NS>(v, cnt, args.partial + blockIdx.x, RED_MAX_BLOCKS, args.pcount + blockIdx.x);
}

}  // namespace

void launch_color_gradients(const ColorGradArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const unsigned point_blocks = (unsigned)((a.n + CG_BLOCK - 1) / CG_BLOCK);
  const unsigned lanes_blocks = (unsigned)(((size_t)a.n * CG_S + CG_BLOCK - 1) / CG_BLOCK);
  hipLaunchKernelGGL(color_gather_kernel, dim3(point_blocks), dim3(CG_BLOCK), 0, s, a.index.t4, a.col, a.n, a.col_sorted);
  hipLaunchKernelGGL(color_gradient_sums_kernel, dim3(lanes_blocks), dim3(CG_BLOCK), 0, s, a);
  hipLaunchKernelGGL(color_gradient_solve_kernel, dim3(point_blocks), dim3(CG_BLOCK), 0, s, a);
}

void launch_colored_reduce(const PairArgs& a, const ColoredArgs& g, hipStream_t s) {
  const int B = red_blocks(a.nq);
  hipLaunchKernelGGL(colored_reduce_kernel, dim3(B), dim3(RED_THREADS), 0, s, a, g);
  if (a.out) launch_reduce_final(a.partial, a.pcount, B, NP2L, a.out, s);
}

}  // namespace icpk
