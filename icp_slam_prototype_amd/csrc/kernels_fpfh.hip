// kernels_fpfh.hip -- K16: FPFH descriptors of a cloud and their matching (icpk_compute_fpfh, icpk_match_features; the
// rule is spelled out in include/icpk.h and restated in tests/fpfh_model.py).
//
//   1. fpfh_prep_kernel   the cloud's normals into the cell order of K1d's index, next to the points the walks read,
//                         with the "described" flag of every point in w.
//   2. fpfh_spfh_kernel   stage 1, the hot path: K12's walk (FP_S adjacent lanes per point share the (y, z) rows of the
//                         cube [p - rr, p + rr], every row one contiguous range of the sorted copy).  Every accepted
//                         pair is binned three times; the 33 counters and m of a point live in LDS and are bumped with
//                         integer LDS atomics by the point's lanes -- no dynamically indexed registers, hence no scratch,
//                         and integer sums do not depend on the order of arrival.  The point's lanes then store the
//                         normalised 16-bit SPFH (g) at the point's position in cell order, where stage 2 gathers it.
//   3. fpfh_final_kernel  stage 2: the same walk; per neighbour 68 bytes of g (17 dwords), 33 int64 accumulators per lane
//                         in statically indexed registers, a butterfly over the point's lanes; the point's first lane
//                         then runs the float64 tail of the rule and stores (the other lanes leave before it).
//   4. match_kernel       brute force: one searching descriptor per lane (33 floats in registers), the searched side
//                         streamed through LDS in tiles of MT_TILE descriptors that every lane reads at the same
//                         address (a broadcast); the searched side is cut into blockIdx.y chunks whose results meet in
//                         a 64-bit unsigned minimum of (bits(D) << 32) | index -- a minimum over distinct keys, whatever
//                         the order.
//   5. match_compact_kernel  the kept pairs in source order (one workgroup: a ballot scan per 1024 sources).
#include "fpfh_table.h"
#include "grid_walk.h"
#include "icpk_internal.h"

namespace icpk {

namespace {

constexpr int FP_S = 8;  // lanes per point (as K12, K13, K15)
constexpr int FP_BLOCK = 256;
constexpr int FP_PTS = FP_BLOCK / FP_S;
constexpr int FP_UNROLL = 2;  // candidates per lane and round trip
constexpr int FP_CNT = FPFH_BINS + 1;  // LDS words per point: the bins, then m

__global__ __launch_bounds__(FP_BLOCK) void fpfh_prep_kernel(const FpfhArgs a) {
  const int ip = blockIdx.x * FP_BLOCK + threadIdx.x;
  if (ip >= a.n) return;
  const float4 p = a.index.t4[ip];
  const int i = __float_as_int(p.w);
  const float nx = a.nx[i], ny = a.ny[i], nz = a.nz[i];
  const bool described = finite3(p.x, p.y, p.z) && finite3(nx, ny, nz) && !(nx == 0.f && ny == 0.f && nz == 0.f);
  a.n4[ip] = make_float4(nx, ny, nz, described ? 1.f : 0.f);
}

// bin of a feature in [-1, 1]: clamp((int)floor(11 ((f + 1) / 2)), 0, 10); NaN: 0
__device__ __forceinline__ int bin11(double f) {
  const double t = __builtin_floor(11.0 * ((f + 1.0) * 0.5));
  return t >= 10.0 ? 10 : (t >= 1.0 ? (int)t : 0);
}

__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return (x0 * y0 + x1 * y1) + x2 * y2;
}

// one candidate of stage 1: i the walking point (normal ni), j the candidate (point cj, normal nj); cnt: the 34 LDS
// words of point i
__device__ __forceinline__ void spfh_pair(int* cnt, float px, float py, float pz, const float4 ni, const float4 cj,
                                          const float4 nj, bool in_range, float r) {
  const float d = pair_dist(px, py, pz, cj.x, cj.y, cj.z);
  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
  if (!(in_range && d > 0.f && d <= r && nj.w != 0.f)) return;
  double d0 = (double)cj.x - (double)px, d1 = (double)cj.y - (double)py, d2 = (double)cj.z - (double)pz;
  const double f4 = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  if (f4 == 0.0) return;
  const double a1 = dot3(ni.x, ni.y, ni.z, d0, d1, d2) / f4;
  const double a2 = dot3(nj.x, nj.y, nj.z, d0, d1, d2) / f4;
  const bool sw = __builtin_fabs(a1) < __builtin_fabs(a2);
  const double n10 = sw ? nj.x : ni.x, n11 = sw ? nj.y : ni.y, n12 = sw ? nj.z : ni.z;
  const double n20 = sw ? ni.x : nj.x, n21 = sw ? ni.y : nj.y, n22 = sw ? ni.z : nj.z;
  if (sw) d0 = -d0, d1 = -d1, d2 = -d2;
  const double f3 = sw ? -a2 : a1;
  double v0 = d1 * n12 - d2 * n11, v1 = d2 * n10 - d0 * n12, v2 = d0 * n11 - d1 * n10;  // v = dp x n1
  const double vn = __builtin_sqrt(dot3(v0, v1, v2, v0, v1, v2));
  if (vn == 0.0) return;
  v0 = v0 / vn, v1 = v1 / vn, v2 = v2 / vn;
  const double w0 = n11 * v2 - n12 * v1, w1 = n12 * v0 - n10 * v2, w2 = n10 * v1 - n11 * v0;  // w = n1 x v
  const double f2 = dot3(v0, v1, v2, n20, n21, n22);
  const double sa = dot3(w0, w1, w2, n20, n21, n22);
  const double sb = dot3(n10, n11, n12, n20, n21, n22);
  // the sector of atan2(sa, sb) among 11 of [-pi, pi], by the signs of e_k = C_k sa - S_k sb (no libm)
  int b1 = 5;
  if (sa == 0.0 && sb == 0.0) {
  } else if (sa >= 0.0) {
#pragma unroll
    for (int k = 6; k <= 10; ++k) b1 += (FPFH_CS[k - 1][0] * sa - FPFH_CS[k - 1][1] * sb) >= 0.0 ? 1 : 0;
  } else {
#pragma unroll
    for (int k = 1; k <= 5; ++k) b1 -= (FPFH_CS[k - 1][0] * sa - FPFH_CS[k - 1][1] * sb) < 0.0 ? 1 : 0;
  }
  atomicAdd(&cnt[b1], 1);
  atomicAdd(&cnt[11 + bin11(f2)], 1);
  atomicAdd(&cnt[22 + bin11(f3)], 1);
  atomicAdd(&cnt[FPFH_BINS], 1);
}

__global__ __launch_bounds__(FP_BLOCK) void fpfh_spfh_kernel(const FpfhArgs a) {
  __shared__ int cnt[FP_PTS][FP_CNT];
  for (int e = threadIdx.x; e < FP_PTS * FP_CNT; e += FP_BLOCK) (&cnt[0][0])[e] = 0;
  __syncthreads();
  const int slice = threadIdx.x & (FP_S - 1), lp = threadIdx.x / FP_S;
  const int ip = (int)((blockIdx.x * (unsigned)FP_BLOCK + threadIdx.x) / FP_S);  // position in cell order
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 ni = live ? a.n4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z, r = a.radius;
  const bool scan = live && ni.w != 0.f;  // only a described point counts pairs (described: finite, so is its cube)
  const Walk w = make_walk(g, px, py, pz, r, scan);
  struct Cand {
    float4 c, nj;
  };
  walk_candidates<FP_S, FP_UNROLL>(
      w, g, a.index.cell_start, slice, [&](int jj) { return Cand{a.index.t4[jj], a.n4[jj]}; },
      [&](const Cand& k, bool in_range) { spfh_pair(cnt[lp], px, py, pz, ni, k.c, k.nj, in_range, r); });
  __syncthreads();
  if (!live) return;
  const int i = __float_as_int(p4.w);
  const int m = cnt[lp][FPFH_BINS];
  unsigned short* const g16 = a.g + (size_t)ip * FPFH_G_STRIDE;
  for (int b = slice; b < FP_CNT; b += FP_S) {
    const int c = cnt[lp][b];
    // g = (c * 32768) / m, an integer quotient <= 32768; word 33: the point has an SPFH (m > 0)
    g16[b] = b == FPFH_BINS ? (unsigned short)(m > 0) : (unsigned short)(m > 0 ? (c * 32768ll) / m : 0);
    if (a.counts && b < FPFH_BINS) a.counts[(size_t)i * FPFH_BINS + b] = c;
    if (a.m && b == FPFH_BINS) a.m[i] = m;
  }
}

__global__ __launch_bounds__(FP_BLOCK) void fpfh_final_kernel(const FpfhArgs a) {
  const int slice = threadIdx.x & (FP_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)FP_BLOCK + threadIdx.x) / FP_S);
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const unsigned* const gi32 = reinterpret_cast<const unsigned*>(a.g + (size_t)(live ? ip : 0) * FPFH_G_STRIDE);
  const bool valid = live && a.n > 0 && (gi32[FPFH_BINS / 2] >> 16) != 0;  // described and m > 0
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z, r = a.radius;
  const double rr = (double)r * (double)r;
  // the rule walks for every described i; a described point with m_i == 0 gets 33 zeros whatever its walk finds, so
  // only valid points walk
  const Walk w = make_walk(g, px, py, pz, r, valid);
  long long A[FPFH_BINS + 1];  // (the odd half of the last dword is the flag: its sum is not used)
#pragma unroll
  for (int b = 0; b <= FPFH_BINS; ++b) A[b] = 0;
  long long Q = 0;
  // (one candidate at a time: its 68 bytes of g are gathered only if it is a neighbour)
  struct Cand {
    float4 c;
    int j;
  };
  walk_candidates<FP_S, 1>(
      w, g, a.index.cell_start, slice, [&](int j) { return Cand{a.index.t4[j], j}; },
      [&](const Cand& k, bool) {
        const float d = pair_dist(px, py, pz, k.c.x, k.c.y, k.c.z);
        if (!(d > 0.f && d <= r)) return;
        const unsigned* const gj = reinterpret_cast<const unsigned*>(a.g + (size_t)k.j * FPFH_G_STRIDE);
        unsigned v[FPFH_G_STRIDE / 2];
#pragma unroll
        for (int e = 0; e < FPFH_G_STRIDE / 2; ++e) v[e] = gj[e];
        if ((v[FPFH_BINS / 2] >> 16) == 0) return;  // m_j == 0
        const double u = rr / ((double)d * (double)d);
        const long long q = (long long)__builtin_rint(__builtin_fmin(u, 16384.0) * 1024.0);
#pragma unroll
        for (int e = 0; e < FPFH_G_STRIDE / 2; ++e) {
          A[2 * e] += q * (long long)(v[e] & 0xffffu);
          A[2 * e + 1] += q * (long long)(v[e] >> 16);
        }
        Q += q;
      });
#pragma unroll
  for (int b = 0; b < FPFH_BINS; ++b) A[b] = sum_over_point<FP_S>(A[b]);
  Q = sum_over_point<FP_S>(Q);
  if (!live || slice != 0) return;
  const int i = __float_as_int(p4.w);
  float* const out = a.desc + (size_t)i * FPFH_BINS;
  a.valid[i] = valid ? 1 : 0;
  double raw[FPFH_BINS];
#pragma unroll
  for (int b = 0; b < FPFH_BINS; ++b) {
    const unsigned word = gi32[b / 2];
    const double gi = (double)((b & 1) ? (word >> 16) : (word & 0xffffu));
    raw[b] = gi + (Q > 0 ? (double)A[b] / (double)Q : 0.0);
  }
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    double tot = raw[11 * h];
#pragma unroll
    for (int b = 1; b < 11; ++b) tot += raw[11 * h + b];
#pragma unroll
    for (int b = 0; b < 11; ++b) out[11 * h + b] = valid && tot > 0.0 ? (float)((100.0 * raw[11 * h + b]) / tot) : 0.f;
  }
}
static_assert(FPFH_G_STRIDE == FPFH_BINS + 1 && FPFH_BINS % 2 == 1, "the flag is the upper half of the last dword");

// ---- matching -------------------------------------------------------------------------------------------------------
constexpr int MT_BLOCK = 256;
constexpr int MT_TILE = 64;          // searched descriptors per LDS tile (8.25 KiB)
constexpr int MT_AIM_BLOCKS = 2048;  // workgroups a launch aims at when it cuts the searched side into chunks

__global__ __launch_bounds__(MT_BLOCK) void match_kernel(const MatchArgs a, int chunk) {
  __shared__ float tile[MT_TILE * FPFH_BINS];
  __shared__ int tv[MT_TILE];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * MT_BLOCK + tid;
  const bool live = i < a.na && a.va[i] != 0;
  float f[FPFH_BINS];
#pragma unroll
  for (int b = 0; b < FPFH_BINS; ++b) f[b] = live ? a.fa[(size_t)i * FPFH_BINS + b] : 0.f;
  const int j0 = blockIdx.y * chunk;
  const int j1 = min(a.nb, j0 + chunk);
  nn_key_t best = NN_KEY_INIT;
  for (int jt = j0; jt < j1; jt += MT_TILE) {
    const int cnt = min(MT_TILE, j1 - jt);
    __syncthreads();
    for (int e = tid; e < cnt * FPFH_BINS; e += MT_BLOCK) tile[e] = a.fb[(size_t)jt * FPFH_BINS + e];
    if (tid < cnt) tv[tid] = a.vb[jt + tid];
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
      if (!tv[t]) continue;  // (uniform)
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < FPFH_BINS; ++b) {
        const double dd = (double)f[b] - (double)tile[t * FPFH_BINS + b];
        s += dd * dd;
      }
      const nn_key_t key = ((nn_key_t)__float_as_uint((float)s) << 32) | (unsigned)(jt + t);
      best = key < best ? key : best;
    }
  }
  if (live && best != NN_KEY_INIT) atomicMin(&a.best[i], best);
}

constexpr int MC_BLOCK = 1024;

__global__ __launch_bounds__(MC_BLOCK) void match_compact_kernel(const nn_key_t* __restrict__ best_s, int ns,
                                                                 const nn_key_t* __restrict__ best_t, int mutual,
                                                                 int* __restrict__ msrc, int* __restrict__ mtgt,
                                                                 float* __restrict__ mD, int* __restrict__ n_out) {
  __shared__ int wsum[MC_BLOCK / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int base = 0;  // (the same on every lane)
  for (int i0 = 0; i0 < ns; i0 += MC_BLOCK) {
    const int i = i0 + tid;
    const nn_key_t key = i < ns ? best_s[i] : NN_KEY_INIT;
    bool keep = key != NN_KEY_INIT;
    const unsigned j = (unsigned)(key & 0xffffffffu);
    if (keep && mutual) keep = (unsigned)(best_t[j] & 0xffffffffu) == (unsigned)i;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
    const int before = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[wave] = __builtin_popcountll(mask);
    __syncthreads();
    int off = base, total = 0;
    for (int k = 0; k < MC_BLOCK / 64; ++k) {
      off += k < wave ? wsum[k] : 0;
      total += wsum[k];
    }
    if (keep) {  // base + total <= i0 + MC_BLOCK and off + before < base + total: inside the ns entries
      msrc[off + before] = i;
      mtgt[off + before] = (int)j;
      mD[off + before] = __uint_as_float((unsigned)(key >> 32));
    }
    base += total;
  }
  if (tid == 0) *n_out = base;
}

}  // namespace

void launch_compute_fpfh(const FpfhArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(fpfh_prep_kernel, dim3((a.n + FP_BLOCK - 1) / FP_BLOCK), dim3(FP_BLOCK), 0, s, a);
  const unsigned blocks = (unsigned)(((size_t)a.n * FP_S + FP_BLOCK - 1) / FP_BLOCK);
  hipLaunchKernelGGL(fpfh_spfh_kernel, dim3(blocks), dim3(FP_BLOCK), 0, s, a);
  hipLaunchKernelGGL(fpfh_final_kernel, dim3(blocks), dim3(FP_BLOCK), 0, s, a);
}

void launch_match_features(const MatchArgs& a, hipStream_t s) {
  if (a.na <= 0 || a.nb <= 0) return;
  const int gx = (a.na + MT_BLOCK - 1) / MT_BLOCK;
  const int tiles = (a.nb + MT_TILE - 1) / MT_TILE;
  int gy = MT_AIM_BLOCKS / gx;
  gy = gy < 1 ? 1 : (gy > tiles ? tiles : gy);
  const int chunk = ((tiles + gy - 1) / gy) * MT_TILE;  // gy chunks of whole tiles cover nb
  gy = (a.nb + chunk - 1) / chunk;
  hipLaunchKernelGGL(match_kernel, dim3(gx, gy), dim3(MT_BLOCK), 0, s, a, chunk);
}

void launch_match_compact(const nn_key_t* best_s, int ns, const nn_key_t* best_t, int mutual, int* msrc, int* mtgt,
                          float* mD, int* n_out, hipStream_t s) {
  hipLaunchKernelGGL(match_compact_kernel, dim3(1), dim3(MC_BLOCK), 0, s, best_s, ns, best_t, mutual, msrc, mtgt, mD, n_out);
}

}  // namespace icpk
