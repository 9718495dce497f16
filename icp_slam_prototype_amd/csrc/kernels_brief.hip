// kernels_brief.hip -- K32: oriented BRIEF descriptors of key points and their exact Hamming matches.  The rule is
// brief_rule.h (THE BRIEF RULE and THE MATCH RULE of include/icpk.h); everything here is integer work, no atomics.
//   brief_describe  a wave per key point, four per workgroup: the 31 x 31 grey window into LDS (BGR -> grey on the way),
//                   the 27 x 27 box sums into LDS as uint16, the two moments by the wave's butterfly, the bin, and four
//                   tests per lane whose four 64-bit ballots are the eight words                         1 launch
//   brief_match     a thread per descriptor of side a, side b going by in LDS tiles of 256; grid.y splits b into runs of
//                   BRIEF_MATCH_CHUNK whose records (H, j, H2) go to slots of their own                  1 launch (2: mutual)
//   brief_finish    one workgroup: the runs' records merged in run order, the three conditions, and the kept pairs
//                   (and, for K16's list, those with two cloud points) scattered in source order         1 launch
// The grey window is 31 x 31 and the box sums 27 x 27, not the 35 x 35 and 31 x 31 a reach of 17 would need: offsets end
// at 13 and the box adds 2, which is the rule's B = 15.
#include "block_scan.h"
#include "brief_rule.h"
#include "icpk.h"
#include "icpk_internal.h"
#include "wave_sum.h"

namespace icpk {

constexpr int BD_THREADS = 256, BD_WAVES = BD_THREADS / 64;
constexpr int BM_THREADS = 256;
constexpr int BF_THREADS = 1024;

// the sum of v over the wave64, in every lane (integers: the order does not show)
__device__ __forceinline__ int wave_total(int v) {
  v = add_xor_swap<32>(v);
  v = add_xor_swap<16>(v);
  v += xor_lane<8>(v);
  v += xor_lane<4>(v);
  v += xor_lane<2>(v);
  v += xor_lane<1>(v);
  return v;
}

__global__ __launch_bounds__(BD_THREADS) void brief_describe_kernel(const uint8_t* __restrict__ img, int rows, int cols,
                                                                    int channels, const float* __restrict__ kp, int n,
                                                                    int upright, const int8_t* __restrict__ table,
                                                                    uint32_t* __restrict__ words, uint8_t* __restrict__ bin,
                                                                    uint8_t* __restrict__ valid) {
  __shared__ uint8_t g[BD_WAVES][BRIEF_GW][BRIEF_GW + 1];
  __shared__ uint16_t S[BD_WAVES][BRIEF_SW][BRIEF_SW + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * BD_WAVES + wave;
  const bool live = k < n;  // (a wave past the list takes the barriers and does nothing else)
  int xi = -1, yi = -1;
  if (live) {
    xi = brief_coord(kp[2 * k], BRIEF_B, cols - BRIEF_B);
    yi = brief_coord(kp[2 * k + 1], BRIEF_B, rows - BRIEF_B);
  }
  const bool ok = xi >= 0 && yi >= 0;  // the whole window lies inside the image
  if (ok)
    for (int i = lane; i < BRIEF_GW * BRIEF_GW; i += 64) {
      const int ly = i / BRIEF_GW, lx = i - ly * BRIEF_GW;
      g[wave][ly][lx] = (uint8_t)brief_pixel(img, cols, channels, xi - BRIEF_B + lx, yi - BRIEF_B + ly);
    }
  __syncthreads();
  int m10 = 0, m01 = 0;
  if (ok) {
    for (int i = lane; i < BRIEF_SW * BRIEF_SW; i += 64) {  // S[sy][sx] = the box around offset (sx - 13, sy - 13)
      const int sy = i / BRIEF_SW, sx = i - sy * BRIEF_SW;
      int s = 0;
#pragma unroll
      for (int dy = 0; dy <= 2 * BRIEF_BOX; ++dy)
#pragma unroll
        for (int dx = 0; dx <= 2 * BRIEF_BOX; ++dx) s += g[wave][sy + dy][sx + dx];
      S[wave][sy][sx] = (uint16_t)s;  // <= 25 * 255
    }
    for (int i = lane; i < BRIEF_GW * BRIEF_GW; i += 64) {
      const int ly = i / BRIEF_GW, lx = i - ly * BRIEF_GW;
      const int dx = lx - BRIEF_B, dy = ly - BRIEF_B;
      if (dx * dx + dy * dy <= BRIEF_R2) {
        const int v = g[wave][ly][lx];
        m10 += dx * v;
        m01 += dy * v;
      }
    }
  }
  m10 = wave_total(m10);  // |m| < 2^22
  m01 = wave_total(m01);
  __syncthreads();
  const int b = ok && !upright ? brief_bin(m10, m01) : 0;
  const char4* tests = reinterpret_cast<const char4*>(table) + b * BRIEF_TESTS;
#pragma unroll
  for (int j = 0; j < BRIEF_TESTS / 64; ++j) {
    const char4 e = tests[64 * j + lane];  // (ax, ay, bx, by)
    const int ax = (signed char)e.x, ay = (signed char)e.y, bx = (signed char)e.z, by = (signed char)e.w;
    const bool bit = ok && S[wave][BRIEF_OFF + ay][BRIEF_OFF + ax] < S[wave][BRIEF_OFF + by][BRIEF_OFF + bx];
    const unsigned long long m = __ballot(bit);
    if (live && lane == 0) {
      words[(size_t)BRIEF_WORDS * k + 2 * j] = (uint32_t)m;
      words[(size_t)BRIEF_WORDS * k + 2 * j + 1] = (uint32_t)(m >> 32);
    }
  }
  if (live && lane == 0) {
    bin[k] = (uint8_t)b;
    valid[k] = ok ? 1 : 0;
  }
}

// the record of one run: (H << 32 | j) and H2; j = -1 (all ones) when the run holds no valid descriptor
__device__ __forceinline__ BriefBest brief_merged(const unsigned long long* __restrict__ key, const unsigned* __restrict__ h2,
                                                  int runs, int n, int i) {
  BriefBest best;
  for (int c = 0; c < runs; ++c) {
    const unsigned long long kk = key[(size_t)c * n + i];
    BriefBest o;
    o.H = (int)(kk >> 32), o.j = (int)(uint32_t)kk, o.H2 = (int)h2[(size_t)c * n + i];
    best.merge(o);
  }
  return best;
}

__global__ __launch_bounds__(BM_THREADS) void brief_match_kernel(const BriefSide a, const BriefSide b,
                                                                 unsigned long long* __restrict__ key,
                                                                 unsigned* __restrict__ h2) {
  __shared__ uint32_t tw[BM_THREADS][BRIEF_WORDS];
  __shared__ uint8_t tv[BM_THREADS];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * BM_THREADS + tid;
  uint32_t s[BRIEF_WORDS];
#pragma unroll
  for (int w = 0; w < BRIEF_WORDS; ++w) s[w] = i < a.n ? a.words[(size_t)BRIEF_WORDS * i + w] : 0u;
  BriefBest best;
  const int j0 = blockIdx.y * BRIEF_MATCH_CHUNK, j1 = min(b.n, j0 + BRIEF_MATCH_CHUNK);
  for (int base = j0; base < j1; base += BM_THREADS) {
    __syncthreads();  // (the tile before has been read)
    const int jt = base + tid;
    const bool in = jt < j1;
#pragma unroll
    for (int w = 0; w < BRIEF_WORDS; ++w) tw[tid][w] = in ? b.words[(size_t)BRIEF_WORDS * jt + w] : 0u;
    tv[tid] = in ? b.valid[jt] : 0;
    __syncthreads();
    const int cnt = min(BM_THREADS, j1 - base);
    for (int jj = 0; jj < cnt; ++jj) {
      if (!tv[jj]) continue;  // (the same for every thread)
      best.take(brief_hamming(s, tw[jj]), base + jj);
    }
  }
  if (i < a.n) {
    key[(size_t)blockIdx.y * a.n + i] = ((unsigned long long)(uint32_t)best.H << 32) | (uint32_t)best.j;
    h2[(size_t)blockIdx.y * a.n + i] = (unsigned)best.H2;
  }
}

__global__ __launch_bounds__(BF_THREADS) void brief_finish_kernel(const BriefFinishArgs a) {
  int off = 0, off2 = 0;
  for (int base = 0; base < a.ns; base += BF_THREADS) {
    const int i = base + (int)threadIdx.x;
    bool keep = false;
    BriefBest bs;
    if (i < a.ns && a.valid_s[i]) {
      bs = brief_merged(a.key[0], a.h2[0], a.runs[0], a.ns, i);
      keep = brief_keep(bs, a.max_hamming, a.ratio_num, a.ratio_den);
      if (keep && a.mutual) keep = brief_merged(a.key[1], a.h2[1], a.runs[1], a.nt, bs.j).j == i;
    }
    int cs = -1, ct = -1;
    if (keep && a.map_s) cs = a.map_s[i], ct = a.map_t[bs.j];
    const bool both = cs >= 0 && ct >= 0;
    int total, total2;
    const int r = block_excl_scan<BF_THREADS>(keep ? 1 : 0, &total);
    const int r2 = block_excl_scan<BF_THREADS>(both ? 1 : 0, &total2);
    if (keep) {
      a.out_src[off + r] = i;
      a.out_tgt[off + r] = bs.j;
      a.out_H[off + r] = bs.H;
      a.out_H2[off + r] = bs.H2;
    }
    if (both) {
      a.cl_src[off2 + r2] = cs;
      a.cl_tgt[off2 + r2] = ct;
      a.cl_D[off2 + r2] = (float)bs.H;
    }
    off += total;
    off2 += total2;
  }
  if (threadIdx.x == 0) {
    a.counts[0] = off;
    a.counts[1] = off2;
    if (a.cl_n) *a.cl_n = off2;
  }
}

void launch_brief_describe(const uint8_t* img, int rows, int cols, int channels, const float* kp, int n, int upright,
                           const int8_t* table, uint32_t* words, uint8_t* bin, uint8_t* valid, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(brief_describe_kernel, dim3((n + BD_WAVES - 1) / BD_WAVES), dim3(BD_THREADS), 0, s, img, rows, cols,
                     channels, kp, n, upright, table, words, bin, valid);
}

void launch_brief_match(const BriefSide& a, const BriefSide& b, unsigned long long* key, unsigned* h2, hipStream_t s) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(brief_match_kernel, dim3((a.n + BM_THREADS - 1) / BM_THREADS, brief_match_runs(b.n)), dim3(BM_THREADS), 0,
                     s, a, b, key, h2);
}

void launch_brief_finish(const BriefFinishArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(brief_finish_kernel, dim3(1), dim3(BF_THREADS), 0, s, a);
}

}  // namespace icpk
