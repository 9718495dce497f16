// kernels_fern.hip -- K27: fern keyframe codes on the device (include/icpk.h, THE FERN RULE; the rule itself is
// csrc/fern_rule.h, shared with the host functions).  Integers only, no atomic.
//   fern_encode_kernel  one workgroup, a lane per fern: one gather from the resident level, four compares, the eight
//                       nibbles of a word OR-combined inside their row of 16 lanes by three DPP stages; V from the
//                       waves' ballots.  The block is the ferns rounded up to whole waves, so every DPP source lane is
//                       live; a lane past F carries nibble 0 and stores nothing.
//   fern_search_kernel  a thread per keyframe over the transposed database (word w of keyframe k at w * capacity + k:
//                       a wave's loads of one word are consecutive), the query words in LDS; each workgroup leaves its
//                       FERN_TOPK smallest keys diss << 16 | index in ascending order.
//   fern_merge_kernel   one workgroup merges the workgroups' lists into the answer.
//   fern_append_kernel  the current code into column n.
// A key is unique (it carries its index), so "remove the winner" is "the thread that holds the minimum drops it".
#include "fern_rule.h"
#include "icpk.h"
#include "icpk_internal.h"
#include "wave_sum.h"

namespace icpk {

static_assert(FERN_TOPK == ICPK_FERN_MAX_K, "the lists hold what a query may ask for");

// the smallest key of the wave in every lane: four in-row DPP stages, then the two cross-row exchanges
__device__ __forceinline__ uint32_t fern_wave_min(uint32_t v) {
  v = min(v, (uint32_t)xor_lane<1>((int)v));
  v = min(v, (uint32_t)xor_lane<2>((int)v));
  v = min(v, (uint32_t)xor_lane<4>((int)v));
  v = min(v, (uint32_t)xor_lane<8>((int)v));
  v = min(v, (uint32_t)xor_lane<16>((int)v));
  v = min(v, (uint32_t)xor_lane<32>((int)v));
  return v;
}

// The FERN_TOPK smallest of the workgroup's keys (NT threads, one candidate at a time per thread: `next` hands a thread
// its following key once its current one has won), ascending, into out[0 .. FERN_TOPK) by thread 0.  wmin: NT / 64 words
// of LDS per parity.
template <int NT, class Next>
__device__ __forceinline__ void fern_block_topk(uint32_t key, Next next, uint32_t (*wmin)[NT / 64], uint32_t* out) {
  const int t = threadIdx.x, wave = t >> 6;
  for (int r = 0; r < FERN_TOPK; ++r) {
    const uint32_t m = fern_wave_min(key);
    if ((t & 63) == 0) wmin[r & 1][wave] = m;
    __syncthreads();  // (the other parity's words are not written again before the barrier of round r + 1)
    uint32_t best = wmin[r & 1][0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) best = min(best, wmin[r & 1][w]);
    if (t == 0) out[r] = best;
    if (key == best && best != FERN_NO_KEY) key = next();
  }
}

__global__ __launch_bounds__(FERN_MAX_F) void fern_encode_kernel(const uint16_t* __restrict__ level, int cols,
                                                                  const int32_t* __restrict__ table, int F,
                                                                  uint32_t* __restrict__ code) {
  __shared__ int wvalid[FERN_MAX_F / 64];
  const int f = threadIdx.x;
  uint32_t nib = 0;
  bool valid = false;
  if (f < F) {
    const int32_t* e = table + (size_t)f * FERN_ENTRY;
    const int d = level[(size_t)e[0] * cols + e[1]];  // (the table's pixel lies inside the level it was drawn for)
    valid = d != 0;
    nib = fern_nibble(d, e + 2) << (4 * (f & 7));
  }
  int v = (int)nib;
  v |= xor_lane<1>(v);
  v |= xor_lane<2>(v);
  v |= xor_lane<4>(v);
  if (f < F && (f & 7) == 0) code[f >> 3] = (uint32_t)v;
  const int nv = __popcll(__ballot(valid));
  if ((f & 63) == 0) wvalid[f >> 6] = nv;
  __syncthreads();
  if (f == 0) {
    int V = 0;
    for (int w = 0; w < (int)blockDim.x / 64; ++w) V += wvalid[w];
    code[F / 8] = (uint32_t)V;  // the word behind the code
  }
}

__global__ __launch_bounds__(FERN_SEARCH_THREADS) void fern_search_kernel(const uint32_t* __restrict__ db, int capacity,
                                                                           int n, const uint32_t* __restrict__ code,
                                                                           int W, uint32_t* __restrict__ lists) {
  __shared__ uint32_t q[FERN_MAX_F / 8];
  __shared__ uint32_t wmin[2][FERN_SEARCH_THREADS / 64];
  const int t = threadIdx.x;
  for (int w = t; w < W; w += FERN_SEARCH_THREADS) q[w] = code[w];
  __syncthreads();
  const int k = blockIdx.x * FERN_SEARCH_THREADS + t;
  uint32_t key = FERN_NO_KEY;
  if (k < n) {
    int diss = 0;
    for (int w = 0; w < W; ++w) diss += fern_word_diss(db[(size_t)w * capacity + k], q[w]);
    key = fern_key(diss, k);
  }
  fern_block_topk<FERN_SEARCH_THREADS>(key, [] { return FERN_NO_KEY; }, wmin, lists + (size_t)blockIdx.x * FERN_TOPK);
}

// n_lists * FERN_TOPK <= FERN_SEARCH_THREADS * FERN_TOPK keys: a thread holds FERN_TOPK of them, smallest first is not
// needed -- it offers its own minimum and moves on to the next smallest when that one has won
__global__ __launch_bounds__(FERN_SEARCH_THREADS) void fern_merge_kernel(const uint32_t* __restrict__ lists, int n_keys,
                                                                          uint32_t* __restrict__ out) {
  __shared__ uint32_t wmin[2][FERN_SEARCH_THREADS / 64];
  const int t = threadIdx.x;
  uint32_t mine[FERN_TOPK];
#pragma unroll
  for (int j = 0; j < FERN_TOPK; ++j) {
    const int i = t + j * FERN_SEARCH_THREADS;
    mine[j] = i < n_keys ? lists[i] : FERN_NO_KEY;
  }
  auto take = [&mine]() {  // the smallest key this thread still holds, removed from its set
    uint32_t m = mine[0];
    int at = 0;
#pragma unroll
    for (int j = 1; j < FERN_TOPK; ++j)
      if (mine[j] < m) m = mine[j], at = j;
#pragma unroll
    for (int j = 0; j < FERN_TOPK; ++j)
      if (j == at) mine[j] = FERN_NO_KEY;
    return m;
  };
  fern_block_topk<FERN_SEARCH_THREADS>(take(), take, wmin, out);
}

__global__ void fern_append_kernel(uint32_t* __restrict__ db, int capacity, int column, const uint32_t* __restrict__ code,
                                   int W) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) db[(size_t)w * capacity + column] = code[w];
}

void launch_fern_encode(const uint16_t* level, int cols, const int32_t* table, int F, uint32_t* code, hipStream_t s) {
  hipLaunchKernelGGL(fern_encode_kernel, dim3(1), dim3((unsigned)((F + 63) / 64 * 64)), 0, s, level, cols, table, F, code);
}

void launch_fern_search(const uint32_t* db, int capacity, int n, const uint32_t* code, int W, uint32_t* lists, uint32_t* out,
                        hipStream_t s) {
  if (n <= 0) return;
  const int blocks = (n + FERN_SEARCH_THREADS - 1) / FERN_SEARCH_THREADS;  // <= 65536 / 256: the merge holds them all
  hipLaunchKernelGGL(fern_search_kernel, dim3((unsigned)blocks), dim3(FERN_SEARCH_THREADS), 0, s, db, capacity, n, code, W,
                     lists);
  hipLaunchKernelGGL(fern_merge_kernel, dim3(1), dim3(FERN_SEARCH_THREADS), 0, s, lists, blocks * FERN_TOPK, out);
}

void launch_fern_append(uint32_t* db, int capacity, int column, const uint32_t* code, int W, hipStream_t s) {
  hipLaunchKernelGGL(fern_append_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, db, capacity, column, code, W);
}

}  // namespace icpk
