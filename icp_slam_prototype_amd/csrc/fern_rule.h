// fern_rule.h -- the fern rule (K27) stated once; include/icpk.h writes it out ("THE FERN RULE").
// Header-inline and __host__ __device__: kernels_fern.hip runs the nibble and the dissimilarity on the device,
// icpk_fern.cpp builds the table and runs the whole rule over host levels (icpk_fern_table, icpk_fern_encode_host,
// icpk_fern_dissimilarity_host).  Integers only: a code is a function of the level and the parameters alone, and a
// search's answer a function of the codes alone.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef ICPK_HD
#define ICPK_HD __host__ __device__ inline
#endif
#else
#ifndef ICPK_HD
#define ICPK_HD inline
#endif
#endif
#include <stdint.h>

namespace icpk {

constexpr int FERN_ENTRY = 6;                // int32 per fern of the table: row, col, tau_0 .. tau_3
constexpr uint32_t FERN_NO_KEY = 0xFFFFFFFFu;  // sorts behind every key diss << 16 | index (27 bits)

// icpk_set_subsample's finaliser
ICPK_HD uint64_t fern_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

ICPK_HD uint32_t fern_draw(uint64_t seed, int f, int j) {
  return (uint32_t)(fern_mix(seed + (uint64_t)(f + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)j * 0xD1B54A32D192ED03ull) >> 32);
}

// fern f of the table for a level of rows x cols: e[0], e[1] the pixel, e[2..5] the thresholds (d_min <= tau < d_max)
ICPK_HD void fern_entry(uint64_t seed, int d_min, int d_max, int rows, int cols, int f, int32_t e[FERN_ENTRY]) {
  e[0] = (int32_t)(fern_draw(seed, f, 0) % (uint32_t)rows);
  e[1] = (int32_t)(fern_draw(seed, f, 1) % (uint32_t)cols);
  for (int k = 0; k < 4; ++k) e[2 + k] = d_min + (int32_t)(fern_draw(seed, f, 2 + k) % (uint32_t)(d_max - d_min));
}

// the nibble of depth d (0: a hole, which gives 0 as every threshold is >= 0): bit k set iff d > tau_k
ICPK_HD uint32_t fern_nibble(int d, const int32_t* tau) {
  return (uint32_t)(d > tau[0]) | (uint32_t)(d > tau[1]) << 1 | (uint32_t)(d > tau[2]) << 2 | (uint32_t)(d > tau[3]) << 3;
}

ICPK_HD int fern_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// the ferns of one packed word (eight nibbles) that differ
ICPK_HD int fern_word_diss(uint32_t a, uint32_t b) {
  uint32_t x = a ^ b;
  x |= x >> 1;
  x |= x >> 2;
  return fern_popcount(x & 0x11111111u);
}

ICPK_HD uint32_t fern_key(int diss, int index) { return (uint32_t)diss << 16 | (uint32_t)index; }

// the harvest rule: V valid ferns, n keyframes held, best_diss the smallest dissimilarity to them (any value for n == 0)
ICPK_HD bool fern_harvest(int V, int n, int best_diss, int min_valid, int capacity, int harvest_above) {
  return V >= min_valid && n < capacity && (n == 0 || best_diss > harvest_above);
}

}  // namespace icpk
