// tests/cpp/fern_host_main.cpp -- the host half of K27 (icpk_fern_table, icpk_fern_encode_host,
// icpk_fern_dissimilarity_host: csrc/icpk_fern.cpp through csrc/fern_rule.h) as a stand-alone program with its own main
// and no GPU, for build.program("fern_host_sanitized"): compiled under -fsanitize=address,undefined, every array allocated
// at exactly the size include/icpk.h asks for, so that one word read or written past an end is reported.  The values
// are checked against the rule restated here from the table (the bytes are the business of tests/test_fern_host.py).
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "icpk.h"

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

static int run(int F, int rows, int cols, int d_min, int d_max, unsigned holes_every) {
  icpk_fern_params p;
  icpk_default_fern_params(&p);
  p.n_ferns = F, p.harvest_above = F / 5, p.min_valid = F / 2, p.d_min = d_min, p.d_max = d_max;
  const size_t npix = (size_t)rows * cols, W = (size_t)F / 8;
  std::unique_ptr<int32_t[]> table(new int32_t[(size_t)F * 6]);
  std::unique_ptr<uint16_t[]> level(new uint16_t[npix]);
  std::unique_ptr<uint32_t[]> code(new uint32_t[W]), other(new uint32_t[W]);
  unsigned state = 27u + (unsigned)F;
  for (size_t i = 0; i < npix; ++i) {
    state = state * 1664525u + 1013904223u;
    level[i] = holes_every && (state >> 8) % holes_every == 0 ? 0 : (uint16_t)(state >> 16);
  }
  CHECK(icpk_fern_table(&p, rows, cols, table.get()) == ICPK_OK);
  int32_t V = -1;
  CHECK(icpk_fern_encode_host(&p, level.get(), rows, cols, code.get(), &V) == ICPK_OK);
  int valid = 0;
  for (int f = 0; f < F; ++f) {
    const int32_t* e = table.get() + (size_t)f * 6;
    CHECK(e[0] >= 0 && e[0] < rows && e[1] >= 0 && e[1] < cols);
    const int d = level[(size_t)e[0] * cols + e[1]];
    unsigned nib = 0;
    for (int k = 0; k < 4; ++k) {
      CHECK(e[2 + k] >= d_min && e[2 + k] < d_max);
      nib |= (unsigned)(d > e[2 + k]) << k;
    }
    valid += d != 0;
    CHECK(((code[(size_t)f / 8] >> (4 * (f % 8))) & 15u) == nib);
  }
  CHECK(V == valid);
  for (size_t w = 0; w < W; ++w) other[w] = ~code[w];
  CHECK(icpk_fern_dissimilarity_host(code.get(), code.get(), F) == 0);
  CHECK(icpk_fern_dissimilarity_host(code.get(), other.get(), F) == F);
  other[W - 1] = code[W - 1] ^ 0x30000000u;  // the last fern alone
  for (size_t w = 0; w + 1 < W; ++w) other[w] = code[w];
  CHECK(icpk_fern_dissimilarity_host(code.get(), other.get(), F) == 1);
  CHECK(icpk_fern_dissimilarity_host(other.get(), code.get(), F) == 1);
  return 0;
}

int main() {
  const int ferns[] = {8, 64, 256, 1024};
  const int shapes[][2] = {{1, 1}, {19, 27}, {30, 40}, {120, 160}};
  for (int F : ferns)
    for (const auto& s : shapes) {
      if (run(F, s[0], s[1], 1000, 20000, 3)) return 1;
      if (run(F, s[0], s[1], 0, 65535, 0)) return 1;
      if (run(F, s[0], s[1], 4999, 5000, 0)) return 1;
    }
  // the refusals write nothing and read nothing
  icpk_fern_params p;
  icpk_default_fern_params(&p);
  std::unique_ptr<int32_t[]> table(new int32_t[1]);
  std::unique_ptr<uint32_t[]> code(new uint32_t[1]);
  std::unique_ptr<uint16_t[]> level(new uint16_t[1]);
  table[0] = 7, code[0] = 7, level[0] = 7;
  p.n_ferns = 12;
  CHECK(icpk_fern_table(&p, 1, 1, table.get()) == ICPK_E_ARG);
  CHECK(icpk_fern_encode_host(&p, level.get(), 1, 1, code.get(), nullptr) == ICPK_E_ARG);
  p.n_ferns = 256, p.d_max = p.d_min;
  CHECK(icpk_fern_table(&p, 1, 1, table.get()) == ICPK_E_ARG);
  CHECK(icpk_fern_encode_host(&p, level.get(), 1, 1, code.get(), nullptr) == ICPK_E_ARG);
  CHECK(icpk_fern_table(nullptr, 0, 1, table.get()) == ICPK_E_ARG && icpk_fern_table(nullptr, 1, 1, nullptr) == ICPK_E_ARG);
  CHECK(icpk_fern_encode_host(nullptr, nullptr, 1, 1, code.get(), nullptr) == ICPK_E_ARG);
  CHECK(icpk_fern_dissimilarity_host(code.get(), code.get(), 12) == ICPK_E_ARG);
  CHECK(icpk_fern_dissimilarity_host(nullptr, code.get(), 8) == ICPK_E_ARG);
  CHECK(icpk_fern_dissimilarity_host(code.get(), code.get(), 8) == 0);
  CHECK(table[0] == 7 && code[0] == 7);
  std::printf("fern host: ok\n");
  return 0;
}
