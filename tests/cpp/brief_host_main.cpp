// tests/cpp/brief_host_main.cpp -- DIAGNOSTIC (build.program("brief_host_sanitized")): icpk_brief_describe_host and
// icpk_brief_match_host, in a program of its own so that the host code (icpk_brief.cpp and so csrc/brief_rule.h and
// brief_table.h) can run under -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.
// Every array is allocated at exactly the size the header asks for -- the image rows x cols x channels bytes, the key
// points 2 n floats, the outputs n (the match: ns) entries -- so a read or write past any of them is caught: the key
// points include every pixel of the describable border, whose windows end on the image's last row and column, and
// positions outside the image.  What the rules promise of their outputs is checked.  Exit status 0 and "brief host: ok"
// when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int popcount256(const uint32_t* a, const uint32_t* b) {
  int h = 0;
  for (int w = 0; w < ICPK_BRIEF_WORDS; ++w) h += __builtin_popcount(a[w] ^ b[w]);
  return h;
}

// returns 0, or the check that failed
static int describe_case(int rows, int cols, int channels, int* described) {
  uint32_t s = 17u + (uint32_t)(rows * 131 + cols + channels);
  std::vector<uint8_t> img((size_t)rows * cols * channels);
  for (uint8_t& v : img) v = (uint8_t)(lcg(s) >> 24);
  // every pixel and a ring of one pixel around the image, then the odd ones
  std::vector<float> kp;
  for (int y = -1; y <= rows; ++y)
    for (int x = -1; x <= cols; ++x) kp.push_back((float)x), kp.push_back((float)y);
  const float odd[][2] = {{std::nanf(""), 20.f}, {20.f, std::numeric_limits<float>::infinity()}, {-3e38f, 3e38f}, {15.5f, 15.49f}};
  for (const auto& o : odd) kp.push_back(o[0]), kp.push_back(o[1]);
  const int n = (int)(kp.size() / 2);
  for (int flags = 0; flags <= ICPK_BRIEF_UPRIGHT; ++flags) {
    std::vector<uint32_t> words((size_t)ICPK_BRIEF_WORDS * n, 0xdeadbeefu);
    std::vector<uint8_t> bin((size_t)n, 77), valid((size_t)n, 77);
    if (icpk_brief_describe_host(img.data(), rows, cols, channels, kp.data(), n, flags, words.data(), bin.data(), valid.data()) != ICPK_OK)
      return 1;
    int count = 0;
    for (int k = 0; k < n; ++k) {
      const float x = kp[2 * (size_t)k], y = kp[2 * (size_t)k + 1];
      const bool want = k < n - 4 ? (x >= 15.f && x < (float)(cols - 15) && y >= 15.f && y < (float)(rows - 15))
                                  : (k == n - 1 && cols > 31 && rows > 30);  // (15.5 -> 16, 15.49 -> 15)
      if ((valid[k] != 0) != want || valid[k] > 1 || bin[k] > 31) return 2;
      if (flags && bin[k] != 0) return 3;
      if (!valid[k]) {
        if (bin[k] != 0) return 4;
        for (int w = 0; w < ICPK_BRIEF_WORDS; ++w)
          if (words[(size_t)ICPK_BRIEF_WORDS * k + w] != 0u) return 5;
      }
      count += valid[k];
    }
    *described = count;
    // any output may be NULL; n = 0 needs no key points
    if (icpk_brief_describe_host(img.data(), rows, cols, channels, kp.data(), n, flags, nullptr, nullptr, nullptr) != ICPK_OK) return 6;
    if (icpk_brief_describe_host(img.data(), rows, cols, channels, nullptr, 0, flags, nullptr, nullptr, nullptr) != ICPK_OK) return 7;
  }
  if (icpk_brief_describe_host(img.data(), rows, cols, 2, kp.data(), n, 0, nullptr, nullptr, nullptr) != ICPK_E_ARG) return 8;
  if (icpk_brief_describe_host(img.data(), rows, cols, channels, nullptr, 1, 0, nullptr, nullptr, nullptr) != ICPK_E_ARG) return 9;
  if (icpk_brief_describe_host(img.data(), rows, cols, channels, kp.data(), n, 4, nullptr, nullptr, nullptr) != ICPK_E_ARG) return 10;
  return 0;
}

static int match_case(int ns, int nt, int* kept_out) {
  uint32_t s = 5u + (uint32_t)(ns * 977 + nt);
  std::vector<uint32_t> ws((size_t)ICPK_BRIEF_WORDS * ns), wt((size_t)ICPK_BRIEF_WORDS * nt);
  std::vector<uint8_t> vs((size_t)ns), vt((size_t)nt);
  for (uint32_t& w : ws) w = lcg(s) & 0x0f0f0f0fu;  // (sparse words: small distances and ties)
  for (uint32_t& w : wt) w = lcg(s) & 0x0f0f0f0fu;
  for (int k = 0; k < ns && k < nt; k += 3)
    for (int w = 0; w < ICPK_BRIEF_WORDS; ++w) wt[(size_t)ICPK_BRIEF_WORDS * k + w] = ws[(size_t)ICPK_BRIEF_WORDS * k + w];
  for (uint8_t& v : vs) v = (lcg(s) >> 8) % 7 != 0;
  for (uint8_t& v : vt) v = (lcg(s) >> 8) % 7 != 0;
  for (int mutual = 0; mutual <= 1; ++mutual)
    for (int ratio = 0; ratio <= 1; ++ratio) {
      icpk_brief_match_params p;
      icpk_default_brief_match_params(&p);
      p.max_hamming = 40, p.ratio_num = ratio ? 9 : 0, p.ratio_den = 10, p.flags = mutual ? ICPK_BRIEF_MUTUAL : 0;
      std::vector<int32_t> i((size_t)ns, -7), j((size_t)ns, -7), H((size_t)ns, -7), H2((size_t)ns, -7);
      int32_t m = -1;
      if (icpk_brief_match_host(ws.data(), vs.data(), ns, wt.data(), vt.data(), nt, &p, i.data(), j.data(), H.data(), H2.data(), &m) != ICPK_OK)
        return 1;
      if (m < 0 || m > ns) return 2;
      for (int k = 0; k < m; ++k) {
        if (i[k] < 0 || i[k] >= ns || j[k] < 0 || j[k] >= nt || !vs[i[k]] || !vt[j[k]]) return 3;
        if (k && i[k] <= i[k - 1]) return 4;  // source order
        if (H[k] != popcount256(&ws[(size_t)ICPK_BRIEF_WORDS * i[k]], &wt[(size_t)ICPK_BRIEF_WORDS * j[k]]) || H[k] > 40) return 5;
        int second = 257;
        for (int t = 0; t < nt; ++t) {
          if (!vt[t] || t == j[k]) continue;
          const int h = popcount256(&ws[(size_t)ICPK_BRIEF_WORDS * i[k]], &wt[(size_t)ICPK_BRIEF_WORDS * t]);
          if (h < H[k] || (h == H[k] && t < j[k])) return 6;  // (H, j) is the least
          if (h < second) second = h;
        }
        if (H2[k] != second) return 7;
        if (ratio && !(H[k] * 10 < H2[k] * 9)) return 8;
        if (mutual)
          for (int u = 0; u < ns; ++u) {
            if (!vs[u] || u == i[k]) continue;
            const int h = popcount256(&ws[(size_t)ICPK_BRIEF_WORDS * u], &wt[(size_t)ICPK_BRIEF_WORDS * j[k]]);
            if (h < H[k] || (h == H[k] && u < i[k])) return 9;
          }
      }
      if (!mutual && !ratio) *kept_out = m;
      if (icpk_brief_match_host(ws.data(), vs.data(), ns, wt.data(), vt.data(), nt, &p, nullptr, nullptr, nullptr, nullptr, &m) != ICPK_OK)
        return 10;
    }
  icpk_brief_match_params bad;
  icpk_default_brief_match_params(&bad);
  bad.max_hamming = 257;
  int32_t m = 5;
  if (icpk_brief_match_host(ws.data(), vs.data(), ns, wt.data(), vt.data(), nt, &bad, nullptr, nullptr, nullptr, nullptr, &m) != ICPK_E_ARG || m != 0)
    return 11;
  icpk_default_brief_match_params(&bad);
  bad.flags = ICPK_BRIEF_TO_CLOUDS;
  if (icpk_brief_match_host(ws.data(), vs.data(), ns, wt.data(), vt.data(), nt, &bad, nullptr, nullptr, nullptr, nullptr, &m) != ICPK_E_ARG)
    return 12;
  return 0;
}

int main() {
  const int shapes[][3] = {{31, 31, 1}, {31, 31, 3}, {30, 64, 1}, {32, 64, 3}, {37, 100, 1}, {37, 100, 3}, {64, 48, 3}};
  for (const auto& sh : shapes) {
    int described = -1;
    if (const int rc = describe_case(sh[0], sh[1], sh[2], &described)) {
      std::fprintf(stderr, "brief host: describe %d x %d x %d failed check %d\n", sh[0], sh[1], sh[2], rc);
      return 1;
    }
    const int want = (sh[0] > 30 ? sh[0] - 30 : 0) * (sh[1] > 30 ? sh[1] - 30 : 0) + (sh[1] > 31 && sh[0] > 30 ? 1 : 0);
    if (described != want) {
      std::fprintf(stderr, "brief host: describe %d x %d: %d described, %d expected\n", sh[0], sh[1], described, want);
      return 1;
    }
    std::printf("describe %d x %d x %d: %d described\n", sh[0], sh[1], sh[2], described);
  }
  const int sizes[][2] = {{0, 5}, {5, 0}, {1, 1}, {63, 65}, {64, 64}, {65, 257}, {300, 257}};
  for (const auto& sz : sizes) {
    int kept = -1;
    if (const int rc = match_case(sz[0], sz[1], &kept)) {
      std::fprintf(stderr, "brief host: match %d x %d failed check %d\n", sz[0], sz[1], rc);
      return 1;
    }
    std::printf("match %d x %d: %d kept\n", sz[0], sz[1], kept);
  }
  std::printf("brief host: ok\n");
  return 0;
}
