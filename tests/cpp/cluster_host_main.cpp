// tests/cpp/cluster_host_main.cpp -- DIAGNOSTIC (build.program("cluster_host_sanitized")): icpk_cluster_host in a
// program of its own so that the host code (icpk_cluster.cpp and so csrc/cluster_rule.h) can run under
// -fsanitize=address,undefined without anything being loaded into an interpreter.  No GPU.  Every array is allocated at
// exactly the size the header asks for -- the points 3 n floats, the per-point outputs n entries, sizes and first
// n_clusters entries (learnt from a first call with both NULL) -- so a read or write past any of them is caught.  What
// the rule promises of its outputs is checked.  Exit status 0 and "cluster host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t& s) { return (float)(lcg(s) >> 8) * (1.0f / 16777216.0f); }

// returns 0, or the check that failed
static int run_case(const std::vector<float>& pts, int n, const icpk_cluster_params& p, int* clusters_out) {
  int32_t nc = -1, noise = -1, kept = -1;
  if (icpk_cluster_host(n ? pts.data() : nullptr, n, &p, &nc, &noise, &kept, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr) != ICPK_OK)
    return 1;
  if (nc < 0 || nc > n || noise < 0 || noise > n || kept < 0 || kept > n) return 2;
  const size_t N = (size_t)n, NC = (size_t)nc;
  std::vector<int32_t> labels(N, -7), count(N, -7), nearest(N, -7), oidx(N, -7), sizes(NC, -7), first(NC, -7);
  std::vector<uint8_t> core(N, 77);
  int32_t nc2 = -1, noise2 = -1, kept2 = -1;
  if (icpk_cluster_host(n ? pts.data() : nullptr, n, &p, &nc2, &noise2, &kept2, labels.data(), core.data(), count.data(),
                        nearest.data(), oidx.data(), sizes.data(), first.data()) != ICPK_OK)
    return 3;
  if (nc2 != nc || noise2 != noise || kept2 != kept) return 4;
  const float* x = pts.data();
  const float *y = x + N, *z = x + 2 * N;
  std::vector<int32_t> members(NC, 0);
  int n_noise = 0, n_kept = 0;
  for (size_t i = 0; i < N; ++i) {
    const bool fin = std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i]);
    if ((count[i] == 0) != !fin || core[i] > 1 || (core[i] != 0) != (count[i] >= p.min_points)) return 5;
    if (labels[i] < -1 || labels[i] >= nc) return 6;
    if (core[i] ? nearest[i] != (int32_t)i : (nearest[i] < -1 || nearest[i] >= n || (nearest[i] >= 0 && !core[(size_t)nearest[i]]))) return 7;
    if ((labels[i] < 0) != (nearest[i] < 0)) return 8;
    if (labels[i] >= 0 && labels[i] != labels[(size_t)nearest[i]]) return 9;
    if (labels[i] >= 0) ++members[(size_t)labels[i]];
    n_noise += labels[i] < 0;
    if (oidx[i] >= 0 && oidx[i] != n_kept) return 10;  // input order
    n_kept += oidx[i] >= 0;
  }
  if (n_noise != noise || n_kept != kept) return 11;
  int32_t greatest = -1;
  for (size_t c = 0; c < NC; ++c) {
    if (sizes[c] != members[c] || sizes[c] < 1) return 12;
    if (first[c] < 0 || first[c] >= n || !core[(size_t)first[c]] || labels[(size_t)first[c]] != (int32_t)c) return 13;
    if (c && first[c] <= first[c - 1]) return 14;  // numbered by ascending representative
    for (int32_t i = 0; i < first[c]; ++i)
      if (core[(size_t)i] && labels[(size_t)i] == (int32_t)c) return 15;  // ... which is the smallest core index
    if (greatest < 0 || sizes[c] > sizes[(size_t)greatest]) greatest = (int32_t)c;
  }
  for (size_t i = 0; i < N; ++i) {
    const int32_t lab = labels[i];
    const bool want = lab >= 0 && sizes[(size_t)lab] >= p.min_size && (p.max_size == 0 || sizes[(size_t)lab] <= p.max_size) &&
                      (!p.largest_only || lab == greatest);
    if ((oidx[i] >= 0) != want) return 16;
  }
  // two core points within eps of one another share a cluster (checked on a stride: the rule is symmetric)
  for (size_t i = 0; i < N; i += 7)
    for (size_t j = 0; j < N; ++j) {
      if (!core[i] || !core[j]) continue;
      const double dx = (double)(x[i] - x[j]), dy = (double)(y[i] - y[j]), dz = (double)(z[i] - z[j]);
      if (std::sqrt((float)((dx * dx + dy * dy) + dz * dz)) <= p.eps && labels[i] != labels[j]) return 17;
    }
  *clusters_out = nc;
  return 0;
}

int main() {
  const int sizes[] = {0, 1, 2, 63, 64, 65, 257, 700};
  for (const int n : sizes) {
    uint32_t s = 29u + (uint32_t)n * 977u;
    std::vector<float> pts(3 * (size_t)n);
    for (float& v : pts) v = unit(s);
    // duplicates, a clump, and non-finite coordinates where there is room for them
    for (int k = 0; k + 20 < n; k += 9)
      for (int c = 0; c < 3; ++c) pts[(size_t)c * n + k + 1] = pts[(size_t)c * n + k];
    if (n > 40) {
      pts[(size_t)n + 17] = std::nanf("");
      pts[23] = std::numeric_limits<float>::infinity();
      pts[2 * (size_t)n + 31] = -std::numeric_limits<float>::infinity();
    }
    const icpk_cluster_params settings[] = {{0.12f, 4, 1, 0, 0}, {0.12f, 1, 0, 0, 0}, {0.2f, 6, 3, 40, 0}, {0.15f, 3, 1, 0, 1},
                                            {2.0f, 2, 1, 0, 0}, {1e-6f, 2, 1, 0, 0}};
    for (const auto& p : settings) {
      int clusters = -1;
      if (const int rc = run_case(pts, n, p, &clusters)) {
        std::fprintf(stderr, "cluster host: n %d eps %g min_points %d failed check %d\n", n, (double)p.eps, p.min_points, rc);
        return 1;
      }
      std::printf("n %d eps %g min_points %d: %d clusters\n", n, (double)p.eps, p.min_points, clusters);
    }
  }
  // the refusals: nothing is read or written
  const icpk_cluster_params good{0.1f, 3, 1, 0, 0};
  const float one[3] = {0.f, 0.f, 0.f};
  const icpk_cluster_params bad[] = {{0.f, 3, 1, 0, 0},  {-1.f, 3, 1, 0, 0}, {std::nanf(""), 3, 1, 0, 0},
                                     {std::numeric_limits<float>::infinity(), 3, 1, 0, 0},
                                     {0.1f, 0, 1, 0, 0}, {0.1f, 3, -1, 0, 0}, {0.1f, 3, 1, -1, 0},
                                     {0.1f, 3, 4, 3, 0}, {0.1f, 3, 1, 0, 2}};
  int32_t nc = 5;
  for (const auto& p : bad)
    if (icpk_cluster_host(one, 1, &p, &nc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG || nc != 0) {
      std::fprintf(stderr, "cluster host: a bad setting was accepted\n");
      return 1;
    }
  if (icpk_cluster_host(one, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_cluster_host(one, -1, &good, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG ||
      icpk_cluster_host(nullptr, 1, &good, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_E_ARG) {
    std::fprintf(stderr, "cluster host: a bad call was accepted\n");
    return 1;
  }
  std::printf("cluster host: ok\n");
  return 0;
}
