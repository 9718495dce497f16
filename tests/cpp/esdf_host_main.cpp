// tests/cpp/esdf_host_main.cpp -- DIAGNOSTIC (build.program("esdf_host_sanitized")): icpk_esdf_host and icpk_esdf_query_host
// over the shapes of the host cases of tests/esdf_cases.py, in a program of its own so that the host code (icpk_esdf.cpp
// and so csrc/esdf_rule.h, tsdf_rule.h) can run under -fsanitize=address,undefined without anything being loaded into an
// interpreter.  No GPU.  Every array is allocated at exactly the size the header asks for -- the planes one entry per
// voxel, the query's arrays n entries -- so a read or write past any of them is caught: the line searches run up to both
// ends of every line, and the query's points include cells whose far corner is the last voxel.  What the rule promises
// of its outputs is checked on every voxel against a search of the whole volume where that is affordable.  Exit status 0
// and "esdf host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

struct Case {
  int dims[3];
  int R;
  int occupied_pct10;  // per mille of OCCUPIED voxels; -1: every voxel unknown; 1001: every voxel occupied
  int flags;
  bool check_all;      // compare every voxel with a search of the whole volume
};

// returns 0, or the check that failed
static int run(const Case& k, long long* far_out) {
  icpk_tsdf_params v;
  icpk_default_tsdf_params(&v);
  for (int a = 0; a < 3; ++a) v.dims[a] = k.dims[a];
  v.voxel = 0.0625f, v.trunc = 0.25f;
  v.origin[0] = -0.4f, v.origin[1] = 0.3f, v.origin[2] = 0.7f;
  icpk_esdf_params e;
  icpk_default_esdf_params(&e);
  e.max_distance = ((float)k.R + 0.5f) * v.voxel, e.flags = k.flags;
  const size_t n = (size_t)k.dims[0] * k.dims[1] * k.dims[2];
  uint32_t s = 31u + (uint32_t)(n % 89);
  std::vector<float> tsdf(n);
  std::vector<uint16_t> weight(n);
  for (size_t i = 0; i < n; ++i) {
    const int r = (int)((lcg(s) >> 8) % 1000);
    const bool occ = k.occupied_pct10 > 1000 || r < k.occupied_pct10;
    tsdf[i] = occ ? -0.5f : 0.5f;
    weight[i] = k.occupied_pct10 < 0 ? 0 : (!occ && (lcg(s) >> 8) % 10 == 0) ? 0 : (uint16_t)(1 + (lcg(s) >> 8) % 3);
  }
  std::vector<int32_t> sq(n, 0);
  std::vector<uint8_t> cls(n, 9);
  std::vector<float> dist(n, -1.f);
  int64_t counts[4] = {-1, -1, -1, -1};
  if (icpk_esdf_host(&v, &e, tsdf.data(), weight.data(), sq.data(), cls.data(), dist.data(), counts) != ICPK_OK) return 1;
  int64_t seen[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    if (cls[i] > 2 || sq[i] == 0) return 2;
    const bool in_O = (k.flags & ICPK_ESDF_UNKNOWN_OCCUPIED) ? cls[i] != 1 : cls[i] == 2;
    if (in_O != (sq[i] < 0)) return 3;
    const int64_t mag = sq[i] < 0 ? -(int64_t)sq[i] : sq[i];
    if (mag != ICPK_ESDF_FAR && mag > (int64_t)k.R * k.R) return 4;
    seen[cls[i]] += 1, seen[3] += mag == ICPK_ESDF_FAR;
    const float want = mag == ICPK_ESDF_FAR ? ((float)(k.R + 1) - 0.5f) * v.voxel : (std::sqrt((float)mag) - 0.5f) * v.voxel;
    if (dist[i] != (sq[i] < 0 ? -want : want)) return 5;
  }
  for (int c = 0; c < 4; ++c)
    if (seen[c] != counts[c]) return 6;
  if (k.check_all) {
    const int dx = k.dims[0], dy = k.dims[1], dz = k.dims[2];
    for (int z = 0; z < dz; ++z)
      for (int y = 0; y < dy; ++y)
        for (int x = 0; x < dx; ++x) {
          const size_t at = (size_t)x + (size_t)dx * ((size_t)y + (size_t)dy * z);
          int64_t best = ICPK_ESDF_FAR;
          for (int w = 0; w < dz; ++w)
            for (int u = 0; u < dy; ++u)
              for (int t = 0; t < dx; ++t) {
                const size_t o = (size_t)t + (size_t)dx * ((size_t)u + (size_t)dy * w);
                if ((sq[o] < 0) == (sq[at] < 0)) continue;
                const int64_t d = (int64_t)(t - x) * (t - x) + (int64_t)(u - y) * (u - y) + (int64_t)(w - z) * (w - z);
                if (d < best) best = d;
              }
          if (best > (int64_t)k.R * k.R) best = ICPK_ESDF_FAR;
          if ((sq[at] < 0 ? -(int64_t)sq[at] : sq[at]) != best) return 7;
        }
  }
  // any output may be NULL
  if (icpk_esdf_host(&v, &e, tsdf.data(), weight.data(), nullptr, nullptr, nullptr, nullptr) != ICPK_OK) return 8;
  // the query: points in and around the volume, on cell borders, in the last cell, a NaN
  const int np = 257;
  std::vector<float> x(np), y(np), z(np), qd(np, -1.f), gx(np, -1.f), gy(np, -1.f), gz(np, -1.f);
  std::vector<uint8_t> st(np, 7);
  for (int i = 0; i < np; ++i) {
    float g[3];
    for (int a = 0; a < 3; ++a) {
      const float u = (float)((lcg(s) >> 8) % 10000) / 10000.f;
      g[a] = i % 4 == 0 ? std::floor(u * (float)k.dims[a]) : i % 4 == 1 ? (float)(k.dims[a] - 1) - u * 1e-3f : u * ((float)k.dims[a] + 2.f) - 1.f;
    }
    x[i] = (g[0] + 0.5f) * v.voxel + v.origin[0], y[i] = (g[1] + 0.5f) * v.voxel + v.origin[1], z[i] = (g[2] + 0.5f) * v.voxel + v.origin[2];
  }
  x[np - 1] = std::nanf("");
  if (icpk_esdf_query_host(&v, &e, sq.data(), cls.data(), x.data(), y.data(), z.data(), np, qd.data(), gx.data(), gy.data(), gz.data(),
                           st.data()) != ICPK_OK)
    return 9;
  const float reach = ((float)(k.R + 1) - 0.5f) * v.voxel;
  int inside = 0;
  for (int i = 0; i < np; ++i) {
    if (st[i] == 0x80) {
      if (qd[i] != 0.f || gx[i] != 0.f || gy[i] != 0.f || gz[i] != 0.f) return 10;
      continue;
    }
    ++inside;
    if (st[i] > 3 || !(std::fabs(qd[i]) <= reach * 1.0001f)) return 11;
    if (!std::isfinite(gx[i]) || !std::isfinite(gy[i]) || !std::isfinite(gz[i])) return 12;
  }
  if (st[np - 1] != 0x80) return 13;
  if ((k.dims[0] < 2 || k.dims[1] < 2 || k.dims[2] < 2) ? inside != 0 : inside < np / 4) return 14;
  // n = 0 and the outputs NULL
  if (icpk_esdf_query_host(&v, &e, sq.data(), cls.data(), nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_OK)
    return 15;
  if (icpk_esdf_query_host(&v, &e, sq.data(), cls.data(), x.data(), y.data(), z.data(), np, nullptr, nullptr, nullptr, nullptr, nullptr) != ICPK_OK)
    return 16;
  // the refusals touch nothing
  icpk_esdf_params bad = e;
  bad.max_distance = 0.f;
  if (icpk_esdf_host(&v, &bad, tsdf.data(), weight.data(), sq.data(), cls.data(), dist.data(), counts) != ICPK_E_ARG) return 17;
  bad = e, bad.min_weight = 0;
  if (icpk_esdf_host(&v, &bad, tsdf.data(), weight.data(), sq.data(), cls.data(), dist.data(), counts) != ICPK_E_ARG) return 18;
  bad = e, bad.flags = 4;
  if (icpk_esdf_query_host(&v, &bad, sq.data(), cls.data(), x.data(), y.data(), z.data(), np, qd.data(), nullptr, nullptr, nullptr, nullptr) !=
      ICPK_E_ARG)
    return 19;
  if (icpk_esdf_query_host(&v, &e, sq.data(), cls.data(), nullptr, y.data(), z.data(), 1, qd.data(), nullptr, nullptr, nullptr, nullptr) !=
      ICPK_E_ARG)
    return 20;
  *far_out = counts[3];
  return 0;
}

int main() {
  const Case cases[] = {
      {{37, 21, 19}, 6, 20, 0, true},                             // nothing is a multiple of anything
      {{37, 21, 19}, 1, 300, 0, true},                            // the smallest radius
      {{700, 5, 3}, 40, 1, 0, false},                             // a thin line per axis
      {{5, 700, 3}, 7, 1, 0, false},
      {{3, 5, 700}, 699, 1, 0, false},
      {{40, 1, 1}, 5, 100, 0, true},                              // dims of 1
      {{1, 33, 1}, 5, 100, 0, true},
      {{1, 1, 1}, 5, 0, 0, true},
      {{16, 16, 16}, 1024, -1, 0, true},                          // no voxel known: everything +FAR
      {{16, 16, 16}, 1024, -1, ICPK_ESDF_UNKNOWN_OCCUPIED, true},  // ... and -FAR with the flag
      {{16, 16, 16}, 1024, 1001, 0, true},                        // every voxel occupied
      {{24, 20, 18}, 9, 30, ICPK_ESDF_UNKNOWN_OCCUPIED, true},    // unknown voxels as obstacles
  };
  for (const Case& k : cases) {
    long long far = 0;
    if (const int rc = run(k, &far)) {
      std::fprintf(stderr, "esdf host: case %d x %d x %d R %d failed check %d\n", k.dims[0], k.dims[1], k.dims[2], k.R, rc);
      return 1;
    }
    std::printf("%d x %d x %d, R %d: %lld far\n", k.dims[0], k.dims[1], k.dims[2], k.R, far);
  }
  std::printf("esdf host: ok\n");
  return 0;
}
