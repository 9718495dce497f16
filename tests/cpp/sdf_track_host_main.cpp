// tests/cpp/sdf_track_host_main.cpp -- DIAGNOSTIC (build.program("sdf_track_host_sanitized")): icpk_sdf_pixels over the shapes
// of the cases of tests/sdf_track_cases.py, in a program of its own so that the host code (icpk_sdf_track.cpp and so
// csrc/sdf_track_rule.h, projective_rule.h, tsdf_rule.h) can run under -fsanitize=address,undefined without anything
// being loaded into an interpreter.  No GPU.  Every array is allocated at exactly the size the header asks for -- the level
// rows_s x cols_s, the two planes one entry per voxel, the outputs `count` entries and count x 28 terms -- so a read or
// write past any of them is caught; the volumes put the surface against their last layers, so that cells whose far
// corner is the last voxel are read.  What the rule promises of its outputs is checked on every pixel.  Exit status 0
// and "sdf track host: ok" when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void pose_of(double yaw_deg, double tx, double ty, double tz, double P[16]) {
  const double a = yaw_deg * 3.14159265358979323846 / 180.0, c = std::cos(a), s = std::sin(a);
  const double R[16] = {c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz, 0, 0, 0, 1};
  for (int k = 0; k < 16; ++k) P[k] = R[k];
}

struct Case {
  int rows_s, cols_s, level;
  int dims[3];
  double yaw, tz;   // of the estimate
  int holes;        // per cent of holes in the frame and of unseen voxels
  float cap, min_cos;
  bool constant;    // every voxel at 0.5
};

// returns 0, or the check that failed; *accepted_out: the accepted pixels of the whole image
static int run(const Case& k, int* accepted_out) {
  const size_t ns = (size_t)k.rows_s * k.cols_s;
  const size_t nvox = (size_t)k.dims[0] * k.dims[1] * k.dims[2];
  uint32_t s = 29u + (uint32_t)(ns % 97);
  std::vector<uint16_t> level(ns);
  for (auto& d : level) d = (int)((lcg(s) >> 8) % 100) < k.holes ? 0 : (uint16_t)(9900 + (lcg(s) >> 8) % 200);  // about 2 m
  // the volume: a plane at z = 2 m, whose distance is linear in z; the box is centred on the optical axis and ends one
  // voxel behind the plane; the small boxes are narrower than the frame's field of view, so pixels fall on both sides
  // of their faces
  icpk_tsdf_params v;
  icpk_default_tsdf_params(&v);
  for (int a = 0; a < 3; ++a) v.dims[a] = k.dims[a];
  v.voxel = 0.0625f, v.trunc = 0.25f;
  v.origin[0] = -0.5f * v.voxel * (float)k.dims[0], v.origin[1] = -0.5f * v.voxel * (float)k.dims[1];
  v.origin[2] = 2.0f + 1.5f * v.voxel - v.voxel * (float)k.dims[2];
  std::vector<float> tsdf(nvox);
  std::vector<uint16_t> weight(nvox);
  for (int z = 0; z < k.dims[2]; ++z)
    for (int y = 0; y < k.dims[1]; ++y)
      for (int x = 0; x < k.dims[0]; ++x) {
        const size_t at = (size_t)x + (size_t)k.dims[0] * ((size_t)y + (size_t)k.dims[1] * z);
        const float zc = ((float)z + 0.5f) * v.voxel + v.origin[2];
        float f = (2.0f - zc) / v.trunc;
        f = f > 1.f ? 1.f : f < -1.f ? -1.f : f;
        tsdf[at] = k.constant ? 0.5f : f;
        weight[at] = (int)((lcg(s) >> 8) % 100) < k.holes ? 0 : (uint16_t)(1 + (lcg(s) >> 8) % 3);
      }
  double E[16];
  pose_of(k.yaw, 0.01, -0.02, k.tz, E);
  icpk_sdf_params p;
  icpk_default_sdf_params(&p);
  p.level = k.level;
  p.fx = (float)k.cols_s * (float)(1 << k.level), p.cx = (float)(k.cols_s - 1) * 0.5f * (float)(1 << k.level);
  p.max_abs_tsdf = k.cap, p.min_normal_cos = k.min_cos;
  // the whole image, then windows of it: exactly-sized outputs each time
  std::vector<int32_t> cell(ns, 12345);
  std::vector<float> value(ns, -1.f);
  std::vector<double> terms(ns * ICPK_NP2L, -1.0);
  const int accepted = icpk_sdf_pixels(&p, &v, E, level.data(), k.rows_s, k.cols_s, tsdf.data(), weight.data(), 0, (int32_t)ns,
                                       cell.data(), value.data(), terms.data());
  if (accepted < 0) return 1;
  int seen = 0;
  for (size_t i = 0; i < ns; ++i) {
    const double* t = terms.data() + i * ICPK_NP2L;
    if (cell[i] >= 0) {
      ++seen;
      if ((size_t)cell[i] >= nvox || !(std::fabs(value[i]) < k.cap * v.trunc + 1e-6f)) return 2;
      if (t[27] != (double)std::fabs(value[i])) return 3;
      const double nn = t[15] + t[18] + t[20];  // J3^2 + J4^2 + J5^2 = |n|^2
      if (!(std::fabs(nn - 1.0) < 1e-5)) return 4;
    } else {
      if (cell[i] < ICPK_SDF_NORMAL || value[i] != 0.f) return 5;
      if (level[i] == 0 && cell[i] != ICPK_SDF_NO_DEPTH) return 6;
      for (int a = 0; a < ICPK_NP2L; ++a)
        if (t[a] != 0.0) return 7;
    }
  }
  if (seen != accepted) return 8;
  if (k.constant && accepted != 0) return 9;
  for (size_t first = 0; first < ns; first += ns / 3 + 1) {
    const size_t count = ns - first < 5 ? ns - first : 5;
    std::vector<int32_t> c2(count);
    std::vector<float> v2(count);
    std::vector<double> t2(count * ICPK_NP2L);
    const int a2 = icpk_sdf_pixels(&p, &v, E, level.data(), k.rows_s, k.cols_s, tsdf.data(), weight.data(), (int64_t)first,
                                   (int32_t)count, c2.data(), v2.data(), t2.data());
    if (a2 < 0) return 10;
    for (size_t e = 0; e < count; ++e) {
      if (c2[e] != cell[first + e] || v2[e] != value[first + e]) return 11;
      for (int a = 0; a < ICPK_NP2L; ++a)
        if (t2[e * ICPK_NP2L + a] != terms[(first + e) * ICPK_NP2L + a]) return 12;
    }
    // without terms
    if (icpk_sdf_pixels(&p, &v, E, level.data(), k.rows_s, k.cols_s, tsdf.data(), weight.data(), (int64_t)first, (int32_t)count,
                        c2.data(), v2.data(), nullptr) != a2)
      return 13;
  }
  // the refusals touch nothing
  if (icpk_sdf_pixels(&p, &v, E, level.data(), k.rows_s, k.cols_s, tsdf.data(), weight.data(), (int64_t)ns, 1, cell.data(),
                      value.data(), nullptr) != ICPK_E_ARG)
    return 14;
  icpk_sdf_params bad = p;
  bad.max_abs_tsdf = 1.5f;
  if (icpk_sdf_pixels(&bad, &v, E, level.data(), k.rows_s, k.cols_s, tsdf.data(), weight.data(), 0, 1, cell.data(), value.data(),
                      nullptr) != ICPK_E_ARG)
    return 15;
  *accepted_out = accepted;
  return 0;
}

int main() {
  const Case cases[] = {
      {120, 160, 0, {40, 32, 8}, 0.0, 0.0, 0, 1.0f, -2.f, false},   // the main shape
      {60, 80, 1, {40, 32, 8}, 2.0, 0.02, 5, 1.0f, -2.f, false},    // a coarser level, holes and unseen voxels
      {1, 1, 0, {2, 2, 2}, 0.0, 0.0, 0, 1.0f, -2.f, false},         // one pixel, one cell
      {7, 9, 0, {3, 5, 2}, 0.0, 0.0, 0, 1.0f, 0.5f, false},         // the normal gate on
      {17, 19, 0, {33, 17, 9}, -3.0, -0.03, 10, 0.5f, 0.9f, false}, // a tighter gate, odd dims
      {260, 260, 0, {12, 10, 10}, 0.0, 0.0, 0, 1.0f, -2.f, false},  // 67 600 pixels
      {48, 64, 0, {12, 10, 10}, 0.0, 50.0, 0, 1.0f, -2.f, false},   // every point outside
      {48, 64, 0, {12, 10, 10}, 0.0, 0.0, 0, 1.0f, -2.f, true},     // no gradient anywhere
      {5, 5, 0, {1, 4, 4}, 0.0, 0.0, 0, 1.0f, -2.f, false},         // a dim of 1: no cell at all
  };
  int total = 0;
  for (const Case& k : cases) {
    int accepted = 0;
    if (const int rc = run(k, &accepted)) {
      std::fprintf(stderr, "sdf track host: case %d x %d failed check %d\n", k.rows_s, k.cols_s, rc);
      return 1;
    }
    std::printf("%d x %d level %d over %d x %d x %d: %d accepted\n", k.rows_s, k.cols_s, k.level, k.dims[0], k.dims[1], k.dims[2],
                accepted);
    total += accepted;
  }
  if (total == 0) {
    std::fprintf(stderr, "sdf track host: no case accepted a pixel\n");
    return 1;
  }
  std::printf("sdf track host: ok\n");
  return 0;
}
