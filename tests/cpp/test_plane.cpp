// tests/cpp/test_plane.cpp -- icp::Engine::segmentPlanes / planes (icp_align.hpp, K34) on one cloud; the Python test
// (tests/test_gpu_plane_cpp.py) makes the same calls by hand through the binding and compares byte for byte.
//
//   test_plane <in.bin> <out.bin>
// in : int32 n, n_hypotheses, max_planes, min_inliers; float distance_threshold; uint64 seed; float cloud[3][n];
//      float normals[3][n]
// out: four calls on the cloud -- labels only on the target; replacing on the source (planes removed); replacing on the
//      target with the normals set (planes removed); replacing on the target, plane 0 kept -- each as: int32 status,
//      n_planes, n_unassigned, n_out, n_in; int32 labels[n_in], out_index[n_in]; double model[n_planes][8]; int32
//      info[n_planes][6]; double sums[n_planes][9]; int32 m = the cloud's size afterwards; float cloud[3][m]; (third call
//      only) float normals[3][m].
//      Then segmentPlanes with distance_threshold = 0, with which = 2 and with select_plane = 0 but no keepInliers: int32
//      status, status, status
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[4];
  float t;
  uint64_t seed;
  if (std::fread(head, 4, 4, f) != 4 || std::fread(&t, 4, 1, f) != 1 || std::fread(&seed, 8, 1, f) != 1 || head[0] < 0) return 4;
  const size_t n = (size_t)head[0];
  std::vector<float> cloud(3 * n), normals(3 * n);
  if (std::fread(cloud.data(), 4, cloud.size(), f) != cloud.size()) return 4;
  if (std::fread(normals.data(), 4, normals.size(), f) != normals.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  icpk_plane_params params;
  icpk_default_plane_params(&params);
  params.seed = seed, params.distance_threshold = t;
  params.n_hypotheses = head[1], params.max_planes = head[2], params.min_inliers = head[3];
  try {
    icp::Engine eng(0);
    icpk_ctx* c = eng.ctx();
    for (int call = 0; call < 4; ++call) {
      const int which = call == 1 ? 0 : 1;
      int rc = which == 1 ? icpk_set_target(c, cloud.data(), cloud.data() + n, cloud.data() + 2 * n, (int32_t)n)
                          : icpk_set_source(c, cloud.data(), cloud.data() + n, cloud.data() + 2 * n, (int32_t)n);
      if (rc == ICPK_OK && call == 2)
        rc = icpk_set_target_normals(c, normals.data(), normals.data() + n, normals.data() + 2 * n, (int32_t)n);
      if (rc != ICPK_OK) return 6;
      icpk_plane_params p = params;
      p.select_plane = call == 3 ? 0 : -1;
      int np = -1, un = -1, n_out = -1;
      rc = eng.segmentPlanes(which, p, call == 0, call == 3, &np, &un, &n_out);
      icp::Engine::Planes rec;
      if (eng.planes(&rec) != ICPK_OK) return 7;
      const int32_t counts[5] = {rc, np, un, n_out, (int32_t)rec.labels.size()};
      std::fwrite(counts, 4, 5, o);
      std::fwrite(rec.labels.data(), 4, rec.labels.size(), o);
      std::fwrite(rec.outIndex.data(), 4, rec.outIndex.size(), o);
      std::fwrite(rec.model.data(), 8, rec.model.size(), o);
      std::fwrite(rec.info.data(), 4, rec.info.size(), o);
      std::fwrite(rec.sums.data(), 8, rec.sums.size(), o);
      const int32_t m = which == 1 ? icpk_target_size(c) : icpk_source_size(c);
      std::vector<float> got(3 * (size_t)m + 1);
      rc = which == 1 ? icpk_get_target(c, got.data(), got.data() + m, got.data() + 2 * (size_t)m)
                      : icpk_get_source(c, got.data(), got.data() + m, got.data() + 2 * (size_t)m);
      if (rc != ICPK_OK) return 8;
      std::fwrite(&m, 4, 1, o);
      std::fwrite(got.data(), 4, 3 * (size_t)m, o);
      if (call == 2) {
        if (icpk_get_target_normals(c, got.data(), got.data() + m, got.data() + 2 * (size_t)m) != ICPK_OK) return 9;
        std::fwrite(got.data(), 4, 3 * (size_t)m, o);
      }
      if (call == 0) std::printf("%d planes, %d unassigned, %d kept of %zu\n", rec.count(), un, n_out, n);
    }
    icpk_plane_params bad = params, sel = params;
    bad.distance_threshold = 0.f;
    sel.select_plane = 0;
    const int32_t refused[3] = {eng.segmentPlanes(1, bad), eng.segmentPlanes(2, params), eng.segmentPlanes(1, sel)};
    std::fwrite(refused, 4, 3, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
