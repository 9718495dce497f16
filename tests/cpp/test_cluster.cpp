// tests/cpp/test_cluster.cpp -- icp::Engine::clusterDbscan / clusters (icp_align.hpp, K33) on one cloud; the Python test
// (tests/test_gpu_cluster_cpp.py) makes the same calls by hand through the binding and compares byte for byte.
//
//   test_cluster <in.bin> <out.bin>
// in : int32 n, min_points, min_size, max_size, largest_only; float eps; float cloud[3][n]; float normals[3][n]
// out: three calls on the cloud -- labels only on the target; replacing on the source; replacing on the target with the
//      normals set -- each as: int32 status, n_clusters, n_noise, n_out, n_in; int32 labels[n_in]; uint8 core[n_in];
//      int32 count[n_in], nearest_core[n_in], out_index[n_in]; int32 sizes[n_clusters], first[n_clusters]; int32 m = the
//      cloud's size afterwards; float cloud[3][m]; (third call only) float normals[3][m].
//      Then clusterDbscan with eps = 0 and with which = 2: int32 status, status
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

static void put(FILE* o, const std::vector<int32_t>& v) { std::fwrite(v.data(), 4, v.size(), o); }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[5];
  float eps;
  if (std::fread(head, 4, 5, f) != 5 || std::fread(&eps, 4, 1, f) != 1 || head[0] < 0) return 4;
  const size_t n = (size_t)head[0];
  std::vector<float> cloud(3 * n), normals(3 * n);
  if (std::fread(cloud.data(), 4, cloud.size(), f) != cloud.size()) return 4;
  if (std::fread(normals.data(), 4, normals.size(), f) != normals.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  const icpk_cluster_params params{eps, head[1], head[2], head[3], head[4]};
  try {
    icp::Engine eng(0);
    icpk_ctx* c = eng.ctx();
    for (int call = 0; call < 3; ++call) {
      const int which = call == 1 ? 0 : 1;
      int rc = which == 1 ? icpk_set_target(c, cloud.data(), cloud.data() + n, cloud.data() + 2 * n, (int32_t)n)
                          : icpk_set_source(c, cloud.data(), cloud.data() + n, cloud.data() + 2 * n, (int32_t)n);
      if (rc == ICPK_OK && call == 2)
        rc = icpk_set_target_normals(c, normals.data(), normals.data() + n, normals.data() + 2 * n, (int32_t)n);
      if (rc != ICPK_OK) return 6;
      int nc = -1, noise = -1, n_out = -1;
      rc = eng.clusterDbscan(which, params, call == 0, &nc, &noise, &n_out);
      icp::Engine::Clusters rec;
      if (eng.clusters(&rec) != ICPK_OK) return 7;
      const int32_t counts[5] = {rc, nc, noise, n_out, (int32_t)rec.labels.size()};
      std::fwrite(counts, 4, 5, o);
      put(o, rec.labels);
      std::fwrite(rec.core.data(), 1, rec.core.size(), o);
      put(o, rec.count), put(o, rec.nearestCore), put(o, rec.outIndex), put(o, rec.sizes), put(o, rec.first);
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
      if (call == 0) std::printf("%d clusters, %d noise, %d kept of %zu\n", nc, noise, n_out, n);
    }
    icpk_cluster_params bad = params;
    bad.eps = 0.f;
    const int32_t refused[2] = {eng.clusterDbscan(1, bad), eng.clusterDbscan(2, params)};
    std::fwrite(refused, 4, 2, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
