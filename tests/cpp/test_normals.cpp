// tests/cpp/test_normals.cpp -- icp::Engine::estimateTargetNormals / normalStats (icp_align.hpp) on one cloud; the
// Python test (tests/test_gpu_normals.py) makes the same calls through the C ABI and compares bit for bit.
//
//   test_normals <cloud.f32> <n> <radius> <min_neighbors> <out.bin>
// in : float x[n], y[n], z[n]; the viewpoint is (5, 5, 5)
// out: int32 status, n, n_valid, status of radius -1, status of min_neighbors 2, status of normalStats before any
//      estimate; float nx[n], ny[n], nz[n]; int32 count[n]; float curvature[n]; int64 moments[10 n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int n = std::atoi(argv[2]), min_nb = std::atoi(argv[4]);
  const float radius = (float)std::atof(argv[3]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || n <= 0) return 3;
  std::vector<float> p((size_t)3 * n);
  if (std::fread(p.data(), 4, p.size(), f) != p.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[5], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    if (icpk_set_target(eng.ctx(), p.data(), p.data() + n, p.data() + 2 * (size_t)n, n) != ICPK_OK) return 6;
    const float vp[3] = {5.f, 5.f, 5.f};
    int a = -1, b = -1;
    const int early = eng.normalStats(&a, &b);
    const int rc = eng.estimateTargetNormals(radius, min_nb, vp, ICPK_NORMALS_KEEP_MOMENTS);
    if (rc != ICPK_OK) {
      std::fprintf(stderr, "estimateTargetNormals failed: %d %s\n", rc, eng.last_error());
      return 7;
    }
    std::vector<float> nrm((size_t)3 * n), curv(n);
    std::vector<int32_t> count(n);
    std::vector<int64_t> mom((size_t)10 * n);
    const int rs = eng.normalStats(&a, &b, count.data(), curv.data(), mom.data());
    if (rs != ICPK_OK || icpk_get_target_normals(eng.ctx(), nrm.data(), nrm.data() + n, nrm.data() + 2 * (size_t)n) != ICPK_OK) return 8;
    const int32_t head[6] = {rc, a, b, eng.estimateTargetNormals(-1.f), eng.estimateTargetNormals(radius, 2), early};
    std::fwrite(head, 4, 6, o);
    std::fwrite(nrm.data(), 4, nrm.size(), o);
    std::fwrite(count.data(), 4, count.size(), o);
    std::fwrite(curv.data(), 4, curv.size(), o);
    std::fwrite(mom.data(), 8, mom.size(), o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 9;
  }
  std::fclose(o);
  return 0;
}
