// tests/cpp/test_bilateral.cpp -- icp::Engine::bilateralDepthImage / backprojectSmoothed (icp_align.hpp, K22) on one
// frame; the Python test (tests/test_gpu_bilateral_cpp.py) makes the same calls through the binding and compares bit
// for bit.
//
//   test_bilateral <depth.u16> <rows> <cols> <radius> <sigma_space> <sigma_range> <range_cutoff> <out.bin>
// in : uint16 depth[rows * cols]; the camera is fx 468.60, cx 318.27, no offset
// out: int32 status of the filter, n of the smoothed target cloud, status of radius 0, status of normals on the source;
//      uint16 smoothed[rows * cols] (filtered in place); float x[n], y[n], z[n]; float nx[n], ny[n], nz[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  icpk_bilateral_params p;
  icpk_default_bilateral_params(&p);
  p.radius = std::atoi(argv[4]);
  p.sigma_space = (float)std::atof(argv[5]);
  p.sigma_range = (float)std::atof(argv[6]);
  p.range_cutoff = std::atoi(argv[7]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || rows <= 0 || cols <= 0) return 3;
  std::vector<uint16_t> depth((size_t)rows * cols);
  if (std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[8], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    const int n = eng.backprojectSmoothed(depth.data(), rows, cols, 468.60f, 318.27f, nullptr, 1, ICPK_NORMALS_CROSS, &p);
    if (n < 0) {
      std::fprintf(stderr, "backprojectSmoothed failed: %d %s\n", n, eng.last_error());
      return 6;
    }
    std::vector<float> pts((size_t)3 * n + 1), nrm((size_t)3 * n + 1);
    if (icpk_get_target(eng.ctx(), pts.data(), pts.data() + n, pts.data() + 2 * (size_t)n) != ICPK_OK ||
        icpk_get_target_normals(eng.ctx(), nrm.data(), nrm.data() + n, nrm.data() + 2 * (size_t)n) != ICPK_OK)
      return 7;
    icpk_bilateral_params bad = p;
    bad.radius = 0;
    const int rb = eng.bilateralDepthImage(depth.data(), depth.data(), rows, cols, &bad);
    const int rn = eng.backprojectSmoothed(depth.data(), rows, cols, 468.60f, 318.27f, nullptr, 0, ICPK_NORMALS_CROSS, &p);
    const int rc = eng.bilateralDepthImage(depth.data(), depth.data(), rows, cols, &p);  // in place
    if (rc != ICPK_OK) {
      std::fprintf(stderr, "bilateralDepthImage failed: %d %s\n", rc, eng.last_error());
      return 8;
    }
    const int32_t head[4] = {rc, n, rb, rn};
    std::fwrite(head, 4, 4, o);
    std::fwrite(depth.data(), 2, depth.size(), o);
    std::fwrite(pts.data(), 4, (size_t)3 * n, o);
    std::fwrite(nrm.data(), 4, (size_t)3 * n, o);
    std::printf("bilateral %d x %d, radius %d: smoothed target of %d points\n", rows, cols, p.radius, n);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 9;
  }
  std::fclose(o);
  return 0;
}
