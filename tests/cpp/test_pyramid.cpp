// tests/cpp/test_pyramid.cpp -- icp::Engine::buildDepthPyramid / depthPyramidLevel / backprojectPyramidLevel
// (icp_align.hpp, K24) on one frame; the Python test (tests/test_gpu_pyramid_cpp.py) makes the same calls through the
// binding and compares bit for bit.
//
//   test_pyramid <depth.u16> <rows> <cols> <levels> <range_cutoff> <smooth 0|1> <out.bin>
// in : uint16 depth[rows * cols]; the camera is fx 468.60, cx 318.27, no offset
// out: int32 status of the build, n of the target cloud of the last level, status of a level the pyramid does not have,
//      status of normals on the source, status of a build with 0 levels, status of depthPyramidLevel before the build;
//      per level int32 rows, cols and uint16 pixels[rows * cols]; float x[n], y[n], z[n]; float nx[n], ny[n], nz[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  icpk_pyramid_params p;
  icpk_default_pyramid_params(&p);
  p.levels = std::atoi(argv[4]);
  p.range_cutoff = std::atoi(argv[5]);
  icpk_bilateral_params b;
  icpk_default_bilateral_params(&b);
  const bool smooth = std::atoi(argv[6]) != 0;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || rows <= 0 || cols <= 0) return 3;
  std::vector<uint16_t> depth((size_t)rows * cols);
  if (std::fread(depth.data(), 2, depth.size(), f) != depth.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[7], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    int r = 0, c = 0;
    const int before = eng.depthPyramidLevel(0, &r, &c);
    const int rc = eng.buildDepthPyramid(depth.data(), rows, cols, &p, smooth ? &b : nullptr);
    if (rc != ICPK_OK) {
      std::fprintf(stderr, "buildDepthPyramid failed: %d %s\n", rc, eng.last_error());
      return 6;
    }
    const int last = p.levels - 1;
    const int n = eng.backprojectPyramidLevel(last, 468.60f, 318.27f, nullptr, 1, ICPK_NORMALS_CROSS);
    if (n < 0) {
      std::fprintf(stderr, "backprojectPyramidLevel failed: %d %s\n", n, eng.last_error());
      return 7;
    }
    std::vector<float> pts((size_t)3 * n + 1), nrm((size_t)3 * n + 1);
    if (icpk_get_target(eng.ctx(), pts.data(), pts.data() + n, pts.data() + 2 * (size_t)n) != ICPK_OK ||
        icpk_get_target_normals(eng.ctx(), nrm.data(), nrm.data() + n, nrm.data() + 2 * (size_t)n) != ICPK_OK)
      return 8;
    const int none = eng.depthPyramidLevel(p.levels, &r, &c);
    const int rn = eng.backprojectPyramidLevel(0, 468.60f, 318.27f, nullptr, 0, ICPK_NORMALS_CROSS);
    icpk_pyramid_params bad = p;
    bad.levels = 0;
    const int rb = eng.buildDepthPyramid(depth.data(), rows, cols, &bad);  // (refused: the pyramid stays)
    const int32_t head[6] = {rc, n, none, rn, rb, before};
    std::fwrite(head, 4, 6, o);
    for (int l = 0; l < p.levels; ++l) {
      if (eng.depthPyramidLevel(l, &r, &c) != ICPK_OK) return 9;  // the shape alone
      std::vector<uint16_t> img((size_t)r * c);
      if (eng.depthPyramidLevel(l, &r, &c, img.data()) != ICPK_OK) return 10;
      const int32_t shape[2] = {r, c};
      std::fwrite(shape, 4, 2, o);
      std::fwrite(img.data(), 2, img.size(), o);
    }
    std::fwrite(pts.data(), 4, (size_t)3 * n, o);
    std::fwrite(nrm.data(), 4, (size_t)3 * n, o);
    std::printf("pyramid %d x %d, %d levels: target of %d points from level %d\n", rows, cols, p.levels, n, last);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 11;
  }
  std::fclose(o);
  return 0;
}
