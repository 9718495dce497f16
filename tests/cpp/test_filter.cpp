// tests/cpp/test_filter.cpp -- icp::Tracker with outlierFilter / outlierSetting and icp::Engine::removeOutliers /
// outlierStats (icp_align.hpp) on a sequence of depth frames; the Python test (tests/test_gpu_filter_cpp.py) makes the
// same calls by hand through the C ABI and compares bit for bit.
//
//   test_filter <frames.u16> <rows> <cols> <nframes> <kind> <k> <std_ratio> <radius> <min_neighbors> <max_iter> <out.bin>
// in : uint16 depth[nframes][rows*cols];  kind < 0: the tracker is left as constructed (no option touched)
// out: per frame pair i=1..nframes-1: int32 status, iterations, source size, target size; float T[16], camR[9], camP[3]
//      then Engine::removeOutliers(0, {RADIUS, r = 0.1, min_neighbors = 6}, stats only) on what the last pair left:
//      int32 status, n_out, n_dropped, source size, n_in; double summary[4]; double value[n_in]; int32 out_index[n_in]
//      then removeOutliers with k = 0 and with which = 2: int32 status, status
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 12) return 2;
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), nframes = std::atoi(argv[4]);
  const int kind = std::atoi(argv[5]), max_iter = std::atoi(argv[10]);
  const icpk_outlier_filter setting{kind, std::atoi(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8]),
                                    std::atoi(argv[9])};
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || rows <= 0 || cols <= 0 || nframes < 2) return 3;
  std::vector<std::vector<uint16_t>> frames(nframes, std::vector<uint16_t>((size_t)rows * cols));
  for (auto& fr : frames)
    if (std::fread(fr.data(), 2, fr.size(), f) != fr.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[11], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    icp::Tracker trk(eng);
    if (kind >= 0) {
      trk.outlierFilter = true;
      trk.outlierSetting = setting;
    }
    for (int i = 1; i < nframes; ++i) {
      float T[16];
      const int rc = trk.getTransformation(frames[i].data(), i == 1 ? frames[0].data() : nullptr, rows, cols, max_iter, 1e-4f, T);
      if (rc < 0) {
        std::fprintf(stderr, "getTransformation failed: %d %s\n", rc, eng.last_error());
        return 6;
      }
      const int32_t head[4] = {rc, trk.lastStats.iterations, icpk_source_size(eng.ctx()), icpk_target_size(eng.ctx())};
      std::fwrite(head, 4, 4, o);
      std::fwrite(T, 4, 16, o);
      std::fwrite(trk.cameraRotation, 4, 9, o);
      std::fwrite(trk.cameraPosition, 4, 3, o);
    }
    const icpk_outlier_filter radius{ICPK_FILTER_RADIUS, 0, 0.f, 0.1f, 6};
    int n_out = -1, n_dropped = -1;
    const int rc = eng.removeOutliers(0, radius, true, &n_out, &n_dropped);
    std::vector<double> value;
    std::vector<int32_t> out_index;
    double summary[4] = {-1, -1, -1, -1};
    const int rs = eng.outlierStats(&value, nullptr, &out_index, summary);
    if (rs != ICPK_OK) return 8;
    const int32_t tail[5] = {rc, n_out, n_dropped, icpk_source_size(eng.ctx()), (int32_t)value.size()};
    std::fwrite(tail, 4, 5, o);
    std::fwrite(summary, 8, 4, o);
    std::fwrite(value.data(), 8, value.size(), o);
    std::fwrite(out_index.data(), 4, out_index.size(), o);
    const icpk_outlier_filter bad_k{ICPK_FILTER_STATISTICAL, 0, 2.f, 0.f, 0};
    const int32_t bad[2] = {eng.removeOutliers(0, bad_k), eng.removeOutliers(2, radius)};
    std::fwrite(bad, 4, 2, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  std::fclose(o);
  return 0;
}
