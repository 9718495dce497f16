// tests/cpp/test_voxel.cpp -- icp::Tracker with voxelLeaf / voxelMode and icp::Engine::voxelDownsample (icp_align.hpp)
// on a sequence of depth frames; the Python test (tests/test_gpu_voxel.py) makes the same calls by hand through the
// C ABI and compares bit for bit.
//
//   test_voxel <frames.u16> <rows> <cols> <nframes> <leaf> <mode> <max_iter> <out.bin>
// in : uint16 depth[nframes][rows*cols];  leaf 0: the tracker is left as constructed (no option touched)
// out: per frame pair i=1..nframes-1: int32 status, iterations, source size, target size; float T[16], camR[9], camP[3]
//      then Engine::voxelDownsample(0, 0.1, ICPK_VOXEL_FIRST, &n) on what the last pair left: int32 status, n, source size
//      then Engine::voxelDownsample(0, -1, ...) and (0, 0.1, mode 7): int32 status, status
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), nframes = std::atoi(argv[4]);
  const float leaf = (float)std::atof(argv[5]);
  const int mode = std::atoi(argv[6]), max_iter = std::atoi(argv[7]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || rows <= 0 || cols <= 0 || nframes < 2) return 3;
  std::vector<std::vector<uint16_t>> frames(nframes, std::vector<uint16_t>((size_t)rows * cols));
  for (auto& fr : frames)
    if (std::fread(fr.data(), 2, fr.size(), f) != fr.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[8], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    icp::Tracker trk(eng);
    if (leaf > 0.f) {
      trk.voxelLeaf = leaf;
      trk.voxelMode = mode;
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
    int n = -1;
    const int rc = eng.voxelDownsample(0, 0.1f, ICPK_VOXEL_FIRST, &n);
    const int32_t tail[5] = {rc, n, icpk_source_size(eng.ctx()), eng.voxelDownsample(0, -1.f), eng.voxelDownsample(0, 0.1f, 7)};
    std::fwrite(tail, 4, 5, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  std::fclose(o);
  return 0;
}
