// test_map_tracker_dense.cpp -- icp::MapTracker (icp_map.hpp) with dense = true over a sequence of depth frames, for
// tests/test_gpu_map_tracker_dense.py.
// in:  int32 rows, cols, frames, max_iterations, n_keypoints, subsample factor; float32 threshold; uint64 subsample
//      seed; frames x rows x cols uint16; n_keypoints x (x, y) float32
// out: per call (frames 1 .. n-1, previous = the frame before): int32 status, iterations, final pairs, key-point list
//      length, point list length; float32 T[16]; the point list (x plane, y plane, z plane)
#include <cstdio>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[6];
  float thr = 0.f;
  uint64_t seed = 0;
  if (std::fread(hdr, sizeof(hdr), 1, f) != 1 || std::fread(&thr, sizeof(thr), 1, f) != 1 ||
      std::fread(&seed, sizeof(seed), 1, f) != 1)
    return 2;
  const int rows = hdr[0], cols = hdr[1], nframes = hdr[2], max_iter = hdr[3], nkp = hdr[4], factor = hdr[5];
  std::vector<uint16_t> frames((size_t)nframes * rows * cols);
  std::vector<float> kp((size_t)2 * nkp);
  if (std::fread(frames.data(), sizeof(uint16_t), frames.size(), f) != frames.size() ||
      std::fread(kp.data(), sizeof(float), kp.size(), f) != kp.size())
    return 2;
  std::fclose(f);

  icp::Engine eng(0);
  if (icpk_set_subsample(eng.ctx(), factor, seed) != ICPK_OK) return 1;
  icp::MapTracker tracker(eng);
  tracker.dense = true;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::vector<float> x, y, z;
  for (int k = 1; k < nframes; ++k) {
    const uint16_t* data = frames.data() + (size_t)k * rows * cols;
    const uint16_t* previous = frames.data() + (size_t)(k - 1) * rows * cols;
    float T[16];
    const int rc = tracker.getTransformation(data, previous, rows, cols, kp.data(), nkp, max_iter, thr, T);
    if (rc < 0) {
      std::fprintf(stderr, "frame %d: status %d (%s)\n", k, rc, eng.last_error());
      return 1;
    }
    if (tracker.map.getList(ICPK_MAP_POINTS, x, y, z) != ICPK_OK) return 1;
    const int32_t head[5] = {rc, tracker.lastStats.iterations, tracker.lastStats.final_pairs,
                             tracker.map.size(ICPK_MAP_KEYPOINTS), (int32_t)x.size()};
    std::fwrite(head, sizeof(head), 1, o);
    std::fwrite(T, sizeof(T), 1, o);
    std::fwrite(x.data(), sizeof(float), x.size(), o);
    std::fwrite(y.data(), sizeof(float), y.size(), o);
    std::fwrite(z.data(), sizeof(float), z.size(), o);
  }
  std::fclose(o);
  return 0;
}
