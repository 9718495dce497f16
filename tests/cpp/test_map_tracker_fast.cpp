// test_map_tracker_fast.cpp -- icp::MapTracker's colour overload (key points detected on the device, icp_map.hpp) over
// a sequence of depth + BGR frames, for tests/test_gpu_live_fast.py.
// in:  int32 rows, cols, frames, max_iterations, fallback frame (min_pairs above any pair count there, -1: none);
//      float32 threshold; frames x rows x cols uint16 depth; frames x rows x cols x 3 uint8 BGR
// out: per call (frames 1 .. n-1, previous = the frame before): int32 status, iterations, key-point list length,
//      point list length, non-zero voxels; float32 T[16]; the key-point list (x plane, y plane, z plane);
//      (voxel offset, certainty) int32 pairs of every non-zero voxel in offset order
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
  int32_t hdr[5];
  float thr = 0.f;
  if (std::fread(hdr, sizeof(hdr), 1, f) != 1 || std::fread(&thr, sizeof(thr), 1, f) != 1) return 2;
  const int rows = hdr[0], cols = hdr[1], nframes = hdr[2], max_iter = hdr[3], fallback = hdr[4];
  std::vector<uint16_t> frames((size_t)nframes * rows * cols);
  std::vector<uint8_t> colors((size_t)nframes * rows * cols * 3);
  if (std::fread(frames.data(), sizeof(uint16_t), frames.size(), f) != frames.size() ||
      std::fread(colors.data(), 1, colors.size(), f) != colors.size())
    return 2;
  std::fclose(f);

  icp::Engine eng(0);
  icp::MapTracker tracker(eng);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::vector<float> x, y, z;
  std::vector<uint8_t> grid;
  for (int k = 1; k < nframes; ++k) {
    const uint16_t* data = frames.data() + (size_t)k * rows * cols;
    const uint16_t* previous = frames.data() + (size_t)(k - 1) * rows * cols;
    const uint8_t* color = colors.data() + (size_t)k * rows * cols * 3;
    float T[16];
    const int32_t min_pairs = tracker.params.min_pairs;
    if (k == fallback) tracker.params.min_pairs = 1 << 30;
    const int rc = tracker.getTransformation(data, previous, rows, cols, color, rows, cols, 3, max_iter, thr, T);
    tracker.params.min_pairs = min_pairs;
    if (rc < 0) {
      std::fprintf(stderr, "frame %d: status %d (%s)\n", k, rc, eng.last_error());
      return 1;
    }
    if (tracker.map.getList(ICPK_MAP_KEYPOINTS, x, y, z) != ICPK_OK || tracker.map.getCertainty(grid) != ICPK_OK) return 1;
    std::vector<int32_t> cells;
    for (size_t v = 0; v < grid.size(); ++v)
      if (grid[v]) {
        cells.push_back((int32_t)v);
        cells.push_back((int32_t)grid[v]);
      }
    const int32_t head[5] = {rc, tracker.lastStats.iterations, (int32_t)x.size(), tracker.map.size(ICPK_MAP_POINTS),
                             (int32_t)(cells.size() / 2)};
    std::fwrite(head, sizeof(head), 1, o);
    std::fwrite(T, sizeof(T), 1, o);
    std::fwrite(x.data(), sizeof(float), x.size(), o);
    std::fwrite(y.data(), sizeof(float), y.size(), o);
    std::fwrite(z.data(), sizeof(float), z.size(), o);
    std::fwrite(cells.data(), sizeof(int32_t), cells.size(), o);
  }
  std::fclose(o);
  // icp::detectFAST on the last colour frame: count, then the key points themselves
  std::vector<float> kp, resp;
  const uint8_t* last = colors.data() + (size_t)(nframes - 1) * rows * cols * 3;
  if (icp::detectFAST(eng, last, rows, cols, 3, kp, &resp) != ICPK_OK) return 1;
  FILE* o2 = std::fopen((std::string(argv[2]) + ".kp").c_str(), "wb");
  if (!o2) return 2;
  const int32_t nk = (int32_t)resp.size();
  std::fwrite(&nk, sizeof(nk), 1, o2);
  std::fwrite(kp.data(), sizeof(float), kp.size(), o2);
  std::fwrite(resp.data(), sizeof(float), resp.size(), o2);
  std::fclose(o2);
  return 0;
}
