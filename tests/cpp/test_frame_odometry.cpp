// tests/cpp/test_frame_odometry.cpp -- icp::Engine::buildFrameView / setProjectiveView and icp::FrameOdometry
// (icp_align.hpp, icp_odometry.hpp, K28) over a few depth frames; the Python test (tests/test_gpu_frame_view_cpp.py)
// compares what it writes with odometry.ProjectiveOdometry and the binding's calls, byte for byte.
//
//   test_frame_odometry <in.bin> <out.bin>
// in : int32 rows, cols, n_frames, levels, counts[levels padded to 3], max_angle_deg_on; float fx, cx, max_angle_deg, 0;
//      double pose[16]; per frame uint16 depth[rows * cols]
// out: per frame double pose[16], int32 views_built, per level icpk_projective_result; then of the LAST view: int32
//      levels, per level int32 rows, cols, n_valid, and its eight planes; then int32 pairs: the pixels of level 0 of the
//      last frame that icpk_projective_associate pairs with level 0 of the view at the last pose, through
//      Engine::setProjectiveView
// The poses' translations are printed as well.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_odometry.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[8];
  float cam[4];
  double pose0[16];
  if (std::fread(head, 4, 8, f) != 8 || std::fread(cam, 4, 4, f) != 4 || std::fread(pose0, 8, 16, f) != 16) return 4;
  const int rows = head[0], cols = head[1], frames = head[2], levels = head[3];
  if (rows < 1 || cols < 1 || frames < 1 || levels < 1 || levels > 3) return 4;
  const size_t npix = (size_t)rows * cols;
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  for (int k = 0; k < frames; ++k)
    if (std::fread(depth[k].data(), 2, npix, f) != npix) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  try {
    icp::Engine eng(0);
    if (eng.frameViewLevels() != 0 || eng.setProjectiveView(ICPK_VIEW_FRAME, 0) != ICPK_E_NOT_SET ||
        eng.buildFrameView(cam[0], cam[1], pose0) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "a frame view before the first pyramid\n");
      return 5;
    }
    icp::FrameOdometry odo(eng, pose0, cam[0], cam[1], std::vector<int>(head + 4, head + 4 + levels));
    if (head[7]) odo.keyframe.on = true, odo.keyframe.maxAngleDeg = cam[2];
    double pose[16];
    for (int k = 0; k < frames; ++k) {
      if (int rc = odo.track(depth[k].data(), rows, cols, pose)) {
        std::fprintf(stderr, "track failed at frame %d: %d %s\n", k, rc, eng.last_error());
        return 5;
      }
      std::fwrite(pose, 8, 16, o);
      const int32_t built = odo.viewsBuilt;
      std::fwrite(&built, 4, 1, o);
      std::fwrite(odo.levelStats.data(), sizeof(icpk_projective_result), odo.levelStats.size(), o);
      std::printf("frame %d: t = %.6f %.6f %.6f, %d views built\n", k, pose[3], pose[7], pose[11], built);
    }
    const int32_t L = eng.frameViewLevels();
    std::fwrite(&L, 4, 1, o);
    for (int l = 0; l < L; ++l) {
      int r = 0, c = 0;
      if (eng.frameViewLevel(l, &r, &c) != ICPK_OK) return 5;
      std::vector<float> planes((size_t)8 * r * c);
      if (eng.frameViewLevel(l, &r, &c, planes.data()) != ICPK_OK) return 5;
      const int32_t shape[3] = {r, c, odo.levelValid[l]};
      std::fwrite(shape, 4, 3, o);
      std::fwrite(planes.data(), 4, planes.size(), o);
    }
    icpk_projective_params p = odo.params;
    p.level = 0;
    std::vector<int32_t> pixel(npix);
    if (eng.setProjectiveView(ICPK_VIEW_FRAME, 0) != ICPK_OK ||
        icpk_projective_associate(eng.ctx(), &p, pose, pixel.data(), nullptr) != ICPK_OK || eng.setProjectiveView(2, 0) != ICPK_E_ARG ||
        eng.setProjectiveView(ICPK_VIEW_RAYCAST) != ICPK_OK || icpk_projective_associate(eng.ctx(), &p, pose, pixel.data(), nullptr) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "setProjectiveView: %s\n", eng.last_error());
      return 5;
    }
    int32_t pairs = 0;
    for (int32_t j : pixel) pairs += j >= 0;
    std::fwrite(&pairs, 4, 1, o);
    if (eng.releaseFrameView() != ICPK_OK || eng.frameViewLevels() != 0) return 5;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  std::fclose(o);
  return 0;
}
