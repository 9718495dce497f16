// tests/cpp/test_tsdf_refuse.cpp -- icp::TsdfVolume::integrate / deintegrate / apply / refuse (icp_tsdf.hpp, K30) over a
// few posed frames; the Python test (tests/test_gpu_tsdf_refuse_cpp.py) compares what it writes with the same calls made
// through the binding, byte for byte.
//
//   test_tsdf_refuse <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame double
//      old_pose[16], new_pose[16]; uint16 depth[rows * cols]; with ICPK_TSDF_COLOR float intensity[rows * cols]
// The frames are fused at their old poses, the last is taken out and put back (deintegrate, apply with one +1 op), and
// all are moved to their new poses (refuse).
// out: int64 removed and added per frame [2 * n_frames]; int32 n of the deintegrate, int64 n of the one-op apply; float
//      tsdf[n]; uint16 weight[n]; with colour float intensity[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_tsdf.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[8];
  float geo[8];
  if (std::fread(head, 4, 8, f) != 8 || std::fread(geo, 4, 8, f) != 8) return 4;
  icpk_tsdf_params p = icp::TsdfVolume::defaults();
  for (int a = 0; a < 3; ++a) p.dims[a] = head[a], p.origin[a] = geo[1 + a];
  p.max_weight = head[3], p.flags = head[4];
  p.voxel = geo[0], p.trunc = geo[4];
  const int rows = head[5], cols = head[6], frames = head[7];
  if (rows < 1 || cols < 1 || frames < 1) return 4;
  const bool color = (p.flags & ICPK_TSDF_COLOR) != 0;
  const size_t npix = (size_t)rows * cols;
  std::vector<double> oldp((size_t)16 * frames), newp((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  std::vector<std::vector<float>> inten(frames, std::vector<float>(color ? npix : 0));
  for (int k = 0; k < frames; ++k) {
    if (std::fread(oldp.data() + 16 * (size_t)k, 8, 16, f) != 16 || std::fread(newp.data() + 16 * (size_t)k, 8, 16, f) != 16) return 4;
    if (std::fread(depth[k].data(), 2, npix, f) != npix) return 4;
    if (color && std::fread(inten[k].data(), 4, npix, f) != npix) return 4;
  }
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    std::vector<const uint16_t*> d;
    std::vector<const float*> c;
    for (int k = 0; k < frames; ++k) {
      d.push_back(depth[k].data());
      if (color) c.push_back(inten[k].data());
    }
    int rc = 0;
    for (int k = 0; k < frames && !rc; ++k)
      rc = vol.integrate(d[k], rows, cols, oldp.data() + 16 * (size_t)k, color ? c[k] : nullptr);
    const int last = frames - 1;
    int32_t taken = -1;
    if (!rc) rc = vol.deintegrate(d[last], rows, cols, oldp.data() + 16 * (size_t)last, color ? c[last] : nullptr, &taken);
    icpk_tsdf_op back;
    back.sign = +1, back.frame = 0;
    for (int q = 0; q < 16; ++q) back.pose[q] = oldp[16 * (size_t)last + q];
    std::vector<int64_t> put, moved;
    if (!rc) rc = vol.apply({d[last]}, rows, cols, {back}, color ? std::vector<const float*>{c[last]} : std::vector<const float*>{}, &put);
    if (!rc) rc = vol.refuse(d, rows, cols, oldp, newp, c, &moved);
    const size_t n = vol.voxels();
    std::vector<float> tsdf(n), ci(color ? n : 0);
    std::vector<uint16_t> weight(n);
    if (!rc) rc = vol.planes(tsdf.data(), weight.data(), color ? ci.data() : nullptr);
    if (rc) {
      std::fprintf(stderr, "a call failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    // the refusals come through the mirror as statuses
    std::vector<icpk_tsdf_op> many(ICPK_TSDF_MAX_OPS + 1, back);
    if (vol.apply({d[0]}, rows, cols, many) != ICPK_E_ARG || vol.apply({d[0]}, rows, cols, {}) != ICPK_E_ARG) return 8;
    if (vol.refuse(d, rows, cols, oldp, std::vector<double>(16), c) != ICPK_E_ARG) return 8;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    std::fwrite(moved.data(), 8, moved.size(), o);
    std::fwrite(&taken, 4, 1, o);
    std::fwrite(put.data(), 8, 1, o);
    std::fwrite(tsdf.data(), 4, n, o);
    std::fwrite(weight.data(), 2, n, o);
    std::fwrite(ci.data(), 4, ci.size(), o);
    std::fclose(o);
    std::printf("refused %d frames; the last one: %d voxels out, %lld back in\n", frames, taken, (long long)put[0]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
