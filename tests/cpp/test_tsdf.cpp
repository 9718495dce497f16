// tests/cpp/test_tsdf.cpp -- icp::TsdfVolume (icp_tsdf.hpp) over a few posed frames; the Python test
// (tests/test_gpu_tsdf_cpp.py) compares what it writes with the same calls made through the binding, byte for byte.
//
//   test_tsdf <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame
//      double pose[16]; uint16 depth[rows * cols]; with ICPK_TSDF_COLOR float intensity[rows * cols]
// out: int32 n_updated[n_frames]; int32 n_points, n_no_normal; float tsdf[n]; uint16 weight[n]; with colour float
//      intensity[n]; float x, y, z, nx, ny, nz, intensity [n_points] each; int32 voxel[n_points]; uint8 axis[n_points]
// The counts are printed as well.
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
  std::vector<double> poses((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  std::vector<std::vector<float>> inten(frames, std::vector<float>(color ? npix : 0));
  for (int k = 0; k < frames; ++k) {
    if (std::fread(poses.data() + 16 * (size_t)k, 8, 16, f) != 16 || std::fread(depth[k].data(), 2, npix, f) != npix) return 4;
    if (color && std::fread(inten[k].data(), 4, npix, f) != npix) return 4;
  }
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    std::vector<int32_t> updated(frames, -1);
    for (int k = 0; k < frames; ++k) {
      const int rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k, color ? inten[k].data() : nullptr,
                                   &updated[k]);
      if (rc) {
        std::fprintf(stderr, "integrate failed: %d %s\n", rc, eng.last_error());
        return 5;
      }
    }
    icp::TsdfSurface s;
    if (int rc = vol.surface(s, 1)) {
      std::fprintf(stderr, "surface failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    const size_t n = vol.voxels();
    std::vector<float> tsdf(n), ci(color ? n : 0);
    std::vector<uint16_t> weight(n);
    if (int rc = vol.planes(tsdf.data(), weight.data(), color ? ci.data() : nullptr)) {
      std::fprintf(stderr, "planes failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[2] = {(int32_t)s.size(), s.noNormal};
    std::fwrite(updated.data(), 4, updated.size(), o);
    std::fwrite(counts, 4, 2, o);
    std::fwrite(tsdf.data(), 4, n, o);
    std::fwrite(weight.data(), 2, n, o);
    std::fwrite(ci.data(), 4, ci.size(), o);
    for (const std::vector<float>* v : {&s.x, &s.y, &s.z, &s.nx, &s.ny, &s.nz, &s.intensity}) std::fwrite(v->data(), 4, v->size(), o);
    std::fwrite(s.voxel.data(), 4, s.voxel.size(), o);
    std::fwrite(s.axis.data(), 1, s.axis.size(), o);
    std::fclose(o);
    for (int k = 0; k < frames; ++k) std::printf("frame %d: %d voxels\n", k, updated[k]);
    std::printf("surface: %zu points, %d without a normal\n", s.size(), s.noNormal);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
