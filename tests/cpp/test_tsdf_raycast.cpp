// tests/cpp/test_tsdf_raycast.cpp -- icp::TsdfVolume::raycast / getRaycast / raycastToTarget (icp_tsdf.hpp, K20) over a
// few posed frames and one view; the Python test (tests/test_gpu_tsdf_raycast_cpp.py) compares what it writes with the
// same calls made through the binding, byte for byte.
//
//   test_tsdf_raycast <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame
//      double pose[16]; uint16 depth[rows * cols]; with ICPK_TSDF_COLOR float intensity[rows * cols]; then the view:
//      int32 rows, cols, min_weight, 0; float z_near, z_far, step, 0; double pose[16]
// out: int32 n_hits, n_no_normal, n_target, hits counted from the depth plane; float x, y, z, nx, ny, nz, depth,
//      intensity [rows * cols] each; float target x, y, z, normals x, y, z [n_target] each
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
  int32_t vi[4];
  float vf[4];
  double view[16];
  if (std::fread(vi, 4, 4, f) != 4 || std::fread(vf, 4, 4, f) != 4 || std::fread(view, 8, 16, f) != 16) return 4;
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    icp::TsdfRaycast none;
    if (vol.getRaycast(none) != ICPK_E_NOT_SET || vol.raycastToTarget() != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "maps before the first ray cast\n");
      return 5;
    }
    for (int k = 0; k < frames; ++k) {
      const int rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k, color ? inten[k].data() : nullptr);
      if (rc) {
        std::fprintf(stderr, "integrate failed: %d %s\n", rc, eng.last_error());
        return 5;
      }
    }
    icpk_tsdf_raycast_params r = vol.raycastDefaults(vi[0], vi[1]);
    r.min_weight = vi[2], r.z_near = vf[0], r.z_far = vf[1], r.step = vf[2];
    int32_t hits = -1, dropped = -1;
    if (int rc = vol.raycast(r, view, &hits, &dropped)) {
      std::fprintf(stderr, "raycast failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    icp::TsdfRaycast m;
    if (int rc = vol.getRaycast(m)) {
      std::fprintf(stderr, "getRaycast failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    if (int rc = vol.raycastToTarget()) {
      std::fprintf(stderr, "raycastToTarget failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    const int32_t nt = icpk_target_size(eng.ctx());
    std::vector<float> t(6 * (size_t)nt);
    float* tp = t.data();
    if (icpk_get_target(eng.ctx(), tp, tp + nt, tp + 2 * (size_t)nt) ||
        icpk_get_target_normals(eng.ctx(), tp + 3 * (size_t)nt, tp + 4 * (size_t)nt, tp + 5 * (size_t)nt)) {
      std::fprintf(stderr, "the target could not be read: %s\n", eng.last_error());
      return 5;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[4] = {hits, dropped, nt, m.hits};
    std::fwrite(counts, 4, 4, o);
    for (const std::vector<float>* v : {&m.x, &m.y, &m.z, &m.nx, &m.ny, &m.nz, &m.depth, &m.intensity}) std::fwrite(v->data(), 4, v->size(), o);
    std::fwrite(t.data(), 4, t.size(), o);
    std::fclose(o);
    std::printf("ray cast %d x %d: %d hits, %d without a normal, target of %d points\n", m.rows, m.cols, hits, dropped, nt);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
