// tests/cpp/test_tsdf_shift.cpp -- icp::TsdfVolume::extractLeaving / getBox / shift / params (icp_tsdf.hpp, K23) over a
// few posed frames; the Python test (tests/test_gpu_tsdf_shift_cpp.py) compares what it writes with the same calls made
// through the binding, byte for byte.
//
//   test_tsdf_shift <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; int32 s[3],
//      lo[3], hi[3]; per frame double pose[16]; uint16 depth[rows * cols]; with ICPK_TSDF_COLOR float intensity[rows * cols]
// out: int32 n_leaving, n_no_normal; the leaving list of s: float x, y, z, nx, ny, nz, intensity [n_leaving] each, int32
//      voxel[n_leaving], uint8 axis[n_leaving]; the box [lo, hi) before the shift: float tsdf[m], uint16 weight[m], with
//      colour float intensity[m]; then, after shift(s): int64 total[3]; float origin[3]; float tsdf[n]; uint16 weight[n];
//      with colour float intensity[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_tsdf.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[8], box[9];
  float geo[8];
  if (std::fread(head, 4, 8, f) != 8 || std::fread(geo, 4, 8, f) != 8 || std::fread(box, 4, 9, f) != 9) return 4;
  icpk_tsdf_params p = icp::TsdfVolume::defaults();
  for (int a = 0; a < 3; ++a) p.dims[a] = head[a], p.origin[a] = geo[1 + a];
  p.max_weight = head[3], p.flags = head[4];
  p.voxel = geo[0], p.trunc = geo[4];
  const int rows = head[5], cols = head[6], frames = head[7];
  if (rows < 1 || cols < 1 || frames < 1) return 4;
  const int32_t *s = box, *lo = box + 3, *hi = box + 6;
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
    int rc = 0;
    for (int k = 0; k < frames && !rc; ++k)
      rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k, color ? inten[k].data() : nullptr);
    icp::TsdfSurface left;
    if (!rc) rc = vol.extractLeaving(left, s, 1);
    size_t m = 1;
    for (int a = 0; a < 3; ++a) m *= hi[a] > lo[a] ? (size_t)(hi[a] - lo[a]) : 0;
    std::vector<float> bf(m), bc(color ? m : 0);
    std::vector<uint16_t> bw(m);
    if (!rc) rc = vol.getBox(lo, hi, bf.data(), bw.data(), color ? bc.data() : nullptr);
    if (!rc) rc = vol.shift(s);
    const size_t n = vol.voxels();
    std::vector<float> tsdf(n), ci(color ? n : 0);
    std::vector<uint16_t> weight(n);
    if (!rc) rc = vol.planes(tsdf.data(), weight.data(), color ? ci.data() : nullptr);
    if (rc) {
      std::fprintf(stderr, "a call failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    // what the shift dropped is gone for the mirror as well
    icp::TsdfMesh mesh;
    if (vol.getMesh(mesh) != ICPK_E_NOT_SET || vol.toTarget() != ICPK_E_NOT_SET) return 8;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[2] = {(int32_t)left.size(), left.noNormal};
    std::fwrite(counts, 4, 2, o);
    for (const std::vector<float>* v : {&left.x, &left.y, &left.z, &left.nx, &left.ny, &left.nz, &left.intensity})
      std::fwrite(v->data(), 4, v->size(), o);
    std::fwrite(left.voxel.data(), 4, left.voxel.size(), o);
    std::fwrite(left.axis.data(), 1, left.axis.size(), o);
    std::fwrite(bf.data(), 4, m, o);
    std::fwrite(bw.data(), 2, m, o);
    std::fwrite(bc.data(), 4, bc.size(), o);
    std::fwrite(vol.total(), 8, 3, o);
    std::fwrite(vol.params().origin, 4, 3, o);
    std::fwrite(tsdf.data(), 4, n, o);
    std::fwrite(weight.data(), 2, n, o);
    std::fwrite(ci.data(), 4, ci.size(), o);
    std::fclose(o);
    std::printf("leaving: %zu points, %d without a normal; shifted by %lld %lld %lld\n", left.size(), left.noNormal,
                (long long)vol.total()[0], (long long)vol.total()[1], (long long)vol.total()[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
