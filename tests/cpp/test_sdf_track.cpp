// tests/cpp/test_sdf_track.cpp -- icp::TsdfVolume::alignSdf / sdfReduce / sdfAssociate / sdfTrace (icp_tsdf.hpp, K29) over
// a few posed frames and one frame's pyramid; the Python test (tests/test_gpu_sdf_track_cpp.py) compares what it writes
// with the same calls made through the binding, byte for byte.
//
//   test_sdf_track <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame
//      double pose[16]; uint16 depth[rows * cols]; then the frame to align: int32 rows, cols, levels, level,
//      max_iterations, min_pairs, min_weight, 0; float fx, cx, max_abs_tsdf, min_normal_cos; double estimate[16];
//      uint16 depth[rows * cols]
// out: int32 status, iterations, n_trace, accepted pixels counted from the cells; int64 count; double mean_dist;
//      double pose[16]; icpk_projective_iter [n_trace]; int32 cell [level pixels]; float value [level pixels];
//      double sums[28]; int64 count of sdfReduce at the estimate
// The result is printed as well.
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
  if (rows < 1 || cols < 1 || frames < 1 || p.flags != 0) return 4;
  const size_t npix = (size_t)rows * cols;
  std::vector<double> poses((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  for (int k = 0; k < frames; ++k)
    if (std::fread(poses.data() + 16 * (size_t)k, 8, 16, f) != 16 || std::fread(depth[k].data(), 2, npix, f) != npix) return 4;
  int32_t fi[8];
  float ff[4];
  double estimate[16];
  if (std::fread(fi, 4, 8, f) != 8 || std::fread(ff, 4, 4, f) != 4 || std::fread(estimate, 8, 16, f) != 16) return 4;
  if (fi[0] < 1 || fi[1] < 1) return 4;
  std::vector<uint16_t> frame((size_t)fi[0] * fi[1]);
  if (std::fread(frame.data(), 2, frame.size(), f) != frame.size()) return 4;
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    icpk_sdf_params sp = vol.sdfDefaults(fi[3]);
    sp.fx = ff[0], sp.cx = ff[1], sp.max_abs_tsdf = ff[2], sp.min_normal_cos = ff[3];
    sp.max_iterations = fi[4], sp.min_pairs = fi[5], sp.min_weight = fi[6];
    double out_pose[16];
    icpk_projective_result res;
    std::vector<int32_t> cell;
    std::vector<float> value;
    if (vol.alignSdf(sp, estimate, out_pose, &res) != ICPK_E_NOT_SET ||
        vol.sdfAssociate(sp, estimate, cell, value) != ICPK_E_NOT_SET || !vol.sdfTrace().empty()) {
      std::fprintf(stderr, "an alignment before the first pyramid\n");
      return 5;
    }
    for (int k = 0; k < frames; ++k)
      if (int rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k)) {
        std::fprintf(stderr, "integrate failed: %d %s\n", rc, eng.last_error());
        return 5;
      }
    icpk_pyramid_params pp;
    icpk_default_pyramid_params(&pp);
    pp.levels = fi[2];
    if (int rc = eng.buildDepthPyramid(frame.data(), fi[0], fi[1], &pp)) {
      std::fprintf(stderr, "buildDepthPyramid failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    const int status = vol.alignSdf(sp, estimate, out_pose, &res);  // (no ray cast was ever made)
    if (status < 0 || status != res.status) {
      std::fprintf(stderr, "alignSdf failed: %d %s\n", status, eng.last_error());
      return 5;
    }
    const std::vector<icpk_projective_iter> trace = vol.sdfTrace();
    if (int rc = vol.sdfAssociate(sp, estimate, cell, value)) {
      std::fprintf(stderr, "sdfAssociate failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    double sums[ICPK_NP2L];
    int64_t count = -1;
    if (int rc = vol.sdfReduce(sp, estimate, sums, &count)) {
      std::fprintf(stderr, "sdfReduce failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    int32_t accepted = 0;
    for (int32_t j : cell) accepted += j >= 0;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[4] = {res.status, res.iterations, (int32_t)trace.size(), accepted};
    std::fwrite(counts, 4, 4, o);
    std::fwrite(&res.count, 8, 1, o);
    std::fwrite(&res.mean_dist, 8, 1, o);
    std::fwrite(out_pose, 8, 16, o);
    std::fwrite(trace.data(), sizeof(icpk_projective_iter), trace.size(), o);
    std::fwrite(cell.data(), 4, cell.size(), o);
    std::fwrite(value.data(), 4, value.size(), o);
    std::fwrite(sums, 8, ICPK_NP2L, o);
    std::fwrite(&count, 8, 1, o);
    std::fclose(o);
    std::printf("sdf level %d: status %d after %d updates, %lld accepted at the last evaluation, %d at the estimate\n", sp.level,
                res.status, res.iterations, (long long)res.count, accepted);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
