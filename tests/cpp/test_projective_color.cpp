// tests/cpp/test_projective_color.cpp -- icp::Engine::setPyramidIntensity, icp::TsdfVolume::raycastColorGradients /
// alignProjectiveColored (icp_align.hpp, icp_tsdf.hpp, K26) over a few posed colour frames, one view and one frame's
// pyramid; the Python test (tests/test_gpu_projective_color_cpp.py) compares what it writes with the same calls made
// through the binding, byte for byte.
//
//   test_projective_color <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame
//      double pose[16]; uint16 depth[rows * cols]; float intensity[rows * cols]; then the view: int32 rows, cols,
//      min_weight, min_neighbors; float z_near, z_far, step, radius; double pose[16]; then the frame to align: int32 rows,
//      cols, levels, level, max_iterations, min_pairs, 0, 0; float fx, cx, max_dist, lambda_geometric; double estimate[16];
//      uint16 depth[rows * cols]; float intensity[rows * cols]
// out: int32 status, iterations, n_trace, 0; int64 count; double mean_dist; double pose[16];
//      icpk_projective_iter [n_trace]; float gx, gy, gz [view pixels each]; float intensity level [level pixels]
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
  if (rows < 1 || cols < 1 || frames < 1 || p.flags != ICPK_TSDF_COLOR) return 4;
  const size_t npix = (size_t)rows * cols;
  std::vector<double> poses((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  std::vector<std::vector<float>> inten(frames, std::vector<float>(npix));
  for (int k = 0; k < frames; ++k)
    if (std::fread(poses.data() + 16 * (size_t)k, 8, 16, f) != 16 || std::fread(depth[k].data(), 2, npix, f) != npix ||
        std::fread(inten[k].data(), 4, npix, f) != npix)
      return 4;
  int32_t vi[4], fi[8];
  float vf[4], ff[4];
  double view[16], estimate[16];
  if (std::fread(vi, 4, 4, f) != 4 || std::fread(vf, 4, 4, f) != 4 || std::fread(view, 8, 16, f) != 16) return 4;
  if (std::fread(fi, 4, 8, f) != 8 || std::fread(ff, 4, 4, f) != 4 || std::fread(estimate, 8, 16, f) != 16) return 4;
  if (fi[0] < 1 || fi[1] < 1 || vi[0] < 1 || vi[1] < 1) return 4;
  std::vector<uint16_t> frame((size_t)fi[0] * fi[1]);
  std::vector<float> frame_i(frame.size());
  if (std::fread(frame.data(), 2, frame.size(), f) != frame.size() || std::fread(frame_i.data(), 4, frame_i.size(), f) != frame_i.size())
    return 4;
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    icpk_projective_params jp = vol.projectiveDefaults(fi[3]);
    jp.fx = ff[0], jp.cx = ff[1], jp.max_dist = ff[2];
    jp.max_iterations = fi[4], jp.min_pairs = fi[5];
    icpk_projective_color_params cp;
    icpk_default_projective_color_params(&cp);
    cp.lambda_geometric = ff[3];
    double out_pose[16];
    icpk_projective_result res;
    if (vol.alignProjectiveColored(jp, &cp, estimate, out_pose, &res) != ICPK_E_NOT_SET ||
        vol.raycastColorGradients(vf[3], vi[3]) != ICPK_E_NOT_SET ||
        eng.setPyramidIntensity(frame_i.data(), fi[0], fi[1]) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "a coloured call before the first ray cast / pyramid\n");
      return 5;
    }
    for (int k = 0; k < frames; ++k)
      if (int rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k, inten[k].data())) {
        std::fprintf(stderr, "integrate failed: %d %s\n", rc, eng.last_error());
        return 5;
      }
    icpk_tsdf_raycast_params r = vol.raycastDefaults(vi[0], vi[1]);
    r.min_weight = vi[2], r.z_near = vf[0], r.z_far = vf[1], r.step = vf[2];
    if (int rc = vol.raycast(r, view)) {
      std::fprintf(stderr, "raycast failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    if (int rc = vol.raycastColorGradients(vf[3], vi[3])) {
      std::fprintf(stderr, "raycastColorGradients failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    icpk_pyramid_params pp;
    icpk_default_pyramid_params(&pp);
    pp.levels = fi[2];
    if (int rc = eng.buildDepthPyramid(frame.data(), fi[0], fi[1], &pp)) {
      std::fprintf(stderr, "buildDepthPyramid failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    if (vol.alignProjectiveColored(jp, &cp, estimate, out_pose, &res) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "an alignment without the frame's intensities\n");
      return 5;
    }
    if (int rc = eng.setPyramidIntensity(frame_i.data(), fi[0], fi[1])) {
      std::fprintf(stderr, "setPyramidIntensity failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    const int status = vol.alignProjectiveColored(jp, &cp, estimate, out_pose, &res);
    if (status < 0 || status != res.status) {
      std::fprintf(stderr, "alignProjectiveColored failed: %d %s\n", status, eng.last_error());
      return 5;
    }
    const std::vector<icpk_projective_iter> trace = vol.projectiveTrace();
    const size_t nview = (size_t)vi[0] * vi[1];
    std::vector<float> g(3 * nview);
    if (int rc = vol.getRaycastColorGradients(g.data(), g.data() + nview, g.data() + 2 * nview)) {
      std::fprintf(stderr, "getRaycastColorGradients failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    int lr = 0, lc = 0;
    if (eng.depthPyramidLevel(jp.level, &lr, &lc) != ICPK_OK) return 5;
    std::vector<float> level((size_t)lr * lc);
    if (int rc = eng.pyramidIntensityLevel(jp.level, level.data())) {
      std::fprintf(stderr, "pyramidIntensityLevel failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[4] = {res.status, res.iterations, (int32_t)trace.size(), 0};
    std::fwrite(counts, 4, 4, o);
    std::fwrite(&res.count, 8, 1, o);
    std::fwrite(&res.mean_dist, 8, 1, o);
    std::fwrite(out_pose, 8, 16, o);
    std::fwrite(trace.data(), sizeof(icpk_projective_iter), trace.size(), o);
    std::fwrite(g.data(), 4, g.size(), o);
    std::fwrite(level.data(), 4, level.size(), o);
    std::fclose(o);
    std::printf("coloured projective level %d: status %d after %d updates, %lld pairs at the last evaluation\n", jp.level, res.status,
                res.iterations, (long long)res.count);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
