// tests/cpp/test_fern.cpp -- icp::FernDatabase and icp::TsdfVolume::relocalise (icp_tsdf.hpp, K27) over a few posed
// frames and one query frame; the Python test (tests/test_gpu_fern_cpp.py) compares what it writes with the same calls
// made through the binding, byte for byte.
//
//   test_fern <in.bin> <out.bin>
// in : int32 dims[3], rows, cols, n_frames, k, level; float voxel, origin[3], trunc, fx, cx, step; per frame double
//      pose[16]; uint16 depth[rows * cols]; then the query frame: uint16 depth[rows * cols]
// out: per frame int32 n, index[8], diss[8], valid, added; int32 n_keyframes; per keyframe uint32 code[F / 8], double
//      pose[16]; then the query: int32 n, index[8], diss[8], valid, keyframe, status, iterations, 0; int64 count; double
//      mean_dist; double pose[16]
// The result is printed as well.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_tsdf.hpp"

static void write_matches(FILE* o, const icp::FernMatches& m) {
  int32_t rec[1 + 2 * ICPK_FERN_MAX_K] = {(int32_t)m.index.size()};
  for (size_t j = 0; j < m.index.size(); ++j) rec[1 + j] = m.index[j], rec[1 + ICPK_FERN_MAX_K + j] = m.diss[j];
  std::fwrite(rec, 4, 1 + 2 * ICPK_FERN_MAX_K, o);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[8];
  float geo[8];
  if (std::fread(head, 4, 8, f) != 8 || std::fread(geo, 4, 8, f) != 8) return 4;
  icpk_tsdf_params p = icp::TsdfVolume::defaults();
  for (int a = 0; a < 3; ++a) p.dims[a] = head[a], p.origin[a] = geo[1 + a];
  p.voxel = geo[0], p.trunc = geo[4];
  const int rows = head[3], cols = head[4], frames = head[5], k = head[6], level = head[7];
  if (rows < 1 || cols < 1 || frames < 1 || level < 0 || level >= ICPK_PYRAMID_MAX_LEVELS) return 4;
  const size_t npix = (size_t)rows * cols;
  std::vector<double> poses((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames + 1, std::vector<uint16_t>(npix));
  for (int i = 0; i < frames; ++i)
    if (std::fread(poses.data() + 16 * (size_t)i, 8, 16, f) != 16 || std::fread(depth[i].data(), 2, npix, f) != npix) return 4;
  if (std::fread(depth[frames].data(), 2, npix, f) != npix) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    icpk_pyramid_params pp;
    icpk_default_pyramid_params(&pp);
    pp.levels = level + 1;
    icpk_fern_params fp = icp::FernDatabase::defaults();
    fp.level = level;
    int lr = rows, lc = cols;
    for (int l = 0; l < level; ++l) lr = (lr + 1) / 2, lc = (lc + 1) / 2;
    icp::FernDatabase db(eng, fp, lr, lc);
    icp::FernMatches m;
    if (db.size() != 0 || db.process(nullptr, k, m) != ICPK_E_NOT_SET || db.query(k, m) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "a fern call before the first pyramid\n");
      return 5;
    }
    for (int i = 0; i < frames; ++i) {
      const double* pose = poses.data() + 16 * (size_t)i;
      int rc = eng.buildDepthPyramid(depth[i].data(), rows, cols, &pp);
      if (!rc) rc = vol.integrate(depth[i].data(), rows, cols, pose);
      if (!rc) rc = db.process(pose, k, m);
      if (rc) {
        std::fprintf(stderr, "frame %d failed: %d %s\n", i, rc, eng.last_error());
        return 5;
      }
      write_matches(o, m);
      const int32_t tail[2] = {m.valid, m.added};
      std::fwrite(tail, 4, 2, o);
    }
    const int32_t n = db.size();
    std::fwrite(&n, 4, 1, o);
    std::vector<uint32_t> code(db.words());
    for (int j = 0; j < n; ++j) {
      double pose[16];
      if (int rc = db.keyframe(j, code.data(), pose)) {
        std::fprintf(stderr, "keyframe %d failed: %d %s\n", j, rc, eng.last_error());
        return 5;
      }
      std::fwrite(code.data(), 4, code.size(), o);
      std::fwrite(pose, 8, 16, o);
    }
    // the query frame: looked up, and the alignment restarted from the keyframes' poses
    if (int rc = eng.buildDepthPyramid(depth[frames].data(), rows, cols, &pp)) {
      std::fprintf(stderr, "buildDepthPyramid failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    if (int rc = db.process(nullptr, k, m)) {
      std::fprintf(stderr, "process failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    write_matches(o, m);
    icpk_tsdf_raycast_params r = vol.raycastDefaults(lr, lc);
    const float scale = (float)(1 << level);
    r.fx = geo[5] / scale, r.cx = geo[6] / scale, r.step = geo[7];
    const icpk_projective_params jp = vol.projectiveDefaults(level);
    double found[16] = {0};
    int32_t keyframe = -1;
    icpk_projective_result res = {0, 0, 0, 0.0};
    if (int rc = vol.relocalise(db, k, r, jp, found, &keyframe, &res)) {
      std::fprintf(stderr, "relocalise failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    const int32_t tail[5] = {m.valid, keyframe, res.status, res.iterations, 0};
    std::fwrite(tail, 4, 5, o);
    std::fwrite(&res.count, 8, 1, o);
    std::fwrite(&res.mean_dist, 8, 1, o);
    std::fwrite(found, 8, 16, o);
    std::fclose(o);
    std::printf("fern database: %d keyframes of %d frames; the query restarted from keyframe %d with %lld pairs\n", n, frames,
                keyframe, (long long)res.count);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
