// tests/cpp/test_score.cpp -- icp::Engine::scorePoses / scoreCurrent (icp_align.hpp) on one pair; the Python test
// (tests/test_gpu_score_cpp.py) compares them with the C ABI's output written alongside and with the same calls made
// through the binding, bit for bit.
//
//   test_score <in.f32> <ns> <nt> <n_poses> <max_dist> <iterations> <out.bin>
// in : float sx[ns], sy[ns], sz[ns], tx[nt], ty[nt], tz[nt], T[16 * n_poses]
// out: per record  int64 inliers; float fitness, inlierRmse, meanDist, 0; double information[36]; double sums[11]
//      n_poses records of Engine::scorePoses; n_poses records made from icpk_score_poses + the two host functions;
//      after an alignment one record of Engine::scoreCurrent and one of Engine::scorePoses(nullptr, 1, ...);
//      then int32 status of the alignment, status of scorePoses with n = 0, final_pairs, 0
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

static void put(FILE* o, const icp::PoseScore& s) {
  const float m[4] = {s.fitness, s.inlierRmse, s.meanDist, 0.f};
  std::fwrite(&s.inliers, 8, 1, o);
  std::fwrite(m, 4, 4, o);
  std::fwrite(s.information, 8, 36, o);
  std::fwrite(s.sums, 8, ICPK_NSCORE, o);
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int ns = std::atoi(argv[2]), nt = std::atoi(argv[3]), np = std::atoi(argv[4]), iters = std::atoi(argv[6]);
  const float max_d = (float)std::atof(argv[5]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || ns <= 0 || nt <= 0 || np <= 0) return 3;
  std::vector<float> s((size_t)3 * ns), t((size_t)3 * nt), T((size_t)16 * np);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size() ||
      std::fread(T.data(), 4, T.size(), f) != T.size())
    return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[7], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    if (icpk_set_target(eng.ctx(), t.data(), t.data() + nt, t.data() + 2 * (size_t)nt, nt) != ICPK_OK) return 6;
    if (icpk_set_source(eng.ctx(), s.data(), s.data() + ns, s.data() + 2 * (size_t)ns, ns) != ICPK_OK) return 6;
    std::vector<icp::PoseScore> v;
    int rc = eng.scorePoses(T.data(), np, max_d, &v);
    if (rc != ICPK_OK || v.size() != (size_t)np) {
      std::fprintf(stderr, "scorePoses failed: %d %s\n", rc, eng.last_error());
      return 7;
    }
    for (const auto& r : v) put(o, r);
    std::vector<double> sums((size_t)np * ICPK_NSCORE);
    std::vector<int64_t> inl((size_t)np);
    if (icpk_score_poses(eng.ctx(), np, T.data(), max_d, 0, sums.data(), inl.data()) != ICPK_OK) return 8;
    for (int k = 0; k < np; ++k) {
      icp::PoseScore r;
      r.inliers = inl[(size_t)k];
      for (int j = 0; j < ICPK_NSCORE; ++j) r.sums[j] = sums[(size_t)k * ICPK_NSCORE + j];
      icpk_score_metrics(r.sums, r.inliers, ns, &r.fitness, &r.inlierRmse, &r.meanDist);
      icpk_information_matrix(r.sums, r.inliers, r.information);
      put(o, r);
    }
    icp::AlignParams p;
    p.solve = ICPK_SOLVE_KABSCH;
    p.max_iterations = iters;
    p.fixed_iterations = 1;
    p.max_nn_dist = max_d;
    icp::AlignResult res;
    res.status = icpk_align(eng.ctx(), &p, res.T, &res.stats);
    icp::PoseScore cur;
    if (eng.scoreCurrent(max_d, &cur) != ICPK_OK) return 9;
    put(o, cur);
    if (eng.scorePoses(nullptr, 1, max_d, &v) != ICPK_OK || v.size() != 1) return 9;
    put(o, v[0]);
    const int32_t tail[4] = {res.status, eng.scorePoses(T.data(), 0, max_d, &v), res.stats.final_pairs, 0};
    std::fwrite(tail, 4, 4, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
