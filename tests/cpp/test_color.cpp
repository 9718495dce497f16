// tests/cpp/test_color.cpp -- icp::Engine::setTargetColors / setSourceColors / estimateTargetColorGradients / setColored
// (icp_align.hpp) and a colored point-to-plane alignment on one pair; the Python test (tests/test_gpu_color_cpp.py)
// makes the same calls through the binding and compares bit for bit.
//
//   test_color <pair.f32> <ns> <nt> <radius> <min_neighbors> <lambda> <max_nn_dist> <iterations> <out.bin>
// in : float sx[ns], sy[ns], sz[ns], si[ns], tx[nt], ty[nt], tz[nt], tnx[nt], tny[nt], tnz[nt], ti[nt]
// out: int32 status of the plain point-to-plane alignment, status, iterations and final_pairs of the colored one,
//      status of setColored(true, 2), of setSourceColors with ns - 1 entries, of a colored alignment after the source
//      was set again (no colours); float T[16]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const int ns = std::atoi(argv[2]), nt = std::atoi(argv[3]), min_nb = std::atoi(argv[5]), iters = std::atoi(argv[8]);
  const float radius = (float)std::atof(argv[4]), lambda = (float)std::atof(argv[6]), max_d = (float)std::atof(argv[7]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || ns <= 0 || nt <= 0) return 3;
  std::vector<float> s((size_t)4 * ns), t((size_t)7 * nt);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    auto set_source = [&] { return icpk_set_source(eng.ctx(), s.data(), s.data() + ns, s.data() + 2 * (size_t)ns, ns); };
    const float* tp = t.data();
    if (icpk_set_target(eng.ctx(), tp, tp + nt, tp + 2 * (size_t)nt, nt) != ICPK_OK) return 6;
    if (icpk_set_target_normals(eng.ctx(), tp + 3 * (size_t)nt, tp + 4 * (size_t)nt, tp + 5 * (size_t)nt, nt) != ICPK_OK) return 6;
    if (set_source() != ICPK_OK) return 6;
    int rc = eng.setTargetColors(tp + 6 * (size_t)nt, nt);
    if (rc == ICPK_OK) rc = eng.setSourceColors(s.data() + 3 * (size_t)ns, ns);
    if (rc == ICPK_OK) rc = eng.estimateTargetColorGradients(radius, min_nb);
    if (rc != ICPK_OK) {
      std::fprintf(stderr, "set-up failed: %d %s\n", rc, eng.last_error());
      return 7;
    }
    icp::AlignParams p;
    p.solve = ICPK_SOLVE_POINT_TO_PLANE;
    p.max_iterations = iters;
    p.fixed_iterations = 1;
    p.max_nn_dist = max_d;
    icp::AlignResult plain, r, r3;
    plain.status = icpk_align(eng.ctx(), &p, plain.T, &plain.stats);
    if (eng.setColored(true, lambda) != ICPK_OK) return 8;
    r.status = icpk_align(eng.ctx(), &p, r.T, &r.stats);
    const int bad = eng.setColored(true, 2.f);
    const int short_n = eng.setSourceColors(s.data() + 3 * (size_t)ns, ns - 1);
    if (set_source() != ICPK_OK) return 6;
    r3.status = icpk_align(eng.ctx(), &p, r3.T, &r3.stats);  // the new source has no colours
    const int32_t head[7] = {plain.status, r.status, r.stats.iterations, r.stats.final_pairs, bad, short_n, r3.status};
    std::fwrite(head, 4, 7, o);
    std::fwrite(r.T, 4, 16, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
