// tests/cpp/test_gicp.cpp -- icp::Engine::estimateSourceNormals / setSourceNormals / sourceNormals / setPlaneToPlane
// (icp_align.hpp) and an ICPK_SOLVE_PLANE_TO_PLANE alignment on one pair; the Python test (tests/test_gpu_gicp_cpp.py)
// makes the same calls through the binding and compares bit for bit.
//
//   test_gicp <pair.f32> <ns> <nt> <radius> <min_neighbors> <epsilon> <max_nn_dist> <iterations> <out.bin>
// in : float sx[ns], sy[ns], sz[ns], tx[nt], ty[nt], tz[nt]
// out: int32 status, iterations, final_pairs, status of setPlaneToPlane(0), of setPlaneToPlane(2), of an alignment
//      after the source was set again (no normals), of setSourceNormals with ns - 1 entries; float T[16];
//      float nx[ns], ny[ns], nz[ns] (the estimated source normals); float T2[16] (the alignment once more with those
//      normals given back through setSourceNormals)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const int ns = std::atoi(argv[2]), nt = std::atoi(argv[3]), min_nb = std::atoi(argv[5]), iters = std::atoi(argv[8]);
  const float radius = (float)std::atof(argv[4]), eps = (float)std::atof(argv[6]), max_d = (float)std::atof(argv[7]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || ns <= 0 || nt <= 0) return 3;
  std::vector<float> s((size_t)3 * ns), t((size_t)3 * nt);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    auto set_source = [&] { return icpk_set_source(eng.ctx(), s.data(), s.data() + ns, s.data() + 2 * (size_t)ns, ns); };
    if (icpk_set_target(eng.ctx(), t.data(), t.data() + nt, t.data() + 2 * (size_t)nt, nt) != ICPK_OK) return 6;
    if (set_source() != ICPK_OK) return 6;
    int rc = eng.estimateTargetNormals(radius, min_nb);
    if (rc == ICPK_OK) rc = eng.estimateSourceNormals(radius, min_nb);
    if (rc == ICPK_OK) rc = eng.setPlaneToPlane(eps);
    if (rc != ICPK_OK) {
      std::fprintf(stderr, "set-up failed: %d %s\n", rc, eng.last_error());
      return 7;
    }
    icp::AlignParams p;
    p.solve = ICPK_SOLVE_PLANE_TO_PLANE;
    p.max_iterations = iters;
    p.fixed_iterations = 1;
    p.max_nn_dist = max_d;
    icp::AlignResult r, r2, r3;
    r.status = icpk_align(eng.ctx(), &p, r.T, &r.stats);
    std::vector<float> nrm;
    if (eng.sourceNormals(&nrm) != ICPK_OK || nrm.size() != (size_t)3 * ns) return 8;
    const int bad0 = eng.setPlaneToPlane(0.f), bad2 = eng.setPlaneToPlane(2.f);
    if (set_source() != ICPK_OK) return 6;
    r3.status = icpk_align(eng.ctx(), &p, r3.T, &r3.stats);  // the new source has no normals
    const int short_n = eng.setSourceNormals(nrm.data(), nrm.data() + ns, nrm.data() + 2 * (size_t)ns, ns - 1);
    if (eng.setSourceNormals(nrm.data(), nrm.data() + ns, nrm.data() + 2 * (size_t)ns, ns) != ICPK_OK) return 9;
    r2.status = icpk_align(eng.ctx(), &p, r2.T, &r2.stats);
    const int32_t head[7] = {r.status, r.stats.iterations, r.stats.final_pairs, bad0, bad2, r3.status, short_n};
    std::fwrite(head, 4, 7, o);
    std::fwrite(r.T, 4, 16, o);
    std::fwrite(nrm.data(), 4, nrm.size(), o);
    std::fwrite(r2.T, 4, 16, o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
