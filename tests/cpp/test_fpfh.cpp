// tests/cpp/test_fpfh.cpp -- icp::Engine::computeFPFH / fpfh / matchFeatures / registerGlobal (icp_align.hpp) on one
// pair with normals from the host; the Python test (tests/test_gpu_fpfh_cpp.py) compares them with the C ABI's output
// written alongside and with the same calls made through the binding, bit for bit.
//
//   test_fpfh <in.f32> <ns> <nt> <radius> <n_hypotheses> <seed> <max_dist> <out.bin>
// in : float sx[ns], sy, sz, snx, sny, snz, then tx[nt], ty, tz, tnx, tny, tnz
// out: twice (Engine, then C ABI):  float desc_s[33 ns]; uint8 valid_s[ns]; float desc_t[33 nt]; uint8 valid_t[nt];
//      int32 n_matches; n_matches x (int32 source, int32 target, float D); icpk_global_result; int32 status
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int ns = std::atoi(argv[2]), nt = std::atoi(argv[3]);
  const float radius = (float)std::atof(argv[4]);
  icpk_global_params gp;
  icpk_default_global_params(&gp);
  gp.n_hypotheses = std::atoi(argv[5]);
  gp.seed = std::strtoull(argv[6], nullptr, 10);
  gp.max_dist = (float)std::atof(argv[7]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || ns <= 0 || nt <= 0) return 3;
  std::vector<float> s((size_t)6 * ns), t((size_t)6 * nt);
  if (std::fread(s.data(), 4, s.size(), f) != s.size() || std::fread(t.data(), 4, t.size(), f) != t.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[8], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    icpk_ctx* c = eng.ctx();
    const size_t S = (size_t)ns, T = (size_t)nt;
    if (icpk_set_target(c, t.data(), t.data() + T, t.data() + 2 * T, nt) != ICPK_OK) return 6;
    if (icpk_set_target_normals(c, t.data() + 3 * T, t.data() + 4 * T, t.data() + 5 * T, nt) != ICPK_OK) return 6;
    if (icpk_set_source(c, s.data(), s.data() + S, s.data() + 2 * S, ns) != ICPK_OK) return 6;
    if (eng.setSourceNormals(s.data() + 3 * S, s.data() + 4 * S, s.data() + 5 * S, ns) != ICPK_OK) return 6;
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<float> ds, dt;
      std::vector<uint8_t> vs, vt;
      std::vector<icp::FeatureMatch> m;
      icpk_global_result res;
      int rc;
      if (pass == 0) {
        if (eng.computeFPFH(0, radius) != ICPK_OK || eng.computeFPFH(1, radius) != ICPK_OK) return 7;
        if (eng.fpfh(0, &ds, &vs) != ICPK_OK || eng.fpfh(1, &dt, &vt) != ICPK_OK) return 7;
        if (eng.matchFeatures(true, &m) != ICPK_OK) return 8;
        rc = eng.registerGlobal(gp, &res);
      } else {
        if (icpk_compute_fpfh(c, 0, radius, 0) != ICPK_OK || icpk_compute_fpfh(c, 1, radius, 0) != ICPK_OK) return 7;
        ds.resize(S * ICPK_FPFH_BINS), dt.resize(T * ICPK_FPFH_BINS), vs.resize(S), vt.resize(T);
        if (icpk_get_fpfh(c, 0, ds.data(), vs.data(), nullptr) != ICPK_OK) return 7;
        if (icpk_get_fpfh(c, 1, dt.data(), vt.data(), nullptr) != ICPK_OK) return 7;
        if (icpk_match_features(c, ICPK_MATCH_MUTUAL) != ICPK_OK) return 8;
        std::vector<int32_t> si(S), ti(S);
        std::vector<float> D(S);
        int32_t n = 0;
        if (icpk_get_feature_matches(c, si.data(), ti.data(), D.data(), &n) != ICPK_OK) return 8;
        for (int32_t k = 0; k < n; ++k) m.push_back(icp::FeatureMatch{si[(size_t)k], ti[(size_t)k], D[(size_t)k]});
        rc = icpk_register_global(c, &gp, &res);
      }
      if (rc < 0) {
        std::fprintf(stderr, "registerGlobal failed: %d %s\n", rc, eng.last_error());
        return 9;
      }
      std::fwrite(ds.data(), 4, ds.size(), o);
      std::fwrite(vs.data(), 1, vs.size(), o);
      std::fwrite(dt.data(), 4, dt.size(), o);
      std::fwrite(vt.data(), 1, vt.size(), o);
      const int32_t n = (int32_t)m.size();
      std::fwrite(&n, 4, 1, o);
      for (const auto& e : m) std::fwrite(&e, sizeof(e), 1, o);
      std::fwrite(&res, sizeof(res), 1, o);
      const int32_t st = rc;
      std::fwrite(&st, 4, 1, o);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 10;
  }
  std::fclose(o);
  return 0;
}
