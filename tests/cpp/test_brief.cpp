// tests/cpp/test_brief.cpp -- icp::Engine::describeKeypoints / describePoints / describedToCloud / matchDescriptors
// (icp_align.hpp, K32) on one pair of colour + depth frames; the Python test (tests/test_gpu_brief_cpp.py) compares the
// output with the same calls made through the binding, byte for byte.
//
//   test_brief <in.bin> <out.bin>
// in : int32 rows, cols, threshold, max_hamming, n_hypotheses; float fx, cx, max_dist; uint8 bgr_a[rows cols 3], bgr_b;
//      uint16 depth_a[rows cols], depth_b
// out: per frame (a = slot 0, b = slot 1): int32 n; float kp[2 n]; uint32 words[8 n]; uint8 bin[n]; uint8 valid[n];
//      int32 cloud points.  Then int32 equal (describePoints on frame a's downloaded list gave describeKeypoints' bytes);
//      int32 n_matches; n_matches x (int32 source, target, hamming, second); int32 n_cloud_pairs; n_cloud_pairs x
//      (int32 source, int32 target, float D); icpk_global_result; int32 status
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icp_align.hpp"

struct Slot {
  std::vector<float> kp;
  std::vector<uint32_t> words;
  std::vector<uint8_t> bin, valid;
};

static int download(icpk_ctx* c, int which, Slot* s) {
  int32_t n = 0;
  if (icpk_get_descriptors(c, which, nullptr, nullptr, nullptr, nullptr, &n) != ICPK_OK) return -1;
  s->kp.assign((size_t)2 * n + 1, 0.f), s->words.assign((size_t)ICPK_BRIEF_WORDS * n + 1, 0u);
  s->bin.assign((size_t)n + 1, 0), s->valid.assign((size_t)n + 1, 0);
  if (icpk_get_descriptors(c, which, s->kp.data(), s->words.data(), s->bin.data(), s->valid.data(), &n) != ICPK_OK) return -1;
  s->kp.resize((size_t)2 * n), s->words.resize((size_t)ICPK_BRIEF_WORDS * n), s->bin.resize((size_t)n), s->valid.resize((size_t)n);
  return n;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[5];
  float cam[3];
  if (std::fread(head, 4, 5, f) != 5 || std::fread(cam, 4, 3, f) != 3) return 4;
  const int rows = head[0], cols = head[1];
  const size_t npix = (size_t)rows * cols;
  std::vector<uint8_t> bgr[2] = {std::vector<uint8_t>(3 * npix), std::vector<uint8_t>(3 * npix)};
  std::vector<uint16_t> depth[2] = {std::vector<uint16_t>(npix), std::vector<uint16_t>(npix)};
  for (auto& b : bgr)
    if (std::fread(b.data(), 1, b.size(), f) != b.size()) return 4;
  for (auto& d : depth)
    if (std::fread(d.data(), 2, d.size(), f) != d.size()) return 4;
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  try {
    icp::Engine eng(0);
    icpk_ctx* c = eng.ctx();
    const float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
    Slot first;
    for (int which = 0; which < 2; ++which) {
      int32_t n = 0;
      if (icpk_detect_fast(c, bgr[which].data(), rows, cols, 3, head[2], 1, ICPK_FAST_TYPE_7_12, 0, nullptr, nullptr, &n) != ICPK_OK) return 6;
      if (eng.describeKeypoints(which) != ICPK_OK) return 7;
      Slot s;
      if (download(c, which, &s) != n) return 7;
      const int m = eng.describedToCloud(which, depth[which].data(), rows, cols, cam[0], cam[1], R, t);
      if (m < 0) return 8;
      std::fwrite(&n, 4, 1, o);
      std::fwrite(s.kp.data(), 4, s.kp.size(), o);
      std::fwrite(s.words.data(), 4, s.words.size(), o);
      std::fwrite(s.bin.data(), 1, s.bin.size(), o);
      std::fwrite(s.valid.data(), 1, s.valid.size(), o);
      const int32_t m32 = m;
      std::fwrite(&m32, 4, 1, o);
      if (which == 0) first = s;
    }
    icpk_brief_match_params mp;
    icpk_default_brief_match_params(&mp);
    mp.max_hamming = head[3];
    mp.flags = ICPK_BRIEF_MUTUAL | ICPK_BRIEF_TO_CLOUDS;
    std::vector<icp::DescriptorMatch> m;
    if (eng.matchDescriptors(mp, &m) != ICPK_OK) return 9;
    std::vector<int32_t> si(first.valid.size() + 1), ti(first.valid.size() + 1);
    std::vector<float> D(first.valid.size() + 1);
    int32_t nc = 0;
    if (icpk_get_feature_matches(c, si.data(), ti.data(), D.data(), &nc) != ICPK_OK) return 9;
    icpk_global_params gp;
    icpk_default_global_params(&gp);
    gp.n_hypotheses = head[4];
    gp.max_dist = cam[2];
    icpk_global_result res;
    const int rc = eng.registerGlobal(gp, &res);
    if (rc < 0) {
      std::fprintf(stderr, "registerGlobal failed: %d %s\n", rc, eng.last_error());
      return 10;
    }
    // describePoints on the downloaded list of frame a: the same bytes as describeKeypoints gave (a scratch engine, so
    // that the slots above stay as they are)
    icp::Engine other(0);
    if (other.describePoints(0, bgr[0].data(), rows, cols, 3, first.kp.data(), (int)first.valid.size()) != ICPK_OK) return 11;
    Slot again;
    if (download(other.ctx(), 0, &again) != (int)first.valid.size()) return 11;
    const int32_t equal = again.words == first.words && again.bin == first.bin && again.valid == first.valid && again.kp == first.kp;
    std::fwrite(&equal, 4, 1, o);
    const int32_t nm = (int32_t)m.size();
    std::fwrite(&nm, 4, 1, o);
    for (const auto& e : m) std::fwrite(&e, sizeof(e), 1, o);
    std::fwrite(&nc, 4, 1, o);
    for (int32_t k = 0; k < nc; ++k) {
      std::fwrite(&si[(size_t)k], 4, 1, o);
      std::fwrite(&ti[(size_t)k], 4, 1, o);
      std::fwrite(&D[(size_t)k], 4, 1, o);
    }
    std::fwrite(&res, sizeof(res), 1, o);
    const int32_t st = rc;
    std::fwrite(&st, 4, 1, o);
    std::printf("%d matches, %d with cloud points, %lld inliers\n", nm, nc, (long long)res.inliers);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 12;
  }
  std::fclose(o);
  return 0;
}
