// tests/cpp/tsdf_apply_host_main.cpp -- a stand-alone program over icpk_tsdf_voxel_apply (the host half of the signed
// update rule, csrc/tsdf_rule.h, and the op-list validation icpk_tsdf_apply shares with it) for sanitizer runs:
// build.program("tsdf_apply_host_sanitized") compiles it together with icpk_tsdf_apply.cpp under
// -fsanitize=address,undefined.  No GPU is touched.  Every array is allocated at exactly its size, so that a read past
// an image, the op list or the voxel state is a heap overflow the sanitizer sees.
//
//   tsdf_apply_host_sanitized        prints one line per scenario; exit status 0 when every check held
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "icpk.h"

namespace {

const int ROWS = 24, COLS = 32;
const float FX = 24.f, CX = 15.5f;

void identity(double pose[16], double tx, double tz) {
  for (int k = 0; k < 16; ++k) pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
  pose[3] = tx, pose[11] = tz;
}

struct Scene {
  icpk_tsdf_params p;
  std::vector<uint16_t*> depth;
  std::vector<float*> inten;
  size_t n;
  Scene(const int dims[3], bool color, int n_frames) {
    icpk_default_tsdf_params(&p);
    for (int a = 0; a < 3; ++a) p.dims[a] = dims[a];
    p.voxel = 0.1f, p.trunc = 0.3f, p.origin[0] = -0.45f, p.origin[1] = -0.35f, p.origin[2] = 0.8f;
    p.max_weight = 3;
    p.flags = color ? ICPK_TSDF_COLOR : 0;
    n = (size_t)dims[0] * dims[1] * dims[2];
    for (int f = 0; f < n_frames; ++f) {
      uint16_t* d = (uint16_t*)std::malloc(ROWS * COLS * sizeof(uint16_t));
      float* c = (float*)std::malloc(ROWS * COLS * sizeof(float));
      for (int i = 0; i < ROWS * COLS; ++i) {
        d[i] = (i * 7 + f) % 13 == 0 ? 0 : (uint16_t)(6000 + 40 * (i % COLS) + 100 * f);  // a tilted plane with holes
        c[i] = (float)((i + f) % 9) / 8.f;
      }
      depth.push_back(d), inten.push_back(c);
    }
  }
  ~Scene() {
    for (uint16_t* d : depth) std::free(d);
    for (float* c : inten) std::free(c);
  }
};

// the ops over the whole volume in one call, and again one op and one voxel at a time: the same bytes and counts
int run(const int dims[3], bool color) {
  Scene s(dims, color, 2);
  const int n_ops = 7;
  icpk_tsdf_op* ops = (icpk_tsdf_op*)std::malloc(n_ops * sizeof(icpk_tsdf_op));
  const int sign[n_ops] = {-1, +1, +1, +1, +1, -1, -1}, frame[n_ops] = {0, 0, 1, 0, 1, 1, 0};
  for (int k = 0; k < n_ops; ++k) {
    ops[k].sign = sign[k], ops[k].frame = frame[k];
    identity(ops[k].pose, 0.02 * frame[k], -0.01 * k);
  }
  const size_t n = s.n;
  float* f = (float*)std::calloc(n, sizeof(float));
  float* c = (float*)std::calloc(n, sizeof(float));
  uint16_t* w = (uint16_t*)std::calloc(n, sizeof(uint16_t));
  int64_t* counts = (int64_t*)std::malloc(n_ops * sizeof(int64_t));
  int rc = icpk_tsdf_voxel_apply(&s.p, 2, s.depth.data(), color ? s.inten.data() : nullptr, ROWS, COLS, FX, CX, n_ops, ops, 0,
                                 (int32_t)n, f, w, color ? c : nullptr, counts);
  int bad = rc != ICPK_OK || counts[0] != 0 || counts[1] <= 0;
  // one op and one voxel at a time
  float* f1 = (float*)std::calloc(n, sizeof(float));
  float* c1 = (float*)std::calloc(n, sizeof(float));
  uint16_t* w1 = (uint16_t*)std::calloc(n, sizeof(uint16_t));
  std::vector<int64_t> sum(n_ops, 0);
  for (int k = 0; k < n_ops && !bad; ++k)
    for (size_t at = 0; at < n && !bad; ++at) {
      int64_t one = -1;
      const uint16_t* d1 = s.depth[ops[k].frame];
      const float* i1 = s.inten[ops[k].frame];
      icpk_tsdf_op op = ops[k];
      op.frame = 0;
      bad = icpk_tsdf_voxel_apply(&s.p, 1, &d1, color ? &i1 : nullptr, ROWS, COLS, FX, CX, 1, &op, (int64_t)at, 1, f1 + at, w1 + at,
                                  color ? c1 + at : nullptr, &one) != ICPK_OK;
      sum[k] += one;
    }
  bad = bad || std::memcmp(f, f1, n * sizeof(float)) || std::memcmp(w, w1, n * sizeof(uint16_t)) || std::memcmp(c, c1, n * sizeof(float));
  for (int k = 0; k < n_ops; ++k) bad = bad || sum[k] != counts[k];
  for (size_t at = 0; at < n && !bad; ++at) bad = !(f[at] >= -1.f && f[at] <= 1.f) || w[at] > 3 || !(c[at] >= 0.f && c[at] <= 1.f);
  std::printf("%d x %d x %d%s: counts", dims[0], dims[1], dims[2], color ? " colour" : "");
  for (int k = 0; k < n_ops; ++k) std::printf(" %lld", (long long)counts[k]);
  std::printf("%s\n", bad ? "  FAILED" : "");
  std::free(ops), std::free(f), std::free(c), std::free(w), std::free(counts), std::free(f1), std::free(c1), std::free(w1);
  return bad;
}

// every refusal, with the state untouched
int refusals() {
  const int dims[3] = {6, 5, 4};
  Scene s(dims, true, 2);
  const size_t n = s.n;
  std::vector<float> f(n, 0.25f), c(n, 0.5f);
  std::vector<uint16_t> w(n, 2);
  icpk_tsdf_op ops[ICPK_TSDF_MAX_OPS + 1];
  for (icpk_tsdf_op& op : ops) {
    op.sign = 1, op.frame = 0;
    identity(op.pose, 0.0, 0.0);
  }
  const uint16_t* const* D = s.depth.data();
  const float* const* I = s.inten.data();
  auto call = [&](int n_frames, const uint16_t* const* depth, const float* const* inten, int n_ops, const icpk_tsdf_op* o,
                  int64_t first, int32_t count, float* cv) {
    return icpk_tsdf_voxel_apply(&s.p, n_frames, depth, inten, ROWS, COLS, FX, CX, n_ops, o, first, count, f.data(), w.data(), cv,
                                 nullptr);
  };
  int bad = 0;
  bad |= call(1, D, I, 0, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // n_ops < 1
  bad |= call(1, D, I, ICPK_TSDF_MAX_OPS + 1, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;  // n_ops > 16
  bad |= call(0, D, I, 1, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // n_frames < 1
  bad |= call(2, D, I, 1, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // n_frames > n_ops
  bad |= call(1, D, nullptr, 1, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                // colour without intensities
  bad |= call(1, D, I, 1, ops, 0, (int32_t)n, nullptr) != ICPK_E_ARG;                       // ... without its state
  bad |= call(1, nullptr, I, 1, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;
  bad |= call(1, D, I, 1, nullptr, 0, (int32_t)n, c.data()) != ICPK_E_ARG;
  bad |= call(1, D, I, 1, ops, 1, (int32_t)n, c.data()) != ICPK_E_ARG;                      // past the volume
  bad |= call(1, D, I, 1, ops, -1, 1, c.data()) != ICPK_E_ARG;
  const uint16_t* none_d[2] = {s.depth[0], nullptr};
  const float* none_i[2] = {s.inten[0], nullptr};
  bad |= call(2, none_d, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                 // a NULL frame
  bad |= call(2, D, none_i, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;
  ops[1].sign = 0;
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // a sign that is neither
  ops[1].sign = 2;
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;
  ops[1].sign = -1, ops[1].frame = 1;
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // a frame index out of range
  ops[1].frame = -1;
  bad |= call(2, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;
  ops[1].frame = 0, ops[1].pose[7] = NAN;
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // a pose that is not finite
  identity(ops[1].pose, 0.0, 0.0);
  s.inten[0][5] = 1.5f;
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_E_ARG;                      // an intensity out of range
  s.inten[0][5] = 0.5f;
  for (size_t at = 0; at < n; ++at) bad |= f[at] != 0.25f || c[at] != 0.5f || w[at] != 2;   // nothing was touched
  bad |= call(1, D, I, 2, ops, 0, (int32_t)n, c.data()) != ICPK_OK;                         // and the list is fine now
  std::printf("refusals%s\n", bad ? "  FAILED" : "");
  return bad;
}

}  // namespace

int main() {
  const int box[3] = {9, 7, 6}, line[3] = {1, 1, 11}, flat[3] = {10, 8, 1};
  int bad = 0;
  bad |= run(box, false);
  bad |= run(box, true);
  bad |= run(line, true);
  bad |= run(flat, false);
  bad |= refusals();
  return bad;
}
