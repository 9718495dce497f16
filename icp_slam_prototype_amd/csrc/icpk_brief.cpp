// icpk_brief.cpp -- host side of K32 (kernels_brief.hip): oriented BRIEF descriptors of key points, their Hamming
// matches, and the two host-only entry points that run the same rule (brief_rule.h) over host arrays.  The state behind
// ctx->brief holds two descriptor slots (0 the source side, 1 the target side: key points, words, bins, validity, and
// the key point -> cloud index map of icpk_described_to_cloud), the image of icpk_describe_points, the committed table
// on the device, the runs' records of a match and its kept pairs.  The rules are written out in include/icpk.h.
#include <cstring>
#include <vector>

#include "brief_rule.h"
#include "icpk_ctx.h"

using namespace icpk;

static_assert(BRIEF_WORDS == ICPK_BRIEF_WORDS, "kernel and ABI agree on the descriptor's length");

struct icpk_brief_state {
  struct Slot {
    DevBuf<float> kp;        // [n][2]
    DevBuf<uint32_t> words;  // [n][8]
    DevBuf<uint8_t> bin, valid;
    DevBuf<int> map;  // [n] icpk_described_to_cloud (current while ctx->brief_map[which])
    int n = -1;       // -1: the slot is empty
  } slot[2];
  DevBuf<int8_t> table;  // BRIEF_TABLE, uploaded once
  bool have_table = false;
  DevBuf<uint8_t> img;  // the image of icpk_describe_points
  DevBuf<unsigned long long> key[2];  // the runs' records of the two directions
  DevBuf<unsigned> h2[2];
  DevBuf<int> out;  // 4 x out_cap: source key point, target key point, H, H2 of the kept pairs
  size_t out_cap = 0;
  DevBuf<int> counts;  // kept pairs, pairs in K16's list
  PinnedBuf<int> counts_host;
  bool have_matches = false;  // the pairs belong to the descriptors both slots hold now
};

void icpk_brief_free(icpk_ctx* ctx) {
  delete ctx->brief;  // (its buffers free themselves)
  ctx->brief = nullptr;
  ctx->brief_map[0] = ctx->brief_map[1] = false;
}

namespace {

bool bad_image(int32_t rows, int32_t cols, int32_t channels) {
  return rows <= 0 || cols <= 0 || (int64_t)rows * cols > (1 << 27) || (channels != 1 && channels != 3);
}

int ensure_brief(icpk_ctx* ctx) {
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->brief) ctx->brief = new icpk_brief_state();
  icpk_brief_state* b = ctx->brief;
  if (!b->have_table) {
    if (int rc = b->table.reserve(ctx, sizeof(BRIEF_TABLE))) return rc;
    ICPK_HIP(ctx, hipMemcpyAsync(b->table, &BRIEF_TABLE[0][0][0], sizeof(BRIEF_TABLE), hipMemcpyHostToDevice, ctx->stream));
    b->have_table = true;
  }
  int rc = b->counts.reserve(ctx, 2);
  if (!rc) rc = b->counts_host.reserve(ctx, 2);
  return rc;
}

// slot `which` is about to be rewritten for n key points: empty until the caller sets n, its map and the matches stale
int reset_slot(icpk_ctx* ctx, int which, int n) {
  icpk_brief_state* b = ctx->brief;
  icpk_brief_state::Slot& s = b->slot[which];
  s.n = -1;
  ctx->brief_map[which] = false;
  b->have_matches = false;
  const size_t cap = n < 1 ? 1 : (size_t)n;
  return reserve_group(ctx, nullptr, need(s.kp, 2 * cap), need(s.words, BRIEF_WORDS * cap), need(s.bin, cap), need(s.valid, cap),
                       need(s.map, cap));
}

const char* check_match(const icpk_brief_match_params& p, int allowed_flags) {
  if (p.max_hamming < 0 || p.max_hamming > BRIEF_TESTS) return "max_hamming outside 0 .. 256";
  if (p.ratio_num < 0 || p.ratio_num > 65536 || p.ratio_den < 1 || p.ratio_den > 65536) return "ratio_num outside 0 .. 65536 or ratio_den outside 1 .. 65536";
  if (p.flags & ~allowed_flags) return "unknown match flag";
  return nullptr;
}

// THE BRIEF RULE for one key point over a host image
void describe_one(const uint8_t* image, int rows, int cols, int channels, float fx, float fy, bool upright, uint32_t w[BRIEF_WORDS],
                  uint8_t* bin, uint8_t* valid) {
  for (int k = 0; k < BRIEF_WORDS; ++k) w[k] = 0u;
  *bin = 0, *valid = 0;
  const int xi = brief_coord(fx, BRIEF_B, cols - BRIEF_B), yi = brief_coord(fy, BRIEF_B, rows - BRIEF_B);
  if (xi < 0 || yi < 0) return;
  uint8_t g[BRIEF_GW][BRIEF_GW];
  int32_t m10 = 0, m01 = 0;
  for (int ly = 0; ly < BRIEF_GW; ++ly)
    for (int lx = 0; lx < BRIEF_GW; ++lx) {
      const int v = brief_pixel(image, cols, channels, xi - BRIEF_B + lx, yi - BRIEF_B + ly);
      g[ly][lx] = (uint8_t)v;
      const int dx = lx - BRIEF_B, dy = ly - BRIEF_B;
      if (dx * dx + dy * dy <= BRIEF_R2) m10 += dx * v, m01 += dy * v;
    }
  uint16_t S[BRIEF_SW][BRIEF_SW];
  for (int sy = 0; sy < BRIEF_SW; ++sy)
    for (int sx = 0; sx < BRIEF_SW; ++sx) {
      int s = 0;
      for (int dy = 0; dy <= 2 * BRIEF_BOX; ++dy)
        for (int dx = 0; dx <= 2 * BRIEF_BOX; ++dx) s += g[sy + dy][sx + dx];
      S[sy][sx] = (uint16_t)s;
    }
  const int b = upright ? 0 : brief_bin(m10, m01);
  for (int t = 0; t < BRIEF_TESTS; ++t) {
    const int8_t* e = BRIEF_TABLE[b][t];
    if (S[BRIEF_OFF + e[1]][BRIEF_OFF + e[0]] < S[BRIEF_OFF + e[3]][BRIEF_OFF + e[2]]) w[t >> 5] |= 1u << (t & 31);
  }
  *bin = (uint8_t)b, *valid = 1;
}

// the best valid descriptor of side b for descriptor i of side a
BriefBest best_of(const uint32_t* wa, int i, const uint32_t* wb, const uint8_t* vb, int nb) {
  BriefBest best;
  for (int j = 0; j < nb; ++j)
    if (vb[j]) best.take(brief_hamming(wa + (size_t)BRIEF_WORDS * i, wb + (size_t)BRIEF_WORDS * j), j);
  return best;
}

}  // namespace

extern "C" {

void icpk_default_brief_match_params(icpk_brief_match_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_hamming = 48;
  p->ratio_num = 0;
  p->ratio_den = 1;
  p->flags = ICPK_BRIEF_MUTUAL;
}

void icpk_brief_pattern(int8_t* out) {
  if (out) std::memcpy(out, &BRIEF_TABLE[0][0][0], sizeof(BRIEF_TABLE));
}

void icpk_brief_boundaries(int32_t* out) {
  if (out) std::memcpy(out, &BRIEF_BOUNDARY[0][0], sizeof(BRIEF_BOUNDARY));
}

int icpk_brief_bin(int32_t m10, int32_t m01) { return brief_bin(m10, m01); }

int icpk_describe_keypoints(icpk_ctx* ctx, int32_t which, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source side) or 1 (target side)");
  if (flags & ~ICPK_BRIEF_UPRIGHT) return fail(ctx, ICPK_E_ARG, "unknown describe flag");
  const FastResident f = fast_resident(ctx);
  if (f.n < 0) return fail(ctx, ICPK_E_NOT_SET, "no detected key points with their image (icpk_detect_fast)");
  if (f.n > ICPK_BRIEF_MAX_KEYPOINTS) return fail(ctx, ICPK_E_ARG, "more than ICPK_BRIEF_MAX_KEYPOINTS key points");
  int rc = ensure_brief(ctx);
  if (!rc) rc = reset_slot(ctx, which, f.n);
  if (rc) return rc;
  icpk_brief_state::Slot& s = ctx->brief->slot[which];
  if (f.n > 0) {
    ICPK_HIP(ctx, hipMemcpyAsync(s.kp, f.kp, (size_t)2 * f.n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    launch_brief_describe(f.img, f.rows, f.cols, f.channels, s.kp, f.n, (flags & ICPK_BRIEF_UPRIGHT) != 0, ctx->brief->table,
                          s.words, s.bin, s.valid, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
  }
  s.n = f.n;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_describe_points(icpk_ctx* ctx, int32_t which, const uint8_t* image, int32_t rows, int32_t cols, int32_t channels,
                         const float* kp_xy, int32_t n, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source side) or 1 (target side)");
  if (flags & ~ICPK_BRIEF_UPRIGHT) return fail(ctx, ICPK_E_ARG, "unknown describe flag");
  if (!image || bad_image(rows, cols, channels)) return fail(ctx, ICPK_E_ARG, "bad image, size or channels");
  if (n < 0 || n > ICPK_BRIEF_MAX_KEYPOINTS) return fail(ctx, ICPK_E_ARG, "n outside 0 .. ICPK_BRIEF_MAX_KEYPOINTS");
  if (n > 0 && !kp_xy) return fail(ctx, ICPK_E_ARG, "kp_xy is NULL");
  int rc = ensure_brief(ctx);
  if (!rc) rc = reset_slot(ctx, which, n);
  if (rc) return rc;
  icpk_brief_state* b = ctx->brief;
  icpk_brief_state::Slot& s = b->slot[which];
  if (n > 0) {
    const size_t bytes = (size_t)rows * cols * channels;
    if ((rc = b->img.reserve(ctx, bytes))) return rc;
    ICPK_HIP(ctx, hipMemcpyAsync(b->img, image, bytes, hipMemcpyHostToDevice, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(s.kp, kp_xy, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    launch_brief_describe(b->img, rows, cols, channels, s.kp, n, (flags & ICPK_BRIEF_UPRIGHT) != 0, b->table, s.words, s.bin,
                          s.valid, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's arrays are free again)
  }
  s.n = n;
  return ICPK_OK;
}

int icpk_get_descriptors(icpk_ctx* ctx, int32_t which, float* kp_xy, uint32_t* words, uint8_t* bin, uint8_t* valid, int32_t* n) {
  if (n) *n = 0;
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source side) or 1 (target side)");
  if (!ctx->brief || ctx->brief->slot[which].n < 0) return fail(ctx, ICPK_E_NOT_SET, "the descriptor slot is empty");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const icpk_brief_state::Slot& s = ctx->brief->slot[which];
  const size_t m = (size_t)s.n;
  if (kp_xy && m) ICPK_HIP(ctx, hipMemcpyAsync(kp_xy, s.kp, 2 * m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (words && m)
    ICPK_HIP(ctx, hipMemcpyAsync(words, s.words, BRIEF_WORDS * m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (bin && m) ICPK_HIP(ctx, hipMemcpyAsync(bin, s.bin, m, hipMemcpyDeviceToHost, ctx->stream));
  if (valid && m) ICPK_HIP(ctx, hipMemcpyAsync(valid, s.valid, m, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = s.n;
  return ICPK_OK;
}

int icpk_set_descriptors(icpk_ctx* ctx, int32_t which, const float* kp_xy, const uint32_t* words, const uint8_t* bin,
                         const uint8_t* valid, int32_t n) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source side) or 1 (target side)");
  if (n < 0 || n > ICPK_BRIEF_MAX_KEYPOINTS) return fail(ctx, ICPK_E_ARG, "n outside 0 .. ICPK_BRIEF_MAX_KEYPOINTS");
  if (n > 0 && (!words || !valid)) return fail(ctx, ICPK_E_ARG, "words or valid is NULL");
  for (int32_t k = 0; k < n; ++k)
    if (valid[k] > 1 || (bin && bin[k] >= BRIEF_BINS)) return fail(ctx, ICPK_E_ARG, "a valid byte above 1 or a bin above 31");
  int rc = ensure_brief(ctx);
  if (!rc) rc = reset_slot(ctx, which, n);
  if (rc) return rc;
  icpk_brief_state::Slot& s = ctx->brief->slot[which];
  if (n > 0) {
    const size_t m = (size_t)n;
    if (kp_xy) ICPK_HIP(ctx, hipMemcpyAsync(s.kp, kp_xy, 2 * m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    else ICPK_HIP(ctx, hipMemsetAsync(s.kp, 0, 2 * m * sizeof(float), ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(s.words, words, BRIEF_WORDS * m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (bin) ICPK_HIP(ctx, hipMemcpyAsync(s.bin, bin, m, hipMemcpyHostToDevice, ctx->stream));
    else ICPK_HIP(ctx, hipMemsetAsync(s.bin, 0, m, ctx->stream));
    ICPK_HIP(ctx, hipMemcpyAsync(s.valid, valid, m, hipMemcpyHostToDevice, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's arrays are free again)
  }
  s.n = n;
  return ICPK_OK;
}

int icpk_described_to_cloud(icpk_ctx* ctx, int32_t which, const uint16_t* depth, int32_t d_rows, int32_t d_cols, float fx,
                            float cx, const float R[9], const float t[3], int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (!ctx->brief || ctx->brief->slot[which].n < 0) return fail(ctx, ICPK_E_NOT_SET, "the descriptor slot is empty");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  icpk_brief_state::Slot& s = ctx->brief->slot[which];
  ctx->brief_map[which] = false;
  const int rc = keypoints_to_cloud(ctx, s.kp, s.n, depth, d_rows, d_cols, fx, cx, R, t, which, s.map, n_out);
  if (rc) return rc;
  ctx->brief_map[which] = true;  // (whatever replaces the cloud clears it again: fpfh_dropped)
  return ICPK_OK;
}

int icpk_get_descriptor_cloud_map(icpk_ctx* ctx, int32_t which, int32_t* map, int32_t* n) {
  if (n) *n = 0;
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (!ctx->brief || ctx->brief->slot[which].n < 0 || !ctx->brief_map[which])
    return fail(ctx, ICPK_E_NOT_SET, "no icpk_described_to_cloud of this slot on the current cloud");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const icpk_brief_state::Slot& s = ctx->brief->slot[which];
  if (map && s.n) ICPK_HIP(ctx, hipMemcpyAsync(map, s.map, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = s.n;
  return ICPK_OK;
}

int icpk_match_descriptors(icpk_ctx* ctx, const icpk_brief_match_params* params, int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!ctx) return ICPK_E_ARG;
  icpk_brief_match_params p;
  icpk_default_brief_match_params(&p);
  if (params) p = *params;
  if (const char* why = check_match(p, ICPK_BRIEF_MUTUAL | ICPK_BRIEF_TO_CLOUDS)) return fail(ctx, ICPK_E_ARG, why);
  icpk_brief_state* b = ctx->brief;
  if (!b || b->slot[0].n < 0 || b->slot[1].n < 0) return fail(ctx, ICPK_E_NOT_SET, "both descriptor slots must be filled");
  const bool mutual = (p.flags & ICPK_BRIEF_MUTUAL) != 0, clouds = (p.flags & ICPK_BRIEF_TO_CLOUDS) != 0;
  if (clouds && !(ctx->brief_map[0] && ctx->brief_map[1]))
    return fail(ctx, ICPK_E_NOT_SET, "ICPK_BRIEF_TO_CLOUDS needs icpk_described_to_cloud of both slots on the current clouds");
  int rc = ensure_brief(ctx);
  if (rc) return rc;
  const icpk_brief_state::Slot &s = b->slot[0], &t = b->slot[1];
  const int ns = s.n, nt = t.n;
  const size_t caps = ns < 1 ? 1 : (size_t)ns, capt = nt < 1 ? 1 : (size_t)nt;
  const int runs_t = brief_match_runs(nt), runs_s = brief_match_runs(ns);
  b->have_matches = false;
  rc = b->key[0].reserve(ctx, caps * runs_t);
  if (!rc) rc = b->h2[0].reserve(ctx, caps * runs_t);
  if (!rc && mutual) rc = b->key[1].reserve(ctx, capt * runs_s);
  if (!rc && mutual) rc = b->h2[1].reserve(ctx, capt * runs_s);
  if (!rc && caps > b->out_cap) {
    b->out_cap = 0;
    rc = b->out.reserve(ctx, 4 * caps);
    if (!rc) b->out_cap = caps;
  }
  if (!rc && clouds) {
    ctx->have_matches = false;  // (K16's list is about to be rewritten)
    rc = ctx->match_src.reserve(ctx, caps);
    if (!rc) rc = ctx->match_tgt.reserve(ctx, caps);
    if (!rc) rc = ctx->match_D.reserve(ctx, caps);
    if (!rc) rc = ctx->match_n.reserve(ctx, 1);
    if (!rc) rc = ctx->match_n_host.reserve(ctx, 1);
  }
  if (rc) return rc;
  const BriefSide sa{s.words, s.valid, ns}, sb{t.words, t.valid, nt};
  launch_brief_match(sa, sb, b->key[0], b->h2[0], ctx->stream);
  if (mutual) launch_brief_match(sb, sa, b->key[1], b->h2[1], ctx->stream);  // the same rule with the roles exchanged
  BriefFinishArgs a{};
  a.key[0] = b->key[0], a.h2[0] = b->h2[0], a.runs[0] = runs_t;
  a.key[1] = b->key[1], a.h2[1] = b->h2[1], a.runs[1] = runs_s;
  a.ns = ns, a.nt = nt;
  a.valid_s = s.valid;
  a.max_hamming = p.max_hamming, a.ratio_num = p.ratio_num, a.ratio_den = p.ratio_den, a.mutual = mutual ? 1 : 0;
  a.map_s = clouds ? s.map.get() : nullptr, a.map_t = clouds ? t.map.get() : nullptr;
  a.out_src = b->out, a.out_tgt = b->out + b->out_cap, a.out_H = b->out + 2 * b->out_cap, a.out_H2 = b->out + 3 * b->out_cap;
  a.cl_src = clouds ? ctx->match_src.get() : nullptr, a.cl_tgt = clouds ? ctx->match_tgt.get() : nullptr;
  a.cl_D = clouds ? ctx->match_D.get() : nullptr;
  a.counts = b->counts;
  a.cl_n = clouds ? ctx->match_n.get() : nullptr;
  launch_brief_finish(a, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  b->have_matches = true;
  if (clouds) ctx->have_matches = true;  // icpk_register_global and icpk_get_feature_matches read the list as K16's
  if (!n_out) return ICPK_OK;  // (nothing is asked: the call does not wait)
  ICPK_HIP(ctx, hipMemcpyAsync(b->counts_host, b->counts, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *n_out = b->counts_host[0];
  return ICPK_OK;
}

int icpk_get_descriptor_matches(icpk_ctx* ctx, int32_t* src_kp, int32_t* tgt_kp, int32_t* H, int32_t* H2, int32_t* n) {
  if (n) *n = 0;
  if (!ctx) return ICPK_E_ARG;
  icpk_brief_state* b = ctx->brief;
  if (!b || !b->have_matches) return fail(ctx, ICPK_E_NOT_SET, "no icpk_match_descriptors call on the current descriptors");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipMemcpyAsync(b->counts_host, b->counts, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t m = (size_t)b->counts_host[0];
  int32_t* const out[4] = {src_kp, tgt_kp, H, H2};
  for (int k = 0; k < 4; ++k)
    if (out[k] && m)
      ICPK_HIP(ctx, hipMemcpyAsync(out[k], b->out + (size_t)k * b->out_cap, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = (int32_t)m;
  return ICPK_OK;
}

int icpk_brief_describe_host(const uint8_t* image, int32_t rows, int32_t cols, int32_t channels, const float* kp_xy, int32_t n,
                             int32_t flags, uint32_t* words, uint8_t* bin, uint8_t* valid) {
  if (!image || bad_image(rows, cols, channels) || n < 0 || n > ICPK_BRIEF_MAX_KEYPOINTS || (n > 0 && !kp_xy)) return ICPK_E_ARG;
  if (flags & ~ICPK_BRIEF_UPRIGHT) return ICPK_E_ARG;
  for (int32_t k = 0; k < n; ++k) {
    uint32_t w[BRIEF_WORDS];
    uint8_t b, v;
    describe_one(image, rows, cols, channels, kp_xy[2 * (size_t)k], kp_xy[2 * (size_t)k + 1], (flags & ICPK_BRIEF_UPRIGHT) != 0, w, &b, &v);
    if (words) std::memcpy(words + (size_t)BRIEF_WORDS * k, w, sizeof(w));
    if (bin) bin[k] = b;
    if (valid) valid[k] = v;
  }
  return ICPK_OK;
}

int icpk_brief_match_host(const uint32_t* words_s, const uint8_t* valid_s, int32_t ns, const uint32_t* words_t,
                          const uint8_t* valid_t, int32_t nt, const icpk_brief_match_params* params, int32_t* src_kp,
                          int32_t* tgt_kp, int32_t* H, int32_t* H2, int32_t* n_out) {
  if (n_out) *n_out = 0;
  if (!params || !n_out || ns < 0 || nt < 0 || ns > ICPK_BRIEF_MAX_KEYPOINTS || nt > ICPK_BRIEF_MAX_KEYPOINTS) return ICPK_E_ARG;
  if ((ns > 0 && (!words_s || !valid_s)) || (nt > 0 && (!words_t || !valid_t))) return ICPK_E_ARG;
  if (check_match(*params, ICPK_BRIEF_MUTUAL)) return ICPK_E_ARG;
  const bool mutual = (params->flags & ICPK_BRIEF_MUTUAL) != 0;
  std::vector<int> back;  // the best source of every target, found on demand (-2: not yet)
  if (mutual) back.assign((size_t)nt, -2);
  int32_t m = 0;
  for (int32_t i = 0; i < ns; ++i) {
    if (!valid_s[i]) continue;
    const BriefBest best = best_of(words_s, i, words_t, valid_t, nt);
    if (!brief_keep(best, params->max_hamming, params->ratio_num, params->ratio_den)) continue;
    if (mutual) {
      int& bj = back[(size_t)best.j];
      if (bj == -2) bj = best_of(words_t, best.j, words_s, valid_s, ns).j;
      if (bj != i) continue;
    }
    if (src_kp) src_kp[m] = i;
    if (tgt_kp) tgt_kp[m] = best.j;
    if (H) H[m] = best.H;
    if (H2) H2[m] = best.H2;
    ++m;
  }
  *n_out = m;
  return ICPK_OK;
}

}  // extern "C"
