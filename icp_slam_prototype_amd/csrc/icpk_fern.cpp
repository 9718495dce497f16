// icpk_fern.cpp -- K27, host side of fern keyframe relocalisation (include/icpk.h, THE FERN RULE; kernels_fern.hip):
// the defaults, the refusals, the rule over host levels through the header the kernel includes (icpk_fern_table,
// icpk_fern_encode_host, icpk_fern_dissimilarity_host -- the host-only half: no context, no device), and the entry
// points that keep a context's keyframe database.  They read the resident pyramid where it lies and write only the
// buffers the context keeps for them; the poses stay on the host beside the codes.
#include <cmath>
#include <cstring>
#include <vector>

#include "fern_rule.h"
#include "icpk_ctx.h"

using namespace icpk;

static_assert(FERN_TOPK == ICPK_FERN_MAX_K && FERN_MAX_F == ICPK_FERN_MAX_FERNS, "the kernels' sizes are the header's");

namespace {

// nullptr: fine; else what is wrong
const char* check_params(const icpk_fern_params& p) {
  if (p.level < 0 || p.level >= ICPK_PYRAMID_MAX_LEVELS) return "a level no pyramid has";
  if (p.n_ferns < 8 || p.n_ferns > ICPK_FERN_MAX_FERNS || p.n_ferns % 8 != 0) return "n_ferns: a multiple of 8 in 8 .. 1024";
  if (p.d_min < 0 || p.d_max > 65535 || p.d_min >= p.d_max) return "0 <= d_min < d_max <= 65535";
  if (p.capacity < 1 || p.capacity > ICPK_FERN_MAX_KEYFRAMES) return "capacity outside 1 .. 65536";
  if (p.harvest_above < 0 || p.harvest_above > p.n_ferns) return "harvest_above outside 0 .. n_ferns";
  if (p.min_valid < 0 || p.min_valid > p.n_ferns) return "min_valid outside 0 .. n_ferns";
  return nullptr;
}

icpk_fern_params params_or_defaults(const icpk_fern_params* params) {
  icpk_fern_params p;
  icpk_default_fern_params(&p);
  if (params) p = *params;
  return p;
}

bool shape_ok(int32_t rows, int32_t cols) { return rows >= 1 && cols >= 1 && (int64_t)rows * cols <= (1 << 28); }

bool pose_ok(const double* pose) {
  if (!pose) return false;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return false;
  return true;
}

int words(const icpk_ctx* ctx) { return ctx->fern_params.n_ferns / 8; }
uint32_t* answer_dev(const icpk_ctx* ctx) { return ctx->fern_code + words(ctx) + 1; }

int need_database(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_fern) return fail(ctx, ICPK_E_NOT_SET, "no fern database (icpk_fern_create)");
  return ICPK_OK;
}

int need_current_code(icpk_ctx* ctx) {
  if (!ctx->fern_code_current)
    return fail(ctx, ICPK_E_NOT_SET, "no current fern code of the resident pyramid (icpk_fern_encode)");
  return ICPK_OK;
}

// the checks of an encode, in the header's order; nothing has changed when this fails
int need_level(icpk_ctx* ctx) {
  if (ctx->pyr_levels == 0) return fail(ctx, ICPK_E_NOT_SET, "no depth pyramid (icpk_depth_pyramid_build)");
  const int l = ctx->fern_params.level;
  if (l >= ctx->pyr_levels) return fail(ctx, ICPK_E_ARG, "a level the pyramid does not have");
  if (ctx->pyr_rows[l] != ctx->fern_rows || ctx->pyr_cols[l] != ctx->fern_cols)
    return fail(ctx, ICPK_E_ARG, "the resident level's shape is not the database's");
  return ICPK_OK;
}

void enqueue_encode(icpk_ctx* ctx) {
  const int l = ctx->fern_params.level;
  launch_fern_encode(ctx->pyr + ctx->pyr_off[l], ctx->fern_cols, ctx->fern_table, ctx->fern_params.n_ferns, ctx->fern_code,
                     ctx->stream);
}

void enqueue_search(icpk_ctx* ctx) {
  launch_fern_search(ctx->fern_db, ctx->fern_params.capacity, ctx->fern_n, ctx->fern_code, words(ctx), ctx->fern_lists,
                     answer_dev(ctx), ctx->stream);
}

// words [first, first + count) of the current code's buffer (code | V | answer) to the pinned mirror, and the one wait
int fetch(icpk_ctx* ctx, int first, int count) {
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->fern_host + first, ctx->fern_code + first, (size_t)count * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// the fetched answer as the first min(k, n) (index, diss) pairs
int unpack_answer(const icpk_ctx* ctx, int k, int32_t* index_out, int32_t* diss_out) {
  const uint32_t* keys = ctx->fern_host + words(ctx) + 1;
  int m = 0;
  for (; m < k && m < ctx->fern_n && keys[m] != FERN_NO_KEY; ++m) {
    index_out[m] = (int32_t)(keys[m] & 0xFFFFu);
    diss_out[m] = (int32_t)(keys[m] >> 16);
  }
  return m;
}

// column n := the current code (stream-ordered), with its pose
void append_current(icpk_ctx* ctx, const double* pose) {
  launch_fern_append(ctx->fern_db, ctx->fern_params.capacity, ctx->fern_n, ctx->fern_code, words(ctx), ctx->stream);
  ctx->fern_poses.insert(ctx->fern_poses.end(), pose, pose + 16);
  ++ctx->fern_n;
}

}  // namespace

extern "C" {

void icpk_default_fern_params(icpk_fern_params* p) {
  if (!p) return;
  p->level = 2;
  p->n_ferns = 256;
  p->seed = 27;
  p->d_min = 1000;
  p->d_max = 20000;
  p->capacity = 4096;
  p->harvest_above = p->n_ferns / 5;
  p->min_valid = p->n_ferns / 2;
  p->reserved = 0;
}

// ---- host only ----
int icpk_fern_table(const icpk_fern_params* params, int32_t rows, int32_t cols, int32_t* table_out) {
  if (!table_out || !shape_ok(rows, cols)) return ICPK_E_ARG;
  const icpk_fern_params p = params_or_defaults(params);
  if (check_params(p)) return ICPK_E_ARG;
  for (int f = 0; f < p.n_ferns; ++f) fern_entry(p.seed, p.d_min, p.d_max, rows, cols, f, table_out + (size_t)f * FERN_ENTRY);
  return ICPK_OK;
}

int icpk_fern_encode_host(const icpk_fern_params* params, const uint16_t* level, int32_t rows, int32_t cols,
                          uint32_t* code_out, int32_t* valid_out) {
  if (!level || !code_out || !shape_ok(rows, cols)) return ICPK_E_ARG;
  const icpk_fern_params p = params_or_defaults(params);
  if (check_params(p)) return ICPK_E_ARG;
  int V = 0;
  for (int w = 0; w < p.n_ferns / 8; ++w) {
    uint32_t word = 0;
    for (int j = 0; j < 8; ++j) {
      int32_t e[FERN_ENTRY];
      fern_entry(p.seed, p.d_min, p.d_max, rows, cols, 8 * w + j, e);
      const int d = level[(size_t)e[0] * cols + e[1]];
      V += d != 0;
      word |= fern_nibble(d, e + 2) << (4 * j);
    }
    code_out[w] = word;
  }
  if (valid_out) *valid_out = V;
  return ICPK_OK;
}

int icpk_fern_dissimilarity_host(const uint32_t* a, const uint32_t* b, int32_t n_ferns) {
  if (!a || !b || n_ferns < 8 || n_ferns > ICPK_FERN_MAX_FERNS || n_ferns % 8 != 0) return ICPK_E_ARG;
  int diss = 0;
  for (int w = 0; w < n_ferns / 8; ++w) diss += fern_word_diss(a[w], b[w]);
  return diss;
}

// ---- the database of a context ----
int icpk_fern_create(icpk_ctx* ctx, const icpk_fern_params* params, int32_t rows, int32_t cols) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_fern_params p = params_or_defaults(params);
  if (const char* why = check_params(p)) return fail(ctx, ICPK_E_ARG, why);
  if (!shape_ok(rows, cols)) return fail(ctx, ICPK_E_ARG, "rows or cols < 1, or more than 2^28 pixels");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (nothing in flight reads the buffers that may be replaced)
  const int W = p.n_ferns / 8;
  ctx->have_fern = false;  // (the old database goes with its memory)
  ctx->fern_code_current = false;
  ctx->fern_n = 0;
  ctx->fern_poses.clear();
  int rc = ICPK_OK;
  if ((rc = ctx->fern_table.reserve(ctx, (size_t)p.n_ferns * FERN_ENTRY))) return rc;
  if ((rc = ctx->fern_db.reserve(ctx, (size_t)W * p.capacity))) return rc;
  if ((rc = ctx->fern_code.reserve(ctx, (size_t)FERN_MAX_F / 8 + 1 + FERN_TOPK))) return rc;
  if ((rc = ctx->fern_host.reserve(ctx, (size_t)FERN_MAX_F / 8 + 1 + FERN_TOPK))) return rc;
  if ((rc = ctx->fern_lists.reserve(ctx, (size_t)((p.capacity + FERN_SEARCH_THREADS - 1) / FERN_SEARCH_THREADS) * FERN_TOPK)))
    return rc;
  std::vector<int32_t> table((size_t)p.n_ferns * FERN_ENTRY);
  for (int f = 0; f < p.n_ferns; ++f) fern_entry(p.seed, p.d_min, p.d_max, rows, cols, f, table.data() + (size_t)f * FERN_ENTRY);
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->fern_table, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemsetAsync(ctx->fern_db, 0, (size_t)W * p.capacity * sizeof(uint32_t), ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the table's host copy has been consumed)
  ctx->fern_params = p;
  ctx->fern_rows = rows, ctx->fern_cols = cols;
  ctx->have_fern = true;
  return ICPK_OK;
}

int icpk_fern_reset(icpk_ctx* ctx) {
  if (int rc = need_database(ctx)) return rc;
  ctx->fern_n = 0;
  ctx->fern_poses.clear();
  return ICPK_OK;
}

int icpk_fern_destroy(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  ctx->have_fern = false;
  ctx->fern_code_current = false;
  ctx->fern_n = 0;
  ctx->fern_poses.clear();
  ctx->fern_poses.shrink_to_fit();
  hipError_t e = hipSuccess;
  for (const hipError_t r : {ctx->fern_table.release(), ctx->fern_db.release(), ctx->fern_code.release(),
                             ctx->fern_lists.release(), ctx->fern_host.release()})
    if (e == hipSuccess) e = r;
  return e == hipSuccess ? ICPK_OK : hip_failure(ctx, "hipFree", e);
}

int icpk_fern_count(icpk_ctx* ctx) {
  if (int rc = need_database(ctx)) return rc;
  return ctx->fern_n;
}

int icpk_fern_encode(icpk_ctx* ctx, uint32_t* code_out, int32_t* valid_out) {
  if (int rc = need_database(ctx)) return rc;
  if (int rc = need_level(ctx)) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ctx->fern_code_current = false;
  enqueue_encode(ctx);
  const int W = words(ctx);
  if (int rc = fetch(ctx, 0, W + 1)) return rc;
  ctx->fern_code_valid = (int)ctx->fern_host[W];
  ctx->fern_code_current = true;
  if (code_out) std::memcpy(code_out, ctx->fern_host.get(), (size_t)W * sizeof(uint32_t));
  if (valid_out) *valid_out = ctx->fern_code_valid;
  return ICPK_OK;
}

int icpk_fern_query(icpk_ctx* ctx, int32_t k, int32_t* index_out, int32_t* diss_out, int32_t* n_out) {
  if (int rc = need_database(ctx)) return rc;
  if (!index_out || !diss_out || !n_out) return fail(ctx, ICPK_E_ARG, "a NULL output");
  if (k < 1 || k > ICPK_FERN_MAX_K) return fail(ctx, ICPK_E_ARG, "k outside 1 .. ICPK_FERN_MAX_K");
  if (int rc = need_current_code(ctx)) return rc;
  *n_out = 0;
  if (ctx->fern_n == 0) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  enqueue_search(ctx);
  if (int rc = fetch(ctx, words(ctx) + 1, FERN_TOPK)) return rc;
  *n_out = unpack_answer(ctx, k, index_out, diss_out);
  return ICPK_OK;
}

int icpk_fern_add(icpk_ctx* ctx, const double pose[16], int32_t* index_out) {
  if (int rc = need_database(ctx)) return rc;
  if (!pose_ok(pose)) return fail(ctx, ICPK_E_ARG, "the pose is NULL or not finite");
  if (int rc = need_current_code(ctx)) return rc;
  if (ctx->fern_n >= ctx->fern_params.capacity) return fail(ctx, ICPK_E_ARG, "the database is full");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  append_current(ctx, pose);
  ICPK_HIP(ctx, hipGetLastError());
  if (index_out) *index_out = ctx->fern_n - 1;
  return ICPK_OK;
}

int icpk_fern_process(icpk_ctx* ctx, const double* pose, int32_t k, int32_t* index_out, int32_t* diss_out, int32_t* n_out,
                      int32_t* valid_out, int32_t* added_out) {
  if (int rc = need_database(ctx)) return rc;
  if (!index_out || !diss_out || !n_out) return fail(ctx, ICPK_E_ARG, "a NULL output");
  if (k < 1 || k > ICPK_FERN_MAX_K) return fail(ctx, ICPK_E_ARG, "k outside 1 .. ICPK_FERN_MAX_K");
  if (pose && !pose_ok(pose)) return fail(ctx, ICPK_E_ARG, "the pose is not finite");
  if (int rc = need_level(ctx)) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  // encode, search, merge; one copy of V and the answer, one wait
  ctx->fern_code_current = false;
  enqueue_encode(ctx);
  enqueue_search(ctx);
  const int W = words(ctx);
  if (int rc = fetch(ctx, W, 1 + (ctx->fern_n > 0 ? FERN_TOPK : 0))) return rc;
  const int V = (int)ctx->fern_host[W];
  ctx->fern_code_valid = V;
  ctx->fern_code_current = true;
  const int m = ctx->fern_n > 0 ? unpack_answer(ctx, k, index_out, diss_out) : 0;
  *n_out = m;
  if (valid_out) *valid_out = V;
  int added = -1;
  const int best = ctx->fern_n > 0 ? (int)(ctx->fern_host[W + 1] >> 16) : 0;
  if (pose && fern_harvest(V, ctx->fern_n, best, ctx->fern_params.min_valid, ctx->fern_params.capacity,
                           ctx->fern_params.harvest_above)) {
    append_current(ctx, pose);  // (stream-ordered: whoever reads the database next comes behind it)
    ICPK_HIP(ctx, hipGetLastError());
    added = ctx->fern_n - 1;
  }
  if (added_out) *added_out = added;
  return ICPK_OK;
}

int icpk_fern_add_code(icpk_ctx* ctx, const uint32_t* code, const double pose[16], int32_t* index_out) {
  if (int rc = need_database(ctx)) return rc;
  if (!code) return fail(ctx, ICPK_E_ARG, "the code is NULL");
  if (!pose_ok(pose)) return fail(ctx, ICPK_E_ARG, "the pose is NULL or not finite");
  if (ctx->fern_n >= ctx->fern_params.capacity) return fail(ctx, ICPK_E_ARG, "the database is full");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t pitch = (size_t)ctx->fern_params.capacity * sizeof(uint32_t);
  ICPK_HIP(ctx, hipMemcpy2DAsync(ctx->fern_db + ctx->fern_n, pitch, code, sizeof(uint32_t), sizeof(uint32_t), (size_t)words(ctx),
                                 hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's code has been consumed)
  ctx->fern_poses.insert(ctx->fern_poses.end(), pose, pose + 16);
  if (index_out) *index_out = ctx->fern_n;
  ++ctx->fern_n;
  return ICPK_OK;
}

int icpk_fern_get_keyframe(icpk_ctx* ctx, int32_t index, uint32_t* code_out, double* pose_out) {
  if (int rc = need_database(ctx)) return rc;
  if (index < 0 || index >= ctx->fern_n) return fail(ctx, ICPK_E_ARG, "no such keyframe");
  if (code_out) {
    ICPK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pitch = (size_t)ctx->fern_params.capacity * sizeof(uint32_t);
    ICPK_HIP(ctx, hipMemcpy2DAsync(code_out, sizeof(uint32_t), ctx->fern_db + index, pitch, sizeof(uint32_t), (size_t)words(ctx),
                                   hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (pose_out) std::memcpy(pose_out, ctx->fern_poses.data() + (size_t)index * 16, 16 * sizeof(double));
  return ICPK_OK;
}

}  // extern "C"
