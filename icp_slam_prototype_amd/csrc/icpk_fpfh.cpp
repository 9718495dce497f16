// icpk_fpfh.cpp -- host side of the FPFH descriptors and their matching (K16; kernels_fpfh.hip): icpk_compute_fpfh
// describes every point of the uploaded source or of the target by 33 floats, icpk_match_features pairs valid source
// points with their nearest valid target descriptors, and the getters bring both to the host.  The registration that
// consumes the pairs is icpk_global.cpp's.
#include <cmath>

#include "icpk_ctx.h"

using namespace icpk;

static_assert(FPFH_BINS == ICPK_FPFH_BINS, "kernel and ABI agree on the descriptor's length");

extern "C" {

int icpk_compute_fpfh(icpk_ctx* ctx, int32_t which, float radius, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (!(radius > 0.f) || !std::isfinite(radius)) return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0");
  if (flags & ~ICPK_FPFH_KEEP_SPFH) return fail(ctx, ICPK_E_ARG, "unknown fpfh flag");
  if (which == 0 && !ctx->have_src) return fail(ctx, ICPK_E_NOT_SET, "source cloud not set");
  if (which == 0 && !ctx->have_src_normals) return fail(ctx, ICPK_E_NOT_SET, "no source normals");
  if (which == 1 && !ctx->have_tgt) return fail(ctx, ICPK_E_NOT_SET, "target cloud not set");
  if (which == 1 && !ctx->have_normals) return fail(ctx, ICPK_E_NOT_SET, "no target normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool keep = (flags & ICPK_FPFH_KEEP_SPFH) != 0;
  const Cloud& cloud = which == 0 ? ctx->src0 : ctx->tgt;
  const Cloud& nrm = which == 0 ? ctx->snrm : ctx->nrm;
  const int n = cloud.n;
  icpk_ctx::FpfhSide& f = ctx->fpfh[which];
  fpfh_dropped(ctx, which);  // (the buffers are about to be rewritten)
  const size_t cap = n < 1 ? 1 : (size_t)n;
  int rc = f.n4.reserve(ctx, cap);
  if (!rc) rc = f.g.reserve(ctx, cap * FPFH_G_STRIDE);
  if (!rc) rc = f.desc.reserve(ctx, cap * FPFH_BINS);
  if (!rc) rc = f.valid.reserve(ctx, cap);
  if (!rc && keep) rc = f.counts.reserve(ctx, cap * FPFH_BINS);
  if (!rc && keep) rc = f.m.reserve(ctx, cap);
  if (rc) return rc;
  if (n > 0) {
    // the source walks an index of its own (aux_grid): the target's is not disturbed.  K1d's index of the target: built
    // here if the target has none yet, and then valid for the alignment that follows
    GridView v;
    if ((rc = which == 0 ? index_aux(ctx, ctx->src0, &v) : index_target(ctx, &v))) return rc;
    FpfhArgs a{};
    a.index = v;
    a.nx = nrm.x(), a.ny = nrm.y(), a.nz = nrm.z();
    a.n = n;
    a.radius = radius;
    a.n4 = f.n4;
    a.g = f.g;
    a.counts = keep ? f.counts.get() : nullptr;
    a.m = keep ? f.m.get() : nullptr;
    a.desc = f.desc;
    a.valid = f.valid;
    launch_compute_fpfh(a, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
  }
  f.n = n;
  f.kept_spfh = keep;
  f.have = true;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_fpfh(icpk_ctx* ctx, int32_t which, float* desc, uint8_t* valid, int32_t* n) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  const icpk_ctx::FpfhSide& f = ctx->fpfh[which];
  if (!f.have) return fail(ctx, ICPK_E_NOT_SET, "no descriptors of the current cloud and normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)f.n;
  if (desc && m)
    ICPK_HIP(ctx, hipMemcpyAsync(desc, f.desc, m * FPFH_BINS * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (valid && m) ICPK_HIP(ctx, hipMemcpyAsync(valid, f.valid, m, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = f.n;
  return ICPK_OK;
}

int icpk_get_spfh(icpk_ctx* ctx, int32_t which, int32_t* counts, int32_t* m_out) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  const icpk_ctx::FpfhSide& f = ctx->fpfh[which];
  if (!f.have) return fail(ctx, ICPK_E_NOT_SET, "no descriptors of the current cloud and normals");
  if (!f.kept_spfh) return fail(ctx, ICPK_E_ARG, "the SPFH counts were not kept (ICPK_FPFH_KEEP_SPFH)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)f.n;
  if (counts && m)
    ICPK_HIP(ctx, hipMemcpyAsync(counts, f.counts, m * FPFH_BINS * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (m_out && m) ICPK_HIP(ctx, hipMemcpyAsync(m_out, f.m, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_match_features(icpk_ctx* ctx, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  if (flags & ~ICPK_MATCH_MUTUAL) return fail(ctx, ICPK_E_ARG, "unknown match flag");
  if (!ctx->fpfh[0].have || !ctx->fpfh[1].have)
    return fail(ctx, ICPK_E_NOT_SET, "both clouds need current descriptors (icpk_compute_fpfh)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool mutual = (flags & ICPK_MATCH_MUTUAL) != 0;
  const icpk_ctx::FpfhSide &s = ctx->fpfh[0], &t = ctx->fpfh[1];
  const size_t caps = s.n < 1 ? 1 : (size_t)s.n, capt = t.n < 1 ? 1 : (size_t)t.n;
  ctx->have_matches = false;
  int rc = ctx->match_best[0].reserve(ctx, caps);
  if (!rc) rc = ctx->match_best[1].reserve(ctx, capt);
  if (!rc) rc = ctx->match_src.reserve(ctx, caps);
  if (!rc) rc = ctx->match_tgt.reserve(ctx, caps);
  if (!rc) rc = ctx->match_D.reserve(ctx, caps);
  if (!rc) rc = ctx->match_n.reserve(ctx, 1);
  if (!rc) rc = ctx->match_n_host.reserve(ctx, 1);
  if (rc) return rc;
  launch_fill_u64(ctx->match_best[0], s.n, NN_KEY_INIT, nullptr, ctx->stream);
  MatchArgs a{};
  a.fa = s.desc, a.va = s.valid, a.na = s.n;
  a.fb = t.desc, a.vb = t.valid, a.nb = t.n;
  a.best = ctx->match_best[0];
  launch_match_features(a, ctx->stream);
  if (mutual) {  // the same rule with the roles exchanged
    launch_fill_u64(ctx->match_best[1], t.n, NN_KEY_INIT, nullptr, ctx->stream);
    MatchArgs b{};
    b.fa = t.desc, b.va = t.valid, b.na = t.n;
    b.fb = s.desc, b.vb = s.valid, b.nb = s.n;
    b.best = ctx->match_best[1];
    launch_match_features(b, ctx->stream);
  }
  launch_match_compact(ctx->match_best[0], s.n, ctx->match_best[1], mutual ? 1 : 0, ctx->match_src, ctx->match_tgt,
                       ctx->match_D, ctx->match_n, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_matches = true;
  return ICPK_OK;  // stream-ordered: no host wait
}

int icpk_get_feature_matches(icpk_ctx* ctx, int32_t* src_index, int32_t* tgt_index, float* D, int32_t* n) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_matches) return fail(ctx, ICPK_E_NOT_SET, "no icpk_match_features call on the current descriptors");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->match_n_host, ctx->match_n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t m = (size_t)ctx->match_n_host[0];
  if (src_index && m)
    ICPK_HIP(ctx, hipMemcpyAsync(src_index, ctx->match_src, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (tgt_index && m)
    ICPK_HIP(ctx, hipMemcpyAsync(tgt_index, ctx->match_tgt, m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (D && m) ICPK_HIP(ctx, hipMemcpyAsync(D, ctx->match_D, m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n) *n = (int32_t)m;
  return ICPK_OK;
}

}  // extern "C"
