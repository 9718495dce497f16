// icpk_tsdf_apply.cpp -- host side of K30 (kernels_tsdf_apply.hip): several signed frame updates of the TSDF volume in
// one pass.  The refusals of an op list, the device stack of the call's frames (owned by the volume's state, reused while
// the shape fits), the op table with its poses inverted on the host, the de-integration of one frame as a list of one
// op, and the rule for a run of voxels on the host (icpk_tsdf_voxel_apply).  The signed update rule is written out in
// include/icpk.h and stated once, in tsdf_rule.h.
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

// What every op-list call refuses (nullptr: fine), and the op table: poses inverted as icpk_tsdf_integrate inverts its
// one.  color: whether the volume keeps intensities
const char* make_ops(bool color, int32_t n_frames, const uint16_t* const* depth, const float* const* intensity, int32_t rows,
                     int32_t cols, float fx, float cx, int32_t n_ops, const icpk_tsdf_op* ops, TsdfApplyOp* table) {
  if (const char* why = tsdf_check_camera(rows, cols, fx, cx)) return why;
  if (n_ops < 1 || n_ops > ICPK_TSDF_MAX_OPS) return "n_ops outside 1 .. ICPK_TSDF_MAX_OPS";
  if (n_frames < 1 || n_frames > n_ops) return "n_frames outside 1 .. n_ops";
  if (!depth || !ops) return "depth or ops is NULL";
  if (color != (intensity != nullptr))
    return color ? "a colour volume needs the frames' intensities" : "intensities given to a volume without ICPK_TSDF_COLOR";
  const size_t npix = (size_t)rows * cols;
  for (int32_t f = 0; f < n_frames; ++f) {
    if (!depth[f] || (color && !intensity[f])) return "a frame is NULL";
    if (color && !tsdf_intensities_ok(intensity[f], npix)) return "intensities must be finite and in [0, 1]";
  }
  for (int32_t k = 0; k < n_ops; ++k) {
    if (ops[k].sign != 1 && ops[k].sign != -1) return "an op's sign is neither +1 nor -1";
    if (ops[k].frame < 0 || ops[k].frame >= n_frames) return "an op's frame index is out of range";
    if (icpk_tsdf_invert_pose(ops[k].pose, table[k].R, table[k].t)) return "an op's pose is not finite";
    table[k].sign = ops[k].sign, table[k].frame = ops[k].frame;
  }
  return nullptr;
}

}  // namespace

extern "C" {

int icpk_tsdf_apply(icpk_ctx* ctx, int32_t n_frames, const uint16_t* const* depth, const float* const* intensity, int32_t rows,
                    int32_t cols, float fx, float cx, int32_t n_ops, const icpk_tsdf_op* ops, int64_t* n_updated) {
  if (!ctx) return ICPK_E_ARG;
  TsdfApplyView v;
  if (int rc = tsdf_apply_view(ctx, &v)) return rc;
  const bool color = v.intensity != nullptr;
  TsdfApplyArgs a{};
  if (const char* why = make_ops(color, n_frames, depth, intensity, rows, cols, fx, cx, n_ops, ops, a.ops))
    return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  TsdfApplyBufs& b = *v.bufs;
  const size_t npix = (size_t)rows * cols;
  int rc = b.depth.reserve(ctx, (size_t)n_frames * npix);
  if (!rc && color) rc = b.intensity.reserve(ctx, (size_t)n_frames * npix);
  if (!rc) rc = b.slots.reserve(ctx, (size_t)TSDF_MAX_BLOCKS * TSDF_MAX_OPS);
  if (!rc) rc = b.totals.reserve(ctx, TSDF_MAX_OPS);
  if (!rc) rc = b.totals_host.reserve(ctx, TSDF_MAX_OPS);
  if (rc) return rc;
  for (int32_t f = 0; f < n_frames; ++f) {
    ICPK_HIP(ctx, hipMemcpyAsync(b.depth + (size_t)f * npix, depth[f], npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    if (color)
      ICPK_HIP(ctx, hipMemcpyAsync(b.intensity + (size_t)f * npix, intensity[f], npix * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  const float none[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  a.fr = tsdf_make_frame(v.p, none, none, rows, cols, fx, cx);  // (R and t: the kernel takes the op's)
  a.depth = b.depth;
  a.intensity_image = color ? b.intensity.get() : nullptr;
  a.tsdf = v.tsdf, a.weight = v.weight, a.intensity = v.intensity;
  a.n = v.n, a.chunk = tsdf_chunk(v.n);
  a.npix = (long long)npix;
  a.n_ops = n_ops;
  a.slots = b.slots;
  launch_tsdf_apply(a, tsdf_blocks(v.n), b.totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(b.totals_host, b.totals, (size_t)n_ops * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's frames are free again)
  if (n_updated)
    for (int32_t k = 0; k < n_ops; ++k) n_updated[k] = b.totals_host[k];
  return ICPK_OK;
}

int icpk_tsdf_deintegrate(icpk_ctx* ctx, const uint16_t* depth, const float* intensity, int32_t rows, int32_t cols, float fx,
                          float cx, const double pose[16], int32_t* n_updated) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->tsdf) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!pose) return fail(ctx, ICPK_E_ARG, "the pose is NULL or not finite");
  icpk_tsdf_op op{};
  op.sign = -1, op.frame = 0;
  for (int k = 0; k < 16; ++k) op.pose[k] = pose[k];
  int64_t n = 0;
  const int rc = icpk_tsdf_apply(ctx, 1, &depth, intensity ? &intensity : nullptr, rows, cols, fx, cx, 1, &op, &n);
  if (!rc && n_updated) *n_updated = (int32_t)n;
  return rc;
}

int icpk_tsdf_voxel_apply(const icpk_tsdf_params* params, int32_t n_frames, const uint16_t* const* depth,
                          const float* const* intensity, int32_t rows, int32_t cols, float fx, float cx, int32_t n_ops,
                          const icpk_tsdf_op* ops, int64_t first, int32_t count, float* tsdf, uint16_t* weight,
                          float* intensity_value, int64_t* n_updated) {
  if (!params || !tsdf || !weight || count < 0 || first < 0) return ICPK_E_ARG;
  if (tsdf_check_volume(*params)) return ICPK_E_ARG;
  const bool color = (params->flags & ICPK_TSDF_COLOR) != 0;
  if (color != (intensity_value != nullptr)) return ICPK_E_ARG;
  TsdfApplyOp table[TSDF_MAX_OPS];
  if (make_ops(color, n_frames, depth, intensity, rows, cols, fx, cx, n_ops, ops, table)) return ICPK_E_ARG;
  const long long n = (long long)params->dims[0] * params->dims[1] * params->dims[2];
  if (first + count > n) return ICPK_E_ARG;
  std::vector<TsdfFrame> frames;
  for (int32_t k = 0; k < n_ops; ++k) frames.push_back(tsdf_make_frame(*params, table[k].R, table[k].t, rows, cols, fx, cx));
  const long long dx = params->dims[0], dxy = dx * params->dims[1];
  if (n_updated)
    for (int32_t k = 0; k < n_ops; ++k) n_updated[k] = 0;
  for (int32_t e = 0; e < count; ++e) {
    const long long at = first + e;
    const int z = (int)(at / dxy), y = (int)((at - z * dxy) / dx), x = (int)(at - z * dxy - y * dx);
    int w = weight[e];
    float unused = 0.f;
    for (int32_t k = 0; k < n_ops; ++k) {
      float f;
      int pix;
      if (!tsdf_sample(frames[k], x, y, z, depth[table[k].frame], &f, &pix)) continue;
      const float c = color ? intensity[table[k].frame][pix] : 0.f;
      const bool wrote = tsdf_state_apply(table[k].sign, params->max_weight, f, c, color, &tsdf[e], &w, color ? &intensity_value[e] : &unused);
      if (wrote && n_updated) n_updated[k] += 1;
    }
    weight[e] = (uint16_t)w;
  }
  return ICPK_OK;
}

}  // extern "C"
