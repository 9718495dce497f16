// icpk_voxel.cpp -- host side of the voxel-grid downsampling (K11; kernels_voxel.hip): icpk_voxel_downsample replaces
// one of the context's clouds by one point per occupied cube of edge `leaf`, through the path icpk_set_*_device take,
// and keeps the grouping on the device for icpk_get_voxel_groups.
#include <cmath>

#include "icpk_ctx.h"

using namespace icpk;

namespace {

// room for a cloud of n points: table of the next power of two >= 2 n slots (at least 64), scratch, outputs
int ensure_voxel_buffers(icpk_ctx* ctx, int n, bool normals, size_t* slots) {
  size_t cap = 64;
  while (cap < 2 * (size_t)n) cap <<= 1;
  *slots = cap;
  int rc = ctx->vox_table.reserve(ctx, cap);
  if (!rc) rc = ctx->vox_slot.reserve(ctx, (size_t)n);
  if (!rc) rc = ctx->vox_bsum.reserve(ctx, ((size_t)n + 1023) / 1024);
  if (!rc) rc = ctx->vox_out.reserve(ctx, (size_t)(normals ? 6 : 3) * n);
  return rc;
}

// the groups of a cloud of n_in points (the contents of a previous call are given up)
int ensure_voxel_groups(icpk_ctx* ctx, int n_in) {
  ctx->have_vox = false;
  const size_t n = n_in < 1 ? 1 : (size_t)n_in;
  int rc = ctx->vox_first.reserve(ctx, n);
  if (!rc) rc = ctx->vox_count.reserve(ctx, n);
  if (!rc) rc = ctx->vox_oop.reserve(ctx, n);
  if (!rc) rc = ctx->vox_counts.reserve(ctx, 2);
  if (!rc) rc = ctx->vox_counts_host.reserve(ctx, 2);
  return rc;
}

}  // namespace

extern "C" {

int icpk_voxel_downsample(icpk_ctx* ctx, int32_t which, float leaf, int32_t mode, int32_t* n_out, int32_t* n_dropped) {
  if (!ctx) return ICPK_E_ARG;
  if (which != 0 && which != 1) return fail(ctx, ICPK_E_ARG, "which must be 0 (source) or 1 (target)");
  if (mode != ICPK_VOXEL_FIRST && mode != ICPK_VOXEL_CENTROID) return fail(ctx, ICPK_E_ARG, "unknown voxel mode");
  if (!(leaf > 0.f) || !std::isfinite(leaf)) return fail(ctx, ICPK_E_ARG, "leaf must be finite and > 0");
  if (which == 0 ? !ctx->have_src : !ctx->have_tgt)
    return fail(ctx, ICPK_E_NOT_SET, which == 0 ? "source cloud not set" : "target cloud not set");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (which == 0)
    if (int ru = ensure_unpacked(ctx)) return ru;  // (the call reads the working source)
  const Cloud& in = which == 0 ? ctx->src : ctx->tgt;
  const int n = in.n;
  const bool normals = which == 1 && ctx->have_normals;
  int rc = ensure_voxel_groups(ctx, n);
  if (rc) return rc;
  int counts[2] = {0, 0};
  float* o = nullptr;
  if (n > 0) {
    size_t slots = 0;
    if ((rc = ensure_voxel_buffers(ctx, n, normals, &slots))) return rc;
    ICPK_HIP(ctx, hipMemsetAsync(ctx->vox_table, 0, slots * sizeof(VoxelSlot), ctx->stream));
    ICPK_HIP(ctx, hipMemsetAsync(ctx->vox_counts, 0, 2 * sizeof(int), ctx->stream));
    o = ctx->vox_out;
    VoxelArgs a{};
    a.x = in.x(), a.y = in.y(), a.z = in.z();
    if (normals) a.nx = ctx->nrm.x(), a.ny = ctx->nrm.y(), a.nz = ctx->nrm.z();
    a.n = n;
    a.centroid = mode == ICPK_VOXEL_CENTROID;
    a.leaf = (double)leaf;
    a.table = ctx->vox_table;
    a.mask = (unsigned)(slots - 1);
    a.slot_of = ctx->vox_slot;
    a.bsum = ctx->vox_bsum;
    a.counts = ctx->vox_counts;
    a.ox = o, a.oy = o + n, a.oz = o + 2 * (size_t)n;
    if (normals) a.onx = o + 3 * (size_t)n, a.ony = o + 4 * (size_t)n, a.onz = o + 5 * (size_t)n;
    a.first_index = ctx->vox_first;
    a.count = ctx->vox_count;
    a.out_of_point = ctx->vox_oop;
    launch_voxel_downsample(a, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    // the one host wait of the call: the size of the new cloud
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->vox_counts_host, ctx->vox_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    counts[0] = ctx->vox_counts_host[0];
    counts[1] = ctx->vox_counts_host[1];
    if (counts[0] < 0 || counts[0] > n) return fail(ctx, ICPK_E_HIP, "voxel downsample: impossible output size");
  }
  const int m = counts[0];
  // the new cloud takes the way of icpk_set_*_device, which drops everything derived from the old one (the copies
  // out of vox_out are stream-ordered; nothing writes vox_out before the next downsample on this stream)
  if (which == 0) {
    rc = set_source_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
  } else {
    rc = set_target_impl(ctx, o, o + n, o + 2 * (size_t)n, m, hipMemcpyDeviceToDevice, false);
    if (!rc && normals) {
      if ((rc = ensure_cloud(ctx, ctx->nrm, m))) return rc;
      const Cloud& c = ctx->nrm;
      float* const planes[3] = {c.x(), c.y(), c.z()};
      for (int k = 0; k < 3; ++k) {
        if (m > 0)
          ICPK_HIP(ctx, hipMemcpyAsync(planes[k], o + (3 + k) * (size_t)n, (size_t)m * sizeof(float), hipMemcpyDeviceToDevice,
                                       ctx->stream));
        launch_fill_f32(planes[k] + m, c.cap - m, 0.f, ctx->stream);
      }
      ICPK_HIP(ctx, hipGetLastError());
      ctx->have_normals = true;
    }
  }
  if (rc) return rc;
  ctx->vox_n_in = n;
  ctx->vox_n_out = m;
  ctx->have_vox = true;
  if (n_out) *n_out = m;
  if (n_dropped) *n_dropped = counts[1];
  return ICPK_OK;
}

int icpk_get_voxel_groups(icpk_ctx* ctx, int32_t* n_in, int32_t* n_out, int32_t* first_index, int32_t* count,
                          int32_t* out_of_point) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_vox) return fail(ctx, ICPK_E_NOT_SET, "no voxel downsample has run on this context");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (n_in) *n_in = ctx->vox_n_in;
  if (n_out) *n_out = ctx->vox_n_out;
  const size_t bo = (size_t)ctx->vox_n_out * sizeof(int32_t), bi = (size_t)ctx->vox_n_in * sizeof(int32_t);
  if (first_index && bo) ICPK_HIP(ctx, hipMemcpyAsync(first_index, ctx->vox_first, bo, hipMemcpyDeviceToHost, ctx->stream));
  if (count && bo) ICPK_HIP(ctx, hipMemcpyAsync(count, ctx->vox_count, bo, hipMemcpyDeviceToHost, ctx->stream));
  if (out_of_point && bi) ICPK_HIP(ctx, hipMemcpyAsync(out_of_point, ctx->vox_oop, bi, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

}  // extern "C"
