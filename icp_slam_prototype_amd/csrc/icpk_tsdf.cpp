// icpk_tsdf.cpp -- host side of the TSDF volume (K19, K20, K21; kernels_tsdf.hip): the volume a context owns, the
// refusals, the inversion of the pose, integration of a frame (uploaded, or the one icpk_backproject_pair left
// resident), extraction of the surface list, the ray cast of the volume into vertex and normal maps, the hand-over of
// either as the context's target, the extraction of the triangle mesh, and the moving volume (K23: the shift, the leaving
// list, the parameters in force, a sub-box of the planes).  The rules are written out in include/icpk.h
// and stated once, in tsdf_rule.h, for the device and for icpk_tsdf_voxel_update / icpk_tsdf_raycast_pixels /
// icpk_tsdf_mesh_host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

struct icpk_tsdf_state {
  icpk_tsdf_params p{};
  long long n = 0;  // voxels
  DevBuf<float> tsdf, intensity;
  DevBuf<uint16_t> weight;
  // K23: the origin the volume was created with and the voxels it has been shifted by since (p.origin follows from
  // the two); the second set of planes a shift writes, allocated by the first one, and the staging of icpk_tsdf_get_box
  float origin0[3] = {0.f, 0.f, 0.f};
  long long total[3] = {0, 0, 0};
  DevBuf<float> tsdf_next, intensity_next, box_f;
  DevBuf<uint16_t> weight_next, box_w;
  // a frame on its way into the volume (the resident frame of icpk_backproject_pair is read where it lies)
  DevBuf<uint16_t> depth;
  DevBuf<float> intensity_image;
  // per chunk: integrate's written voxels / extract's listed crossings, extract's dropped ones; the scan; the totals
  DevBuf<int> slots, dropped;
  DevBuf<long long> offsets;
  DevBuf<long long> totals;  // 2
  PinnedBuf<long long> totals_host;
  // the surface list of the last extraction: 7 planes of surf_cap floats, the voxel and the axis of every entry
  DevBuf<float> surf;
  DevBuf<int> surf_voxel;
  DevBuf<uint8_t> surf_axis;
  size_t surf_cap = 0;
  bool have_surface = false;
  int surf_n = 0, surf_dropped = 0;
  float* plane(int k) const { return surf + (size_t)k * surf_cap; }
  // the maps of the last ray cast (K20): 8 planes of ray_rows x ray_cols floats; their valid pixels as a list of 7
  // planes of ray_list_cap floats, made by icpk_tsdf_raycast_to_target
  DevBuf<float> ray_maps, ray_list;
  size_t ray_list_cap = 0;
  bool have_raycast = false;
  int ray_rows = 0, ray_cols = 0;
  float ray_fx = 0.f, ray_cx = 0.f;  // ... and the camera and pose they were cast with (K25 projects into them)
  double ray_pose[16] = {0};
  // K26, behind the maps: the colour gradients of the current ray cast (3 planes) and, with ICPK_COLOR_KEEP_SUMS, the
  // ten int64 per pixel; both dropped by the next ray cast and with the maps
  DevBuf<float> ray_grad;
  DevBuf<long long> ray_grad_sums;
  bool have_ray_grad = false, have_ray_grad_sums = false;
  // the mesh of the last mesh extraction (K21): 7 planes of mesh_vcap floats, every vertex's key (owner voxel, edge
  // type), 3 x mesh_tcap indices; and its own per-chunk counts, scans and totals, so that K19's stay as they are
  DevBuf<float> mesh;
  DevBuf<int> mesh_voxel, mesh_tri;
  DevBuf<uint8_t> mesh_edge;
  size_t mesh_vcap = 0, mesh_tcap = 0;
  DevBuf<int> mesh_vcounts, mesh_tcounts, mesh_nonormal;
  DevBuf<long long> mesh_voffsets, mesh_toffsets, mesh_totals;  // (mesh_totals: 3)
  PinnedBuf<long long> mesh_totals_host;
  bool have_mesh = false;
  int mesh_nv = 0, mesh_nt = 0, mesh_nn = 0;
  float* mesh_plane(int k) const { return mesh + (size_t)k * mesh_vcap; }
  // K30: the frame stack and the counts of icpk_tsdf_apply (icpk_tsdf_apply.cpp), allocated by its first call
  TsdfApplyBufs apply;
  // the volume's intensity plane; null for a volume without ICPK_TSDF_COLOR
  float* intensity_plane() const { return (p.flags & ICPK_TSDF_COLOR) ? intensity.get() : nullptr; }
};

void icpk_tsdf_free(icpk_ctx* ctx) {
  delete ctx->tsdf;  // (its buffers free themselves)
  ctx->tsdf = nullptr;
  icpk_esdf_drop(ctx);  // (K31: the map of a volume that is gone)
}

int icpk::tsdf_raycast_view(icpk_ctx* ctx, TsdfRayView* out) {
  const icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!v->have_raycast) return fail(ctx, ICPK_E_NOT_SET, "no ray cast (icpk_tsdf_raycast)");
  out->maps = v->ray_maps;
  out->rows = v->ray_rows, out->cols = v->ray_cols;
  out->fx = v->ray_fx, out->cx = v->ray_cx;
  std::memcpy(out->pose, v->ray_pose, sizeof(out->pose));
  return ICPK_OK;
}

int icpk::tsdf_volume_view(icpk_ctx* ctx, TsdfVolumeView* out) {
  const icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  out->tsdf = v->tsdf, out->weight = v->weight;
  out->p = v->p;
  return ICPK_OK;
}

int icpk::tsdf_apply_view(icpk_ctx* ctx, TsdfApplyView* out) {
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  out->tsdf = v->tsdf, out->weight = v->weight, out->intensity = v->intensity_plane();
  out->n = v->n;
  out->p = v->p;
  out->bufs = &v->apply;
  return ICPK_OK;
}

void icpk::tsdf_raycast_color_view(icpk_ctx* ctx, bool* color, const float** grad) {
  const icpk_tsdf_state* v = ctx->tsdf;
  *color = v && (v->p.flags & ICPK_TSDF_COLOR);
  *grad = v && v->have_raycast && v->have_ray_grad ? v->ray_grad.get() : nullptr;
}

namespace {

bool positive(float v) { return std::isfinite(v) && v > 0.f; }

// nullptr: fine; else what is wrong
const char* check_params(const icpk_tsdf_params& p) {
  long long n = 1;
  for (int a = 0; a < 3; ++a) {
    if (p.dims[a] < 1) return "a dim is < 1";
    n *= p.dims[a];  // (each factor <= 2^31 and the running product is checked: no overflow)
    if (n > ICPK_TSDF_MAX_VOXELS) return "more than ICPK_TSDF_MAX_VOXELS voxels";
    if (!std::isfinite(p.origin[a])) return "the origin is not finite";
  }
  if (!positive(p.voxel) || !positive(p.trunc) || !positive(p.depth_scale)) return "voxel, trunc and depth_scale must be finite and > 0";
  if (p.max_weight < 1 || p.max_weight > 65535) return "max_weight outside 1 .. 65535";
  if (p.flags & ~ICPK_TSDF_COLOR) return "unknown TSDF flag";
  return nullptr;
}

const char* check_camera(int32_t rows, int32_t cols, float fx, float cx) {
  if (rows < 1 || cols < 1 || (int64_t)rows * cols > (1 << 28)) return "rows or cols < 1, or more than 2^28 pixels";
  if (!positive(fx) || !std::isfinite(cx)) return "fx must be finite and > 0, cx finite";
  return nullptr;
}

TsdfFrame make_frame(const icpk_tsdf_params& p, const float R[9], const float t[3], int rows, int cols, float fx, float cx) {
  TsdfFrame fr{};
  for (int a = 0; a < 3; ++a) fr.dims[a] = p.dims[a], fr.origin[a] = p.origin[a], fr.t[a] = t[a];
  std::memcpy(fr.R, R, sizeof(fr.R));
  fr.voxel = p.voxel, fr.trunc = p.trunc, fr.depth_scale = p.depth_scale, fr.max_weight = p.max_weight;
  fr.rows = rows, fr.cols = cols, fr.fx = fx, fr.cx = cx;
  return fr;
}

int clear_volume(icpk_ctx* ctx, icpk_tsdf_state* v) {
  ICPK_HIP(ctx, hipMemsetAsync(v->tsdf, 0, (size_t)v->n * sizeof(float), ctx->stream));
  ICPK_HIP(ctx, hipMemsetAsync(v->weight, 0, (size_t)v->n * sizeof(uint16_t), ctx->stream));
  if (v->p.flags & ICPK_TSDF_COLOR) ICPK_HIP(ctx, hipMemsetAsync(v->intensity, 0, (size_t)v->n * sizeof(float), ctx->stream));
  v->have_surface = false;
  v->have_raycast = false;
  v->have_mesh = false;
  for (int a = 0; a < 3; ++a) v->total[a] = 0, v->p.origin[a] = v->origin0[a];  // (the box is back where it was created)
  return ICPK_OK;
}

TsdfPlanes make_planes(const icpk_tsdf_params& p, const float* tsdf, const uint16_t* weight, const float* intensity, int min_weight) {
  TsdfPlanes v{};
  v.tsdf = tsdf, v.weight = weight, v.intensity = intensity;
  for (int k = 0; k < 3; ++k) v.dims[k] = p.dims[k], v.origin[k] = p.origin[k];
  v.voxel = p.voxel;
  v.min_weight = min_weight;
  return v;
}

// the refusals of a ray cast's own parameters (nullptr: fine), and the camera of the ray rule: rules 0 and 3
const char* make_ray(const icpk_tsdf_params& p, const icpk_tsdf_raycast_params& rp, const double pose[16], TsdfRay* r) {
  if (const char* why = check_camera(rp.rows, rp.cols, rp.fx, rp.cx)) return why;
  if ((int64_t)rp.rows * rp.cols > ICPK_TSDF_MAX_RAYCAST_PIXELS) return "more than ICPK_TSDF_MAX_RAYCAST_PIXELS pixels";
  if (!pose) return "the pose is NULL";
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return "the pose is not finite";
  if (!std::isfinite(rp.z_near) || !std::isfinite(rp.z_far) || !std::isfinite(rp.step)) return "z_near, z_far and step must be finite";
  if (!(rp.z_near > 0.f) || !(rp.z_far > rp.z_near) || rp.step < 0.f) return "0 < z_near < z_far and step >= 0 expected";
  if (rp.min_weight < 1 || rp.min_weight > 65535) return "min_weight outside 1 .. 65535";
  const float step = rp.step == 0.f ? p.trunc * 0.5f : rp.step;
  if (!(step > 0.f)) return "trunc / 2 is not a step";  // (a denormal trunc)
  const double n = std::floor(((double)rp.z_far - (double)rp.z_near) / (double)step) + 1.0;
  if (!(n <= (double)ICPK_TSDF_MAX_RAY_SAMPLES)) return "more than ICPK_TSDF_MAX_RAY_SAMPLES samples per ray";
  r->rows = rp.rows, r->cols = rp.cols, r->fx = rp.fx, r->cx = rp.cx;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r->R[3 * i + j] = (float)pose[4 * i + j];
    r->c[i] = (float)pose[4 * i + 3];
  }
  r->z_near = rp.z_near, r->step = step, r->nsamples = (int)n;
  return nullptr;
}

// a list of n points with normals and intensities on the device (7 planes: x, y, z, nx, ny, nz, intensity) becomes the
// context's target
int list_to_target(icpk_ctx* ctx, const icpk_tsdf_state* v, float* const list[7], int n) {
  const size_t bytes = (size_t)n * sizeof(float);
  // (the target first: target_changed drops the normals and the colours the old target had)
  int rc = set_target_impl(ctx, list[0], list[1], list[2], n, hipMemcpyDeviceToDevice, false);
  if (!rc) rc = ensure_cloud(ctx, ctx->nrm, n);
  if (rc) return rc;
  const Cloud& m = ctx->nrm;
  float* const planes[3] = {m.x(), m.y(), m.z()};
  for (int k = 0; k < 3; ++k) {
    ICPK_HIP(ctx, hipMemcpyAsync(planes[k], list[3 + k], bytes, hipMemcpyDeviceToDevice, ctx->stream));
    launch_fill_f32(planes[k] + n, m.cap - n, 0.f, ctx->stream);  // (as icpk_set_target_normals pads them)
  }
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_normals = true;
  ctx->have_nstats = false;
  fpfh_dropped(ctx, 1);
  if (v->p.flags & ICPK_TSDF_COLOR) {
    if ((rc = ctx->tcol.reserve(ctx, (size_t)n))) return rc;
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->tcol, list[6], bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->have_tgt_colors = true;
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// a list on the device: seven planes of cap floats (plane k at planes + k * cap), the voxel of every entry and its byte
// plane (the axis, or the edge type)
struct DevList {
  const float* planes;
  size_t cap;
  const int* voxel;
  const uint8_t* byte;
};

// the first n entries of the list to the host; a null destination is skipped.  The caller synchronises
int download_list(icpk_ctx* ctx, const DevList& l, size_t n, float* const out[7], int32_t* voxel_out, uint8_t* byte_out) {
  if (n == 0) return ICPK_OK;
  for (int k = 0; k < 7; ++k)
    if (out[k]) ICPK_HIP(ctx, hipMemcpyAsync(out[k], l.planes + (size_t)k * l.cap, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (voxel_out) ICPK_HIP(ctx, hipMemcpyAsync(voxel_out, l.voxel, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (byte_out) ICPK_HIP(ctx, hipMemcpyAsync(byte_out, l.byte, n, hipMemcpyDeviceToHost, ctx->stream));
  return ICPK_OK;
}

bool intensities_ok(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!(v[i] >= 0.f && v[i] <= 1.f)) return false;  // (false for NaN)
  return true;
}

}  // namespace

// K30: the refusals and the frame above, for icpk_tsdf_apply.cpp
const char* icpk::tsdf_check_volume(const icpk_tsdf_params& p) { return check_params(p); }
const char* icpk::tsdf_check_camera(int32_t rows, int32_t cols, float fx, float cx) { return check_camera(rows, cols, fx, cx); }
bool icpk::tsdf_intensities_ok(const float* v, size_t n) { return intensities_ok(v, n); }
TsdfFrame icpk::tsdf_make_frame(const icpk_tsdf_params& p, const float R[9], const float t[3], int rows, int cols, float fx, float cx) {
  return make_frame(p, R, t, rows, cols, fx, cx);
}

extern "C" {

void icpk_default_tsdf_params(icpk_tsdf_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->dims[0] = p->dims[1] = p->dims[2] = 256;
  p->voxel = 0.02f;
  p->origin[0] = p->origin[1] = -2.56f;
  p->origin[2] = 0.f;
  p->trunc = 0.08f;
  p->max_weight = 255;
  p->depth_scale = ICPK_DEPTH_SCALE;
  p->flags = 0;
}

int icpk_tsdf_create(icpk_ctx* ctx, const icpk_tsdf_params* params) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_params p;
  icpk_default_tsdf_params(&p);
  if (params) p = *params;
  if (const char* why = check_params(p)) return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (nothing still reads the volume that is replaced)
  icpk_tsdf_free(ctx);
  icpk_tsdf_state* v = new icpk_tsdf_state();
  v->p = p;
  for (int a = 0; a < 3; ++a) v->origin0[a] = p.origin[a];
  v->n = (long long)p.dims[0] * p.dims[1] * p.dims[2];
  const size_t n = (size_t)v->n;
  int rc = v->tsdf.reserve(ctx, n);
  if (!rc) rc = v->weight.reserve(ctx, n);
  if (!rc && (p.flags & ICPK_TSDF_COLOR)) rc = v->intensity.reserve(ctx, n);
  if (!rc) rc = v->slots.reserve(ctx, TSDF_MAX_BLOCKS);
  if (!rc) rc = v->dropped.reserve(ctx, TSDF_MAX_BLOCKS);
  if (!rc) rc = v->offsets.reserve(ctx, TSDF_MAX_BLOCKS + 1);
  if (!rc) rc = v->totals.reserve(ctx, 2);
  if (!rc) rc = v->totals_host.reserve(ctx, 2);
  if (!rc) rc = clear_volume(ctx, v);
  if (rc) {
    delete v;
    return rc;
  }
  ctx->tsdf = v;
  return ICPK_OK;
}

int icpk_tsdf_reset(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->tsdf) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  icpk_esdf_drop(ctx);
  return clear_volume(ctx, ctx->tsdf);
}

int icpk_tsdf_release(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->tsdf) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  icpk_tsdf_free(ctx);
  return ICPK_OK;
}

int icpk_tsdf_invert_pose(const double pose[16], float R[9], float t[3]) {
  if (!pose || !R || !t) return ICPK_E_ARG;
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(pose[k])) return ICPK_E_ARG;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (float)pose[4 * c + r];
    t[r] = (float)-((pose[r] * pose[3] + pose[4 + r] * pose[7]) + pose[8 + r] * pose[11]);
  }
  return ICPK_OK;
}

int icpk_tsdf_integrate(icpk_ctx* ctx, const uint16_t* depth, const float* intensity, int32_t rows, int32_t cols, float fx,
                        float cx, const double pose[16], int32_t* n_updated) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (const char* why = check_camera(rows, cols, fx, cx)) return fail(ctx, ICPK_E_ARG, why);
  float R[9], t[3];
  if (icpk_tsdf_invert_pose(pose, R, t)) return fail(ctx, ICPK_E_ARG, "the pose is NULL or not finite");
  const bool color = (v->p.flags & ICPK_TSDF_COLOR) != 0;
  if (color != (intensity != nullptr))
    return fail(ctx, ICPK_E_ARG, color ? "a colour volume needs the frame's intensities" : "intensities given to a volume without ICPK_TSDF_COLOR");
  const size_t npix = (size_t)rows * cols;
  if (intensity && !intensities_ok(intensity, npix)) return fail(ctx, ICPK_E_ARG, "intensities must be finite and in [0, 1]");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const uint16_t* image = nullptr;
  if (depth) {
    if (int rc = v->depth.reserve(ctx, npix)) return rc;
    ICPK_HIP(ctx, hipMemcpyAsync(v->depth, depth, npix * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    image = v->depth;
  } else {
    if (ctx->frame_slot < 0 || ctx->frame_rows != rows || ctx->frame_cols != cols)
      return fail(ctx, ICPK_E_NOT_SET, "no resident frame of this size (icpk_backproject_pair), pass depth");
    // (two slots of rows x cols in either buffer; the filtered copy is the frame when the filter was on)
    image = (ctx->frame_filter[0] ? ctx->depth_flt.get() : ctx->depth_dev.get()) + (size_t)ctx->frame_slot * npix;
  }
  if (intensity) {
    if (int rc = v->intensity_image.reserve(ctx, npix)) return rc;
    ICPK_HIP(ctx, hipMemcpyAsync(v->intensity_image, intensity, npix * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  TsdfIntegrateArgs a{};
  a.fr = make_frame(v->p, R, t, rows, cols, fx, cx);
  a.depth = image;
  a.intensity_image = color ? v->intensity_image.get() : nullptr;
  a.tsdf = v->tsdf, a.weight = v->weight, a.intensity = v->intensity_plane();
  a.n = v->n, a.chunk = tsdf_chunk(v->n);
  a.slots = v->slots;
  launch_tsdf_integrate(a, tsdf_blocks(v->n), v->totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  if (!depth && !intensity && !n_updated) return ICPK_OK;  // (nothing of the caller's is in flight, nothing is asked)
  ICPK_HIP(ctx, hipMemcpyAsync(v->totals_host, v->totals, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_updated) *n_updated = (int32_t)v->totals_host[0];
  return ICPK_OK;
}

int icpk_tsdf_get(icpk_ctx* ctx, float* tsdf, uint16_t* weight, float* intensity) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (intensity && !(v->p.flags & ICPK_TSDF_COLOR)) return fail(ctx, ICPK_E_ARG, "the volume keeps no intensities");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)v->n;
  if (tsdf) ICPK_HIP(ctx, hipMemcpyAsync(tsdf, v->tsdf, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (weight) ICPK_HIP(ctx, hipMemcpyAsync(weight, v->weight, n * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  if (intensity) ICPK_HIP(ctx, hipMemcpyAsync(intensity, v->intensity, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_set(icpk_ctx* ctx, const float* tsdf, const uint16_t* weight, const float* intensity) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!tsdf || !weight) return fail(ctx, ICPK_E_ARG, "tsdf or weight is NULL");
  const bool color = (v->p.flags & ICPK_TSDF_COLOR) != 0;
  if (color != (intensity != nullptr))
    return fail(ctx, ICPK_E_ARG, color ? "a colour volume needs the intensity plane" : "intensities given to a volume without ICPK_TSDF_COLOR");
  const size_t n = (size_t)v->n;
  for (size_t i = 0; i < n; ++i)
    if (!(tsdf[i] >= -1.f && tsdf[i] <= 1.f)) return fail(ctx, ICPK_E_ARG, "tsdf must be finite and in [-1, 1]");  // (false for NaN)
  if (intensity && !intensities_ok(intensity, n)) return fail(ctx, ICPK_E_ARG, "intensities must be finite and in [0, 1]");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ICPK_HIP(ctx, hipMemcpyAsync(v->tsdf, tsdf, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(v->weight, weight, n * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
  if (intensity) ICPK_HIP(ctx, hipMemcpyAsync(v->intensity, intensity, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the caller's arrays are free again)
  icpk_esdf_drop(ctx);
  v->have_surface = false;
  v->have_raycast = false;
  v->have_mesh = false;
  return ICPK_OK;
}

// icpk_tsdf_extract_surface (s null), or icpk_tsdf_extract_leaving: the crossings a shift by s would lose
static int extract_list(icpk_ctx* ctx, int32_t min_weight, const int32_t* s, int32_t* n_points, int32_t* n_no_normal) {
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (min_weight < 1 || min_weight > 65535) return fail(ctx, ICPK_E_ARG, "min_weight outside 1 .. 65535");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool had_surface = v->have_surface;
  v->have_surface = false;
  TsdfExtractArgs a{};
  a.v = make_planes(v->p, v->tsdf, v->weight, v->intensity_plane(), min_weight);
  a.leaving = s != nullptr;
  if (s) a.keep = tsdf_keep_box(v->p.dims, s);
  a.n = v->n, a.chunk = tsdf_chunk(v->n);
  a.counts = v->slots, a.dropped = v->dropped, a.offsets = v->offsets;
  const int nblocks = tsdf_blocks(v->n);
  launch_tsdf_count(a, nblocks, v->totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  // the one host wait: the list is allocated for the count
  ICPK_HIP(ctx, hipMemcpyAsync(v->totals_host, v->totals, 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long listed = v->totals_host[0], dropped = v->totals_host[1];
  if (listed > ICPK_TSDF_MAX_SURFACE) {
    if (s) v->have_surface = had_surface;  // (a refused icpk_tsdf_extract_leaving: the list is as it was, nothing was written)
    return fail(ctx, ICPK_E_ARG, "more than ICPK_TSDF_MAX_SURFACE crossings");
  }
  if ((size_t)listed > v->surf_cap) {
    const size_t cap = (size_t)listed;
    v->surf_cap = 0;
    int rc = reserve_group(ctx, nullptr, need(v->surf, 7 * cap), need(v->surf_voxel, cap), need(v->surf_axis, cap));
    if (rc) return rc;
    v->surf_cap = cap;
  }
  if (listed > 0) {
    a.capacity = listed;
    a.x = v->plane(0), a.y = v->plane(1), a.z = v->plane(2);
    a.nx = v->plane(3), a.ny = v->plane(4), a.nz = v->plane(5);
    a.intensity = v->plane(6);
    a.voxel_index = v->surf_voxel, a.axis = v->surf_axis;
    launch_tsdf_scatter(a, nblocks, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
  }
  v->surf_n = (int)listed;
  v->surf_dropped = dropped > INT32_MAX ? INT32_MAX : (int)dropped;
  v->have_surface = true;
  if (n_points) *n_points = v->surf_n;
  if (n_no_normal) *n_no_normal = v->surf_dropped;
  return ICPK_OK;
}

int icpk_tsdf_extract_surface(icpk_ctx* ctx, int32_t min_weight, int32_t* n_points, int32_t* n_no_normal) {
  if (!ctx) return ICPK_E_ARG;
  return extract_list(ctx, min_weight, nullptr, n_points, n_no_normal);
}

int icpk_tsdf_extract_leaving(icpk_ctx* ctx, int32_t min_weight, const int32_t s[3], int32_t* n_points, int32_t* n_no_normal) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->tsdf) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!s) return fail(ctx, ICPK_E_ARG, "the shift is NULL");
  return extract_list(ctx, min_weight, s, n_points, n_no_normal);
}

int icpk_tsdf_shift(icpk_ctx* ctx, const int32_t s[3]) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!s) return fail(ctx, ICPK_E_ARG, "the shift is NULL");
  if (s[0] == 0 && s[1] == 0 && s[2] == 0) return ICPK_OK;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const bool color = (v->p.flags & ICPK_TSDF_COLOR) != 0;
  const size_t n = (size_t)v->n;
  // (the second set of planes: by the first shift, kept with the volume.  A failure here leaves the volume as it was)
  int rc = v->tsdf_next.reserve(ctx, n);
  if (!rc) rc = v->weight_next.reserve(ctx, n);
  if (!rc && color) rc = v->intensity_next.reserve(ctx, n);
  if (rc) return rc;
  TsdfShiftArgs a{};
  a.tsdf_in = v->tsdf, a.weight_in = v->weight, a.intensity_in = v->intensity_plane();
  a.tsdf_out = v->tsdf_next, a.weight_out = v->weight_next, a.intensity_out = color ? v->intensity_next.get() : nullptr;
  const TsdfKeep box = tsdf_keep_box(v->p.dims, s);
  for (int k = 0; k < 3; ++k) a.dims[k] = v->p.dims[k], a.s[k] = box.lo[k];  // (lo: s clamped to -dims .. dims)
  a.n = v->n, a.chunk = tsdf_chunk(v->n);
  launch_tsdf_shift(a, tsdf_blocks(v->n), ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  // the sets change places: everything later on the stream reads the new one, the old one is the next shift's room
  std::swap(v->tsdf, v->tsdf_next);
  std::swap(v->weight, v->weight_next);
  if (color) std::swap(v->intensity, v->intensity_next);
  for (int k = 0; k < 3; ++k) {
    v->total[k] += s[k];
    v->p.origin[k] = tsdf_shifted_origin(v->origin0[k], v->total[k], v->p.voxel);
  }
  icpk_esdf_drop(ctx);
  v->have_surface = false;
  v->have_raycast = false;
  v->have_mesh = false;
  return ICPK_OK;
}

int icpk_tsdf_get_params(icpk_ctx* ctx, icpk_tsdf_params* out, int64_t total[3]) {
  if (!ctx) return ICPK_E_ARG;
  const icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (out) *out = v->p;
  if (total)
    for (int k = 0; k < 3; ++k) total[k] = v->total[k];
  return ICPK_OK;
}

int icpk_tsdf_get_box(icpk_ctx* ctx, const int32_t lo[3], const int32_t hi[3], float* tsdf, uint16_t* weight, float* intensity) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!lo || !hi) return fail(ctx, ICPK_E_ARG, "lo or hi is NULL");
  TsdfBoxArgs a{};
  a.m = 1;
  for (int k = 0; k < 3; ++k) {
    if (lo[k] < 0 || hi[k] > v->p.dims[k] || lo[k] >= hi[k]) return fail(ctx, ICPK_E_ARG, "the box is empty or out of bounds");
    a.dims[k] = v->p.dims[k], a.lo[k] = lo[k], a.size[k] = hi[k] - lo[k];
    a.m *= a.size[k];  // (<= n <= 2^30)
  }
  if (intensity && !(v->p.flags & ICPK_TSDF_COLOR)) return fail(ctx, ICPK_E_ARG, "the volume keeps no intensities");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)a.m;
  if (tsdf || intensity)
    if (int rc = v->box_f.reserve(ctx, m)) return rc;
  if (weight)
    if (int rc = v->box_w.reserve(ctx, m)) return rc;
  // (one staging buffer for both float planes: the copy of the first is in front of the second's kernel on the stream)
  const float* const planes[2] = {v->tsdf.get(), v->intensity.get()};
  float* const out[2] = {tsdf, intensity};
  for (int k = 0; k < 2; ++k) {
    if (!out[k]) continue;
    launch_tsdf_box(a, planes[k], v->box_f.get(), ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    ICPK_HIP(ctx, hipMemcpyAsync(out[k], v->box_f, m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (weight) {
    launch_tsdf_box(a, v->weight.get(), v->box_w.get(), ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
    ICPK_HIP(ctx, hipMemcpyAsync(weight, v->box_w, m * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_get_surface(icpk_ctx* ctx, float* x, float* y, float* z, float* nx, float* ny, float* nz, float* intensity,
                          int32_t* voxel_index, uint8_t* axis) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_surface) return fail(ctx, ICPK_E_NOT_SET, "no surface list (icpk_tsdf_extract_surface)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  float* const out[7] = {x, y, z, nx, ny, nz, intensity};
  const DevList surface{v->surf, v->surf_cap, v->surf_voxel, v->surf_axis};
  if (int rc = download_list(ctx, surface, (size_t)v->surf_n, out, voxel_index, axis)) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_surface_to_target(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_surface) return fail(ctx, ICPK_E_NOT_SET, "no surface list (icpk_tsdf_extract_surface)");
  if (v->surf_n == 0) return fail(ctx, ICPK_E_EMPTY_TARGET, "the surface list is empty");
  float* const list[7] = {v->plane(0), v->plane(1), v->plane(2), v->plane(3), v->plane(4), v->plane(5), v->plane(6)};
  return list_to_target(ctx, v, list, v->surf_n);
}

int icpk_tsdf_extract_mesh(icpk_ctx* ctx, int32_t min_weight, int32_t* n_vertices, int32_t* n_triangles, int32_t* n_no_normal) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (min_weight < 1 || min_weight > 65535) return fail(ctx, ICPK_E_ARG, "min_weight outside 1 .. 65535");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  v->have_mesh = false;
  int rc = v->mesh_vcounts.reserve(ctx, TSDF_MAX_BLOCKS);
  if (!rc) rc = v->mesh_tcounts.reserve(ctx, TSDF_MAX_BLOCKS);
  if (!rc) rc = v->mesh_nonormal.reserve(ctx, TSDF_MAX_BLOCKS);
  if (!rc) rc = v->mesh_voffsets.reserve(ctx, TSDF_MAX_BLOCKS + 1);
  if (!rc) rc = v->mesh_toffsets.reserve(ctx, TSDF_MAX_BLOCKS + 1);
  if (!rc) rc = v->mesh_totals.reserve(ctx, 3);
  if (!rc) rc = v->mesh_totals_host.reserve(ctx, 3);
  if (rc) return rc;
  TsdfMeshArgs a{};
  a.v = make_planes(v->p, v->tsdf, v->weight, v->intensity_plane(), min_weight);
  a.n = v->n, a.chunk = tsdf_chunk(v->n);
  a.vcounts = v->mesh_vcounts, a.tcounts = v->mesh_tcounts, a.nonormal = v->mesh_nonormal;
  a.voffsets = v->mesh_voffsets, a.toffsets = v->mesh_toffsets;
  const int nblocks = tsdf_blocks(v->n);
  launch_tsdf_mesh_count(a, nblocks, v->mesh_totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  // the one host wait: the lists are allocated for the counts
  ICPK_HIP(ctx, hipMemcpyAsync(v->mesh_totals_host, v->mesh_totals, 3 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long nv = v->mesh_totals_host[0], nn = v->mesh_totals_host[1], nt = v->mesh_totals_host[2];
  if (nv > ICPK_TSDF_MAX_SURFACE || nt > ICPK_TSDF_MAX_SURFACE)
    return fail(ctx, ICPK_E_ARG, "more than ICPK_TSDF_MAX_SURFACE vertices or triangles");
  if ((size_t)nv > v->mesh_vcap) {
    const size_t cap = (size_t)nv;
    v->mesh_vcap = 0;
    rc = reserve_group(ctx, nullptr, need(v->mesh, 7 * cap), need(v->mesh_voxel, cap), need(v->mesh_edge, cap));
    if (rc) return rc;
    v->mesh_vcap = cap;
  }
  if ((size_t)nt > v->mesh_tcap) {
    v->mesh_tcap = 0;
    if ((rc = v->mesh_tri.reserve(ctx, 3 * (size_t)nt))) return rc;
    v->mesh_tcap = (size_t)nt;
  }
  if (nv > 0) {
    a.vcapacity = nv, a.tcapacity = nt;
    a.x = v->mesh_plane(0), a.y = v->mesh_plane(1), a.z = v->mesh_plane(2);
    a.nx = v->mesh_plane(3), a.ny = v->mesh_plane(4), a.nz = v->mesh_plane(5);
    a.intensity = v->mesh_plane(6);
    a.voxel_index = v->mesh_voxel, a.edge = v->mesh_edge, a.triangles = v->mesh_tri;
    launch_tsdf_mesh_scatter(a, nblocks, ctx->stream);
    ICPK_HIP(ctx, hipGetLastError());
  }
  v->mesh_nv = (int)nv, v->mesh_nt = (int)nt, v->mesh_nn = (int)nn;
  v->have_mesh = true;
  if (n_vertices) *n_vertices = v->mesh_nv;
  if (n_triangles) *n_triangles = v->mesh_nt;
  if (n_no_normal) *n_no_normal = v->mesh_nn;
  return ICPK_OK;
}

int icpk_tsdf_get_mesh(icpk_ctx* ctx, float* x, float* y, float* z, float* nx, float* ny, float* nz, float* intensity,
                       int32_t* voxel_index, uint8_t* edge, int32_t* triangles) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_mesh) return fail(ctx, ICPK_E_NOT_SET, "no mesh (icpk_tsdf_extract_mesh)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)v->mesh_nt;
  float* const out[7] = {x, y, z, nx, ny, nz, intensity};
  const DevList vertices{v->mesh, v->mesh_vcap, v->mesh_voxel, v->mesh_edge};
  if (int rc = download_list(ctx, vertices, (size_t)v->mesh_nv, out, voxel_index, edge)) return rc;
  if (triangles && m > 0)
    ICPK_HIP(ctx, hipMemcpyAsync(triangles, v->mesh_tri, 3 * m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_mesh_host(const icpk_tsdf_params* params, int32_t min_weight, const float* tsdf, const uint16_t* weight,
                        const float* intensity, int64_t cap_vertices, int64_t cap_triangles, float* x, float* y, float* z,
                        float* nx, float* ny, float* nz, float* intensity_out, int32_t* voxel_index, uint8_t* edge,
                        int32_t* triangles, int64_t counts[3]) {
  if (!params || !tsdf || !weight || !counts || cap_vertices < 0 || cap_triangles < 0) return ICPK_E_ARG;
  if (check_params(*params) || min_weight < 1 || min_weight > 65535) return ICPK_E_ARG;
  if (((params->flags & ICPK_TSDF_COLOR) != 0) != (intensity != nullptr)) return ICPK_E_ARG;
  const TsdfPlanes v = make_planes(*params, tsdf, weight, intensity, min_weight);
  const long long dx = v.dims[0], dxy = dx * v.dims[1], n = dxy * v.dims[2];
  // the count pass
  long long nv = 0, nt = 0, nn = 0;
  for (long long at = 0; at < n; ++at) {
    const int k = (int)(at / dxy), j = (int)((at - k * dxy) / dx);
    const int c[3] = {(int)(at - k * dxy - j * dx), j, k};
    TsdfMeshVoxel mv;
    tsdf_mesh_voxel(v, c, at, true, &mv);
    nt += mv.triangles;
    for (int m = 1; m < 8; ++m)
      if ((mv.vertices >> (m - 1)) & 1) nv += 1, nn += !tsdf_mesh_vertex(v, c, at, m, nullptr);
  }
  counts[0] = nv, counts[1] = nt, counts[2] = nn;
  if (nv > cap_vertices || nt > cap_triangles || nv > ICPK_TSDF_MAX_SURFACE || nt > ICPK_TSDF_MAX_SURFACE) return ICPK_E_ARG;
  // the vertices in (voxel, m) order, with their keys, then the triangles by a search over the keys
  std::vector<long long> keys;
  keys.reserve((size_t)nv);
  std::vector<std::pair<long long, TsdfMeshVoxel>> cells;
  for (long long at = 0; at < n; ++at) {
    const int k = (int)(at / dxy), j = (int)((at - k * dxy) / dx);
    const int c[3] = {(int)(at - k * dxy - j * dx), j, k};
    TsdfMeshVoxel mv;
    tsdf_mesh_voxel(v, c, at, true, &mv);
    if (mv.triangles > 0) cells.emplace_back(at, mv);
    for (int m = 1; m < 8; ++m) {
      if (!((mv.vertices >> (m - 1)) & 1)) continue;
      TsdfMeshVertex vx;
      tsdf_mesh_vertex(v, c, at, m, &vx);
      const size_t pos = keys.size();
      keys.push_back(at * 8 + m);
      float* const out[7] = {x, y, z, nx, ny, nz, intensity_out};
      const float val[7] = {vx.p[0], vx.p[1], vx.p[2], vx.n[0], vx.n[1], vx.n[2], vx.intensity};
      for (int q = 0; q < 7; ++q)
        if (out[q]) out[q][pos] = val[q];
      if (voxel_index) voxel_index[pos] = (int32_t)at;
      if (edge) edge[pos] = (uint8_t)m;
    }
  }
  if (!triangles) return ICPK_OK;
  long long pos = 0;
  for (const auto& cell : cells) {
    for (int tet = 0; tet < 6; ++tet) {
      int vc[4];
      tsdf_tet_corners(tet, vc);
      const int cs = tsdf_tet_case(cell.second.signs, vc);
      const unsigned code = tsdf_case_table(cs);
      for (int tri = 0; tri < tsdf_case_triangles(cs); ++tri, ++pos)
        for (int q = 0; q < 3; ++q) {
          int corner, m;
          tsdf_triangle_edge(vc, tsdf_tet_odd(tet), code, tri, q, &corner, &m);
          const long long key = (cell.first + tsdf_mask_offset(v, corner)) * 8 + m;
          const auto it = std::lower_bound(keys.begin(), keys.end(), key);
          triangles[3 * pos + q] = it != keys.end() && *it == key ? (int32_t)(it - keys.begin()) : -1;
        }
    }
  }
  return ICPK_OK;
}

int icpk_tsdf_voxel_update(const icpk_tsdf_params* params, const float R[9], const float t[3], const uint16_t* depth,
                           const float* intensity, int32_t rows, int32_t cols, float fx, float cx, int64_t first,
                           int32_t count, float* tsdf, uint16_t* weight, float* intensity_value) {
  if (!params || !R || !t || !depth || !tsdf || !weight || count < 0 || first < 0) return ICPK_E_ARG;
  if (check_params(*params) || check_camera(rows, cols, fx, cx)) return ICPK_E_ARG;
  const bool color = (params->flags & ICPK_TSDF_COLOR) != 0;
  if (color != (intensity != nullptr) || color != (intensity_value != nullptr)) return ICPK_E_ARG;
  const long long n = (long long)params->dims[0] * params->dims[1] * params->dims[2];
  if (first + count > n) return ICPK_E_ARG;
  const TsdfFrame fr = make_frame(*params, R, t, rows, cols, fx, cx);
  const long long dx = fr.dims[0], dxy = dx * fr.dims[1];
  int written = 0;
  for (int32_t e = 0; e < count; ++e) {
    const long long at = first + e;
    const int k = (int)(at / dxy), j = (int)((at - k * dxy) / dx), i = (int)(at - k * dxy - j * dx);
    written += tsdf_voxel_update(fr, i, j, k, depth, intensity, &tsdf[e], &weight[e], color ? &intensity_value[e] : nullptr);
  }
  return written;
}

void icpk_default_tsdf_raycast_params(icpk_tsdf_raycast_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->rows = 480, p->cols = 640;
  p->fx = 468.60f, p->cx = 318.27f;
  p->z_near = 0.25f, p->z_far = 6.0f;
  p->step = 0.f;
  p->min_weight = 1;
}

int icpk_tsdf_raycast(icpk_ctx* ctx, const icpk_tsdf_raycast_params* params, const double pose[16], int32_t* n_hits,
                      int32_t* n_no_normal) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  icpk_tsdf_raycast_params rp;
  icpk_default_tsdf_raycast_params(&rp);
  if (params) rp = *params;
  TsdfRaycastArgs a{};
  if (const char* why = make_ray(v->p, rp, pose, &a.r)) return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)rp.rows * rp.cols;
  bool grown = false;
  if (int rc = v->ray_maps.reserve(ctx, 8 * npix, &grown)) {
    if (grown) v->have_raycast = false;
    return rc;
  }
  v->have_raycast = false;  // (the planes change place with the image's size)
  v->have_ray_grad = v->have_ray_grad_sums = false;  // (K26: the gradients are those of the maps they were made from)
  a.v = make_planes(v->p, v->tsdf, v->weight, v->intensity_plane(), rp.min_weight);
  a.maps = v->ray_maps;
  a.tiles_x = tsdf_ray_tiles(rp.cols);
  a.ntiles = a.tiles_x * tsdf_ray_tiles(rp.rows);
  a.hits = v->slots, a.dropped = v->dropped;
  launch_tsdf_raycast(a, tsdf_ray_blocks(rp.rows, rp.cols), v->totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  v->ray_rows = rp.rows, v->ray_cols = rp.cols;
  v->ray_fx = rp.fx, v->ray_cx = rp.cx;
  std::memcpy(v->ray_pose, pose, sizeof(v->ray_pose));
  v->have_raycast = true;
  if (!n_hits && !n_no_normal) return ICPK_OK;  // (nothing is asked: the call does not wait)
  ICPK_HIP(ctx, hipMemcpyAsync(v->totals_host, v->totals, 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (n_hits) *n_hits = (int32_t)v->totals_host[0];
  if (n_no_normal) *n_no_normal = (int32_t)v->totals_host[1];
  return ICPK_OK;
}

int icpk_tsdf_get_raycast(icpk_ctx* ctx, float* x, float* y, float* z, float* nx, float* ny, float* nz, float* depth,
                          float* intensity) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_raycast) return fail(ctx, ICPK_E_NOT_SET, "no ray cast (icpk_tsdf_raycast)");
  if (intensity && !(v->p.flags & ICPK_TSDF_COLOR)) return fail(ctx, ICPK_E_ARG, "the volume keeps no intensities");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)v->ray_rows * v->ray_cols;
  float* const out[8] = {x, y, z, nx, ny, nz, depth, intensity};
  for (int k = 0; k < 8; ++k)
    if (out[k])
      ICPK_HIP(ctx, hipMemcpyAsync(out[k], v->ray_maps + (size_t)k * npix, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

// ---- K26: the colour gradients of the view (include/icpk.h, THE VIEW GRADIENT RULE; kernels_raycast_color.hip) ----
int icpk_tsdf_raycast_color_gradients(icpk_ctx* ctx, float radius, int32_t min_neighbors, int32_t flags) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v) return fail(ctx, ICPK_E_NOT_SET, "no TSDF volume (icpk_tsdf_create)");
  if (!v->have_raycast) return fail(ctx, ICPK_E_NOT_SET, "no ray cast (icpk_tsdf_raycast)");
  if (!(v->p.flags & ICPK_TSDF_COLOR)) return fail(ctx, ICPK_E_ARG, "the volume keeps no intensities");
  if (!positive(radius) || min_neighbors < 1 || (flags & ~ICPK_COLOR_KEEP_SUMS))
    return fail(ctx, ICPK_E_ARG, "radius must be finite and > 0, min_neighbors >= 1, flags known");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)v->ray_rows * v->ray_cols;
  const bool keep = (flags & ICPK_COLOR_KEEP_SUMS) != 0;
  v->have_ray_grad = v->have_ray_grad_sums = false;
  if (int rc = v->ray_grad.reserve(ctx, 3 * npix)) return rc;
  if (keep)
    if (int rc = v->ray_grad_sums.reserve(ctx, (size_t)COLOR_SUMS * npix)) return rc;
  launch_raycast_color_gradients(v->ray_maps, v->ray_rows, v->ray_cols, radius, min_neighbors, v->ray_grad,
                                 keep ? v->ray_grad_sums.get() : nullptr, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  v->have_ray_grad = true;
  v->have_ray_grad_sums = keep;
  return ICPK_OK;
}

int icpk_tsdf_get_raycast_color_gradients(icpk_ctx* ctx, float* gx, float* gy, float* gz) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_raycast || !v->have_ray_grad)
    return fail(ctx, ICPK_E_NOT_SET, "no colour gradients of the view (icpk_tsdf_raycast_color_gradients)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)v->ray_rows * v->ray_cols;
  float* const out[3] = {gx, gy, gz};
  for (int k = 0; k < 3; ++k)
    if (out[k])
      ICPK_HIP(ctx, hipMemcpyAsync(out[k], v->ray_grad + (size_t)k * npix, npix * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_get_raycast_color_gradient_sums(icpk_ctx* ctx, int64_t* sums) {
  if (!ctx || !sums) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_raycast || !v->have_ray_grad || !v->have_ray_grad_sums)
    return fail(ctx, ICPK_E_NOT_SET, "no kept sums (icpk_tsdf_raycast_color_gradients with ICPK_COLOR_KEEP_SUMS)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)v->ray_rows * v->ray_cols;
  ICPK_HIP(ctx, hipMemcpyAsync(sums, v->ray_grad_sums.get(), npix * COLOR_SUMS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_tsdf_raycast_to_target(icpk_ctx* ctx) {
  if (!ctx) return ICPK_E_ARG;
  icpk_tsdf_state* v = ctx->tsdf;
  if (!v || !v->have_raycast) return fail(ctx, ICPK_E_NOT_SET, "no ray cast (icpk_tsdf_raycast)");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  TsdfRayCompactArgs a{};
  a.maps = v->ray_maps;
  a.npix = v->ray_rows * v->ray_cols;
  a.counts = v->slots, a.offsets = v->offsets;
  launch_tsdf_ray_count(a, v->totals, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  // the one host wait: the target is allocated for the count
  ICPK_HIP(ctx, hipMemcpyAsync(v->totals_host, v->totals, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const long long n = v->totals_host[0];
  if (n == 0) return fail(ctx, ICPK_E_EMPTY_TARGET, "the ray cast hit nothing");
  if ((size_t)n > v->ray_list_cap) {
    v->ray_list_cap = 0;
    if (int rc = v->ray_list.reserve(ctx, 7 * (size_t)n)) return rc;
    v->ray_list_cap = (size_t)n;
  }
  a.capacity = (long long)v->ray_list_cap;
  a.list = v->ray_list;
  launch_tsdf_ray_scatter(a, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  float* list[7];
  for (int k = 0; k < 7; ++k) list[k] = v->ray_list + (size_t)k * v->ray_list_cap;
  return list_to_target(ctx, v, list, (int)n);
}

int icpk_tsdf_raycast_pixels(const icpk_tsdf_params* params, const icpk_tsdf_raycast_params* ray, const double pose[16],
                             const float* tsdf, const uint16_t* weight, const float* intensity, int64_t first, int32_t count,
                             float* out) {
  if (!params || !ray || !tsdf || !weight || !out || count < 0 || first < 0) return ICPK_E_ARG;
  if (check_params(*params)) return ICPK_E_ARG;
  if (((params->flags & ICPK_TSDF_COLOR) != 0) != (intensity != nullptr)) return ICPK_E_ARG;
  TsdfRay r{};
  if (make_ray(*params, *ray, pose, &r)) return ICPK_E_ARG;
  if (first + count > (int64_t)r.rows * r.cols) return ICPK_E_ARG;
  const TsdfPlanes v = make_planes(*params, tsdf, weight, intensity, ray->min_weight);
  int listed = 0;
  for (int32_t e = 0; e < count; ++e) {
    const int64_t pix = first + e;
    float px[8];
    listed += tsdf_raycast_pixel(v, r, (int)(pix / r.cols), (int)(pix % r.cols), px) == TSDF_RAY_HIT;
    for (int k = 0; k < 8; ++k) out[(size_t)k * count + e] = px[k];
  }
  return listed;
}

}  // extern "C"
