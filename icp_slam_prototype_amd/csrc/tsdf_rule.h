// tsdf_rule.h -- the per-voxel rule and the surface rule of the TSDF volume (K19; include/icpk.h writes both out).
// Header-inline and __host__ __device__: kernels_tsdf.hip runs it per voxel on the device, icpk_tsdf.cpp exports it
// for one voxel on the host (icpk_tsdf_voxel_update), compiled with -ffp-contract=off on both sides.  float32 only,
// +, -, *, / and sqrt in the order written, no libm: the same bits wherever those five are correctly rounded.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef ICPK_HD
#define ICPK_HD __host__ __device__ inline
#endif
#else
#ifndef ICPK_HD
#define ICPK_HD inline
#endif
#endif
#include <stdint.h>

namespace icpk {

// what one integration reads besides the image: the volume's geometry and the frame's camera
struct TsdfFrame {
  int dims[3];
  float voxel;
  float origin[3];
  float trunc;
  float depth_scale;
  int max_weight;
  int rows, cols;
  float fx, cx;
  float R[9], t[3];  // world -> camera: the inverted pose, rounded to float once
};

// the centre of voxel i along one axis (rule 1)
ICPK_HD float tsdf_centre(int i, float voxel, float origin) { return ((float)i + 0.5f) * voxel + origin; }

// Rules 1 - 7 for voxel (i, j, k): false when the voxel is left alone; else *f = min(1, sdf / trunc) and *pixel = the
// pixel it projects onto.  Nothing of the volume is read.
ICPK_HD bool tsdf_sample(const TsdfFrame& fr, int i, int j, int k, const uint16_t* __restrict__ depth, float* f, int* pixel) {
  const float px = tsdf_centre(i, fr.voxel, fr.origin[0]);
  const float py = tsdf_centre(j, fr.voxel, fr.origin[1]);
  const float pz = tsdf_centre(k, fr.voxel, fr.origin[2]);
  const float qx = ((fr.R[0] * px + fr.R[1] * py) + fr.R[2] * pz) + fr.t[0];
  const float qy = ((fr.R[3] * px + fr.R[4] * py) + fr.R[5] * pz) + fr.t[1];
  const float qz = ((fr.R[6] * px + fr.R[7] * py) + fr.R[8] * pz) + fr.t[2];
  if (!(qz > 0.f)) return false;
  const float u = (qx * fr.fx) / qz + fr.cx;
  const float v = (qy * fr.fx) / qz + fr.cx;  // (cx and fx serve both axes: pointcloud.cpp:37-39)
  // floor(u + 0.5) inside [0, cols): for a >= 0 the conversion truncates to the floor; a in (-1, 0) would floor to -1,
  // NaN and +-inf compare false
  const float a = u + 0.5f, b = v + 0.5f;
  if (!(a >= 0.f && a < (float)fr.cols && b >= 0.f && b < (float)fr.rows)) return false;
  const int pix = (int)b * fr.cols + (int)a;
  const uint16_t d = depth[pix];
  if (d == 0) return false;
  const float sdf = (float)d / fr.depth_scale - qz;
  if (sdf < -fr.trunc) return false;
  const float r = sdf / fr.trunc;
  *f = r > 1.f ? 1.f : r;
  *pixel = pix;
  return true;
}

// rule 8 (and 9): the running mean of `value` after w samples takes one more
ICPK_HD float tsdf_blend(float value, int w, float sample) { return (value * (float)w + sample) / ((float)w + 1.f); }

// The whole rule for one voxel; tsdf / weight / intensity: the voxel's state, in and out (intensity and
// intensity_image may both be null).  Returns whether the voxel was written.
ICPK_HD bool tsdf_voxel_update(const TsdfFrame& fr, int i, int j, int k, const uint16_t* __restrict__ depth,
                               const float* __restrict__ intensity_image, float* tsdf, uint16_t* weight, float* intensity) {
  float f;
  int pix;
  if (!tsdf_sample(fr, i, j, k, depth, &f, &pix)) return false;
  const int w = *weight;
  *tsdf = tsdf_blend(*tsdf, w, f);
  if (intensity && intensity_image) *intensity = tsdf_blend(*intensity, w, intensity_image[pix]);
  *weight = (uint16_t)(w + 1 < fr.max_weight ? w + 1 : fr.max_weight);
  return true;
}

// ---- the surface rule ----
struct TsdfPlanes {
  const float* tsdf;
  const uint16_t* weight;
  const float* intensity;  // or null
  int dims[3];
  float voxel;
  float origin[3];
  int min_weight;
};

struct TsdfCrossing {
  float p[3], n[3], intensity;
};

// the three central differences of tsdf at voxel (c[0], c[1], c[2]) with linear index `at`: false unless all six
// neighbours are in bounds with weight >= min_weight
ICPK_HD bool tsdf_gradient(const TsdfPlanes& v, const int c[3], long long at, float g[3]) {
  long long stride = 1;
  for (int a = 0; a < 3; ++a) {
    if (c[a] < 1 || c[a] + 1 >= v.dims[a]) return false;
    const long long lo = at - stride, hi = at + stride;
    if ((int)v.weight[lo] < v.min_weight || (int)v.weight[hi] < v.min_weight) return false;
    g[a] = v.tsdf[hi] - v.tsdf[lo];
    stride *= v.dims[a];
  }
  return true;
}

enum { TSDF_NO_CROSSING = 0, TSDF_CROSSING = 1, TSDF_NO_NORMAL = 2 };

// the crossing between voxel V = (c[0], c[1], c[2]) (linear index `at`, weight >= min_weight already seen, value fv)
// and its +1 neighbour along `axis`.  out may be null (the counting pass)
ICPK_HD int tsdf_crossing(const TsdfPlanes& v, const int c[3], long long at, float fv, int axis, TsdfCrossing* out) {
  if (c[axis] + 1 >= v.dims[axis]) return TSDF_NO_CROSSING;
  const long long stride = axis == 0 ? 1 : axis == 1 ? (long long)v.dims[0] : (long long)v.dims[0] * v.dims[1];
  const long long nb = at + stride;
  if ((int)v.weight[nb] < v.min_weight) return TSDF_NO_CROSSING;
  const float fn = v.tsdf[nb];
  if ((fv < 0.f) == (fn < 0.f)) return TSDF_NO_CROSSING;
  const float t = fv / (fv - fn);
  float gv[3], gn[3];
  int cn[3] = {c[0], c[1], c[2]};
  cn[axis] += 1;
  if (!tsdf_gradient(v, c, at, gv) || !tsdf_gradient(v, cn, nb, gn)) return TSDF_NO_NORMAL;
  float n[3];
  for (int a = 0; a < 3; ++a) n[a] = gv[a] + t * (gn[a] - gv[a]);
  const float len = __builtin_sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(len > 0.f)) return TSDF_NO_NORMAL;
  if (out) {
    for (int a = 0; a < 3; ++a) {
      out->p[a] = tsdf_centre(c[a], v.voxel, v.origin[a]);
      out->n[a] = n[a] / len;
    }
    out->p[axis] = out->p[axis] + t * v.voxel;
    out->intensity = v.intensity ? v.intensity[at] + t * (v.intensity[nb] - v.intensity[at]) : 0.f;
  }
  return TSDF_CROSSING;
}

}  // namespace icpk
