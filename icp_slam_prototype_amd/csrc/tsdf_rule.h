// tsdf_rule.h -- the per-voxel rule, the surface rule (K19), the ray rule (K20), the mesh rule (K21) and the signed
// update rule (K30, kernels_tsdf_apply.hip and icpk_tsdf_voxel_apply) of the TSDF volume; include/icpk.h writes them out.
// Header-inline and __host__ __device__: kernels_tsdf.hip runs it per voxel on the device, icpk_tsdf.cpp exports it
// for one voxel, for one pixel and for a whole mesh on the host (icpk_tsdf_voxel_update, icpk_tsdf_raycast_pixels,
// icpk_tsdf_mesh_host), compiled with -ffp-contract=off on both sides.  float32 only, +, -, *, / and sqrt in the order
// written, no libm: the same bits wherever those five are correctly rounded.
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

// ---- the signed update rule (K30) ----
// the inverse of tsdf_blend: the running mean of w >= 2 samples gives `sample` back, clamped to [lo, 1] (the mean of
// the samples that stay lies there; the rounding of the three operations may not)
ICPK_HD float tsdf_unblend(float value, int w, float sample, float lo) {
  const float r = (value * (float)w - sample) / ((float)w - 1.f);
  return r < lo ? lo : r > 1.f ? 1.f : r;
}

// One op on a voxel's state, after rules 1 - 7 have produced the sample f (and the pixel's intensity c).  color: whether
// the volume keeps intensities; *intensity is read and written only then (it points somewhere either way).  sign +1:
// rules 8 - 10 as they are.  sign -1: w == 0 leaves the voxel alone, w == 1 gives the fresh state back, else the
// inverse of the blend and w - 1.  Returns whether the voxel was written.
ICPK_HD bool tsdf_state_apply(int sign, int max_weight, float f, float c, bool color, float* tsdf, int* weight, float* intensity) {
  const int w = *weight;
  if (sign > 0) {
    *tsdf = tsdf_blend(*tsdf, w, f);
    if (color) *intensity = tsdf_blend(*intensity, w, c);
    *weight = w + 1 < max_weight ? w + 1 : max_weight;
    return true;
  }
  if (w == 0) return false;
  if (w == 1) {
    *tsdf = 0.f;
    if (color) *intensity = 0.f;
    *weight = 0;
    return true;
  }
  *tsdf = tsdf_unblend(*tsdf, w, f, -1.f);
  if (color) *intensity = tsdf_unblend(*intensity, w, c, 0.f);
  *weight = w - 1;
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

// ---- the shift rule (K23) ----
// the old voxel indices a shift by s keeps: lo[a] <= v_a < hi[a], lo = s and hi = dims + s with s clamped to
// -dims .. dims (a larger shift keeps nothing either way, and the sums stay ints)
struct TsdfKeep {
  int lo[3], hi[3];
};

ICPK_HD TsdfKeep tsdf_keep_box(const int dims[3], const int s[3]) {
  TsdfKeep b;
  for (int a = 0; a < 3; ++a) {
    const int sa = s[a] < -dims[a] ? -dims[a] : s[a] > dims[a] ? dims[a] : s[a];
    b.lo[a] = sa, b.hi[a] = dims[a] + sa;
  }
  return b;
}

// the origin after a cumulative shift of `total` voxels: from the creation origin, in double, rounded once
ICPK_HD float tsdf_shifted_origin(float origin0, long long total, float voxel) {
  return (float)((double)origin0 + (double)total * (double)voxel);
}

// stays(V) and stays(N) for the crossing between V = c and its +1 neighbour N along `axis`
ICPK_HD bool tsdf_ends_stay(const TsdfKeep& b, const int c[3], int axis) {
  for (int a = 0; a < 3; ++a)
    if (c[a] < b.lo[a] || c[a] + (a == axis) >= b.hi[a]) return false;
  return true;
}

// whether the shift keeps that crossing: V, N and the six axis neighbours of each stay, so that both gradients are
// still there in the shifted volume
ICPK_HD bool tsdf_crossing_kept(const TsdfKeep& b, const int c[3], int axis) {
  for (int a = 0; a < 3; ++a)
    if (c[a] - 1 < b.lo[a] || c[a] + 1 + (a == axis) >= b.hi[a]) return false;
  return true;
}

// what the leaving list makes of a crossing's status: a listed crossing the shift keeps, and a dropped one whose two
// ends stay, are none of its business
ICPK_HD int tsdf_leaving_status(const TsdfKeep& b, const int c[3], int axis, int status) {
  if (status == TSDF_CROSSING && tsdf_crossing_kept(b, c, axis)) return TSDF_NO_CROSSING;
  if (status == TSDF_NO_NORMAL && tsdf_ends_stay(b, c, axis)) return TSDF_NO_CROSSING;
  return status;
}

// ---- the ray rule (K20) ----
// the camera of one ray cast: camera-to-world, its nine R and three c rounded to float once (rule 0)
struct TsdfRay {
  int rows, cols;
  float fx, cx;
  float R[9], c[3];
  float z_near, step;
  int nsamples;  // N of rule 3
};

enum { TSDF_RAY_NONE = 0, TSDF_RAY_HIT = 1, TSDF_RAY_NO_NORMAL = 2, TSDF_RAY_BACK_FACE = 3 };

ICPK_HD float tsdf_lerp(float u, float v, float w) { return u + w * (v - u); }

// e[x + 2 y + 4 z]: along x for the four (y, z) pairs, then along y, then along z
ICPK_HD float tsdf_trilerp(const float e[8], const float w[3]) {
  const float c00 = tsdf_lerp(e[0], e[1], w[0]), c10 = tsdf_lerp(e[2], e[3], w[0]);
  const float c01 = tsdf_lerp(e[4], e[5], w[0]), c11 = tsdf_lerp(e[6], e[7], w[0]);
  return tsdf_lerp(tsdf_lerp(c00, c10, w[1]), tsdf_lerp(c01, c11, w[1]), w[2]);
}

// the gradient of tsdf_trilerp's interpolant at the fractions w, from the same eight corners e[x + 2 y + 4 z], per
// voxel: THE SDF TRACKING RULE's rule 6 (K29, sdf_track_rule.h: only its direction is used) and THE QUERY RULE's
// gradient (K31, esdf_rule.h: divided by the voxel)
ICPK_HD void sdf_gradient(const float e[8], const float w[3], float g[3]) {
  const float c00 = tsdf_lerp(e[0], e[1], w[0]), c10 = tsdf_lerp(e[2], e[3], w[0]);
  const float c01 = tsdf_lerp(e[4], e[5], w[0]), c11 = tsdf_lerp(e[6], e[7], w[0]);
  const float b0 = tsdf_lerp(c00, c10, w[1]), b1 = tsdf_lerp(c01, c11, w[1]);
  const float dx00 = e[1] - e[0], dx10 = e[3] - e[2], dx01 = e[5] - e[4], dx11 = e[7] - e[6];
  g[0] = tsdf_lerp(tsdf_lerp(dx00, dx10, w[1]), tsdf_lerp(dx01, dx11, w[1]), w[2]);
  g[1] = tsdf_lerp(c10 - c00, c11 - c01, w[2]);
  g[2] = b1 - b0;
}

// the cell of rule 5: its lowest corner, that corner's linear index and the three fractions
struct TsdfCell {
  int c[3];
  long long at;
  float w[3];
};

// rule 5's range test; no index is formed before it has passed on all three axes
ICPK_HD bool tsdf_cell(const TsdfPlanes& v, const float p[3], TsdfCell* cell) {
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g[a] = (p[a] - v.origin[a]) / v.voxel - 0.5f;
    if (!(g[a] >= 0.f && g[a] < (float)(v.dims[a] - 1))) return false;  // (false for NaN; never true for a dim of 1)
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cell->c[a] = (int)g[a];  // (0 <= g < dims - 1: the conversion truncates to the floor, and c + 1 is in bounds)
    cell->w[a] = g[a] - (float)cell->c[a];
  }
  cell->at = cell->c[0] + (long long)v.dims[0] * (cell->c[1] + (long long)v.dims[1] * cell->c[2]);
  return true;
}

// the linear index of corner e (x + 2 y + 4 z) of a cell
ICPK_HD long long tsdf_corner(const TsdfPlanes& v, const TsdfCell& cell, int e) {
  return cell.at + (e & 1) + (long long)v.dims[0] * (((e >> 1) & 1) + (long long)v.dims[1] * (e >> 2));
}

// whether all eight corners have weight >= min_weight
ICPK_HD bool tsdf_cell_known(const TsdfPlanes& v, const TsdfCell& cell) {
  bool known = true;
#pragma unroll
  for (int e = 0; e < 8; ++e) known = known && (int)v.weight[tsdf_corner(v, cell, e)] >= v.min_weight;
  return known;
}

// SAMPLE(p): false when p is out of range or its cell is not known
ICPK_HD bool tsdf_sample_point(const TsdfPlanes& v, const float p[3], float* f) {
  TsdfCell cell;
  if (!tsdf_cell(v, p, &cell) || !tsdf_cell_known(v, cell)) return false;
  float e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = v.tsdf[tsdf_corner(v, cell, k)];
  *f = tsdf_trilerp(e, cell.w);
  return true;
}

// rule 8 at p: the normal, and the intensity; false when the crossing is not to be listed
ICPK_HD bool tsdf_ray_normal(const TsdfPlanes& v, const float p[3], float n[3], float* intensity) {
  TsdfCell cell;
  if (!tsdf_cell(v, p, &cell) || !tsdf_cell_known(v, cell)) return false;
  float gx[8], gy[8], gz[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c[3] = {cell.c[0] + (e & 1), cell.c[1] + ((e >> 1) & 1), cell.c[2] + (e >> 2)};
    float g[3];
    if (!tsdf_gradient(v, c, tsdf_corner(v, cell, e), g)) return false;
    gx[e] = g[0], gy[e] = g[1], gz[e] = g[2];
  }
  const float m[3] = {tsdf_trilerp(gx, cell.w), tsdf_trilerp(gy, cell.w), tsdf_trilerp(gz, cell.w)};
  const float len = __builtin_sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  if (!(len > 0.f)) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) n[a] = m[a] / len;
  *intensity = 0.f;
  if (v.intensity) {
    float e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = v.intensity[tsdf_corner(v, cell, k)];
    *intensity = tsdf_trilerp(e, cell.w);
  }
  return true;
}

// Rules 1 - 8 for pixel (row, col).  out: x, y, z, nx, ny, nz, depth, intensity -- all 0 unless TSDF_RAY_HIT comes back
ICPK_HD int tsdf_raycast_pixel(const TsdfPlanes& v, const TsdfRay& r, int row, int col, float out[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = 0.f;
  const float a = ((float)col - r.cx) / r.fx, b = ((float)row - r.cx) / r.fx;
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = (r.R[3 * k] * a + r.R[3 * k + 1] * b) + r.R[3 * k + 2];
  bool have_prev = false;
  float f_prev = 0.f, z_prev = 0.f;
  for (int n = 0; n < r.nsamples; ++n) {
    const float z = (float)n * r.step + r.z_near;
    const float p[3] = {r.c[0] + z * d[0], r.c[1] + z * d[1], r.c[2] + z * d[2]};
    float f;
    if (!tsdf_sample_point(v, p, &f)) {
      have_prev = false;
      continue;
    }
    if (have_prev) {
      if (f_prev < 0.f) {
        if (!(f < 0.f)) return TSDF_RAY_BACK_FACE;
      } else if (f < 0.f) {
        const float t = f_prev / (f_prev - f);
        const float zs = z_prev + t * (z - z_prev);
        const float ps[3] = {r.c[0] + zs * d[0], r.c[1] + zs * d[1], r.c[2] + zs * d[2]};
        float nrm[3], inten;
        if (!tsdf_ray_normal(v, ps, nrm, &inten)) return TSDF_RAY_NO_NORMAL;
        out[0] = ps[0], out[1] = ps[1], out[2] = ps[2];
        out[3] = nrm[0], out[4] = nrm[1], out[5] = nrm[2];
        out[6] = zs, out[7] = inten;
        return TSDF_RAY_HIT;
      }
    }
    have_prev = true, f_prev = f, z_prev = z;
  }
  return TSDF_RAY_NONE;
}

// ---- the mesh rule (K21) ----
// Marching tetrahedra over the Kuhn split of a cell.  Corners and edge types are masks e = x + 2 y + 4 z (K20's corner
// order); the edge (V, m) joins voxel V to V + m and is owned by V.

// the distance of V + e from V in linear index
ICPK_HD long long tsdf_mask_offset(const TsdfPlanes& v, int e) {
  return (e & 1) + (long long)v.dims[0] * (((e >> 1) & 1) + (long long)v.dims[1] * (e >> 2));
}

// whether the cell with lower corner cc is in range and known; no index is formed before the range test has passed
ICPK_HD bool tsdf_cell_known_at(const TsdfPlanes& v, const int cc[3]) {
  for (int a = 0; a < 3; ++a)
    if (cc[a] < 0 || cc[a] + 1 >= v.dims[a]) return false;
  TsdfCell cell;
  cell.c[0] = cc[0], cell.c[1] = cc[1], cell.c[2] = cc[2];
  cell.at = cc[0] + (long long)v.dims[0] * (cc[1] + (long long)v.dims[1] * cc[2]);
  return tsdf_cell_known(v, cell);
}

// rule 2: the four corners of tetrahedron `tet` (0 .. 5: xyz, xzy, yxz, yzx, zxy, zyx) and whether it is odd
ICPK_HD void tsdf_tet_corners(int tet, int vc[4]) {
  vc[0] = 0, vc[1] = (0x442211 >> (4 * tet)) & 7, vc[2] = (0x656353 >> (4 * tet)) & 7, vc[3] = 7;
}
ICPK_HD bool tsdf_tet_odd(int tet) { return (0x26 >> tet) & 1; }

// the case of a tetrahedron (rule 4) from the cell's sign mask (bit e: corner e is negative)
ICPK_HD int tsdf_tet_case(int signs, const int vc[4]) {
  return (signs & 1) | (((signs >> vc[1]) & 1) << 1) | (((signs >> vc[2]) & 1) << 2) | (((signs >> 7) & 1) << 3);
}

ICPK_HD int tsdf_case_triangles(int cs) {
  const int inside = (cs & 1) + ((cs >> 1) & 1) + ((cs >> 2) & 1) + (cs >> 3);
  return inside == 2 ? 2 : inside == 0 || inside == 4 ? 0 : 1;
}

// rule 4's table for an even tetrahedron: six nibbles, the vertices of the first triangle and then of the second, each
// the edge between two positions: 0 = 01, 1 = 02, 2 = 03, 3 = 12, 4 = 13, 5 = 23
ICPK_HD unsigned tsdf_case_table(int cs) {
  switch (cs) {
    case 1: return 0x210u;      // (01,02,03)
    case 2: return 0x340u;      // (10,13,12)
    case 3: return 0x341421u;   // (02,03,13) (02,13,12)
    case 4: return 0x531u;      // (20,21,23)
    case 5: return 0x530250u;   // (01,23,03) (01,21,23)
    case 6: return 0x150540u;   // (10,13,23) (10,23,20)
    case 7: return 0x542u;      // (30,31,32)
    case 8: return 0x452u;      // (30,32,31)
    case 9: return 0x450510u;   // (01,02,32) (01,32,31)
    case 10: return 0x520350u;  // (10,32,12) (10,30,32)
    case 11: return 0x351u;     // (20,23,21)
    case 12: return 0x241431u;  // (20,21,31) (20,31,30)
    case 13: return 0x430u;     // (10,12,13)
    case 14: return 0x120u;     // (01,03,02)
    default: return 0u;
  }
}

// vertex k (0 .. 2) of triangle `tri` of a tetrahedron with corners vc and table entry `code`: the corner that owns
// its edge and the edge type.  An odd tetrahedron swaps the second and the third vertex
ICPK_HD void tsdf_triangle_edge(const int vc[4], bool odd, unsigned code, int tri, int k, int* corner, int* m) {
  const int kk = odd && k > 0 ? 3 - k : k;
  const int id = (int)(code >> (4 * (3 * tri + kk))) & 7;
  const int p = (0x940 >> (2 * id)) & 3, q = (0xfb9 >> (2 * id)) & 3;  // (p < q: vc[p] is a subset of vc[q])
  *corner = vc[p];
  *m = vc[q] ^ vc[p];
}

// what voxel V contributes: as the owner of seven edges and as the lower corner of a cell
struct TsdfMeshVoxel {
  int vertices;   // bit m - 1: the vertex on edge (V, m) is listed
  int triangles;  // of cell V: 0 .. 12
  int signs;      // of cell V, where triangles > 0: bit e = corner e is negative
};

// Rules 1 - 4 for voxel V = (c[0], c[1], c[2]) with linear index `at`.  The cheap test comes first: no crossing on the
// seven edges V owns means no vertex of V's and no triangle of cell V's.  with_vertices false: only triangles and signs
ICPK_HD void tsdf_mesh_voxel(const TsdfPlanes& v, const int c[3], long long at, bool with_vertices, TsdfMeshVoxel* o) {
  o->vertices = o->triangles = o->signs = 0;
  const bool up[3] = {c[0] + 1 < v.dims[0], c[1] + 1 < v.dims[1], c[2] + 1 < v.dims[2]};
  int inr = 0, neg = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (((e & 1) && !up[0]) || ((e & 2) && !up[1]) || ((e & 4) && !up[2])) continue;
    inr |= 1 << e;
    neg |= (int)(v.tsdf[at + tsdf_mask_offset(v, e)] < 0.f) << e;  // (V + e is in range)
  }
  const int cross = ((neg & 1) ? ~neg : neg) & inr & 0xfe;  // bit m: (f_V < 0) != (f_{V + m} < 0)
  if (!cross) return;  // (nearly every voxel ends here, with the distances read and no weight)
  bool self = inr == 0xff;  // cell V is in range ...
  if (self) {
    TsdfCell cell;
    cell.c[0] = c[0], cell.c[1] = c[1], cell.c[2] = c[2], cell.at = at;
    self = tsdf_cell_known(v, cell);  // ... and known
  }
  if (self) {
    o->signs = neg;
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
      int vc[4];
      tsdf_tet_corners(tet, vc);
      o->triangles += tsdf_case_triangles(tsdf_tet_case(neg, vc));
    }
  }
  if (!with_vertices) return;
  for (int m = 1; m < 8; ++m) {
    if (!((cross >> m) & 1)) continue;
    bool listed = self;
    for (int u = 1; u < 8 && !listed; ++u) {
      if (u & m) continue;
      const int cc[3] = {c[0] - (u & 1), c[1] - ((u >> 1) & 1), c[2] - (u >> 2)};
      listed = tsdf_cell_known_at(v, cc);
    }
    if (listed) o->vertices |= 1 << (m - 1);
  }
}

struct TsdfMeshVertex {
  float p[3], n[3], intensity;
};

// rule 3 for the listed vertex on edge (V, m): false when it has no normal (out->n is then 0).  out may be null
ICPK_HD bool tsdf_mesh_vertex(const TsdfPlanes& v, const int c[3], long long at, int m, TsdfMeshVertex* out) {
  const long long nb = at + tsdf_mask_offset(v, m);
  const float fv = v.tsdf[at], fn = v.tsdf[nb];
  const float t = fv / (fv - fn);
  if (out) {
    const float step = t * v.voxel;
    for (int a = 0; a < 3; ++a) {
      out->p[a] = tsdf_centre(c[a], v.voxel, v.origin[a]);
      if ((m >> a) & 1) out->p[a] = out->p[a] + step;
      out->n[a] = 0.f;
    }
    out->intensity = v.intensity ? v.intensity[at] + t * (v.intensity[nb] - v.intensity[at]) : 0.f;
  }
  const int cn[3] = {c[0] + (m & 1), c[1] + ((m >> 1) & 1), c[2] + (m >> 2)};
  float gv[3], gn[3], n[3];
  if (!tsdf_gradient(v, c, at, gv) || !tsdf_gradient(v, cn, nb, gn)) return false;
  for (int a = 0; a < 3; ++a) n[a] = gv[a] + t * (gn[a] - gv[a]);
  const float len = __builtin_sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(len > 0.f)) return false;
  if (out)
    for (int a = 0; a < 3; ++a) out->n[a] = n[a] / len;
  return true;
}

}  // namespace icpk
