// kernels_normals.hip -- K12: surface normals of the target from its own geometry (icpk_estimate_target_normals; the
// rule is spelled out in include/icpk.h and restated in tests/normals_model.py).
//
//   1. normals_moments_kernel  the radius search and the moment sums, the hot path.  It walks K1d's index of the target
//                              (kernels_grid.hip: the target sorted by cell, `cell_start`): the points are taken in cell
//                              order, NRM_S adjacent lanes per point, so that the lanes of a wave read the same few rows
//                              of cells.  A point's lanes share the (y, z) rows of the cube [p - rr, p + rr] (the walk
//                              of grid_walk.h).  Each lane keeps ten integer partial sums; a butterfly over the
//                              point's lanes adds them, and the lanes store the ten words side by side.
//   2. normals_solve_kernel    one lane per point: covariance, cyclic Jacobi eigen-solve of the symmetric 3x3 in
//                              float64, the tests of the rule, orientation, curvature.  A launch of its own and not the
//                              tail of the first: there the solve would run with one lane in NRM_S active (a wave pays
//                              for 64 whatever the mask says), here every lane has a point.
// Every sum is an integer sum, so nothing depends on the order in which neighbours arrive or on how a point's rows are
// dealt to its lanes: the moments are the same bits on every run, for every order of the cloud, and the bits of the
// CPU model.
#include "grid_walk.h"
#include "icpk_internal.h"

namespace icpk {

namespace {

constexpr int NRM_S = 8;          // lanes per point (a cube of 3-5 cells per axis has 9-25 rows)
constexpr int NRM_BLOCK = 256;
constexpr int NRM_UNROLL = 4;     // candidates per lane and round trip
constexpr double NRM_FIX = 32768.0;  // F = 2^15

struct Moments {
  long long m, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz;
};

__device__ __forceinline__ void accumulate(Moments& M, float px, float py, float pz, const float4 c, bool in_range, float r,
                                           double rd, double inv_r) {
  const float d = pair_dist(px, py, pz, c.x, c.y, c.z);
  if (in_range && d <= r) {  // (NaN and inf compare false: a non-finite point is nobody's neighbour)
    const int qx = quantise((double)c.x - (double)px, rd, inv_r, NRM_FIX);
    const int qy = quantise((double)c.y - (double)py, rd, inv_r, NRM_FIX);
    const int qz = quantise((double)c.z - (double)pz, rd, inv_r, NRM_FIX);
    // |q| <= F + 1: the products fit 32 bits, the sums of fewer than 2^31 of them 64
    M.m += 1;
    M.sx += qx;
    M.sy += qy;
    M.sz += qz;
    M.sxx += (long long)(qx * qx);
    M.sxy += (long long)(qx * qy);
    M.sxz += (long long)(qx * qz);
    M.syy += (long long)(qy * qy);
    M.syz += (long long)(qy * qz);
    M.szz += (long long)(qz * qz);
  }
}

__global__ __launch_bounds__(NRM_BLOCK) void normals_moments_kernel(const NormalsArgs a) {
  const int slice = threadIdx.x & (NRM_S - 1);
  const int ip = (int)((blockIdx.x * (unsigned)NRM_BLOCK + threadIdx.x) / NRM_S);  // position in cell order
  const bool live = ip < a.n;
  const float4 p4 = live ? a.index.t4[ip] : make_float4(0.f, 0.f, 0.f, 0.f);
  const GridInfo g = *a.index.gi;
  const float px = p4.x, py = p4.y, pz = p4.z;
  const float r = a.radius;
  const double rd = (double)r, inv_r = 1.0 / rd;
  // a non-finite point has an empty neighbourhood (and its cube would be the whole grid)
  const bool scan = live && __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz);
  const Walk walk = make_walk(g, px, py, pz, r, scan);
  Moments M{};
  walk_candidates<NRM_S, NRM_UNROLL>(
      walk, g, a.index.cell_start, slice, [&](int jj) { return a.index.t4[jj]; },
      [&](const float4 c, bool in_range) { accumulate(M, px, py, pz, c, in_range, r, rd, inv_r); });
  long long w[NRM_MOMENTS] = {M.m, M.sx, M.sy, M.sz, M.sxx, M.sxy, M.sxz, M.syy, M.syz, M.szz};
#pragma unroll
  for (int k = 0; k < NRM_MOMENTS; ++k) w[k] = sum_over_point<NRM_S>(w[k]);
  if (!live) return;
  store_point_words<NRM_S>(a.moments + (size_t)__float_as_int(p4.w) * NRM_MOMENTS, slice, w);
}

// one Jacobi rotation of the symmetric 3x3 in the plane (p, q); r is the third axis.  Rutishauser's formulas: the
// smaller root t of t^2 + 2 theta t - 1 = 0, so |angle| <= pi / 4.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                              double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = __builtin_fabs(theta);
  double t = 1.0 / (at + __builtin_sqrt(theta * theta + 1.0));  // (theta^2 = inf: t = 0, the rotation is the identity)
  t = theta < 0.0 ? -t : t;
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0, v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1, v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2, v2q = s * a2 + c * b2;
}

__global__ __launch_bounds__(NRM_BLOCK) void normals_solve_kernel(const NormalsArgs a) {
  const int i = blockIdx.x * NRM_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  const long long* const M = a.moments + (size_t)i * NRM_MOMENTS;
  const long long m = M[0];
  const double md = (double)m, sx = (double)M[1], sy = (double)M[2], sz = (double)M[3];
  double a00 = (double)M[4] - sx * sx / md, a01 = (double)M[5] - sx * sy / md, a02 = (double)M[6] - sx * sz / md;
  double a11 = (double)M[7] - sy * sy / md, a12 = (double)M[8] - sy * sz / md, a22 = (double)M[9] - sz * sz / md;
  // cyclic Jacobi: columns of V are the eigenvectors.  Convergence is quadratic; the loop ends when the off-diagonal
  // part is below 2^-70 of the trace (an eigenvector error of 2^-70 l2 / (l1 - l0), far inside what the rule's users
  // can see) or has vanished, which a 3x3 reaches in 4-6 sweeps; 12 is a guard.
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = __builtin_fabs(a01) + __builtin_fabs(a02) + __builtin_fabs(a12);
    const double tr = __builtin_fabs(a00) + __builtin_fabs(a11) + __builtin_fabs(a22);
    if (!(off > 0x1p-70 * tr)) break;  // (NaN ends the loop too)
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // l0 <= l1 <= l2 and the eigenvector of l0
  double l0 = a00, l1 = a11, l2 = a22, ex = v00, ey = v10, ez = v20;
  if (l1 < l0) {
    const double t = l0;
    l0 = l1, l1 = t;
    ex = v01, ey = v11, ez = v21;
  }
  if (l2 < l0) {
    const double t = l0;
    l0 = l2, l2 = t;
    ex = v02, ey = v12, ez = v22;
  }
  if (l2 < l1) {
    const double t = l1;
    l1 = l2, l2 = t;
  }
  const double len = __builtin_sqrt(ex * ex + ey * ey + ez * ez);
  ex /= len, ey /= len, ez /= len;
  const double curv = l0 / (l0 + l1 + l2);
  bool ok = m >= (long long)a.min_neighbors && !(l1 <= 0x1p-20 * l2);
  ok = ok && __builtin_isfinite(l0) && __builtin_isfinite(l1) && __builtin_isfinite(l2) && __builtin_isfinite(ex) &&
       __builtin_isfinite(ey) && __builtin_isfinite(ez) && __builtin_isfinite(curv);
  double s = 0.0;
  if (a.has_viewpoint)
    s = ex * ((double)a.viewpoint[0] - (double)a.x[i]) + ey * ((double)a.viewpoint[1] - (double)a.y[i]) +
        ez * ((double)a.viewpoint[2] - (double)a.z[i]);
  bool flip = s < 0.0;
  if (!(s < 0.0) && !(s > 0.0)) {  // no viewpoint, s == 0 (or NaN): the component of largest magnitude is positive
    double big = ex;
    if (__builtin_fabs(ey) > __builtin_fabs(big)) big = ey;
    if (__builtin_fabs(ez) > __builtin_fabs(big)) big = ez;
    flip = big < 0.0;
  }
  if (flip) ex = -ex, ey = -ey, ez = -ez;
  a.nx[i] = ok ? (float)ex : 0.f;
  a.ny[i] = ok ? (float)ey : 0.f;
  a.nz[i] = ok ? (float)ez : 0.f;
  a.count[i] = (int)m;
  a.curvature[i] = ok ? (float)curv : 0.f;
  if (ok) atomicAdd(a.n_valid, 1);  // (an integer count: the order of arrival does not show)
}

}  // namespace

void launch_estimate_normals(const NormalsArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  const unsigned lanes_blocks = (unsigned)(((size_t)a.n * NRM_S + NRM_BLOCK - 1) / NRM_BLOCK);
  hipLaunchKernelGGL(normals_moments_kernel, dim3(lanes_blocks), dim3(NRM_BLOCK), 0, s, a);
  hipLaunchKernelGGL(normals_solve_kernel, dim3((a.n + NRM_BLOCK - 1) / NRM_BLOCK), dim3(NRM_BLOCK), 0, s, a);
}

}  // namespace icpk
