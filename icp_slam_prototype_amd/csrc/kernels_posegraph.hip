// kernels_posegraph.hip -- K18: pose-graph optimisation (include/icpk.h, "pose-graph optimisation"; host side:
// icpk_posegraph.cpp).  Float64 throughout.  One thread per edge in the edge pass, one thread per node everywhere
// else; a node walks its incident edges in ascending edge index (the adjacency list the host built), so every sum
// over edges has one order and there is no atomic anywhere.  Every sum over nodes or edges that ends in a scalar goes
// through the canonical tree (pair_reduce.h): per-block partials, then the 256 slots summed by every block that needs
// the scalar -- the consumer of a dot product is a launch of its own, never a wait inside one.
#include <hip/hip_runtime.h>

#include "icpk_internal.h"
#include "pair_reduce.h"

namespace icpk {
namespace {

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// the workgroup's maximum, in every thread (max is exact: no order to keep)
__device__ __forceinline__ double block_max(double v) {
  __shared__ double wm[RED_THREADS / 64];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  __syncthreads();  // (a second call: the first one's reads are over)
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
}

// slot b of `partial` = the value of block b, +0.0 beyond nblocks: stage 2 of the canonical tree, in every block
__device__ __forceinline__ double slot(const double* __restrict__ partial, int which, int nblocks) {
  return (int)threadIdx.x < nblocks ? partial[which * RED_MAX_BLOCKS + threadIdx.x] : 0.0;
}

// ---- the rule's pieces -------------------------------------------------------------------------------------------
// No libm: the device's sin, cos and atan2 are another library's than a host's, and the rule (include/icpk.h) is to give
// the same bytes wherever it is evaluated.  Everything below is +, -, *, / and sqrt in a fixed order.
// a = sin(th) / th and b = (1 - cos(th)) / th^2 from t2 = th^2: their power series in nested form, 20 terms
__device__ __forceinline__ void rod_coeffs(double t2, double& a, double& b) {
  double pa = 1.0, pb = 1.0;
  for (int k = 20; k >= 1; --k) {
    pa = 1.0 - (t2 / (double)((2 * k) * (2 * k + 1))) * pa;
    pb = 1.0 - (t2 / (double)((2 * k + 1) * (2 * k + 2))) * pb;
  }
  a = pa, b = 0.5 * pb;
}

// atan(x), x >= 0: the reciprocal above 1, three halvings of the angle (x <- x / (1 + sqrt(1 + x^2))), 14 terms
__device__ __forceinline__ double atan_pos(double x) {
  const bool inv = x > 1.0;
  if (inv) x = 1.0 / x;
  for (int k = 0; k < 3; ++k) x = x / (1.0 + sqrt(1.0 + x * x));
  const double x2 = x * x;
  double p = 1.0 / 27.0;
  for (int k = 12; k >= 0; --k) p = 1.0 / (double)(2 * k + 1) - x2 * p;
  const double r = 8.0 * (x * p);
  return inv ? 1.5707963267948966 - r : r;
}

// the angle of (c, s), s > 0 or c > 0
__device__ __forceinline__ double angle_pos(double s, double c) {
  return c > 0.0 ? atan_pos(s / c) : 1.5707963267948966 + atan_pos(-c / s);
}

// rotation vector of R (row-major 3x3)
__device__ __forceinline__ void rot_log(const double* R, double* w) {
  const double v0 = (R[7] - R[5]) / 2.0, v1 = (R[2] - R[6]) / 2.0, v2 = (R[3] - R[1]) / 2.0;
  const double s = sqrt(dot3(v0, v1, v2, v0, v1, v2));
  const double c = ((R[0] + R[4]) + R[8] - 1.0) / 2.0;
  const double f = (s < 1e-8 && c > 0.0) ? 1.0 + s * s / 6.0 : s > 0.0 ? angle_pos(s, c) / s : 0.0;
  w[0] = v0 * f, w[1] = v1 * f, w[2] = v2 * f;
}

// Rodrigues(w), row-major
__device__ __forceinline__ void rot_exp(const double* w, double* R) {
  const double t2 = dot3(w[0], w[1], w[2], w[0], w[1], w[2]);
  double a, b;
  rod_coeffs(t2, a, b);
  // [w]x^2 = w w^T - |w|^2 I
  const double x = w[0], y = w[1], z = w[2];
  R[0] = 1.0 + b * (x * x - t2), R[1] = -a * z + b * (x * y), R[2] = a * y + b * (x * z);
  R[3] = a * z + b * (x * y), R[4] = 1.0 + b * (y * y - t2), R[5] = -a * x + b * (y * z);
  R[6] = -a * y + b * (x * z), R[7] = a * x + b * (y * z), R[8] = 1.0 + b * (z * z - t2);
}

// inverse left Jacobian of SO(3) at th, row-major
__device__ __forceinline__ void jl_inv(const double* th, double* J) {
  const double t2 = dot3(th[0], th[1], th[2], th[0], th[1], th[2]);
  const double t = sqrt(t2);
  double k;
  if (t < 1e-2) {
    k = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
  } else {
    double a, b;
    rod_coeffs(t2, a, b);  // sin t = a t, cos t = 1 - b t^2
    k = 1.0 / t2 - (1.0 + (1.0 - b * t2)) / (2.0 * t * (a * t));
  }
  const double x = th[0], y = th[1], z = th[2];
  J[0] = 1.0 + k * (x * x - t2), J[1] = 0.5 * z + k * (x * y), J[2] = -0.5 * y + k * (x * z);
  J[3] = -0.5 * z + k * (x * y), J[4] = 1.0 + k * (y * y - t2), J[5] = 0.5 * x + k * (y * z);
  J[6] = 0.5 * y + k * (x * z), J[7] = -0.5 * x + k * (y * z), J[8] = 1.0 + k * (z * z - t2);
}

// ---- edge pass ---------------------------------------------------------------------------------------------------
// per edge: E, r, chi2, l, the cost term, and -- with blocks -- A = J_s^T (l L) J_s, b = J_s^T (l L) r
__global__ __launch_bounds__(RED_THREADS) void pg_edge_kernel(const PgArgs a, const PgLin lin, int nblocks) {
  const int P = nblocks * RED_THREADS;
  double v[1] = {0.0};
  for (int e = blockIdx.x * RED_THREADS + (int)threadIdx.x; e < a.n_edges; e += P) {
    const PgEdge& ed = a.edges[e];
    const double* Ps = lin.poses + 16 * (size_t)ed.source;
    const double* Pt = lin.poses + 16 * (size_t)ed.target;
    const double* T = ed.T;
    // T^-1 = [R^T | -R^T t]
    double Ri[9], ti[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) Ri[3 * r + c] = T[4 * c + r];
      ti[r] = -dot3(Ri[3 * r], Ri[3 * r + 1], Ri[3 * r + 2], T[3], T[7], T[11]);
    }
    // B = P_s T^-1
    double RB[9], tB[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) RB[3 * r + c] = dot3(Ps[4 * r], Ps[4 * r + 1], Ps[4 * r + 2], Ri[c], Ri[3 + c], Ri[6 + c]);
      tB[r] = dot3(Ps[4 * r], Ps[4 * r + 1], Ps[4 * r + 2], ti[0], ti[1], ti[2]) + Ps[4 * r + 3];
    }
    // E = P_t^-1 B; Rt^T kept: it is J's lower right block
    double RtT[9], RE[9], res[6];
    const double d0 = tB[0] - Pt[3], d1 = tB[1] - Pt[7], d2 = tB[2] - Pt[11];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) RtT[3 * r + c] = Pt[4 * c + r];
#pragma unroll
      for (int c = 0; c < 3; ++c) RE[3 * r + c] = dot3(RtT[3 * r], RtT[3 * r + 1], RtT[3 * r + 2], RB[c], RB[3 + c], RB[6 + c]);
      res[3 + r] = dot3(RtT[3 * r], RtT[3 * r + 1], RtT[3 * r + 2], d0, d1, d2);
    }
    rot_log(RE, res);
    // u = L r, chi2 = r . u
    double u[6];
    double chi2 = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += ed.info[6 * i + k] * res[k];
      u[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) chi2 += res[i] * u[i];
    double l = 1.0, term = chi2;
    if (ed.uncertain && a.mu > 0.0) {
      const double qq = a.mu / (a.mu + chi2);
      l = qq * qq;
      term = l * chi2 + a.mu * ((qq - 1.0) * (qq - 1.0));
    }
    lin.chi2[e] = chi2;
    lin.l[e] = l;
    v[0] += term;
    if (lin.A) {  // (uniform)
      // J_s = [ Ja 0 ; Jb Jc ]: Ja = Jl^-1(th) Rt^T, Jb = -Rt^T [tB]x, Jc = Rt^T
      double Jl[9], J[36];
      jl_inv(res, Jl);
      const double X[9] = {0.0, -tB[2], tB[1], tB[2], 0.0, -tB[0], -tB[1], tB[0], 0.0};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          J[6 * r + c] = dot3(Jl[3 * r], Jl[3 * r + 1], Jl[3 * r + 2], RtT[c], RtT[3 + c], RtT[6 + c]);
          J[6 * r + 3 + c] = 0.0;
          J[6 * (3 + r) + c] = -dot3(RtT[3 * r], RtT[3 * r + 1], RtT[3 * r + 2], X[c], X[3 + c], X[6 + c]);
          J[6 * (3 + r) + 3 + c] = RtT[3 * r + c];
        }
      double* A = lin.A + 36 * (size_t)e;
      double* b = lin.b + 6 * (size_t)e;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double wj[6];  // (l L) J[:, j]
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) s += (l * ed.info[6 * k + m]) * J[6 * m + j];
          wj[k] = s;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) s += J[6 * k + i] * wj[k];
          A[6 * i + j] = s;
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += J[6 * k + i] * (l * u[k]);
        b[i] = s;
      }
    }
  }
  const BlockTotals<1> t = block_tree<1>(v, 0);
  if (threadIdx.x == 0) a.partial[PG_P_COST * RED_MAX_BLOCKS + blockIdx.x] = t.sum(0);
}

// ---- node pass ---------------------------------------------------------------------------------------------------
// D_i = sum A, g_i = sum +-b over the incident edges in ascending index; per block max |g| and max diag D over the
// free nodes
__global__ __launch_bounds__(RED_THREADS) void pg_node_kernel(const PgArgs a, const PgLin lin, int nblocks) {
  const int P = nblocks * RED_THREADS;
  double gmax = 0.0, hmax = 0.0;
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P) {
    double D[36], g[6];
#pragma unroll
    for (int k = 0; k < 36; ++k) D[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
    const int k1 = a.adj_start[i + 1];
    for (int k = a.adj_start[i]; k < k1; ++k) {
      const int c = a.adj[k];
      const double* A = lin.A + 36 * (size_t)(c >> 1);
      const double* b = lin.b + 6 * (size_t)(c >> 1);
#pragma unroll
      for (int m = 0; m < 36; ++m) D[m] += A[m];
      if (c & 1) {
#pragma unroll
        for (int m = 0; m < 6; ++m) g[m] -= b[m];
      } else {
#pragma unroll
        for (int m = 0; m < 6; ++m) g[m] += b[m];
      }
    }
#pragma unroll
    for (int m = 0; m < 36; ++m) lin.D[36 * (size_t)i + m] = D[m];
#pragma unroll
    for (int m = 0; m < 6; ++m) lin.g[6 * (size_t)i + m] = g[m];
    if (i != a.ref) {
#pragma unroll
      for (int m = 0; m < 6; ++m) gmax = fmax(gmax, fabs(g[m])), hmax = fmax(hmax, D[7 * m]);
    }
  }
  gmax = block_max(gmax);
  hmax = block_max(hmax);
  if (threadIdx.x == 0) {
    a.partial[PG_P_GMAX * RED_MAX_BLOCKS + blockIdx.x] = gmax;
    a.partial[PG_P_HMAX * RED_MAX_BLOCKS + blockIdx.x] = hmax;
  }
}

// one workgroup: the blocks' partials into the scalars the host reads
__global__ __launch_bounds__(RED_THREADS) void pg_finish_kernel(const PgArgs a, int nb_edges, int nb_nodes) {
  const double v[2] = {slot(a.partial, PG_P_COST, nb_edges), slot(a.partial, PG_P_PRED, nb_nodes)};
  const BlockTotals<2> t = block_tree<2>(v, 0);
  const double dmax = block_max(slot(a.partial, PG_P_DMAX, nb_nodes));
  const double gmax = block_max(slot(a.partial, PG_P_GMAX, nb_nodes));
  const double hmax = block_max(slot(a.partial, PG_P_HMAX, nb_nodes));
  if (threadIdx.x == 0) {
    a.scal->cost = t.sum(0);
    a.scal->pred = t.sum(1);
    a.scal->dmax = dmax;
    a.scal->gmax = gmax;
    a.scal->hmax = hmax;
  }
}

// ---- the linear solve --------------------------------------------------------------------------------------------
// z = (L L^T)^-1 r
__device__ __forceinline__ void chol_solve(const double* L, const double* r, double* z) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k];
    y[i] = s / L[7 * i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * z[k];
    z[i] = s / L[7 * i];
  }
}

// per node: the Cholesky factor of D + lambda diag D, and the start of PCG: x = 0, r = -g, z = M^-1 r, p = z; per
// block r . z and r . r.  The reference node: everything zero
__global__ __launch_bounds__(RED_THREADS) void pg_damp_kernel(const PgArgs a, const PgLin lin, double lambda, int nblocks) {
  const int P = nblocks * RED_THREADS;
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P) {
    double L[36], r[6], z[6];
    const double* D = lin.D + 36 * (size_t)i;
    if (i == a.ref) {
#pragma unroll
      for (int m = 0; m < 36; ++m) L[m] = (m % 7 == 0) ? 1.0 : 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) r[m] = 0.0, z[m] = 0.0;
    } else {
#pragma unroll
      for (int m = 0; m < 36; ++m) L[m] = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double s = D[7 * j] + lambda * D[7 * j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[6 * j + k] * L[6 * j + k];
        const bool ok = s > 0.0;
        const double d = ok ? sqrt(s) : 1.0;
        L[7 * j] = d;
#pragma unroll
        for (int ii = j + 1; ii < 6; ++ii) {
          double t = D[6 * ii + j];
#pragma unroll
          for (int k = 0; k < j; ++k) t -= L[6 * ii + k] * L[6 * j + k];
          L[6 * ii + j] = ok ? t / d : 0.0;
        }
      }
#pragma unroll
      for (int m = 0; m < 6; ++m) r[m] = -lin.g[6 * (size_t)i + m];
      chol_solve(L, r, z);
    }
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      a.x[6 * (size_t)i + m] = 0.0;
      a.r[6 * (size_t)i + m] = r[m];
      a.z[6 * (size_t)i + m] = z[m];
      a.p[6 * (size_t)i + m] = z[m];
      rz += r[m] * z[m];
      rr += r[m] * r[m];
    }
#pragma unroll
    for (int m = 0; m < 36; ++m) a.L[36 * (size_t)i + m] = L[m];
    v[0] += rz, v[1] += rr;
  }
  const BlockTotals<2> t = block_tree<2>(v, 0);
  if (threadIdx.x == 0) {
    a.partial[PG_P_RZ * RED_MAX_BLOCKS + blockIdx.x] = t.sum(0);
    a.partial[PG_P_RR * RED_MAX_BLOCKS + blockIdx.x] = t.sum(1);
  }
}

// one workgroup: r . z, |g|^2 and whether there is anything to solve
__global__ __launch_bounds__(RED_THREADS) void pg_pcg_begin_kernel(const PgArgs a, double pcg_tol, int nb_nodes) {
  const double v[2] = {slot(a.partial, PG_P_RZ, nb_nodes), slot(a.partial, PG_P_RR, nb_nodes)};
  const BlockTotals<2> t = block_tree<2>(v, 0);
  if (threadIdx.x == 0) {
    const double rz = t.sum(0), rr = t.sum(1);
    a.scal->rz[0] = rz;
    a.scal->gnorm2 = rr;
    a.scal->pcg_iters = 0;
    a.scal->breakdown = 0;
    // met already (g = 0, or a tolerance >= 1), or nothing to descend along
    a.scal->done[0] = sqrt(rr) <= pcg_tol * sqrt(rr) || !(rz > 0.0);
  }
}

// PCG iteration k, first launch: q = (H + lambda diag H) p as a gather per node; per block p . q
__global__ __launch_bounds__(RED_THREADS) void pg_pcg_q_kernel(const PgArgs a, const PgLin lin, double lambda, int k, int nblocks) {
  if (a.scal->done[k & 1]) return;  // (uniform)
  const int P = nblocks * RED_THREADS;
  double v[1] = {0.0};
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P) {
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, pi[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) pi[m] = a.p[6 * (size_t)i + m];
    if (i != a.ref) {
      const int k1 = a.adj_start[i + 1];
      for (int kk = a.adj_start[i]; kk < k1; ++kk) {
        const int c = a.adj[kk];
        const int e = c >> 1;
        const int o = (c & 1) ? a.edges[e].source : a.edges[e].target;
        const double* A = lin.A + 36 * (size_t)e;
        double d[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) d[m] = pi[m] - a.p[6 * (size_t)o + m];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double s = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) s += A[6 * r + m] * d[m];
          q[r] += s;
        }
      }
#pragma unroll
      for (int m = 0; m < 6; ++m) q[m] += (lambda * lin.D[36 * (size_t)i + 7 * m]) * pi[m];
    }
    double pq = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      a.q[6 * (size_t)i + m] = q[m];
      pq += pi[m] * q[m];
    }
    v[0] += pq;
  }
  const BlockTotals<1> t = block_tree<1>(v, 0);
  if (threadIdx.x == 0) a.partial[PG_P_PQ * RED_MAX_BLOCKS + blockIdx.x] = t.sum(0);
}

// second launch: alpha = r . z / p . q (every block sums the slots), x += alpha p, r -= alpha q, z = M^-1 r; per block
// r . z and r . r
__global__ __launch_bounds__(RED_THREADS) void pg_pcg_update_kernel(const PgArgs a, int k, int nblocks) {
  if (a.scal->done[k & 1]) return;  // (uniform)
  const double s1[1] = {slot(a.partial, PG_P_PQ, nblocks)};
  const BlockTotals<1> t1 = block_tree<1>(s1, 0);
  const double pq = t1.sum(0);
  const bool ok = pq > 0.0;
  const double alpha = ok ? a.scal->rz[k & 1] / pq : 0.0;
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0) a.scal->breakdown = 1;
  const int P = nblocks * RED_THREADS;
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P) {
    double r[6], z[6], L[36];
#pragma unroll
    for (int m = 0; m < 36; ++m) L[m] = a.L[36 * (size_t)i + m];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      a.x[6 * (size_t)i + m] += alpha * a.p[6 * (size_t)i + m];
      r[m] = a.r[6 * (size_t)i + m] - alpha * a.q[6 * (size_t)i + m];
      a.r[6 * (size_t)i + m] = r[m];
    }
    chol_solve(L, r, z);
    double rz = 0.0, rr = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      a.z[6 * (size_t)i + m] = z[m];
      rz += r[m] * z[m];
      rr += r[m] * r[m];
    }
    v[0] += rz, v[1] += rr;
  }
  const BlockTotals<2> t = block_tree<2>(v, 0);
  if (threadIdx.x == 0) {
    a.partial[PG_P_RZ * RED_MAX_BLOCKS + blockIdx.x] = t.sum(0);
    a.partial[PG_P_RR * RED_MAX_BLOCKS + blockIdx.x] = t.sum(1);
  }
}

// third launch: beta, p = z + beta p, and the words of iteration k + 1
__global__ __launch_bounds__(RED_THREADS) void pg_pcg_dir_kernel(const PgArgs a, double pcg_tol, int k, int nblocks) {
  if (a.scal->done[k & 1]) {  // (uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) a.scal->done[(k + 1) & 1] = 1;
    return;
  }
  const double s2[2] = {slot(a.partial, PG_P_RZ, nblocks), slot(a.partial, PG_P_RR, nblocks)};
  const BlockTotals<2> t = block_tree<2>(s2, 0);
  const double rzn = t.sum(0), rr = t.sum(1);
  const double beta = rzn / a.scal->rz[k & 1];
  const int P = nblocks * RED_THREADS;
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P)
#pragma unroll
    for (int m = 0; m < 6; ++m) a.p[6 * (size_t)i + m] = a.z[6 * (size_t)i + m] + beta * a.p[6 * (size_t)i + m];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.scal->rz[(k + 1) & 1] = rzn;
    a.scal->pcg_iters = k + 1;
    a.scal->done[(k + 1) & 1] = sqrt(rr) <= pcg_tol * sqrt(a.scal->gnorm2) || a.scal->breakdown || !(rzn > 0.0);
  }
}

// ---- trial update ------------------------------------------------------------------------------------------------
// trial_i = Exp(x_i) P_i (the reference node: its bytes); per block the predicted decrease and max |x|
__global__ __launch_bounds__(RED_THREADS) void pg_trial_kernel(const PgArgs a, const PgLin lin, double lambda, double* __restrict__ trial,
                                                               int nblocks) {
  const int P = nblocks * RED_THREADS;
  double v[1] = {0.0};
  double dmax = 0.0;
  for (int i = blockIdx.x * RED_THREADS + (int)threadIdx.x; i < a.n_nodes; i += P) {
    const double* Pi = lin.poses + 16 * (size_t)i;
    double* Po = trial + 16 * (size_t)i;
    if (i == a.ref) {
#pragma unroll
      for (int m = 0; m < 16; ++m) Po[m] = Pi[m];
      continue;
    }
    double d[6], R[9];
    double pred = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      d[m] = a.x[6 * (size_t)i + m];
      pred += d[m] * ((lambda * lin.D[36 * (size_t)i + 7 * m]) * d[m] - lin.g[6 * (size_t)i + m]);
      dmax = fmax(dmax, fabs(d[m]));
    }
    v[0] += pred;
    rot_exp(d, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) Po[4 * r + c] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], Pi[c], Pi[4 + c], Pi[8 + c]);
      Po[4 * r + 3] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], Pi[3], Pi[7], Pi[11]) + d[3 + r];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) Po[12 + c] = Pi[12 + c];
  }
  const BlockTotals<1> t = block_tree<1>(v, 0);
  dmax = block_max(dmax);
  if (threadIdx.x == 0) {
    a.partial[PG_P_PRED * RED_MAX_BLOCKS + blockIdx.x] = t.sum(0);
    a.partial[PG_P_DMAX * RED_MAX_BLOCKS + blockIdx.x] = dmax;
  }
}

}  // namespace

void launch_pg_linearise(const PgArgs& a, const PgLin& lin, bool with_finish, hipStream_t s) {
  const int nbe = red_blocks(a.n_edges), nbn = red_blocks(a.n_nodes);
  hipLaunchKernelGGL(pg_edge_kernel, dim3(nbe), dim3(RED_THREADS), 0, s, a, lin, nbe);
  if (lin.A) hipLaunchKernelGGL(pg_node_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, lin, nbn);
  if (with_finish) hipLaunchKernelGGL(pg_finish_kernel, dim3(1), dim3(RED_THREADS), 0, s, a, nbe, nbn);
}

void launch_pg_solve(const PgArgs& a, const PgLin& lin, double lambda, double pcg_tol, int max_pcg, double* trial,
                     hipStream_t s) {
  const int nbn = red_blocks(a.n_nodes);
  hipLaunchKernelGGL(pg_damp_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, lin, lambda, nbn);
  hipLaunchKernelGGL(pg_pcg_begin_kernel, dim3(1), dim3(RED_THREADS), 0, s, a, pcg_tol, nbn);
  for (int k = 0; k < max_pcg; ++k) {
    hipLaunchKernelGGL(pg_pcg_q_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, lin, lambda, k, nbn);
    hipLaunchKernelGGL(pg_pcg_update_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, k, nbn);
    hipLaunchKernelGGL(pg_pcg_dir_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, pcg_tol, k, nbn);
  }
  hipLaunchKernelGGL(pg_trial_kernel, dim3(nbn), dim3(RED_THREADS), 0, s, a, lin, lambda, trial, nbn);
}

}  // namespace icpk
