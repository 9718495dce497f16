// tests/cpp/solve_probe.hip -- TEST INFRASTRUCTURE ONLY: runs the dense algebra of csrc/solve_impl.h
// (polar3, svd3, solve_reference, solve_kabsch, solve_p2l, invert3f, mul3f) and the scalar operations it
// relies on (sqrt and / in float64 and float32) over arrays of cases, either on the device (one thread per
// case, plain global loads and stores) or on the host, from the same source and with the same compiler
// flags as libicpk.so.  Loaded by tests/test_gpu_solve_device.py and tests/test_solve_probe_host.py only;
// never shipped, never used by bench.py.
//
// Every entry point is  int probe_<op>(int on_device, int n, <inputs>, <outputs>)  over host arrays of n
// cases: 0 on success, the hipError_t of the first failing HIP call otherwise.  This file includes
// solve_impl.h on its own, first: it is the check that the header stands alone in a HIP translation unit.
#include "solve_impl.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int BLOCK = 256;

// device copies of the host arrays of one call, freed on every exit path
struct Dev {
  void* p[8] = {};
  int n = 0;
  hipError_t err = hipSuccess;
  template <class T>
  T* in(const T* h, size_t count) {
    T* d = alloc<T>(count);
    if (d && err == hipSuccess) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* alloc(size_t count) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, count * sizeof(T) + 1);  // +1: n == 0 still gets a valid pointer
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    return static_cast<T*>(d);
  }
  template <class T>
  void out(T* h, const T* d, size_t count) {
    if (err == hipSuccess) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  int launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return (int)err;
  }
  ~Dev() {
    for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
  }
};

unsigned blocks(int n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// ---- one case of each operation (host and device) -------------------------------------------
__host__ __device__ inline void one_polar3(int i, const double* A, int* ok, double* Q) {
  ok[i] = icpk::polar3(A + 9 * i, Q + 9 * i) ? 1 : 0;
}

__host__ __device__ inline void one_svd3(int i, const double* A, double* U, double* S, double* V) {
  icpk::Mat3 a, u, v;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) a.m[r][c] = A[9 * i + 3 * r + c];
  icpk::svd3(a, u, S + 3 * i, v);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      U[9 * i + 3 * r + c] = u.m[r][c];
      V[9 * i + 3 * r + c] = v.m[r][c];
    }
}

__host__ __device__ inline void one_reference(int i, const float* M, float* R) {
  icpk::solve_reference(M + 9 * i, R + 9 * i);
}

__host__ __device__ inline void one_kabsch(int i, const int64_t* cnt, const double* sa, const double* sb, const double* sab,
                                           double* R, double* t) {
  icpk::solve_kabsch(cnt[i], sa + 3 * i, sb + 3 * i, sab + 9 * i, R + 9 * i, t + 3 * i);
}

__host__ __device__ inline void one_p2l(int i, const double* sums, int* ok, double* R, double* t) {
  ok[i] = icpk::solve_p2l(sums + 28 * i, R + 9 * i, t + 3 * i) ? 1 : 0;
}

__host__ __device__ inline void one_invert3f(int i, const float* Rin, int* ok, float* out) {
  ok[i] = icpk::invert3f(Rin + 9 * i, out + 9 * i) ? 1 : 0;
}

__host__ __device__ inline void one_mul3f(int i, const float* A, const float* B, float* C) {
  icpk::mul3f(A + 9 * i, B + 9 * i, C + 9 * i);
}

// the scalar operations solve_impl.h takes to be correctly rounded on both sides
__host__ __device__ inline void one_sqrt_f64(int i, const double* a, double* o) { o[i] = std::sqrt(a[i]); }
__host__ __device__ inline void one_div_f64(int i, const double* a, const double* b, double* o) { o[i] = a[i] / b[i]; }
__host__ __device__ inline void one_sqrt_f32(int i, const float* a, float* o) { o[i] = std::sqrt(a[i]); }
__host__ __device__ inline void one_div_f32(int i, const float* a, const float* b, float* o) { o[i] = a[i] / b[i]; }

__global__ void k_polar3(int n, const double* A, int* ok, double* Q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_polar3(i, A, ok, Q);
}
__global__ void k_svd3(int n, const double* A, double* U, double* S, double* V) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_svd3(i, A, U, S, V);
}
__global__ void k_reference(int n, const float* M, float* R) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_reference(i, M, R);
}
__global__ void k_kabsch(int n, const int64_t* cnt, const double* sa, const double* sb, const double* sab, double* R,
                         double* t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_kabsch(i, cnt, sa, sb, sab, R, t);
}
__global__ void k_p2l(int n, const double* sums, int* ok, double* R, double* t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_p2l(i, sums, ok, R, t);
}
__global__ void k_invert3f(int n, const float* Rin, int* ok, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_invert3f(i, Rin, ok, out);
}
__global__ void k_mul3f(int n, const float* A, const float* B, float* C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_mul3f(i, A, B, C);
}
__global__ void k_sqrt_f64(int n, const double* a, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_sqrt_f64(i, a, o);
}
__global__ void k_div_f64(int n, const double* a, const double* b, double* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_div_f64(i, a, b, o);
}
__global__ void k_sqrt_f32(int n, const float* a, float* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_sqrt_f32(i, a, o);
}
__global__ void k_div_f32(int n, const float* a, const float* b, float* o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one_div_f32(i, a, b, o);
}

}  // namespace

extern "C" {

int probe_polar3(int on_device, int n, const double* A, int* ok, double* Q) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_polar3(i, A, ok, Q);
    return 0;
  }
  Dev d;
  const double* dA = d.in(A, 9 * (size_t)n);
  int* dok = d.alloc<int>(n);
  double* dQ = d.alloc<double>(9 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_polar3, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dA, dok, dQ);
  d.launched();
  d.out(ok, dok, n);
  d.out(Q, dQ, 9 * (size_t)n);
  return (int)d.err;
}

int probe_svd3(int on_device, int n, const double* A, double* U, double* S, double* V) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_svd3(i, A, U, S, V);
    return 0;
  }
  Dev d;
  const double* dA = d.in(A, 9 * (size_t)n);
  double* dU = d.alloc<double>(9 * (size_t)n);
  double* dS = d.alloc<double>(3 * (size_t)n);
  double* dV = d.alloc<double>(9 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_svd3, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dA, dU, dS, dV);
  d.launched();
  d.out(U, dU, 9 * (size_t)n);
  d.out(S, dS, 3 * (size_t)n);
  d.out(V, dV, 9 * (size_t)n);
  return (int)d.err;
}

int probe_solve_reference(int on_device, int n, const float* M, float* R) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_reference(i, M, R);
    return 0;
  }
  Dev d;
  const float* dM = d.in(M, 9 * (size_t)n);
  float* dR = d.alloc<float>(9 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_reference, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dM, dR);
  d.launched();
  d.out(R, dR, 9 * (size_t)n);
  return (int)d.err;
}

int probe_solve_kabsch(int on_device, int n, const int64_t* cnt, const double* sa, const double* sb, const double* sab,
                       double* R, double* t) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_kabsch(i, cnt, sa, sb, sab, R, t);
    return 0;
  }
  Dev d;
  const int64_t* dc = d.in(cnt, n);
  const double* dsa = d.in(sa, 3 * (size_t)n);
  const double* dsb = d.in(sb, 3 * (size_t)n);
  const double* dsab = d.in(sab, 9 * (size_t)n);
  double* dR = d.alloc<double>(9 * (size_t)n);
  double* dt = d.alloc<double>(3 * (size_t)n);
  if (d.err == hipSuccess && n)
    hipLaunchKernelGGL(k_kabsch, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dc, dsa, dsb, dsab, dR, dt);
  d.launched();
  d.out(R, dR, 9 * (size_t)n);
  d.out(t, dt, 3 * (size_t)n);
  return (int)d.err;
}

int probe_solve_p2l(int on_device, int n, const double* sums, int* ok, double* R, double* t) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_p2l(i, sums, ok, R, t);
    return 0;
  }
  Dev d;
  const double* ds = d.in(sums, 28 * (size_t)n);
  int* dok = d.alloc<int>(n);
  double* dR = d.alloc<double>(9 * (size_t)n);
  double* dt = d.alloc<double>(3 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_p2l, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, ds, dok, dR, dt);
  d.launched();
  d.out(ok, dok, n);
  d.out(R, dR, 9 * (size_t)n);
  d.out(t, dt, 3 * (size_t)n);
  return (int)d.err;
}

int probe_invert3f(int on_device, int n, const float* Rin, int* ok, float* out) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_invert3f(i, Rin, ok, out);
    return 0;
  }
  Dev d;
  const float* dR = d.in(Rin, 9 * (size_t)n);
  int* dok = d.alloc<int>(n);
  float* dout = d.alloc<float>(9 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_invert3f, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dR, dok, dout);
  d.launched();
  d.out(ok, dok, n);
  d.out(out, dout, 9 * (size_t)n);
  return (int)d.err;
}

int probe_mul3f(int on_device, int n, const float* A, const float* B, float* C) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_mul3f(i, A, B, C);
    return 0;
  }
  Dev d;
  const float* dA = d.in(A, 9 * (size_t)n);
  const float* dB = d.in(B, 9 * (size_t)n);
  float* dC = d.alloc<float>(9 * (size_t)n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_mul3f, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, dA, dB, dC);
  d.launched();
  d.out(C, dC, 9 * (size_t)n);
  return (int)d.err;
}

int probe_sqrt_f64(int on_device, int n, const double* a, double* o) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_sqrt_f64(i, a, o);
    return 0;
  }
  Dev d;
  const double* da = d.in(a, n);
  double* dout = d.alloc<double>(n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_sqrt_f64, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, da, dout);
  d.launched();
  d.out(o, dout, n);
  return (int)d.err;
}

int probe_div_f64(int on_device, int n, const double* a, const double* b, double* o) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_div_f64(i, a, b, o);
    return 0;
  }
  Dev d;
  const double* da = d.in(a, n);
  const double* db = d.in(b, n);
  double* dout = d.alloc<double>(n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_div_f64, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, da, db, dout);
  d.launched();
  d.out(o, dout, n);
  return (int)d.err;
}

int probe_sqrt_f32(int on_device, int n, const float* a, float* o) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_sqrt_f32(i, a, o);
    return 0;
  }
  Dev d;
  const float* da = d.in(a, n);
  float* dout = d.alloc<float>(n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_sqrt_f32, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, da, dout);
  d.launched();
  d.out(o, dout, n);
  return (int)d.err;
}

int probe_div_f32(int on_device, int n, const float* a, const float* b, float* o) {
  if (n < 0) return -1;
  if (!on_device) {
    for (int i = 0; i < n; ++i) one_div_f32(i, a, b, o);
    return 0;
  }
  Dev d;
  const float* da = d.in(a, n);
  const float* db = d.in(b, n);
  float* dout = d.alloc<float>(n);
  if (d.err == hipSuccess && n) hipLaunchKernelGGL(k_div_f32, dim3(blocks(n)), dim3(BLOCK), 0, 0, n, da, db, dout);
  d.launched();
  d.out(o, dout, n);
  return (int)d.err;
}

}  // extern "C"
