// tests/cpp/scan_probe.hip -- TEST INFRASTRUCTURE ONLY: runs the workgroup scans of csrc/block_scan.h on host arrays,
// one workgroup per call, from the same source and with the same compiler flags as libicpk.so.  Loaded by
// tests/test_gpu_scan_probe.py only; never shipped, never used by bench.py.
//
// Every entry point returns 0 on success, the hipError_t of the first failing HIP call otherwise, -1 for an argument
// it does not take.  This file includes block_scan.h on its own, first: it is the check that the header stands alone
// in a HIP translation unit.
#include "block_scan.h"

#include <hip/hip_runtime.h>

namespace {

// device copies of the host arrays of one call, freed on every exit path
struct Dev {
  void* p[8] = {};
  int n = 0;
  hipError_t err = hipSuccess;
  template <class T>
  T* alloc(size_t count) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, count * sizeof(T) + 1);  // +1: count == 0 still gets a valid pointer
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    return static_cast<T*>(d);
  }
  template <class T>
  T* in(const T* h, size_t count) {
    T* d = alloc<T>(count);
    if (d && err == hipSuccess) err = hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  void out(T* h, const T* d, size_t count) {
    if (err == hipSuccess) err = hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
  ~Dev() {
    for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
  }
};

// The contract: block_excl_scan on a, then at once on b, then block_total on a and on b, with no barrier of the
// kernel's own anywhere.  Every thread writes what it got: out[0..5][THREADS] = rank a, total a, rank b, total b,
// block_total a, block_total b.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_pair(const int* a, const int* b, int* out) {
  const int t = threadIdx.x;
  int ta, tb;
  const int ra = icpk::block_excl_scan<THREADS>(a[t], &ta);
  const int rb = icpk::block_excl_scan<THREADS>(b[t], &tb);
  const int sa = icpk::block_total<THREADS>(a[t]);
  const int sb = icpk::block_total<THREADS>(b[t]);
  out[t] = ra, out[THREADS + t] = ta, out[2 * THREADS + t] = rb, out[3 * THREADS + t] = tb;
  out[4 * THREADS + t] = sa, out[5 * THREADS + t] = sb;
}

constexpr int ROUNDS_THREADS = 256, RUNS_THREADS = 1024;

template <class Out>
__global__ __launch_bounds__(ROUNDS_THREADS) void k_rounds(const int* in, Out* out, int m, Out* totals) {
  totals[threadIdx.x] = icpk::scan_rounds<ROUNDS_THREADS>(in, out, m);
}

__global__ __launch_bounds__(RUNS_THREADS) void k_runs(int* a, int m, int* totals) {
  totals[threadIdx.x] = icpk::scan_runs<RUNS_THREADS>(a, m);
}

template <class Out>
int rounds(int m, const int* in, Out* out, Out* totals, bool in_place) {
  if (m < 0) return -1;
  Dev d;
  int* din = d.in(in, m);
  Out* dout = in_place ? reinterpret_cast<Out*>(din) : d.alloc<Out>(m);
  Out* dt = d.alloc<Out>(ROUNDS_THREADS);
  if (d.err == hipSuccess) hipLaunchKernelGGL(k_rounds<Out>, dim3(1), dim3(ROUNDS_THREADS), 0, 0, din, dout, m, dt);
  d.launched();
  d.out(out, dout, m);
  d.out(totals, dt, ROUNDS_THREADS);
  return (int)d.err;
}

}  // namespace

extern "C" {

// a, b: [threads] values; out: [6][threads] (see k_pair); threads: 256 or 1024
int probe_scan_pair(int threads, const int* a, const int* b, int* out) {
  if (threads != 256 && threads != 1024) return -1;
  Dev d;
  const int* da = d.in(a, threads);
  const int* db = d.in(b, threads);
  int* dout = d.alloc<int>(6 * (size_t)threads);
  if (d.err == hipSuccess) {
    if (threads == 256)
      hipLaunchKernelGGL(k_pair<256>, dim3(1), dim3(256), 0, 0, da, db, dout);
    else
      hipLaunchKernelGGL(k_pair<1024>, dim3(1), dim3(1024), 0, 0, da, db, dout);
  }
  d.launched();
  d.out(out, dout, 6 * (size_t)threads);
  return (int)d.err;
}

// scan_rounds<256, int> in place over a[m]; totals: [256], what every thread got back
int probe_scan_rounds_i32(int m, int* a, int* totals) { return rounds<int>(m, a, a, totals, true); }

// scan_rounds<256, long long> from in[m] to out[m]; totals: [256]
int probe_scan_rounds_i64(int m, const int* in, long long* out, long long* totals) {
  return rounds<long long>(m, in, out, totals, false);
}

// scan_runs<1024> in place over a[m]; totals: [1024]
int probe_scan_runs(int m, int* a, int* totals) {
  if (m < 0) return -1;
  Dev d;
  int* da = d.in(a, m);
  int* dt = d.alloc<int>(RUNS_THREADS);
  if (d.err == hipSuccess) hipLaunchKernelGGL(k_runs, dim3(1), dim3(RUNS_THREADS), 0, 0, da, m, dt);
  d.launched();
  d.out(a, da, m);
  d.out(totals, dt, RUNS_THREADS);
  return (int)d.err;
}

}  // extern "C"
