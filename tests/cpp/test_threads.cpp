// tests/cpp/test_threads.cpp -- one icp::Engine + icp::Tracker per std::thread (icp_align.hpp: "one Engine per host
// thread"), all threads started together, against the same sequences tracked one after the other; the Python test
// (tests/test_gpu_threads_cpp.py) compares the two passes byte for byte and both with SequenceRunner through the binding.
//
//   test_threads <in.bin> <out.bin>
// in : int32 S, F, rows, cols;  uint16 depth[S][F][rows*cols];  per sequence: int32 ns, nt; float source[3][ns] (x, y, z
//      planes); float target[3][nt]  -- the clouds of icp::align
// out: two passes (serial, then threaded), each: per sequence s: int32 status, iterations; float T[16] of icp::align on
//      the sequence's engine, then per frame pair i = 1..F-1: int32 status, iterations; float T[16]; then float camR[9],
//      camP[3].  Odd sequences track with voxelLeaf = 0.03 and outlierFilter = true.
//      Then per thread of the threaded pass: double start, end of its tracking loop (seconds on one steady clock).  The
//      threads wait for each other twice: before they create their engines and before they start to track.
// Exit status: 0, or non-zero after any negative icpk status (the failing call on stderr).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <thread>
#include <vector>

#include "icp_align.hpp"

namespace {

struct Sequence {
  std::vector<std::vector<uint16_t>> frames;
  std::vector<float> src, tgt;  // 3 planes each
  int32_t ns = 0, nt = 0;
};

struct Record {
  int32_t status, iterations;
  float T[16];
};

struct Result {
  std::vector<Record> recs;  // icp::align, then one per frame pair
  float camR[9], camP[3];
  int failed = 0;  // the first negative status
  double t0 = 0, t1 = 0;  // the tracking loop
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// every thread counts down, then waits for the others (a thread that has failed counts down too)
void rendezvous(std::atomic<int>* waiting) {
  if (!waiting) return;
  waiting->fetch_sub(1);
  while (waiting->load() > 0) std::this_thread::yield();
}

// a thread that leaves before the meeting point must not keep the others waiting
struct Meeting {
  std::atomic<int>* waiting;
  bool met = false;
  void meet() {
    met = true;
    rendezvous(waiting);
  }
  ~Meeting() {
    if (!met) rendezvous(waiting);
  }
};

int rows = 0, cols = 0;

void track(const Sequence& seq, int s, Result* out, std::atomic<int>* waiting) {
  Meeting meeting{waiting};
  try {
    icp::Engine eng(0);
    icp::AlignResult ar;
    const icp::CloudView src{seq.src.data(), seq.src.data() + seq.ns, seq.src.data() + 2 * (size_t)seq.ns, seq.ns};
    const icp::CloudView tgt{seq.tgt.data(), seq.tgt.data() + seq.nt, seq.tgt.data() + 2 * (size_t)seq.nt, seq.nt};
    int rc = icp::align(eng, src, tgt, icp::AlignParams(), &ar);
    if (rc < 0) {
      std::fprintf(stderr, "sequence %d: icp::align failed: %d %s\n", s, rc, eng.last_error());
      out->failed = rc;
      return;
    }
    Record r{rc, ar.stats.iterations, {}};
    std::memcpy(r.T, ar.T, sizeof(r.T));
    out->recs.push_back(r);
    icp::Tracker trk(eng);
    if (s % 2) {
      trk.voxelLeaf = 0.03f;
      trk.outlierFilter = true;
    }
    meeting.meet();
    out->t0 = now();
    for (size_t i = 1; i < seq.frames.size(); ++i) {
      rc = trk.getTransformation(seq.frames[i].data(), i == 1 ? seq.frames[0].data() : nullptr, rows, cols, 16, 1e-4f, r.T);
      if (rc < 0) {
        std::fprintf(stderr, "sequence %d frame %zu: getTransformation failed: %d %s\n", s, i, rc, eng.last_error());
        out->failed = rc;
        return;
      }
      r.status = rc;
      r.iterations = trk.lastStats.iterations;
      out->recs.push_back(r);
    }
    out->t1 = now();
    std::memcpy(out->camR, trk.cameraRotation, sizeof(out->camR));
    std::memcpy(out->camP, trk.cameraPosition, sizeof(out->camP));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sequence %d: %s\n", s, e.what());
    out->failed = -100;
  }
}

bool read_exact(FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  int32_t head[4];
  if (!f || !read_exact(f, head, sizeof(head))) return 3;
  const int S = head[0], F = head[1];
  rows = head[2];
  cols = head[3];
  if (S < 1 || S > 16 || F < 2 || rows <= 0 || cols <= 0) return 3;
  std::vector<Sequence> seqs((size_t)S);
  for (auto& q : seqs) {
    q.frames.assign((size_t)F, std::vector<uint16_t>((size_t)rows * cols));
    for (auto& fr : q.frames)
      if (!read_exact(f, fr.data(), fr.size() * 2)) return 4;
  }
  for (auto& q : seqs) {
    int32_t n[2];
    if (!read_exact(f, n, sizeof(n)) || n[0] < 0 || n[1] < 0) return 4;
    q.ns = n[0];
    q.nt = n[1];
    q.src.resize(3 * (size_t)q.ns);
    q.tgt.resize(3 * (size_t)q.nt);
    if (!read_exact(f, q.src.data(), q.src.size() * 4) || !read_exact(f, q.tgt.data(), q.tgt.size() * 4)) return 4;
  }
  std::fclose(f);

  std::vector<Result> serial((size_t)S), threaded((size_t)S);
  for (int s = 0; s < S; ++s) {
    track(seqs[(size_t)s], s, &serial[(size_t)s], nullptr);
    if (serial[(size_t)s].failed) return 6;
  }
  std::atomic<int> waiting(S), engines(S);  // the count-downs every thread starts, and starts to track, behind
  std::vector<std::thread> threads;
  for (int s = 0; s < S; ++s)
    threads.emplace_back([&, s] {
      rendezvous(&waiting);
      track(seqs[(size_t)s], s, &threaded[(size_t)s], &engines);
    });
  for (auto& t : threads) t.join();
  for (const auto& r : threaded)
    if (r.failed) return 7;

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  for (const auto* pass : {&serial, &threaded})
    for (const auto& r : *pass) {
      for (const auto& rec : r.recs) {
        const int32_t h[2] = {rec.status, rec.iterations};
        std::fwrite(h, 4, 2, o);
        std::fwrite(rec.T, 4, 16, o);
      }
      std::fwrite(r.camR, 4, 9, o);
      std::fwrite(r.camP, 4, 3, o);
    }
  for (const auto& r : threaded) {
    const double t[2] = {r.t0, r.t1};
    std::fwrite(t, 8, 2, o);
  }
  std::fclose(o);
  return 0;
}
