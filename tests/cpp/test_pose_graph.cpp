// tests/cpp/test_pose_graph.cpp -- icp::PoseGraph (icp_pose_graph.hpp) on one graph; the Python test
// (tests/test_gpu_posegraph_cpp.py) compares what it writes with the same call made through the binding, byte for byte.
//
//   test_pose_graph <in.bin> <out.bin>
// in : int32 n_nodes, n_edges, flags, 0; double mu; double poses[16 * n_nodes]; per edge int32 source, target,
//      uncertain, 0; double T[16]; double info[36]
// out: int32 status, iterations, accepted, pcg_iterations, n_pruned, 0; double initial_cost, final_cost, final_lambda;
//      double poses[16 * n_nodes]; double weights[n_edges]; double chi2[n_edges]; uint8 pruned[n_edges]
// The poses are printed as well.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_align.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[4];
  double mu;
  if (std::fread(head, 4, 4, f) != 4 || std::fread(&mu, 8, 1, f) != 1 || head[0] < 1 || head[1] < 1) return 4;
  const int n = head[0], m = head[1];
  std::vector<double> poses((size_t)16 * n);
  if (std::fread(poses.data(), 8, poses.size(), f) != poses.size()) return 4;
  icp::PoseGraph g;
  for (int i = 0; i < n; ++i) g.addNode(poses.data() + 16 * (size_t)i);
  for (int e = 0; e < m; ++e) {
    int32_t h[4];
    double T[16], info[36];
    if (std::fread(h, 4, 4, f) != 4 || std::fread(T, 8, 16, f) != 16 || std::fread(info, 8, 36, f) != 36) return 4;
    g.addEdge(h[0], h[1], T, info, h[2] != 0);
  }
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icpk_pg_params p = icp::PoseGraph::defaults();
    p.flags = head[2];
    p.preference_loop_closure = mu;
    icpk_pg_result r{};
    const int rc = g.optimize(eng, p, &r);
    if (rc < 0) {
      std::fprintf(stderr, "optimize failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t ints[6] = {rc, r.iterations, r.accepted, r.pcg_iterations, r.n_pruned, 0};
    const double costs[3] = {r.initial_cost, r.final_cost, r.final_lambda};
    std::fwrite(ints, 4, 6, o);
    std::fwrite(costs, 8, 3, o);
    std::fwrite(g.poses().data(), 8, g.poses().size(), o);
    std::fwrite(g.weights().data(), 8, g.weights().size(), o);
    std::fwrite(g.chi2().data(), 8, g.chi2().size(), o);
    std::fwrite(g.pruned().data(), 1, g.pruned().size(), o);
    std::fclose(o);
    for (size_t i = 0; i < g.nodes(); ++i) {
      const double* P = g.pose(i);
      std::printf("node %zu:", i);
      for (int k = 0; k < 12; ++k) std::printf(" %.17g", P[k]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
