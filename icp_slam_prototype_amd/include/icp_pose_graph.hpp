// icp_pose_graph.hpp -- C++ host side of pose-graph optimisation (icpk_pose_graph_* of include/icpk.h, K18), included
// by icp_align.hpp.
//
//   * icp::PoseGraph -- nodes (4 x 4 poses, node i's cloud into the world) and edges (the alignment of cloud s onto
//                       cloud t with its 6 x 6 information matrix); optimize() runs Levenberg-Marquardt on an Engine's
//                       GPU, with the line process over the uncertain edges when preference_loop_closure > 0
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "icp_align.hpp"

namespace icp {

class PoseGraph {
 public:
  // P: 16 doubles, row-major.  Returns the node's index
  int addNode(const double* P) {
    poses_.insert(poses_.end(), P, P + 16);
    return (int)(poses_.size() / 16) - 1;
  }
  // T moves cloud s onto cloud t (what Engine::align returns with s as source and t as target); info: row-major 6 x 6,
  // rotation first (PoseScore::information).  Returns the edge's index; the indices are checked by optimize()
  int addEdge(int s, int t, const double* T, const double* info, bool uncertain = false) {
    icpk_pg_edge e{};
    e.source = s, e.target = t, e.uncertain = uncertain ? 1 : 0;
    std::memcpy(e.T, T, sizeof(e.T));
    std::memcpy(e.info, info, sizeof(e.info));
    edges_.push_back(e);
    return (int)edges_.size() - 1;
  }
  static icpk_pg_params defaults() {
    icpk_pg_params p;
    icpk_default_pg_params(&p);
    return p;
  }
  // icpk_pose_graph_optimize: the poses are replaced by the optimised ones; weights(), chi2() and pruned() describe the
  // edges afterwards.  Returns a status of icpk.h (ICPK_W_NOT_CONVERGED: the loop ran into max_iterations)
  int optimize(Engine& eng, const icpk_pg_params& p = defaults(), icpk_pg_result* result = nullptr) {
    weights_.assign(edges_.size(), 0.0);
    chi2_.assign(edges_.size(), 0.0);
    pruned_.assign(edges_.size(), 0);
    return icpk_pose_graph_optimize(eng.ctx(), (int32_t)nodes(), poses_.data(), (int32_t)edges_.size(), edges_.data(), &p,
                                    result, weights_.data(), chi2_.data(), pruned_.data());
  }
  size_t nodes() const { return poses_.size() / 16; }
  size_t edges() const { return edges_.size(); }
  const double* pose(size_t i) const { return poses_.data() + 16 * i; }
  const std::vector<double>& poses() const { return poses_; }
  const std::vector<double>& weights() const { return weights_; }
  const std::vector<double>& chi2() const { return chi2_; }
  const std::vector<uint8_t>& pruned() const { return pruned_; }

 private:
  std::vector<double> poses_;
  std::vector<icpk_pg_edge> edges_;
  std::vector<double> weights_, chi2_;
  std::vector<uint8_t> pruned_;
};

}  // namespace icp
