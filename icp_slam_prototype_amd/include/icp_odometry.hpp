// icp_odometry.hpp -- icp::FrameOdometry: projective frame-to-frame odometry (K28) over one icp::Engine, the C++ mirror
// of odometry.ProjectiveOdometry.  Every frame is aligned by the projective loop (icpk_align_projective, or
// icpk_align_projective_colored with `color`) to a frame view -- the previous frame's, or a keyframe's, vertex and
// normal map (Engine::buildFrameView) -- coarse to fine over the resident pyramid.  No TSDF volume is involved.
// Header only; links -licpk.
#pragma once
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "icp_align.hpp"

namespace icp {

class FrameOdometry {
 public:
  // when the view is rebuilt from the current frame; off: after every frame (frame to frame).  A bound < 0 does not apply
  struct Keyframe {
    bool on = false;
    double minOverlap = -1.0, maxAngleDeg = -1.0, maxShift = -1.0;
  };
  // the photometric term; off: the geometric loop.  gradientRadius: metres at level 0, level l takes 2^l times it
  struct Color {
    bool on = false;
    float lambdaGeometric = 0.968f, gradientRadius = 0.1f;
    int minNeighbors = 4;
  };

  // pose: the first frame's camera-to-world pose (nullptr: the identity); counts: iterations per level, finest first
  FrameOdometry(Engine& eng, const double* pose, float fx, float cx, std::vector<int> counts = {10, 5, 4})
      : eng_(eng), counts_(std::move(counts)), fx_(fx), cx_(cx) {
    if (counts_.empty() || counts_.size() > ICPK_PYRAMID_MAX_LEVELS) throw std::invalid_argument("1 .. 8 iteration counts");
    for (int k = 0; k < 16; ++k) pose_[k] = pose ? pose[k] : (k % 5 == 0 ? 1.0 : 0.0);
    icpk_default_projective_params(&params);
    params.fx = fx, params.cx = cx, params.max_dist = 0.5f;
    levelStats.resize(counts_.size());
    levelValid.assign(counts_.size(), 0);
  }

  icpk_projective_params params;  // max_dist, min_normal_cos, min_pairs are read; level and max_iterations are set per level
  Keyframe keyframe;
  Color color;
  const icpk_bilateral_params* bilateral = nullptr;  // non-null: level 0 is smoothed (the intensity never is)
  // per level of the last frame, finest first (status ICPK_E_NOT_SET: skipped); the view's valid pixels per level
  std::vector<icpk_projective_result> levelStats;
  std::vector<int32_t> levelValid;
  int frames = 0, viewsBuilt = 0, levelsSkipped = 0;

  const double* pose() const { return pose_; }
  const double* viewPose() const { return viewPose_; }

  // One frame (with its rows x cols intensities when color.on).  poseOut (or nullptr): the frame's pose.  Returns
  // ICPK_OK or a negative status; the first frame takes the initial pose.  A level whose view has fewer valid pixels
  // than min_pairs is skipped and counted; at level 0 that is ICPK_E_EMPTY_TARGET.
  int track(const uint16_t* depth, int rows, int cols, double* poseOut = nullptr, const float* intensity = nullptr) {
    if (color.on && !intensity) return ICPK_E_ARG;
    icpk_pyramid_params pp;
    icpk_default_pyramid_params(&pp);
    pp.levels = (int32_t)counts_.size();
    if (int rc = eng_.buildDepthPyramid(depth, rows, cols, &pp, bilateral)) return rc;
    if (color.on)
      if (int rc = eng_.setPyramidIntensity(intensity, rows, cols)) return rc;
    if (frames == 0) {
      if (int rc = buildView()) return rc;
    } else {
      const int rc = align();
      eng_.setProjectiveView(ICPK_VIEW_RAYCAST);
      if (rc < 0) return rc;
      long long valid = 0;
      for (size_t i = 0; i < (size_t)rows * cols; ++i) valid += depth[i] != 0;
      if (viewIsSpent(valid))
        if (int rc2 = buildView()) return rc2;
    }
    frames += 1;
    if (poseOut) std::memcpy(poseOut, pose_, sizeof(pose_));
    return ICPK_OK;
  }

 private:
  int buildView() {
    int32_t none[ICPK_PYRAMID_MAX_LEVELS];
    int32_t valid[ICPK_PYRAMID_MAX_LEVELS];
    if (int rc = eng_.buildFrameView(fx_, cx_, pose_, valid, none)) return rc;
    for (size_t l = 0; l < counts_.size(); ++l) levelValid[l] = valid[l];
    std::memcpy(viewPose_, pose_, sizeof(pose_));
    viewsBuilt += 1;
    if (color.on)
      for (size_t l = 0; l < counts_.size(); ++l)
        if (int rc = eng_.frameViewColorGradients((int)l, color.gradientRadius * (float)(1 << l), color.minNeighbors)) return rc;
    return ICPK_OK;
  }

  int align() {
    double estimate[16];
    std::memcpy(estimate, pose_, sizeof(pose_));
    const icpk_projective_color_params cp{color.lambdaGeometric};
    for (int l = (int)counts_.size() - 1; l >= 0; --l) {
      icpk_projective_params p = params;
      p.level = l, p.max_iterations = counts_[l];
      levelStats[l] = icpk_projective_result{ICPK_E_NOT_SET, 0, 0, 0.0};
      if (levelValid[l] < p.min_pairs) {
        if (l == 0) return ICPK_E_EMPTY_TARGET;
        levelsSkipped += 1;
        continue;
      }
      if (int rc = eng_.setProjectiveView(ICPK_VIEW_FRAME, l)) return rc;
      double next[16];
      const int rc = color.on ? icpk_align_projective_colored(eng_.ctx(), &p, &cp, estimate, next, &levelStats[l])
                              : icpk_align_projective(eng_.ctx(), &p, estimate, next, &levelStats[l]);
      if (rc < 0) return rc;
      std::memcpy(estimate, next, sizeof(next));
    }
    std::memcpy(pose_, estimate, sizeof(pose_));
    return ICPK_OK;
  }

  // the motion from the view's pose to the current one passes a bound, or level 0 paired too few of the valid pixels
  bool viewIsSpent(long long valid) const {
    if (!keyframe.on) return true;
    // E = inverse(view) * pose for rigid poses: R = Rv^T Rp, t = Rv^T (tp - tv)
    double tr = 0.0, t[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) tr += viewPose_[4 * b + a] * pose_[4 * b + a];
      for (int b = 0; b < 3; ++b) t[a] += viewPose_[4 * b + a] * (pose_[4 * b + 3] - viewPose_[4 * b + 3]);
    }
    double c = (tr - 1.0) / 2.0;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double angle = std::acos(c) * 180.0 / 3.14159265358979323846;
    const double shift = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    return (keyframe.minOverlap >= 0 && (double)levelStats[0].count < keyframe.minOverlap * (double)valid) ||
           (keyframe.maxAngleDeg >= 0 && angle > keyframe.maxAngleDeg) || (keyframe.maxShift >= 0 && shift > keyframe.maxShift);
  }

  Engine& eng_;
  std::vector<int> counts_;
  float fx_, cx_;
  double pose_[16], viewPose_[16] = {0};
};

}  // namespace icp
