// icp_map.hpp -- C++ host side of the voxel certainty map (icpk_map_* of include/icpk.h), included by icp_align.hpp.
//
//   * icp::Map         -- map::Map (map.hpp, map.cpp) on an Engine's GPU: update per rule, isOccupied,
//                         getVoxelCoordinates, list access
//   * icp::MapTracker  -- the live icp::getTransformation (icp.cpp:27-271): the frame's key points aligned against the
//                         map's key points, the rejected ones folded back into the map.  Key points either come from
//                         the caller (cv::KeyPoint::pt as (x, y) pairs) or are detected on the device from the colour
//                         frame (SLAM.cpp:255-256, K8)
//   * icp::detectFAST  -- cv::cvtColor(BGR -> GRAY) + cv::FAST on the device (icpk_detect_fast)
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "icp_align.hpp"

namespace icp {

// cv::FAST settings (SLAM.cpp:256: threshold 60, suppression on, TYPE_7_12)
struct FastSettings {
  int threshold = 60;
  bool nonmax = true;
  int type = ICPK_FAST_TYPE_7_12;
};

// SLAM.cpp:255-256 on the device: image rows x cols, channels 3 (BGR) or 1 (grey).  kp_xy: (x, y) per key point in
// FAST_t's order; response (or null): the score of each.  The key points also stay on the engine's device as its
// detected list (icpk_detected_to_cloud).  Returns a status of icpk.h.
inline int detectFAST(Engine& eng, const uint8_t* image, int rows, int cols, int channels, std::vector<float>& kp_xy,
                      std::vector<float>* response = nullptr, const FastSettings& s = FastSettings()) {
  const size_t cap = rows > 6 && cols > 6 ? (size_t)(rows - 6) * (size_t)(cols - 6) : 0;  // every candidate pixel
  kp_xy.resize(2 * cap + 2);
  if (response) response->resize(cap + 1);
  int32_t n = 0;
  const int rc = icpk_detect_fast(eng.ctx(), image, rows, cols, channels, s.threshold, s.nonmax ? 1 : 0, s.type,
                                  (int32_t)cap, kp_xy.data(), response ? response->data() : nullptr, &n);
  kp_xy.resize(rc == ICPK_OK ? 2 * (size_t)n : 0);
  if (response) response->resize(rc == ICPK_OK ? (size_t)n : 0);
  return rc;
}

// map::Map on the GPU of an Engine (one map per Engine; the first call allocates it, empty)
class Map {
 public:
  explicit Map(Engine& eng) : eng_(eng) {}
  Engine& engine() const { return eng_; }

  // map.cpp:17-31 Map::Map()
  int reset() { return icpk_map_reset(eng_.ctx()); }
  // one of the three rules (ICPK_MAP_ADD_*) over host points, in order:
  //   ICPK_MAP_ADD_CLOUD         map.cpp:220-269 update(PointCloud data, delta, ...): the cloud's key points
  //   ICPK_MAP_ADD_ASSOCIATED    map.cpp:88-119  update(associations, delta): the associations' data points
  //   ICPK_MAP_ADD_UNASSOCIATED  map.cpp:122-206 update(associations, errors, nonAssociations, delta)
  int update(int rule, const CloudView& points, int delta) {
    return icpk_map_update_points(eng_.ctx(), rule, points.x, points.y, points.z, points.n, delta);
  }
  // the same over the engine's source or target cloud (ICPK_MAP_FROM_*) where it lies; indices: null = all, in order
  int updateFrom(int rule, int from, int delta, const int32_t* indices = nullptr, int32_t n = 0) {
    return icpk_map_update(eng_.ctx(), rule, from, indices, n, delta);
  }
  // icp.cpp:63 map.mapCloud.points = cloud.points (the engine's source or target)
  int setPoints(int from) { return icpk_map_set_points(eng_.ctx(), from); }
  // map.cpp:441-444
  bool isOccupied(const float p[3]) {
    uint8_t occ = 0;
    return icpk_map_query(eng_.ctx(), &p[0], &p[1], &p[2], 1, nullptr, &occ, nullptr, nullptr) == ICPK_OK && occ != 0;
  }
  // map.cpp:55-85
  static void getVoxelCoordinates(const float p[3], int32_t v[3]) { icpk_map_voxel(p, v); }
  int32_t size(int list) const { return icpk_map_size(eng_.ctx(), list); }
  int getList(int list, std::vector<float>& x, std::vector<float>& y, std::vector<float>& z) const {
    const int32_t n = size(list);
    if (n < 0) return n;
    x.resize((size_t)n);
    y.resize((size_t)n);
    z.resize((size_t)n);
    return icpk_map_get_list(eng_.ctx(), list, x.data(), y.data(), z.data());
  }
  int getCertainty(std::vector<uint8_t>& grid) const {
    grid.resize((size_t)ICPK_MAP_CELLS);
    return icpk_map_get_certainty(eng_.ctx(), grid.data());
  }

 private:
  Engine& eng_;
};

// The live icp::getTransformation (icp.cpp:27-271) with the map on the device.  Per frame: the data depth image and
// the frame's key-point pixels (FAST runs outside).
//   * first call, taken while the map's point list is empty (icp.cpp:47-68): the pose is reset; the key points and
//     the full cloud of `previous`, posed by the identity and (5, 5, 5), go into the map (ADD_CLOUD with d = 180 on the
//     key points, :62; the point list := the full cloud, :63);
//   * every call: the data key points posed by cameraRotation / cameraPosition (:70-71) are aligned against the map's
//     key points with the key-point acceptance 0.1 (icpk_align_to_map with d = 25, :98-271); the pose is kept as
//     icp::Tracker keeps it (:235-246, :260-261).
// Uses the engine's source and target clouds.
class MapTracker {
 public:
  explicit MapTracker(Engine& eng, float fx = ICPK_FX, float cx = ICPK_CX) : map(eng), eng_(eng), fx_(fx), cx_(cx) {
    reset();
  }

  void reset() {
    static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(cameraRotation, I, sizeof(I));  // icp.cpp:49
    std::memcpy(lastRotation, I, sizeof(I));    // icp.cpp:50
    cameraPosition[0] = cameraPosition[1] = cameraPosition[2] = 5.f;     // icp.cpp:53
    lastTranslation[0] = lastTranslation[1] = lastTranslation[2] = 0.f;  // icp.cpp:54
    params = AlignParams();
    params.solve = ICPK_SOLVE_REFERENCE;
    params.max_nn_dist = ICPK_MAX_NN_KEYPOINT_DISTANCE;  // icp.hpp:10, icp.cpp:503
  }

  // data / previous: rows x cols CV_16UC1 row-major; kp_xy: n_kp key-point pixel positions (x, y).  `previous` is read
  // only by the first call (the map's point list empty) and may be null afterwards.  T: row-major 4x4.
  int getTransformation(const uint16_t* data, const uint16_t* previous, int rows, int cols, const float* kp_xy,
                        int n_kp, int maxIterations, float threshold, float T[16]) {
    icpk_ctx* c = eng_.ctx();
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    std::vector<float> kp((size_t)3 * (n_kp > 0 ? n_kp : 1));
    if (map.size(ICPK_MAP_POINTS) == 0) {  // icp.cpp:47-68
      if (!previous) return ICPK_E_ARG;
      reset();
      int n = icpk_backproject_keypoints(previous, rows, cols, kp_xy, n_kp, fx_, cx_, kp.data(), nullptr);
      if (n < 0) return n;
      std::vector<float> x, y, z;
      pose(kp.data(), n, x, y, z);                                                              // icp.cpp:58-59
      int rc = map.update(ICPK_MAP_ADD_CLOUD, CloudView{x.data(), y.data(), z.data(), n}, ICPK_MAP_MAX_CONFIDENCE);  // :62
      if (rc != ICPK_OK) return rc;
      const float no_offset[3] = {0.f, 0.f, 0.f};
      rc = icpk_backproject(c, previous, rows, cols, fx_, cx_, no_offset, 1);  // icp.cpp:39
      if (rc < 0) return rc;
      rc = icpk_transform_target(c, cameraRotation, cameraPosition);
      if (rc == ICPK_OK) rc = map.setPoints(ICPK_MAP_FROM_TARGET);  // :63
      if (rc != ICPK_OK) return rc;
    }
    const int n = icpk_backproject_keypoints(data, rows, cols, kp_xy, n_kp, fx_, cx_, kp.data(), nullptr);
    if (n < 0) return n;
    std::vector<float> x, y, z;
    pose(kp.data(), n, x, y, z);  // icp.cpp:70-71
    if (dense) return alignDense(data, rows, cols, maxIterations, threshold, T);
    int rc = icpk_set_source(c, x.data(), y.data(), z.data(), n);
    if (rc != ICPK_OK) return rc;
    return alignToMap(maxIterations, threshold, T, false);
  }

  // The same with the key points of the colour frame detected on the device (SLAM.cpp:255-256, `fast`): color is
  // c_rows x c_cols with channels 3 (BGR) or 1 (grey), and may differ in size from the depth images.  As the reference,
  // the first call back-projects the CURRENT colour frame's key points from `previous` for the map seed (icp.cpp:38-39,
  // 58-62) and from `data` for the alignment (:70-71).  Detection -> cloud -> map update / alignment without the key
  // points crossing PCIe.
  int getTransformation(const uint16_t* data, const uint16_t* previous, int rows, int cols, const uint8_t* color,
                        int c_rows, int c_cols, int channels, int maxIterations, float threshold, float T[16]) {
    icpk_ctx* c = eng_.ctx();
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    int rc = icpk_detect_fast(c, color, c_rows, c_cols, channels, fast.threshold, fast.nonmax ? 1 : 0, fast.type, 0, nullptr,
                              nullptr, nullptr);
    if (rc != ICPK_OK) return rc;
    if (map.size(ICPK_MAP_POINTS) == 0) {  // icp.cpp:47-68
      if (!previous) return ICPK_E_ARG;
      reset();
      rc = icpk_detected_to_cloud(c, previous, rows, cols, fx_, cx_, cameraRotation, cameraPosition, 0, nullptr);  // :58-59
      if (rc == ICPK_OK) rc = map.updateFrom(ICPK_MAP_ADD_CLOUD, ICPK_MAP_FROM_SOURCE, ICPK_MAP_MAX_CONFIDENCE);  // :62
      if (rc != ICPK_OK) return rc;
      const float no_offset[3] = {0.f, 0.f, 0.f};
      rc = icpk_backproject(c, previous, rows, cols, fx_, cx_, no_offset, 1);  // icp.cpp:39
      if (rc < 0) return rc;
      rc = icpk_transform_target(c, cameraRotation, cameraPosition);
      if (rc == ICPK_OK) rc = map.setPoints(ICPK_MAP_FROM_TARGET);  // :63
      if (rc != ICPK_OK) return rc;
    }
    if (dense) return alignDense(data, rows, cols, maxIterations, threshold, T);
    rc = icpk_detected_to_cloud(c, data, rows, cols, fx_, cx_, cameraRotation, cameraPosition, 0, nullptr);  // :70-71
    if (rc != ICPK_OK) return rc;
    return alignToMap(maxIterations, threshold, T, false);
  }

  Map map;
  FastSettings fast;  // the colour overload's cv::FAST settings
  // true: every frame after the seed aligns its whole (subsampled: the engine's icpk_set_subsample) depth cloud
  // against the map with the reference's mapped association (icp.cpp:150, :254; icpk_align_to_map_dense, max
  // distance 0.75, then ADD_ASSOCIATED with d = 25) instead of its key points
  bool dense = false;
  float cameraRotation[9];
  float lastRotation[9];
  float cameraPosition[3];
  float lastTranslation[3];
  AlignParams params;
  icpk_stats lastStats{};

 private:
  // the data frame back-projected (pointcloud.cpp:19-58), posed by the camera (icp.cpp:70-71) and aligned densely
  int alignDense(const uint16_t* data, int rows, int cols, int maxIterations, float threshold, float T[16]) {
    icpk_ctx* c = eng_.ctx();
    const float no_offset[3] = {0.f, 0.f, 0.f};
    int rc = icpk_backproject(c, data, rows, cols, fx_, cx_, no_offset, 0);
    if (rc < 0) return rc;
    rc = icpk_transform_source(c, cameraRotation, cameraPosition);
    if (rc == ICPK_OK) rc = icpk_commit_source(c);
    if (rc != ICPK_OK) return rc;
    return alignToMap(maxIterations, threshold, T, true);
  }

  // icp.cpp:98-271 on the engine's source against the map, then the pose kept as icp::Tracker keeps it
  int alignToMap(int maxIterations, float threshold, float T[16], bool mapped) {
    icpk_ctx* c = eng_.ctx();
    params.max_iterations = maxIterations;
    params.threshold = threshold;
    std::memcpy(params.last_rotation, lastRotation, sizeof(lastRotation));
    std::memcpy(params.last_translation, lastTranslation, sizeof(lastTranslation));
    icpk_stats st;
    int rc;
    if (mapped) {
      AlignParams q = params;
      q.max_nn_dist = ICPK_MAX_NN_DISTANCE;  // icp.cpp:363
      rc = icpk_align_to_map_dense(c, &q, ICPK_MAP_DELTA_CONFIDENCE, T, &st);
    } else {
      rc = icpk_align_to_map(c, &params, ICPK_MAP_DELTA_CONFIDENCE, T, &st);
    }
    if (rc < 0) return rc;
    lastStats = st;
    int32_t niter = 0;
    std::vector<float> R((size_t)maxIterations * 9 + 9), t((size_t)maxIterations * 3 + 3);
    icpk_get_trace(c, &niter, R.data(), t.data(), nullptr, nullptr);
    for (int i = 0; i < niter; ++i) {  // icp.cpp:235-237, 245-246
      float Rinv[9], prod[9];
      invert3(R.data() + 9 * i, Rinv);
      mul3(cameraRotation, Rinv, prod);
      std::memcpy(cameraRotation, prod, sizeof(prod));
      for (int k = 0; k < 3; ++k) cameraPosition[k] -= t[3 * i + k];
    }
    for (int k = 0; k < 3; ++k) lastTranslation[k] = -T[4 * k + 3];  // icp.cpp:260-261
    if (rc != ICPK_W_TOO_FEW_PAIRS) {
      static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      std::memcpy(lastRotation, I, sizeof(I));
    }
    return rc;
  }

  // PointCloud::rotate + translate (pointcloud.cpp:321-359) as the device does it: p' = fl32(fl32(R p) + t)
  void pose(const float* xyz, int n, std::vector<float>& x, std::vector<float>& y, std::vector<float>& z) const {
    x.resize((size_t)(n > 0 ? n : 1));
    y.resize(x.size());
    z.resize(x.size());
    const float* Rm = cameraRotation;
    for (int i = 0; i < n; ++i) {
      const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
      float r[3];
      for (int k = 0; k < 3; ++k)
        r[k] = (float)std::fma((double)Rm[3 * k + 2], pz, std::fma((double)Rm[3 * k + 1], py, (double)Rm[3 * k] * px));
      x[(size_t)i] = r[0] + cameraPosition[0];
      y[(size_t)i] = r[1] + cameraPosition[1];
      z[(size_t)i] = r[2] + cameraPosition[2];
    }
  }
  static void mul3(const float A[9], const float B[9], float C[9]) {  // CV_32F product, double accumulate
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (double)A[3 * r + k] * (double)B[3 * k + cc];
        C[3 * r + cc] = (float)s;
      }
  }
  static void invert3(const float m[9], float out[9]) {  // icp.cpp:235 Mat::inv on a 3x3 (as icp::Tracker)
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double s = det != 0.0 ? 1.0 / det : 0.0;
    const double t[9] = {(e * i - f * h) * s, (c * h - b * i) * s, (b * f - c * e) * s,
                         (f * g - d * i) * s, (a * i - c * g) * s, (c * d - a * f) * s,
                         (d * h - e * g) * s, (b * g - a * h) * s, (a * e - b * d) * s};
    for (int k = 0; k < 9; ++k) out[k] = (float)t[k];
  }

  Engine& eng_;
  float fx_, cx_;
};

}  // namespace icp
