// icp_align.hpp -- C++ host side above the C ABI (include/icpk.h).
//
// Mirrors the reference's operator surface for the ICP path without OpenCV:
//   * icp::align(source, target, params, &result)      -- the inner loop on SoA views
//     (north_star's call surface; runs on the calling thread's default Engine, or pass one)
//   * icp::alignBatch(engine, pairs, params, results)  -- frame-batch mode
//   * icp::Comm                                        -- RCCL collectives of the multi-GPU modes
//   * icp::filterDepthImage / icp::findGlobalKeyPointAssociations -- SLAM.cpp:553-574,
//     icp.cpp:488-515 with the reference's names and argument meaning
//   * icp::Tracker                                     -- the per-frame state machine of
//     icp::getTransformation (icp.cpp:22-26 file-scope pose state, :38-71 cloud set-up,
//     :98-268 loop, :237/:246 pose update), fed with raw CV_16UC1 depth buffers
//   * icp::makeRotationMatrix / meanSquareError / toEulerianAngle helpers with the
//     reference's names and argument meaning (icp.hpp:25-27, SLAM.hpp:44-46)
//   * icp::Map / icp::MapTracker / icp::detectFAST (icp_map.hpp, included at the end) -- the
//     voxel certainty map, the live getTransformation against it, and FAST on the device
// icp_opencv_adapter.hpp adds the exact cv::Mat signature when OpenCV is present.
//
// Header-only; link with -licpk.  Errors: status codes of icpk.h, never exceptions
// from the hot path (the Engine constructor throws std::runtime_error when no GPU
// is usable -- there is no CPU fallback).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "icpk.h"

namespace icp {

// xyz structure-of-arrays view of a point cloud in host memory (replaces
// point_list_t / color_point_t, pointcloud.hpp:13-23; colour weight is 0)
struct CloudView {
  const float* x = nullptr;
  const float* y = nullptr;
  const float* z = nullptr;
  int32_t n = 0;
};

struct AlignParams : icpk_params {
  AlignParams() { icpk_default_params(this); }
};

struct AlignResult {
  float T[16];        // row-major 4x4, same content as the cv::Mat of icp.cpp:29,284
  icpk_stats stats{};
  int status = ICPK_OK;
  float (*rotation())[4] { return reinterpret_cast<float(*)[4]>(T); }
};

// one pair of Engine::matchFeatures: source index, target index, the squared descriptor distance
struct FeatureMatch {
  int32_t source, target;
  float distance;
};

// one pair of Engine::matchDescriptors: the key points' indices in their slots, the Hamming distance, and the least
// distance to any other target descriptor (257: none)
struct DescriptorMatch {
  int32_t source, target, hamming, second;
};

// one candidate pose as icpk_score_poses judges it: the inliers within maxDist, the metrics of icpk_score_metrics, the
// 6x6 information matrix of the pair (row-major; rotation vector, then translation) and the sums they are made of
struct PoseScore {
  int64_t inliers = 0;
  float fitness = 0.f, inlierRmse = 0.f, meanDist = 0.f;
  double information[36] = {};
  double sums[ICPK_NSCORE] = {};
};

// RAII owner of one icpk_ctx (one GPU, one HIP stream).  One Engine per host
// thread / per GPU; calls on one Engine are serialised.
class Engine {
 public:
  explicit Engine(int device = 0) {
    const int rc = icpk_create(&ctx_, device);
    if (rc != ICPK_OK) throw std::runtime_error("icpk_create failed (status " + std::to_string(rc) + "): no usable HIP device");
  }
  ~Engine() { icpk_destroy(ctx_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  icpk_ctx* ctx() const { return ctx_; }
  const char* last_error() const { return icpk_last_error(ctx_); }
  // pointcloud.cpp:27-30 (SUBSAMPLE_FACTOR, pointcloud.hpp:11) with a reproducible choice instead of rand(): every
  // cloud this engine back-projects from now on keeps one valid pixel in `factor` (0 / 1: all of them)
  int setSubsample(int factor = ICPK_SUBSAMPLE_FACTOR, uint64_t seed = 0) { return icpk_set_subsample(ctx_, factor, seed); }
  // the bilateral filter of a CV_16UC1 depth buffer (icpk_bilateral_depth_image, K22): holes stay holes, noise is
  // averaged, never across a depth step; out may be the input buffer; params nullptr: icpk_default_bilateral_params
  int bilateralDepthImage(const uint16_t* image, uint16_t* out, int rows, int cols,
                          const icpk_bilateral_params* params = nullptr) {
    return icpk_bilateral_depth_image(ctx_, params, image, out, rows, cols);
  }
  // ... and the cloud of the smoothed frame without the image leaving the device (icpk_backproject_smoothed): the source
  // (which = 0) or the target (1; normalsMode >= 0: with its normals, as icpk_backproject_with_normals).  Returns the
  // number of points or a negative status.
  int backprojectSmoothed(const uint16_t* image, int rows, int cols, float fx, float cx, const float* offset, int which,
                          int normalsMode = -1, const icpk_bilateral_params* params = nullptr) {
    return icpk_backproject_smoothed(ctx_, image, rows, cols, fx, cx, offset, which, normalsMode, params);
  }
  // the depth pyramid of a CV_16UC1 depth buffer on the device (icpk_depth_pyramid_build, K24), resident until the
  // next build; params nullptr: icpk_default_pyramid_params; smooth non-null: level 0 is the frame after the bilateral
  // filter
  int buildDepthPyramid(const uint16_t* image, int rows, int cols, const icpk_pyramid_params* params = nullptr,
                        const icpk_bilateral_params* smooth = nullptr) {
    return icpk_depth_pyramid_build(ctx_, image, rows, cols, params, smooth);
  }
  // one level of it: its shape (out nullptr: the shape alone) and its pixels into `out`, rows x cols of that level
  int depthPyramidLevel(int level, int* rows, int* cols, uint16_t* out = nullptr) {
    const int rc = icpk_depth_pyramid_shape(ctx_, level, rows, cols);
    return rc != ICPK_OK || !out ? rc : icpk_depth_pyramid_get(ctx_, level, out);
  }
  // the frame's intensities (rows x cols floats in [0, 1], level 0's shape) beside the resident pyramid, every level
  // built (icpk_depth_pyramid_set_intensity, K26); the next buildDepthPyramid drops them.  out: one level of them
  int setPyramidIntensity(const float* intensity, int rows, int cols) {
    return icpk_depth_pyramid_set_intensity(ctx_, intensity, rows, cols);
  }
  int pyramidIntensityLevel(int level, float* out) { return icpk_depth_pyramid_get_intensity(ctx_, level, out); }
  // ... and the cloud of a level read where it lies (icpk_depth_pyramid_backproject): fx, cx are the LEVEL-0 intrinsics.
  // Returns the number of points or a negative status.
  int backprojectPyramidLevel(int level, float fx, float cx, const float* offset, int which, int normalsMode = -1) {
    return icpk_depth_pyramid_backproject(ctx_, level, fx, cx, offset, which, normalsMode);
  }
  // the frame view (icpk_frame_view_build, K28): every level of the resident pyramid as eight planes in world coordinates
  // at `pose` (double[16], camera-to-world), kept by the engine until the next build or releaseFrameView; fx, cx are
  // the LEVEL-0 intrinsics.  nValid / nNoNormal: one entry per level, or nullptr (both nullptr: no host wait)
  int buildFrameView(float fx, float cx, const double* pose, int32_t* nValid = nullptr, int32_t* nNoNormal = nullptr) {
    return icpk_frame_view_build(ctx_, fx, cx, pose, nValid, nNoNormal);
  }
  int frameViewLevels() { return icpk_frame_view_levels(ctx_); }
  // one level of it: its shape, and its eight planes into `out` (8 x rows x cols floats; nullptr: the shape alone)
  int frameViewLevel(int level, int* rows, int* cols, float* out = nullptr) {
    int r = 0, c = 0;
    const int rc = icpk_frame_view_shape(ctx_, level, &r, &c);
    if (rc != ICPK_OK) return rc;
    if (rows) *rows = r;
    if (cols) *cols = c;
    if (!out) return ICPK_OK;
    float* planes[8];
    for (int k = 0; k < 8; ++k) planes[k] = out + (size_t)k * r * c;
    return icpk_frame_view_get(ctx_, level, planes);
  }
  int releaseFrameView() { return icpk_frame_view_release(ctx_); }
  int frameViewColorGradients(int level, float radius, int minNeighbors = 4) {
    return icpk_frame_view_color_gradients(ctx_, level, radius, minNeighbors, 0);
  }
  // which planes the projective calls read (icpk_projective_set_view): ICPK_VIEW_RAYCAST (the default) or
  // ICPK_VIEW_FRAME with the level of the frame view
  int setProjectiveView(int which, int viewLevel = 0) { return icpk_projective_set_view(ctx_, which, viewLevel); }
  // robust alignment (icpk_set_robust): trimmed pairs and Huber / Tukey weights for every later alignment of this
  // engine (Kabsch and point-to-plane flavours); clearRobust() turns it off again (the default)
  int setRobust(const icpk_robust& r) { return icpk_set_robust(ctx_, &r); }
  int clearRobust() { return icpk_set_robust(ctx_, nullptr); }
  // voxel-grid downsampling (icpk_voxel_downsample): one point per occupied cube of edge `leaf` in place of the
  // working source (which = 0) or the target (1); n_out: the size of the new cloud
  int voxelDownsample(int which, float leaf, int mode = ICPK_VOXEL_CENTROID, int* n_out = nullptr) {
    int32_t n = 0;
    const int rc = icpk_voxel_downsample(ctx_, which, leaf, mode, &n, nullptr);
    if (n_out && rc == ICPK_OK) *n_out = n;
    return rc;
  }
  // outlier removal (icpk_remove_outliers): the statistical or the radius filter on the working source (which = 0) or
  // the target (1); statsOnly: the cloud stays as it is and only outlierStats changes
  int removeOutliers(int which, const icpk_outlier_filter& f, bool statsOnly = false, int* n_out = nullptr,
                     int* n_dropped = nullptr) {
    int32_t n = 0, d = 0;
    const int rc = icpk_remove_outliers(ctx_, which, &f, statsOnly ? ICPK_FILTER_STATS_ONLY : 0, &n, &d);
    if (n_out && rc == ICPK_OK) *n_out = n;
    if (n_dropped && rc == ICPK_OK) *n_dropped = d;
    return rc;
  }
  // what the last removeOutliers found (icpk_get_outlier_stats): the vectors are resized to n_in; summary: 4 doubles
  int outlierStats(std::vector<double>* value, std::vector<float>* kth, std::vector<int32_t>* out_index,
                   double* summary = nullptr, int* n_out = nullptr) {
    int32_t n_in = 0, m = 0;
    int rc = icpk_get_outlier_stats(ctx_, &n_in, &m, nullptr, nullptr, nullptr, nullptr);
    if (rc != ICPK_OK) return rc;
    if (value) value->assign((size_t)n_in, 0.0);
    if (kth) kth->assign((size_t)n_in, 0.f);
    if (out_index) out_index->assign((size_t)n_in, -1);
    rc = icpk_get_outlier_stats(ctx_, nullptr, nullptr, value ? value->data() : nullptr, kth ? kth->data() : nullptr,
                                out_index ? out_index->data() : nullptr, summary);
    if (n_out && rc == ICPK_OK) *n_out = m;
    return rc;
  }
  // target normals from the target's own geometry (icpk_estimate_target_normals): the plane fitted to every target
  // point's neighbours within `radius`, oriented towards `viewpoint` (3 floats, or nullptr), installed as the target
  // normals ICPK_SOLVE_POINT_TO_PLANE reads; no host wait
  int estimateTargetNormals(float radius, int minNeighbors = 5, const float* viewpoint = nullptr, int flags = 0) {
    return icpk_estimate_target_normals(ctx_, radius, minNeighbors, viewpoint, flags);
  }
  // ... and what it found (icpk_get_normal_stats): any pointer may be null; count / curvature sized for the target,
  // moments for 10 words per point (only after flags = ICPK_NORMALS_KEEP_MOMENTS)
  int normalStats(int* n, int* n_valid, int32_t* count = nullptr, float* curvature = nullptr, int64_t* moments = nullptr) {
    int32_t a = 0, b = 0;
    const int rc = icpk_get_normal_stats(ctx_, &a, &b, count, curvature, moments);
    if (rc == ICPK_OK && n) *n = a;
    if (rc == ICPK_OK && n_valid) *n_valid = b;
    return rc;
  }
  // plane-to-plane flavour (ICPK_SOLVE_PLANE_TO_PLANE): normals of the uploaded source -- estimated by
  // estimateTargetNormals' rule (no host wait) or given from the host (n = the source size) --, their read-back
  // (resized to 3 planes of icpk_source_size floats: x | y | z) and epsilon of the surface model, finite and in (0, 1].
  // The normals stay with the source until it is replaced: set the source, then its normals, then icpk_align.
  int estimateSourceNormals(float radius, int minNeighbors = 5, const float* viewpoint = nullptr) {
    return icpk_estimate_source_normals(ctx_, radius, minNeighbors, viewpoint, 0);
  }
  int setSourceNormals(const float* nx, const float* ny, const float* nz, int32_t n) {
    return icpk_set_source_normals(ctx_, nx, ny, nz, n);
  }
  int sourceNormals(std::vector<float>* planes) {
    if (!planes) return ICPK_E_ARG;
    const size_t n = (size_t)icpk_source_size(ctx_);
    planes->assign(3 * n + 1, 0.f);  // (+1: valid pointers for an empty source)
    const int rc = icpk_get_source_normals(ctx_, planes->data(), planes->data() + n, planes->data() + 2 * n);
    planes->resize(3 * n);
    return rc;
  }
  int setPlaneToPlane(float epsilon = 1e-3f) { return icpk_set_plane_to_plane(ctx_, epsilon); }
  // colored ICP (icpk_set_colored): one intensity in [0, 1] per point of the target and of the uploaded source (n = the
  // cloud's size; they stay with the cloud until it is replaced), the target's colour gradients from its normals and
  // intensities (no host wait), and the setting: while on, ICPK_SOLVE_POINT_TO_PLANE runs the joint geometric +
  // photometric step with lambdaGeometric in [0, 1] on the geometric part.  Set the clouds, the target normals, the
  // colours, estimate the gradients, then icpk_align.  minNeighbors must be at least 1 (ICPK_E_ARG otherwise): a point
  // with fewer neighbours within the radius gets the zero gradient.
  int setTargetColors(const float* intensity, int32_t n) { return icpk_set_target_colors(ctx_, intensity, n); }
  int setSourceColors(const float* intensity, int32_t n) { return icpk_set_source_colors(ctx_, intensity, n); }
  int estimateTargetColorGradients(float radius, int minNeighbors = 4, int flags = 0) {
    return icpk_estimate_target_color_gradients(ctx_, radius, minNeighbors, flags);
  }
  int setColored(bool on, float lambdaGeometric = 0.968f) { return icpk_set_colored(ctx_, on ? 1 : 0, lambdaGeometric); }
  // pose scoring (icpk_score_poses): n candidate poses (T: 16 floats each, row-major 4x4) of the uploaded source
  // against the target in one call -- fitness, inlier RMSE, mean distance and the information matrix of each; the
  // engine's clouds, associations and seeds stay as they are.  flags: ICPK_SCORE_KEEP_ASSOC.
  int scorePoses(const float* T, int n, float maxDist, std::vector<PoseScore>* out, int flags = 0) {
    if (!out) return ICPK_E_ARG;
    const size_t m = n > 0 ? (size_t)n : 1;
    std::vector<double> sums(m * ICPK_NSCORE, 0.0);
    std::vector<int64_t> inl(m, 0);
    const int rc = icpk_score_poses(ctx_, n, T, maxDist, flags, sums.data(), inl.data());
    if (rc != ICPK_OK) return rc;
    const int32_t ns = icpk_source_size(ctx_);
    out->assign((size_t)n, PoseScore{});
    for (int k = 0; k < n; ++k) {
      PoseScore& s = (*out)[(size_t)k];
      const double* sk = sums.data() + (size_t)k * ICPK_NSCORE;
      s.inliers = inl[(size_t)k];
      std::memcpy(s.sums, sk, sizeof(s.sums));
      icpk_score_metrics(sk, s.inliers, ns, &s.fitness, &s.inlierRmse, &s.meanDist);
      icpk_information_matrix(sk, s.inliers, s.information);
    }
    return ICPK_OK;
  }
  // ... and the working source as it stands (after icpk_align: the alignment just computed)
  int scoreCurrent(float maxDist, PoseScore* out) {
    if (!out) return ICPK_E_ARG;
    std::vector<PoseScore> v;
    const int rc = scorePoses(nullptr, 1, maxDist, &v);
    if (rc == ICPK_OK) *out = v[0];
    return rc;
  }
  // global registration (include/icpk.h, K16): FPFH descriptors of the uploaded source (which = 0, needs source
  // normals) or of the target (which = 1, needs target normals); their matches, brought to the host if asked for; and
  // the seeded RANSAC over the matches that scorePoses' path ranks.  The pose of *out moves the source onto the target:
  // icpk_transform_source with it, then icpk_align, refines it.
  int computeFPFH(int which, float radius, int flags = 0) { return icpk_compute_fpfh(ctx_, which, radius, flags); }
  int fpfh(int which, std::vector<float>* desc, std::vector<uint8_t>* valid) {
    const size_t n = (size_t)(which == 0 ? icpk_source_size(ctx_) : icpk_target_size(ctx_));
    if (desc) desc->assign(n * ICPK_FPFH_BINS + 1, 0.f);  // (+1: valid pointers for an empty cloud)
    if (valid) valid->assign(n + 1, 0);
    int32_t m = 0;
    const int rc = icpk_get_fpfh(ctx_, which, desc ? desc->data() : nullptr, valid ? valid->data() : nullptr, &m);
    if (desc) desc->resize(rc == ICPK_OK ? (size_t)m * ICPK_FPFH_BINS : 0);
    if (valid) valid->resize(rc == ICPK_OK ? (size_t)m : 0);
    return rc;
  }
  int matchFeatures(bool mutual, std::vector<FeatureMatch>* out = nullptr) {
    int rc = icpk_match_features(ctx_, mutual ? ICPK_MATCH_MUTUAL : 0);
    if (rc != ICPK_OK || !out) return rc;
    const size_t cap = (size_t)icpk_source_size(ctx_) + 1;
    std::vector<int32_t> si(cap), ti(cap);
    std::vector<float> D(cap);
    int32_t m = 0;
    rc = icpk_get_feature_matches(ctx_, si.data(), ti.data(), D.data(), &m);
    if (rc != ICPK_OK) return rc;
    out->resize((size_t)m);
    for (int32_t k = 0; k < m; ++k) (*out)[(size_t)k] = FeatureMatch{si[(size_t)k], ti[(size_t)k], D[(size_t)k]};
    return ICPK_OK;
  }
  int registerGlobal(const icpk_global_params& params, icpk_global_result* out) {
    return icpk_register_global(ctx_, &params, out);
  }
  // appearance matching of key points (include/icpk.h, K32): oriented BRIEF descriptors of the list icpk_detect_fast
  // left on the device (describeKeypoints) or of a caller's image and key points (describePoints) into slot `which` (0
  // the source side, 1 the target side); the slot's key points back-projected into cloud `which` (describedToCloud,
  // returns the number of points or a negative status); and the Hamming matches of the two slots, brought to the host if
  // asked for.  With ICPK_BRIEF_TO_CLOUDS in params.flags the pairs are also K16's match list: registerGlobal runs on them.
  int describeKeypoints(int which, int flags = 0) { return icpk_describe_keypoints(ctx_, which, flags); }
  int describePoints(int which, const uint8_t* image, int rows, int cols, int channels, const float* kp_xy, int n,
                     int flags = 0) {
    return icpk_describe_points(ctx_, which, image, rows, cols, channels, kp_xy, n, flags);
  }
  int describedToCloud(int which, const uint16_t* depth, int rows, int cols, float fx, float cx, const float R[9],
                       const float t[3]) {
    int32_t n = 0;
    const int rc = icpk_described_to_cloud(ctx_, which, depth, rows, cols, fx, cx, R, t, &n);
    return rc < 0 ? rc : n;
  }
  int matchDescriptors(const icpk_brief_match_params& params, std::vector<DescriptorMatch>* out = nullptr) {
    int32_t m = 0;
    int rc = icpk_match_descriptors(ctx_, &params, out ? &m : nullptr);
    if (rc != ICPK_OK || !out) return rc;
    const size_t cap = (size_t)m + 1;
    std::vector<int32_t> si(cap), ti(cap), H(cap), H2(cap);
    rc = icpk_get_descriptor_matches(ctx_, si.data(), ti.data(), H.data(), H2.data(), &m);
    if (rc != ICPK_OK) return rc;
    out->resize((size_t)m);
    for (int32_t k = 0; k < m; ++k) (*out)[(size_t)k] = DescriptorMatch{si[(size_t)k], ti[(size_t)k], H[(size_t)k], H2[(size_t)k]};
    return ICPK_OK;
  }
  // DBSCAN clustering of the working source (which = 0) or the target (1) (include/icpk.h, K33, THE CLUSTER RULE):
  // labels every point and, unless labelsOnly, keeps the points of the clusters params selects; labelsOnly: the cloud
  // stays as it is and only clusters() changes
  int clusterDbscan(int which, const icpk_cluster_params& params, bool labelsOnly = false, int* n_clusters = nullptr,
                    int* n_noise = nullptr, int* n_out = nullptr) {
    int32_t c = 0, z = 0, o = 0;
    const int rc = icpk_cluster_dbscan(ctx_, which, &params, labelsOnly ? ICPK_CLUSTER_LABELS_ONLY : 0, &c, &z, &o);
    if (rc != ICPK_OK) return rc;
    if (n_clusters) *n_clusters = c;
    if (n_noise) *n_noise = z;
    if (n_out) *n_out = o;
    return rc;
  }
  // what the last clusterDbscan found (icpk_get_clusters)
  struct Clusters {
    std::vector<int32_t> labels, count, nearestCore, outIndex;  // per point
    std::vector<uint8_t> core;
    std::vector<int32_t> sizes, first;  // per cluster
  };
  int clusters(Clusters* out) {
    int32_t n = 0, nc = 0;
    int rc = icpk_get_clusters(ctx_, &n, &nc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != ICPK_OK || !out) return rc;
    out->labels.assign((size_t)n, -1), out->count.assign((size_t)n, 0), out->nearestCore.assign((size_t)n, -1);
    out->outIndex.assign((size_t)n, -1), out->core.assign((size_t)n, 0);
    out->sizes.assign((size_t)nc, 0), out->first.assign((size_t)nc, 0);
    return icpk_get_clusters(ctx_, nullptr, nullptr, out->labels.data(), out->core.data(), out->count.data(),
                             out->nearestCore.data(), out->outIndex.data(), out->sizes.data(), out->first.data());
  }
  // RANSAC plane segmentation of the working source (which = 0) or the target (1) (include/icpk.h, K34, THE PLANE
  // RULE): labels every point with its plane and, unless labelsOnly, keeps what is left when the planes are taken out --
  // or, with keepInliers, the points of the planes (of params.select_plane alone if >= 0); labelsOnly: the cloud stays
  // as it is and only planes() changes
  int segmentPlanes(int which, const icpk_plane_params& params, bool labelsOnly = false, bool keepInliers = false,
                    int* n_planes = nullptr, int* n_unassigned = nullptr, int* n_out = nullptr) {
    int32_t p = 0, u = 0, o = 0;
    const int32_t flags = (labelsOnly ? ICPK_PLANE_LABELS_ONLY : 0) | (keepInliers ? ICPK_PLANE_KEEP_INLIERS : 0);
    const int rc = icpk_segment_planes(ctx_, which, &params, flags, &p, &u, &o);
    if (rc != ICPK_OK) return rc;
    if (n_planes) *n_planes = p;
    if (n_unassigned) *n_unassigned = u;
    if (n_out) *n_out = o;
    return rc;
  }
  // what the last segmentPlanes found (icpk_get_planes)
  struct Planes {
    std::vector<int32_t> labels, outIndex;  // per point
    std::vector<double> model;              // per plane 8: normal, d, centre, curvature
    std::vector<int32_t> info;              // per plane 6: hypothesis, its three samples, RANSAC count, final count
    std::vector<double> sums;               // per plane 9
    int count() const { return (int)(info.size() / 6); }
  };
  int planes(Planes* out) {
    int32_t n = 0, np = 0;
    int rc = icpk_get_planes(ctx_, &n, &np, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != ICPK_OK || !out) return rc;
    out->labels.assign((size_t)n, -1), out->outIndex.assign((size_t)n, -1);
    out->model.assign((size_t)np * 8, 0.0), out->info.assign((size_t)np * 6, 0), out->sums.assign((size_t)np * 9, 0.0);
    return icpk_get_planes(ctx_, nullptr, nullptr, out->labels.data(), out->outIndex.data(), out->model.data(),
                           out->info.data(), out->sums.data());
  }

 private:
  icpk_ctx* ctx_ = nullptr;
};

// The inner loop on explicit clouds (frame-pair formulation of icp.cpp:98-268).
inline int align(Engine& eng, const CloudView& source, const CloudView& target, const AlignParams& params,
                 AlignResult* out) {
  if (!out) return ICPK_E_ARG;
  int rc = icpk_set_target(eng.ctx(), target.x, target.y, target.z, target.n);
  if (rc == ICPK_OK) rc = icpk_set_source(eng.ctx(), source.x, source.y, source.z, source.n);
  if (rc != ICPK_OK) {
    for (int k = 0; k < 16; ++k) out->T[k] = (k % 5 == 0) ? 1.f : 0.f;
    out->status = rc;
    return rc;
  }
  out->status = icpk_align(eng.ctx(), &params, out->T, &out->stats);
  return out->status;
}

// north_star's call surface: align(source, target, params, &result) on the calling thread's
// default Engine (device ICPK_DEVICE or 0; created on first use; one per host thread, as one
// context serialises its calls).  Throws std::runtime_error on first use if no GPU is usable.
inline Engine& defaultEngine() {
  static thread_local Engine eng([] {
    const char* e = std::getenv("ICPK_DEVICE");
    return e ? std::atoi(e) : 0;
  }());
  return eng;
}
inline int align(const CloudView& source, const CloudView& target, const AlignParams& params, AlignResult* out) {
  return align(defaultEngine(), source, target, params, out);
}

// Frame-batch mode (BASELINE config 4): independent pairs, lock-step groups on the
// engine's GPU (icpk_align_batch).  results is resized to pairs.size(); returns the first
// negative status, else the largest.
struct FramePair {
  CloudView source, target;
};
inline int alignBatch(Engine& eng, const std::vector<FramePair>& pairs, const AlignParams& params,
                      std::vector<AlignResult>* results) {
  if (!results) return ICPK_E_ARG;
  const size_t n = pairs.size();
  std::vector<icpk_pair> raw(n);
  for (size_t k = 0; k < n; ++k) {
    raw[k] = icpk_pair{pairs[k].source.x, pairs[k].source.y, pairs[k].source.z, pairs[k].source.n,
                       pairs[k].target.x, pairs[k].target.y, pairs[k].target.z, pairs[k].target.n, nullptr, nullptr};
  }
  std::vector<float> T(16 * (n ? n : 1));
  std::vector<icpk_stats> st(n ? n : 1);
  const int rc = icpk_align_batch(eng.ctx(), (int32_t)n, raw.data(), &params, T.data(), st.data());
  results->resize(n);
  for (size_t k = 0; k < n; ++k) {
    std::memcpy((*results)[k].T, T.data() + 16 * k, sizeof((*results)[k].T));
    (*results)[k].stats = st[k];
    (*results)[k].status = st[k].status;
  }
  return rc;
}

// RCCL collectives of the multi-GPU modes on an Engine (icpk_comm_* of icpk.h): one process or
// host thread + one Engine per GPU; the 128-byte id made by rank 0 (Comm::uniqueId) reaches the
// other ranks by the host's own means.
class Comm {
 public:
  static int uniqueId(unsigned char id[ICPK_COMM_ID_BYTES]) { return icpk_comm_unique_id(id); }
  Comm(Engine& eng, const unsigned char id[ICPK_COMM_ID_BYTES], int rank, int world) : eng_(eng) {
    status = icpk_comm_init_rccl(eng.ctx(), id, rank, world);
  }
  ~Comm() { icpk_comm_destroy(eng_.ctx()); }
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  int rank() const { return icpk_comm_rank(eng_.ctx()); }
  int world() const { return icpk_comm_world(eng_.ctx()); }
  // this rank's block [start, start + count) of n_items
  void partition(int32_t n_items, int32_t* start, int32_t* count) const {
    icpk_comm_partition(n_items, world(), rank(), start, count);
  }
  int broadcastTarget(int root = 0) { return icpk_comm_broadcast_target(eng_.ctx(), root); }
  // ONE large pair, queries sharded over the ranks (collective call): the engine's source is this rank's slice of
  // the queries, the target the same on every rank (broadcastTarget); one in-stream all-reduce per iteration, no host
  // round trip.  Every rank gets the same result.
  int alignQuerySharded(const AlignParams& params, AlignResult* result) {
    if (!result) return ICPK_E_ARG;
    result->status = icpk_align_query_sharded(eng_.ctx(), &params, result->T, &result->stats);
    return result->status;
  }
  // local: this rank's block of results; all: resized to n_total, global pair order
  int gatherResults(const std::vector<AlignResult>& local, int32_t n_total, std::vector<AlignResult>* all) {
    if (!all) return ICPK_E_ARG;
    std::vector<float> Tl(16 * (local.size() ? local.size() : 1)), Ta(16 * (size_t)(n_total > 0 ? n_total : 1)),
        Sa(4 * (size_t)(n_total > 0 ? n_total : 1));
    std::vector<icpk_stats> sl(local.size() ? local.size() : 1);
    for (size_t k = 0; k < local.size(); ++k) {
      std::memcpy(Tl.data() + 16 * k, local[k].T, 16 * sizeof(float));
      sl[k] = local[k].stats;
      sl[k].status = local[k].status;
    }
    const int rc = icpk_comm_gather_results(eng_.ctx(), Tl.data(), sl.data(), (int32_t)local.size(), n_total, Ta.data(),
                                            Sa.data());
    if (rc != ICPK_OK) return rc;
    all->assign((size_t)n_total, AlignResult{});
    for (int32_t k = 0; k < n_total; ++k) {
      AlignResult& r = (*all)[(size_t)k];
      std::memcpy(r.T, Ta.data() + 16 * (size_t)k, 16 * sizeof(float));
      int32_t iv[3];  // (int32 bit patterns in the first three slots of a row)
      std::memcpy(iv, Sa.data() + 4 * (size_t)k, sizeof(iv));
      r.stats.iterations = iv[0];
      r.status = r.stats.status = iv[1];
      r.stats.final_pairs = iv[2];
      r.stats.final_mse = Sa[4 * (size_t)k + 3];
    }
    return ICPK_OK;
  }
  int status = ICPK_OK;

 private:
  Engine& eng_;
};

// SLAM.cpp:553-574 (SLAM.hpp:34): filterDepthImage(image, rgbImage, maxDistance, minDistance) on a
// CV_16UC1 buffer, in place; the colour image is not touched by the reference either
inline int filterDepthImage(Engine& eng, uint16_t* image, int rows, int cols, int maxDistance = 25000,
                            int minDistance = 1000) {
  return icpk_filter_depth_image(eng.ctx(), image, image, rows, cols, maxDistance, minDistance, 1, -1, -1);
}

// pointcloud.cpp:60-98: the 3-D points of a frame's key points (cv::KeyPoint::pt as (x, y) pairs), the cloud that
// findGlobalKeyPointAssociations below takes as dataKeypoints.  Host only.  out_xyz: n x 3 floats, kept: n ints or null.
inline int backprojectKeyPoints(const uint16_t* depth, int rows, int cols, const float* kp_xy, int n, float* out_xyz,
                                int32_t* kept = nullptr, float fx = ICPK_FX, float cx = ICPK_CX) {
  return icpk_backproject_keypoints(depth, rows, cols, kp_xy, n, fx, cx, out_xyz, kept);
}

// icp.cpp:488-515: data key points vs map key points.  errors / associations are rebuilt (pairs of
// (query index, nearest index) in query order), nonAssociations is appended to; an empty map
// returns ICPK_W_EMPTY_MAP and touches nothing (icp.cpp:490-491).
inline int findGlobalKeyPointAssociations(Engine& eng, const CloudView& dataKeypoints, const CloudView& mapKeypoints,
                                          std::vector<float>& errors,
                                          std::vector<std::pair<int32_t, int32_t>>& associations,
                                          std::vector<int32_t>& nonAssociations,
                                          float maxDistance = ICPK_MAX_NN_KEYPOINT_DISTANCE) {
  if (mapKeypoints.n <= 0) return ICPK_W_EMPTY_MAP;
  int rc = icpk_set_target(eng.ctx(), mapKeypoints.x, mapKeypoints.y, mapKeypoints.z, mapKeypoints.n);
  if (rc == ICPK_OK) rc = icpk_set_source(eng.ctx(), dataKeypoints.x, dataKeypoints.y, dataKeypoints.z, dataKeypoints.n);
  if (rc != ICPK_OK) return rc;
  const size_t nq = (size_t)(dataKeypoints.n > 0 ? dataKeypoints.n : 0), had = nonAssociations.size();
  std::vector<int32_t> q(nq + 1), t(nq + 1);
  std::vector<float> d(nq + 1);
  nonAssociations.resize(had + nq);
  int32_t na = 0, nr = (int32_t)had;
  rc = icpk_associate_keypoints(eng.ctx(), ICPK_NN_GRID, maxDistance, q.data(), t.data(), d.data(), &na,
                                nonAssociations.data(), (int32_t)nonAssociations.size(), &nr);
  if (rc != ICPK_OK) {
    nonAssociations.resize(had);
    return rc;
  }
  nonAssociations.resize((size_t)nr);
  errors.assign(d.begin(), d.begin() + na);
  associations.clear();
  for (int32_t k = 0; k < na; ++k) associations.emplace_back(q[(size_t)k], t[(size_t)k]);
  return ICPK_OK;
}

// icp.cpp:640-653
inline void makeRotationMatrix(float x, float y, float z, float out[9]) { icpk_make_rotation_matrix(x, y, z, out); }

// icp.cpp:622-638: (mean error)^2, sequential float accumulation like the reference
inline float meanSquareError(const std::vector<float>& errors) {
  float s = 0.f;
  for (float e : errors) s += e;
  if (!errors.empty()) {
    s /= (float)errors.size();
    s = (float)((double)s * (double)s);
  }
  return s;
}

// quaternion.cpp:23-79 + SLAM.cpp:613-636: rotation matrix -> roll/pitch/yaw degrees
inline void toEulerianAngle(const float rotation[9], float& x, float& y, float& z) {
  float q[4], e[3];
  icpk_matrix_to_quaternion(rotation, q);
  icpk_quaternion_to_euler(q, e);
  x = e[0];
  y = e[1];
  z = e[2];
}

// The state icp.cpp keeps at file scope (cameraRotation, lastRotation,
// cameraPosition, lastTranslation, icp.cpp:22-25) plus the per-frame procedure of
// getTransformation, with the accumulated key-point map replaced by the previous
// frame's full cloud (the association the reference keeps commented at
// icp.cpp:253).  Depth buffers are CV_16UC1 row-major (rows x cols uint16).
class Tracker {
 public:
  explicit Tracker(Engine& eng, float fx = ICPK_FX, float cx = ICPK_CX) : eng_(eng), fx_(fx), cx_(cx) { reset(); }
  Engine& engine() const { return eng_; }

  void reset() {
    static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(cameraRotation, I, sizeof(I));  // icp.cpp:49
    std::memcpy(lastRotation, I, sizeof(I));    // icp.cpp:50
    cameraPosition[0] = cameraPosition[1] = cameraPosition[2] = 5.f;   // icp.cpp:53
    lastTranslation[0] = lastTranslation[1] = lastTranslation[2] = 0.f;  // icp.cpp:54
    params = AlignParams();
    params.solve = ICPK_SOLVE_REFERENCE;
  }

  // Same meaning as icp::getTransformation(data, previous, ..., maxIterations, threshold):
  // returns the status, writes the 4x4 into T (row-major).  `data` is the current
  // frame, `previous` the frame before it.  previous == nullptr: the frame that was `data` in the
  // last call -- what SLAM.cpp hands back (SLAM.cpp:305, previous = filtered.clone()); it has stayed
  // on the device, so only the new frame is uploaded (same results as passing it again).
  int getTransformation(const uint16_t* data, const uint16_t* previous, int rows, int cols, int maxIterations,
                        float threshold, float T[16]) {
    icpk_ctx* c = eng_.ctx();
    // icp.cpp:38-39: back-project both frames; :58-59 / :70-71: rotate by the camera
    // rotation, translate by the camera position (both clouds get the current pose)
    // -- one call: both uploads, 3 launches (5 with filterFrames), one host wait; the posed source is the
    // starting point of the alignment
    int rc = icpk_backproject_pair(c, data, previous, rows, cols, fx_, cx_, nullptr, cameraRotation, cameraPosition,
                                   filterFrames ? 1 : 0, maxDistance, minDistance, 1, -1, -1, nullptr, nullptr);
    if (rc != ICPK_OK) return rc;
    if (outlierFilter) {  // strays go before anything reads neighbourhoods (target first, then source)
      rc = eng_.removeOutliers(1, outlierSetting);
      if (rc == ICPK_OK) rc = eng_.removeOutliers(0, outlierSetting);
      if (rc != ICPK_OK) return rc;
    }
    if (voxelLeaf > 0.f) {  // thin both clouds by space before the loop sees them (target first, then source)
      rc = eng_.voxelDownsample(1, voxelLeaf, voxelMode);
      if (rc == ICPK_OK) rc = eng_.voxelDownsample(0, voxelLeaf, voxelMode);
      if (rc != ICPK_OK) return rc;
    }
    params.max_iterations = maxIterations;
    params.threshold = threshold;
    std::memcpy(params.last_rotation, lastRotation, sizeof(lastRotation));
    std::memcpy(params.last_translation, lastTranslation, sizeof(lastTranslation));
    icpk_stats st;
    rc = icpk_align(c, &params, T, &st);
    if (rc < 0) return rc;
    lastStats = st;
    // pose bookkeeping exactly as the loop does it (icp.cpp:235-237, 245-246)
    int32_t niter = 0;
    std::vector<float> R((size_t)maxIterations * 9 + 9), t((size_t)maxIterations * 3 + 3);
    icpk_get_trace(c, &niter, R.data(), t.data(), nullptr, nullptr);
    for (int i = 0; i < niter; ++i) {
      float Rinv[9], prod[9];
      invert3(R.data() + 9 * i, Rinv);
      mul3(cameraRotation, Rinv, prod);  // cameraRotation *= R
      std::memcpy(cameraRotation, prod, sizeof(prod));
      for (int k = 0; k < 3; ++k) cameraPosition[k] -= t[3 * i + k];  // cameraPosition -= offset
    }
    // icp.cpp:260-261: lastTranslation = -offset; lastRotation = R (the outer R: identity
    // on the normal path because the inner R shadows it)
    for (int k = 0; k < 3; ++k) lastTranslation[k] = -T[4 * k + 3];
    if (rc != ICPK_W_TOO_FEW_PAIRS) {
      static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      std::memcpy(lastRotation, I, sizeof(I));
    }
    return rc;
  }

  // SLAM.cpp:229 filters every frame before it reaches getTransformation; set this to have the filter run
  // on the device inside the same call instead (SLAM.hpp:15-16 limits)
  bool filterFrames = false;
  int maxDistance = 25000, minDistance = 1000;
  // > 0: both clouds of every frame pair are voxel-grid downsampled with this leaf (metres) between back-projection
  // and alignment (icpk_voxel_downsample); 0, the default: the calls are exactly those made without it
  float voxelLeaf = 0.f;
  int voxelMode = ICPK_VOXEL_CENTROID;
  // true: both clouds of every frame pair go through icpk_remove_outliers with outlierSetting between back-projection
  // and the voxel downsample; false, the default: the calls are exactly those made without it
  bool outlierFilter = false;
  icpk_outlier_filter outlierSetting{ICPK_FILTER_STATISTICAL, 16, 2.0f, 0.05f, 5};
  float cameraRotation[9];
  float lastRotation[9];
  float cameraPosition[3];
  float lastTranslation[3];
  AlignParams params;
  icpk_stats lastStats{};

 private:
  static void mul3(const float A[9], const float B[9], float C[9]) {  // CV_32F product, double accumulate
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (double)A[3 * r + k] * (double)B[3 * k + cc];
        C[3 * r + cc] = (float)s;
      }
  }
  static void invert3(const float m[9], float out[9]) {  // icp.cpp:235 Mat::inv on a 3x3
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

#include "icp_map.hpp"
#include "icp_pose_graph.hpp"
