// icp_tsdf.hpp -- C++ host side of the TSDF volume (icpk_tsdf_* of include/icpk.h, K19 - K21).  Include it next to
// icp_align.hpp.
//
//   * icp::TsdfVolume -- the dense volume of truncated signed distances an Engine's context owns: posed depth frames
//                        are fused into it on the GPU (integrate), the surface comes back as points with normals
//                        (surface) or becomes the Engine's target for scan-to-model alignment (toTarget).  An Engine
//                        holds one volume: constructing another replaces it.  raycast gives the surface visible from
//                        one pose as vertex and normal maps (K20); raycastToTarget makes it the Engine's target.
//                        alignProjective / projectiveAssociate pair a level of the Engine's depth pyramid with those maps
//                        pixel by pixel and refine a pose against the model (K25).  alignSdf / sdfAssociate refine
//                        it against the distance field itself, with no ray cast (K29).
//                        extractMesh / getMesh give the surface as a triangle mesh (K21); setPlanes restores a saved
//                        model.  shift / extractLeaving / getBox let the volume follow the camera (K23): the box
//                        moves by whole voxels, what is about to leave it is listed first.  computeEsdf / esdfPlanes /
//                        queryEsdf give the exact Euclidean distance map of the volume (K31): how far a voxel, or
//                        any point, is from the nearest obstacle.
//   * icp::FernDatabase -- the fern keyframe database of an Engine's context (icpk_fern_*, K27): every tracked frame's
//                        coarse pyramid level is encoded, looked up and harvested on the GPU (process); a tracker
//                        that has lost the camera restarts from the nearest keyframes' poses (TsdfVolume::relocalise).
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "icp_align.hpp"

namespace icp {

// the surface list of one extraction: structure of arrays, ordered by voxel, then axis
struct TsdfSurface {
  std::vector<float> x, y, z, nx, ny, nz, intensity;
  std::vector<int32_t> voxel;  // linear index of the voxel the crossing starts at
  std::vector<uint8_t> axis;   // 0, 1, 2: towards its +1 neighbour along x, y, z
  int32_t noNormal = 0;        // crossings not listed: an end without a gradient
  size_t size() const { return x.size(); }
};

// the maps of one ray cast: rows x cols entries each, row-major; a pixel without a hit holds 0 everywhere
struct TsdfRaycast {
  int rows = 0, cols = 0;
  std::vector<float> x, y, z, nx, ny, nz, depth, intensity;
  int32_t hits = 0;      // pixels that hold a hit (depth > 0)
  int32_t noNormal = 0;  // crossings not listed: no normal where the ray met the surface
};

// the triangle mesh of one extraction: vertices ordered by owner voxel, then edge type; a vertex without a normal holds
// (0, 0, 0)
struct TsdfMesh {
  std::vector<float> x, y, z, nx, ny, nz, intensity;
  std::vector<int32_t> voxel;      // linear index of the voxel that owns the vertex's edge
  std::vector<uint8_t> edge;       // the edge's type 1 .. 7: bit 0 +x, bit 1 +y, bit 2 +z
  std::vector<int32_t> triangles;  // three vertex indices each
  int32_t noNormal = 0;            // vertices listed without a normal
  size_t vertices() const { return x.size(); }
  size_t size() const { return triangles.size() / 3; }
};

// K27: the fern keyframe database of an Engine's context (icpk_fern_* of include/icpk.h, THE FERN RULE): the codes on
// the device, the poses on the host beside them.  An Engine holds one database: constructing another replaces it.
struct FernMatches {
  std::vector<int32_t> index, diss;  // the nearest keyframes in ascending (diss, index) order
  int32_t valid = 0;                 // V of the frame
  int32_t added = -1;                // the keyframe the frame became, or -1
};

class FernDatabase {
 public:
  static icpk_fern_params defaults() {
    icpk_fern_params p;
    icpk_default_fern_params(&p);
    return p;
  }
  // rows, cols: the shape of level p.level of the pyramids the Engine will hold.  Throws std::runtime_error when the
  // parameters are refused or the memory is not there
  FernDatabase(Engine& eng, const icpk_fern_params& p, int rows, int cols) : eng_(eng), p_(p) {
    const int rc = icpk_fern_create(eng_.ctx(), &p_, rows, cols);
    if (rc != ICPK_OK) throw std::runtime_error("icpk_fern_create failed (status " + std::to_string(rc) + "): " + eng_.last_error());
  }
  FernDatabase(const FernDatabase&) = delete;
  FernDatabase& operator=(const FernDatabase&) = delete;
  ~FernDatabase() { icpk_fern_destroy(eng_.ctx()); }

  const icpk_fern_params& params() const { return p_; }
  size_t words() const { return (size_t)p_.n_ferns / 8; }
  int size() { return icpk_fern_count(eng_.ctx()); }
  int reset() { return icpk_fern_reset(eng_.ctx()); }
  // the database's level of the Engine's resident pyramid into the current code; code: words() entries
  int encode(std::vector<uint32_t>* code = nullptr, int32_t* valid = nullptr) {
    if (code) code->assign(words(), 0u);
    return icpk_fern_encode(eng_.ctx(), code ? code->data() : nullptr, valid);
  }
  int query(int k, FernMatches& m) {
    int32_t n = 0;
    m.index.assign(ICPK_FERN_MAX_K, 0), m.diss.assign(ICPK_FERN_MAX_K, 0);
    const int rc = icpk_fern_query(eng_.ctx(), k, m.index.data(), m.diss.data(), &n);
    m.index.resize(rc == ICPK_OK ? (size_t)n : 0), m.diss.resize(rc == ICPK_OK ? (size_t)n : 0);
    return rc;
  }
  int add(const double* pose, int32_t* index = nullptr) { return icpk_fern_add(eng_.ctx(), pose, index); }
  // the per-frame call: encode, search and -- with a pose (16 doubles, row-major), when the harvest rule says so -- append
  int process(const double* pose, int k, FernMatches& m) {
    int32_t n = 0;
    m.index.assign(ICPK_FERN_MAX_K, 0), m.diss.assign(ICPK_FERN_MAX_K, 0);
    m.valid = 0, m.added = -1;
    const int rc = icpk_fern_process(eng_.ctx(), pose, k, m.index.data(), m.diss.data(), &n, &m.valid, &m.added);
    m.index.resize(rc == ICPK_OK ? (size_t)n : 0), m.diss.resize(rc == ICPK_OK ? (size_t)n : 0);
    return rc;
  }
  int addCode(const uint32_t* code, const double* pose, int32_t* index = nullptr) {
    return icpk_fern_add_code(eng_.ctx(), code, pose, index);
  }
  // one keyframe back: code (words() entries) and pose (16 doubles), either may be null
  int keyframe(int index, uint32_t* code, double* pose) { return icpk_fern_get_keyframe(eng_.ctx(), index, code, pose); }

 private:
  Engine& eng_;
  icpk_fern_params p_;
};

class TsdfVolume {
 public:
  static icpk_tsdf_params defaults() {
    icpk_tsdf_params p;
    icpk_default_tsdf_params(&p);
    return p;
  }
  // fx, cx: the depth camera's intrinsics (cx and fx serve both axes, as in Engine::backproject).  Throws
  // std::runtime_error when the parameters are refused or the memory is not there
  TsdfVolume(Engine& eng, const icpk_tsdf_params& p, float fx, float cx) : eng_(eng), p_(p), fx_(fx), cx_(cx) {
    const int rc = icpk_tsdf_create(eng_.ctx(), &p_);
    if (rc != ICPK_OK) throw std::runtime_error("icpk_tsdf_create failed (status " + std::to_string(rc) + "): " + eng_.last_error());
  }
  TsdfVolume(const TsdfVolume&) = delete;
  TsdfVolume& operator=(const TsdfVolume&) = delete;
  ~TsdfVolume() { icpk_tsdf_release(eng_.ctx()); }

  const icpk_tsdf_params& params() const { return p_; }
  size_t voxels() const { return (size_t)p_.dims[0] * p_.dims[1] * p_.dims[2]; }

  // one rows x cols frame at the camera-to-world pose (16 doubles, row-major); intensity: rows x cols floats on a colour
  // volume, else null.  nUpdated (optional): the voxels written.  Returns a status of icpk.h
  int integrate(const uint16_t* depth, int rows, int cols, const double* pose, const float* intensity = nullptr,
                int32_t* nUpdated = nullptr) {
    return icpk_tsdf_integrate(eng_.ctx(), depth, intensity, rows, cols, fx_, cx_, pose, nUpdated);
  }
  // the frame Engine's backproject_pair path has just left on the device, without a second upload
  int integrateResident(int rows, int cols, const double* pose, const float* intensity = nullptr, int32_t* nUpdated = nullptr) {
    return icpk_tsdf_integrate(eng_.ctx(), nullptr, intensity, rows, cols, fx_, cx_, pose, nUpdated);
  }
  // frames and their poses (16 doubles each), e.g. PoseGraph::poses()
  int integrateAll(const std::vector<const uint16_t*>& depths, int rows, int cols, const std::vector<double>& poses) {
    if (poses.size() != 16 * depths.size()) return ICPK_E_ARG;
    for (size_t k = 0; k < depths.size(); ++k)
      if (int rc = integrate(depths[k], rows, cols, poses.data() + 16 * k)) return rc;
    return ICPK_OK;
  }
  // K30 -- the inverse of integrate: the frame taken out again at the pose it was fused at (exact on voxels the frame
  // alone had written, up to rounding elsewhere, no inverse on voxels that reached max_weight)
  int deintegrate(const uint16_t* depth, int rows, int cols, const double* pose, const float* intensity = nullptr,
                  int32_t* nUpdated = nullptr) {
    return icpk_tsdf_deintegrate(eng_.ctx(), depth, intensity, rows, cols, fx_, cx_, pose, nUpdated);
  }
  // signed updates in one pass over the volume: op k integrates (sign +1) or de-integrates (-1) depths[ops[k].frame] at
  // ops[k].pose; at most ICPK_TSDF_MAX_OPS ops over at most as many frames.  intensities: one image per frame on a
  // colour volume, else empty.  nUpdated (optional): the voxels every op wrote
  int apply(const std::vector<const uint16_t*>& depths, int rows, int cols, const std::vector<icpk_tsdf_op>& ops,
            const std::vector<const float*>& intensities = {}, std::vector<int64_t>* nUpdated = nullptr) {
    if (!intensities.empty() && intensities.size() != depths.size()) return ICPK_E_ARG;
    if (nUpdated) nUpdated->assign(ops.size(), 0);
    return icpk_tsdf_apply(eng_.ctx(), (int32_t)depths.size(), depths.data(), intensities.empty() ? nullptr : intensities.data(),
                           rows, cols, fx_, cx_, (int32_t)ops.size(), ops.data(), nUpdated ? nUpdated->data() : nullptr);
  }
  // frames fused at oldPoses moved to newPoses (16 doubles each, e.g. PoseGraph::poses() after a loop closure): each is
  // taken out at its old pose and put in at its new one, ICPK_TSDF_MAX_OPS / 2 frames per pass over the volume, every
  // frame uploaded once.  nUpdated (optional): per frame the voxels removed, then the voxels added
  int refuse(const std::vector<const uint16_t*>& depths, int rows, int cols, const std::vector<double>& oldPoses,
             const std::vector<double>& newPoses, const std::vector<const float*>& intensities = {},
             std::vector<int64_t>* nUpdated = nullptr) {
    const size_t n = depths.size(), batch = ICPK_TSDF_MAX_OPS / 2;
    if (oldPoses.size() != 16 * n || newPoses.size() != 16 * n || (!intensities.empty() && intensities.size() != n)) return ICPK_E_ARG;
    if (nUpdated) nUpdated->assign(2 * n, 0);
    for (size_t lo = 0; lo < n; lo += batch) {
      const size_t m = std::min(batch, n - lo);
      std::vector<icpk_tsdf_op> ops(2 * m);
      for (size_t k = 0; k < m; ++k) {
        ops[k].sign = -1, ops[m + k].sign = +1;
        ops[k].frame = ops[m + k].frame = (int32_t)k;
        std::copy_n(oldPoses.data() + 16 * (lo + k), 16, ops[k].pose);
        std::copy_n(newPoses.data() + 16 * (lo + k), 16, ops[m + k].pose);
      }
      const std::vector<const uint16_t*> d(depths.begin() + lo, depths.begin() + lo + m);
      std::vector<const float*> c;
      if (!intensities.empty()) c.assign(intensities.begin() + lo, intensities.begin() + lo + m);
      std::vector<int64_t> wrote;
      if (int rc = apply(d, rows, cols, ops, c, &wrote)) return rc;
      for (size_t k = 0; k < m && nUpdated; ++k) (*nUpdated)[2 * (lo + k)] = wrote[k], (*nUpdated)[2 * (lo + k) + 1] = wrote[m + k];
    }
    return ICPK_OK;
  }
  // the zero crossings between voxels of weight >= minWeight; the list also stays on the device for toTarget()
  int surface(TsdfSurface& s, int minWeight = 1) {
    int32_t n = 0;
    int rc = icpk_tsdf_extract_surface(eng_.ctx(), minWeight, &n, &s.noNormal);
    if (rc) return rc;
    for (std::vector<float>* v : {&s.x, &s.y, &s.z, &s.nx, &s.ny, &s.nz, &s.intensity}) v->assign((size_t)n, 0.f);
    s.voxel.assign((size_t)n, 0);
    s.axis.assign((size_t)n, 0);
    return icpk_tsdf_get_surface(eng_.ctx(), s.x.data(), s.y.data(), s.z.data(), s.nx.data(), s.ny.data(), s.nz.data(),
                                 s.intensity.data(), s.voxel.data(), s.axis.data());
  }
  // the last extraction's list becomes the Engine's target, with its normals (and colours): device to device.
  // ICPK_E_EMPTY_TARGET (the target stays) when the list is empty
  int toTarget() { return icpk_tsdf_surface_to_target(eng_.ctx()); }
  // the ray cast's parameters with this volume's intrinsics (z_near 0.25, z_far 6, step 0: trunc / 2, min_weight 1)
  icpk_tsdf_raycast_params raycastDefaults(int rows, int cols) const {
    icpk_tsdf_raycast_params r;
    icpk_default_tsdf_raycast_params(&r);
    r.rows = rows, r.cols = cols, r.fx = fx_, r.cx = cx_;
    return r;
  }
  // the volume seen from the camera-to-world pose (16 doubles, row-major); the maps stay on the device.  nHits,
  // nNoNormal (optional): the counts -- with both null the call does not wait
  int raycast(const icpk_tsdf_raycast_params& r, const double* pose, int32_t* nHits = nullptr, int32_t* nNoNormal = nullptr) {
    const int rc = icpk_tsdf_raycast(eng_.ctx(), &r, pose, nHits, nNoNormal);
    if (rc == ICPK_OK) rayRows_ = r.rows, rayCols_ = r.cols;
    return rc;
  }
  // the maps of the last ray cast (the intensity plane stays 0 on a volume without colour)
  int getRaycast(TsdfRaycast& m) {
    const size_t n = (size_t)rayRows_ * rayCols_;
    m.rows = rayRows_, m.cols = rayCols_;
    for (std::vector<float>* v : {&m.x, &m.y, &m.z, &m.nx, &m.ny, &m.nz, &m.depth, &m.intensity}) v->assign(n, 0.f);
    const bool color = (p_.flags & ICPK_TSDF_COLOR) != 0;
    const int rc = icpk_tsdf_get_raycast(eng_.ctx(), m.x.data(), m.y.data(), m.z.data(), m.nx.data(), m.ny.data(), m.nz.data(),
                                         m.depth.data(), color ? m.intensity.data() : nullptr);
    if (rc) return rc;
    m.hits = 0;
    for (float d : m.depth) m.hits += d > 0.f;
    return ICPK_OK;
  }
  // the last ray cast's hits become the Engine's target, with their normals (and colours), in row-major pixel order:
  // device to device.  ICPK_E_EMPTY_TARGET (the target stays) without a hit
  int raycastToTarget() { return icpk_tsdf_raycast_to_target(eng_.ctx()); }
  // projective frame-to-model alignment (K25): the parameters with this volume's intrinsics as the LEVEL-0 ones
  // (10 iterations, max_dist 0.5, the normal gate off, min_pairs 6)
  icpk_projective_params projectiveDefaults(int level = 0) const {
    icpk_projective_params p;
    icpk_default_projective_params(&p);
    p.level = level, p.fx = fx_, p.cx = cx_;
    return p;
  }
  // a level of the Engine's resident depth pyramid (Engine::buildDepthPyramid) against the maps of the last ray cast,
  // from the camera-to-world estimate poseIn (16 doubles, row-major) to poseOut; nothing of the Engine's clouds is
  // touched.  Returns ICPK_OK, ICPK_W_TOO_FEW_PAIRS, ICPK_W_DEGENERATE or a negative status
  int alignProjective(const icpk_projective_params& p, const double* poseIn, double* poseOut,
                      icpk_projective_result* result = nullptr) {
    return icpk_align_projective(eng_.ctx(), &p, poseIn, poseOut, result);
  }
  // K27, for a tracker that has lost the camera: the frame of the Engine's resident pyramid is looked up in `db`
  // (FernDatabase::process without a pose) and, for each of its k nearest keyframes in order, the volume is ray-cast at
  // the keyframe's pose (r: the ray cast's parameters for level p.level) and alignProjective starts from it.  The first
  // keyframe whose alignment ends with ICPK_OK, at least minPairs pairs and a mean distance of at most maxMeanDist
  // wins: *keyframe is its index, poseOut its refined pose.  None (or a frame with fewer than min_valid valid ferns):
  // *keyframe = -1 and poseOut is untouched.  Returns ICPK_OK or a negative status
  int relocalise(FernDatabase& db, int k, const icpk_tsdf_raycast_params& r, const icpk_projective_params& p,
                 double* poseOut, int32_t* keyframe, icpk_projective_result* result = nullptr, int64_t minPairs = 0,
                 double maxMeanDist = 1e300) {
    *keyframe = -1;
    FernMatches m;
    int rc = db.process(nullptr, k, m);
    if (rc != ICPK_OK || m.valid < db.params().min_valid) return rc;
    for (size_t c = 0; c < m.index.size(); ++c) {
      double start[16], found[16];
      icpk_projective_result res;
      int32_t hits = 0;
      if ((rc = db.keyframe(m.index[c], nullptr, start)) != ICPK_OK) return rc;
      if ((rc = raycast(r, start, &hits)) != ICPK_OK) return rc;
      if (hits < p.min_pairs) continue;
      if ((rc = alignProjective(p, start, found, &res)) < 0) return rc;
      if (rc != ICPK_OK || res.count < minPairs || !(res.mean_dist <= maxMeanDist)) continue;
      for (int i = 0; i < 16; ++i) poseOut[i] = found[i];
      if (result) *result = res;
      *keyframe = m.index[c];
      return ICPK_OK;
    }
    return ICPK_OK;
  }
  // per pixel of that level at `pose`: the view pixel it pairs with or its ICPK_PROJ_* code, and the distance (0
  // without a pair); both vectors are sized to the level
  int projectiveAssociate(const icpk_projective_params& p, const double* pose, std::vector<int32_t>& pixel,
                          std::vector<float>& dist) {
    int32_t rows = 0, cols = 0;
    if (icpk_depth_pyramid_shape(eng_.ctx(), p.level, &rows, &cols) != ICPK_OK)
      return icpk_projective_associate(eng_.ctx(), &p, pose, nullptr, nullptr);  // (its own refusal)
    pixel.assign((size_t)rows * cols, 0);
    dist.assign((size_t)rows * cols, 0.f);
    return icpk_projective_associate(eng_.ctx(), &p, pose, pixel.data(), dist.data());
  }
  // K26: the colour gradients of the last ray cast (a colour volume), kept on the device behind the maps; no host wait.
  // gx / gy / gz (any may be null): rows x cols floats of that ray cast
  int raycastColorGradients(float radius, int minNeighbors = 4, int flags = 0) {
    return icpk_tsdf_raycast_color_gradients(eng_.ctx(), radius, minNeighbors, flags);
  }
  int getRaycastColorGradients(float* gx, float* gy, float* gz) {
    return icpk_tsdf_get_raycast_color_gradients(eng_.ctx(), gx, gy, gz);
  }
  // alignProjective with K17's photometric term beside every pair: it needs Engine::setPyramidIntensity and
  // raycastColorGradients for the current ray cast.  color null: the defaults.  projectiveTrace reads its iterations
  int alignProjectiveColored(const icpk_projective_params& p, const icpk_projective_color_params* color, const double* poseIn,
                             double* poseOut, icpk_projective_result* result = nullptr) {
    return icpk_align_projective_colored(eng_.ctx(), &p, color, poseIn, poseOut, result);
  }
  // the iterations the last alignProjective / alignProjectiveColored evaluated: E_k, the sums and count at E_k, the status
  std::vector<icpk_projective_iter> projectiveTrace() {
    std::vector<icpk_projective_iter> t(ICPK_PROJECTIVE_MAX_ITERATIONS);
    const int n = icpk_get_projective_trace(eng_.ctx(), t.data(), (int32_t)t.size());
    t.resize(n > 0 ? (size_t)n : 0);
    return t;
  }
  // K29, the frame aligned directly against the distance field, with no ray cast: the parameters with this volume's
  // intrinsics as the LEVEL-0 ones (10 iterations, max_abs_tsdf 1, min_weight 1, the normal gate off, min_pairs 6)
  icpk_sdf_params sdfDefaults(int level = 0) const {
    icpk_sdf_params p;
    icpk_default_sdf_params(&p);
    p.level = level, p.fx = fx_, p.cx = cx_;
    return p;
  }
  // a level of the Engine's resident depth pyramid against the volume's own planes at its current origin, from the
  // camera-to-world estimate poseIn (16 doubles, row-major) to poseOut; the maps, the lists, the projective trace and
  // the Engine's clouds are not touched.  Returns ICPK_OK, ICPK_W_TOO_FEW_PAIRS, ICPK_W_DEGENERATE or a negative status
  int alignSdf(const icpk_sdf_params& p, const double* poseIn, double* poseOut, icpk_projective_result* result = nullptr) {
    return icpk_align_sdf(eng_.ctx(), &p, poseIn, poseOut, result);
  }
  // one evaluation at `pose`: the ICPK_NP2L sums and the accepted pixels
  int sdfReduce(const icpk_sdf_params& p, const double* pose, double* sums, int64_t* count) {
    return icpk_sdf_reduce(eng_.ctx(), &p, pose, sums, count);
  }
  // per pixel of that level at `pose`: the linear index of the cell it lands in or its ICPK_SDF_* code, and the signed
  // distance there (0 when rejected); both vectors are sized to the level
  int sdfAssociate(const icpk_sdf_params& p, const double* pose, std::vector<int32_t>& cell, std::vector<float>& value) {
    int32_t rows = 0, cols = 0;
    if (icpk_depth_pyramid_shape(eng_.ctx(), p.level, &rows, &cols) != ICPK_OK)
      return icpk_sdf_associate(eng_.ctx(), &p, pose, nullptr, nullptr);  // (its own refusal)
    cell.assign((size_t)rows * cols, 0);
    value.assign((size_t)rows * cols, 0.f);
    return icpk_sdf_associate(eng_.ctx(), &p, pose, cell.data(), value.data());
  }
  // the iterations the last alignSdf evaluated: E_k, the sums and count at E_k, the status
  std::vector<icpk_projective_iter> sdfTrace() {
    std::vector<icpk_projective_iter> t(ICPK_PROJECTIVE_MAX_ITERATIONS);
    const int n = icpk_get_sdf_trace(eng_.ctx(), t.data(), (int32_t)t.size());
    t.resize(n > 0 ? (size_t)n : 0);
    return t;
  }
  // the surface as a triangle mesh over the cells whose eight voxels have weight >= minWeight; it stays on the device
  // for getMesh.  Any count may be null
  int extractMesh(int minWeight = 1, int32_t* nVertices = nullptr, int32_t* nTriangles = nullptr, int32_t* nNoNormal = nullptr) {
    int32_t nv = 0, nt = 0, nn = 0;
    const int rc = icpk_tsdf_extract_mesh(eng_.ctx(), minWeight, &nv, &nt, &nn);
    if (rc) return rc;
    meshVertices_ = nv, meshTriangles_ = nt, meshNoNormal_ = nn;
    if (nVertices) *nVertices = nv;
    if (nTriangles) *nTriangles = nt;
    if (nNoNormal) *nNoNormal = nn;
    return ICPK_OK;
  }
  // the mesh of the last extractMesh (ICPK_E_NOT_SET before it)
  int getMesh(TsdfMesh& m) {
    const size_t n = (size_t)meshVertices_;
    for (std::vector<float>* v : {&m.x, &m.y, &m.z, &m.nx, &m.ny, &m.nz, &m.intensity}) v->assign(n, 0.f);
    m.voxel.assign(n, 0);
    m.edge.assign(n, 0);
    m.triangles.assign(3 * (size_t)meshTriangles_, 0);
    m.noNormal = meshNoNormal_;
    return icpk_tsdf_get_mesh(eng_.ctx(), m.x.data(), m.y.data(), m.z.data(), m.nx.data(), m.ny.data(), m.nz.data(),
                              m.intensity.data(), m.voxel.data(), m.edge.data(), m.triangles.data());
  }
  // the counterpart of planes(): voxels() entries each, x fastest; intensity exactly on a colour volume.  Drops the surface
  // list, the maps and the mesh
  int setPlanes(const float* tsdf, const uint16_t* weight, const float* intensity = nullptr) {
    const int rc = icpk_tsdf_set(eng_.ctx(), tsdf, weight, intensity);
    if (rc == ICPK_OK) forget();
    return rc;
  }
  // the planes, voxels() entries each, x fastest; any pointer may be null
  int planes(float* tsdf, uint16_t* weight, float* intensity = nullptr) { return icpk_tsdf_get(eng_.ctx(), tsdf, weight, intensity); }
  int reset() {
    forget();
    const int rc = icpk_tsdf_reset(eng_.ctx());
    if (rc == ICPK_OK) refresh();  // (the box is back where it was created)
    return rc;
  }
  // the moving volume (K23).  shift: the new voxel v holds the old voxel v + s (three ints), what falls off is gone, the
  // origin follows (params(), total()); drops the surface list, the maps and the mesh.  No host wait
  int shift(const int32_t s[3]) {
    const int rc = icpk_tsdf_shift(eng_.ctx(), s);
    if (rc != ICPK_OK) return rc;
    if (s[0] || s[1] || s[2]) forget();
    return refresh();
  }
  // the crossings a shift by s would lose, as surface() lists them (voxel: the index before the shift); the list also
  // replaces the one on the device (toTarget).  Call it before shift(s)
  int extractLeaving(TsdfSurface& out, const int32_t s[3], int minWeight = 1) {
    int32_t n = 0;
    int rc = icpk_tsdf_extract_leaving(eng_.ctx(), minWeight, s, &n, &out.noNormal);
    if (rc) return rc;
    for (std::vector<float>* v : {&out.x, &out.y, &out.z, &out.nx, &out.ny, &out.nz, &out.intensity}) v->assign((size_t)n, 0.f);
    out.voxel.assign((size_t)n, 0);
    out.axis.assign((size_t)n, 0);
    return icpk_tsdf_get_surface(eng_.ctx(), out.x.data(), out.y.data(), out.z.data(), out.nx.data(), out.ny.data(),
                                 out.nz.data(), out.intensity.data(), out.voxel.data(), out.axis.data());
  }
  // the cumulative shift since the volume was created or reset (params().origin is the origin it amounts to)
  const int64_t* total() const { return total_; }
  // the planes of the sub-box lo <= (x, y, z) < hi, x fastest, (hi - lo) entries per axis; any pointer may be null
  int getBox(const int32_t lo[3], const int32_t hi[3], float* tsdf, uint16_t* weight, float* intensity = nullptr) {
    return icpk_tsdf_get_box(eng_.ctx(), lo, hi, tsdf, weight, intensity);
  }
  // K31 -- the exact Euclidean distance map of the volume as it stands: per voxel the signed squared distance, in voxels,
  // to the nearest voxel of the other kind, exact up to p.max_distance and ICPK_ESDF_FAR beyond.  It stays on the device,
  // a snapshot: integrate leaves it as it was (stale); setPlanes, shift, reset and the destructor drop it
  static icpk_esdf_params esdfDefaults() {
    icpk_esdf_params p;
    icpk_default_esdf_params(&p);
    return p;
  }
  // counts (optional): voxels of class unknown, free, occupied, and those with |q| == FAR; null: the call does not wait
  int computeEsdf(const icpk_esdf_params& p, int64_t* counts = nullptr) { return icpk_esdf_compute(eng_.ctx(), &p, counts); }
  // the map, voxels() entries each, x fastest: sq, the class (0 unknown, 1 free, 2 occupied), the metric distance; any
  // pointer may be null
  int esdfPlanes(int32_t* sq, uint8_t* cls, float* dist) { return icpk_esdf_get(eng_.ctx(), sq, cls, dist); }
  int esdfBox(const int32_t lo[3], const int32_t hi[3], int32_t* sq, uint8_t* cls, float* dist) {
    return icpk_esdf_get_box(eng_.ctx(), lo, hi, sq, cls, dist);
  }
  // the map at n world points, trilinear between voxel centres; all five vectors are sized to n.  status: 0x80 outside
  // (dist and gradient 0), else bit 0 a FAR corner, bit 1 a corner of unknown class
  int queryEsdf(const std::vector<float>& x, const std::vector<float>& y, const std::vector<float>& z, std::vector<float>& dist,
                std::vector<float>& gx, std::vector<float>& gy, std::vector<float>& gz, std::vector<uint8_t>& status) {
    if (y.size() != x.size() || z.size() != x.size()) return ICPK_E_ARG;
    for (std::vector<float>* v : {&dist, &gx, &gy, &gz}) v->assign(x.size(), 0.f);
    status.assign(x.size(), 0);
    return icpk_esdf_query(eng_.ctx(), x.data(), y.data(), z.data(), (int32_t)x.size(), dist.data(), gx.data(), gy.data(),
                           gz.data(), status.data());
  }
  int releaseEsdf() { return icpk_esdf_release(eng_.ctx()); }

 private:
  void forget() { rayRows_ = rayCols_ = 0, meshVertices_ = meshTriangles_ = meshNoNormal_ = 0; }
  int refresh() { return icpk_tsdf_get_params(eng_.ctx(), &p_, total_); }
  Engine& eng_;
  icpk_tsdf_params p_;
  int64_t total_[3] = {0, 0, 0};
  float fx_, cx_;
  int rayRows_ = 0, rayCols_ = 0;
  int32_t meshVertices_ = 0, meshTriangles_ = 0, meshNoNormal_ = 0;
};

}  // namespace icp
