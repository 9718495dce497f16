// tests/cpp/test_tsdf_mesh.cpp -- icp::TsdfVolume::extractMesh / getMesh / setPlanes (icp_tsdf.hpp, K21) over a few
// posed frames; the Python test (tests/test_gpu_tsdf_mesh_cpp.py) compares what it writes with the same calls made
// through the binding, byte for byte.
//
//   test_tsdf_mesh <in.bin> <out.bin>
// in : int32 dims[3], max_weight, flags, rows, cols, n_frames; float voxel, origin[3], trunc, fx, cx, 0; per frame
//      double pose[16]; uint16 depth[rows * cols]; with ICPK_TSDF_COLOR float intensity[rows * cols]; then int32
//      min_weight
// out: int32 n_vertices, n_triangles, n_no_normal, 0; float x, y, z, nx, ny, nz, intensity [n_vertices] each; int32
//      voxel [n_vertices]; uint8 edge [n_vertices]; int32 triangles [3 * n_triangles]
// The planes are then read back, the volume is reset, the planes are handed to setPlanes, and the mesh extracted again
// must be the first one.  The counts are printed as well.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_tsdf.hpp"

static bool same(const icp::TsdfMesh& a, const icp::TsdfMesh& b) {
  return a.x == b.x && a.y == b.y && a.z == b.z && a.nx == b.nx && a.ny == b.ny && a.nz == b.nz && a.intensity == b.intensity &&
         a.voxel == b.voxel && a.edge == b.edge && a.triangles == b.triangles && a.noNormal == b.noNormal;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[8];
  float geo[8];
  if (std::fread(head, 4, 8, f) != 8 || std::fread(geo, 4, 8, f) != 8) return 4;
  icpk_tsdf_params p = icp::TsdfVolume::defaults();
  for (int a = 0; a < 3; ++a) p.dims[a] = head[a], p.origin[a] = geo[1 + a];
  p.max_weight = head[3], p.flags = head[4];
  p.voxel = geo[0], p.trunc = geo[4];
  const int rows = head[5], cols = head[6], frames = head[7];
  if (rows < 1 || cols < 1 || frames < 1) return 4;
  const bool color = (p.flags & ICPK_TSDF_COLOR) != 0;
  const size_t npix = (size_t)rows * cols;
  std::vector<double> poses((size_t)16 * frames);
  std::vector<std::vector<uint16_t>> depth(frames, std::vector<uint16_t>(npix));
  std::vector<std::vector<float>> inten(frames, std::vector<float>(color ? npix : 0));
  for (int k = 0; k < frames; ++k) {
    if (std::fread(poses.data() + 16 * (size_t)k, 8, 16, f) != 16 || std::fread(depth[k].data(), 2, npix, f) != npix) return 4;
    if (color && std::fread(inten[k].data(), 4, npix, f) != npix) return 4;
  }
  int32_t min_weight = 0;
  if (std::fread(&min_weight, 4, 1, f) != 1) return 4;
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, geo[5], geo[6]);
    icp::TsdfMesh none;
    if (vol.getMesh(none) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "a mesh before the first extraction\n");
      return 5;
    }
    for (int k = 0; k < frames; ++k) {
      const int rc = vol.integrate(depth[k].data(), rows, cols, poses.data() + 16 * (size_t)k, color ? inten[k].data() : nullptr);
      if (rc) {
        std::fprintf(stderr, "integrate failed: %d %s\n", rc, eng.last_error());
        return 5;
      }
    }
    int32_t nv = -1, nt = -1, nn = -1;
    icp::TsdfMesh m;
    if (vol.extractMesh(min_weight, &nv, &nt, &nn) || vol.getMesh(m)) {
      std::fprintf(stderr, "extractMesh / getMesh failed: %s\n", eng.last_error());
      return 5;
    }
    if ((size_t)nv != m.vertices() || (size_t)nt != m.size() || nn != m.noNormal) return 5;
    // the planes out, a fresh volume, the planes in: the same mesh
    std::vector<float> tsdf(vol.voxels()), plane(color ? vol.voxels() : 0);
    std::vector<uint16_t> weight(vol.voxels());
    if (vol.planes(tsdf.data(), weight.data(), color ? plane.data() : nullptr) || vol.reset()) return 5;
    if (vol.getMesh(none) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "the mesh outlived a reset\n");
      return 5;
    }
    if (vol.extractMesh(min_weight, &nv) || nv != 0) return 5;
    if (int rc = vol.setPlanes(tsdf.data(), weight.data(), color ? plane.data() : nullptr)) {
      std::fprintf(stderr, "setPlanes failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    if (vol.getMesh(none) != ICPK_E_NOT_SET) {
      std::fprintf(stderr, "the mesh outlived setPlanes\n");
      return 5;
    }
    icp::TsdfMesh again;
    if (vol.extractMesh(min_weight) || vol.getMesh(again) || !same(m, again)) {
      std::fprintf(stderr, "the mesh of the restored planes differs\n");
      return 5;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    const int32_t counts[4] = {(int32_t)m.vertices(), (int32_t)m.size(), m.noNormal, 0};
    std::fwrite(counts, 4, 4, o);
    for (const std::vector<float>* v : {&m.x, &m.y, &m.z, &m.nx, &m.ny, &m.nz, &m.intensity}) std::fwrite(v->data(), 4, v->size(), o);
    std::fwrite(m.voxel.data(), 4, m.voxel.size(), o);
    std::fwrite(m.edge.data(), 1, m.edge.size(), o);
    std::fwrite(m.triangles.data(), 4, m.triangles.size(), o);
    std::fclose(o);
    std::printf("mesh: %d vertices, %d triangles, %d without a normal\n", counts[0], counts[1], counts[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 7;
  }
  return 0;
}
