// tests/cpp/tsdf_mesh_host_main.cpp -- a stand-alone program over icpk_tsdf_mesh_host (the host half of the mesh rule,
// csrc/tsdf_rule.h) for sanitizer runs: build.program("tsdf_mesh_host_sanitized") compiles it together with icpk_tsdf.cpp
// under -fsanitize=address,undefined.  No GPU is touched.  Every output array is allocated at exactly the size the
// counting call asked for, so that a write past the mesh is a heap overflow the sanitizer sees.
//
//   tsdf_mesh_host_sanitized        prints the counts per field; exit status 0 when every check held
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icpk.h"

static int run(const int dims[3], bool color, bool holes, double cz) {
  icpk_tsdf_params p;
  icpk_default_tsdf_params(&p);
  for (int a = 0; a < 3; ++a) p.dims[a] = dims[a];
  p.voxel = 0.05f, p.trunc = 0.15f, p.origin[0] = -0.4f, p.origin[1] = -0.35f, p.origin[2] = 0.3f;
  p.flags = color ? ICPK_TSDF_COLOR : 0;
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<float> f(n), c(color ? n : 0);
  std::vector<uint16_t> w(n, 1);
  for (int k = 0; k < dims[2]; ++k)
    for (int j = 0; j < dims[1]; ++j)
      for (int i = 0; i < dims[0]; ++i) {
        const size_t at = i + (size_t)dims[0] * (j + (size_t)dims[1] * k);
        const double d = std::sqrt((i - 8.0) * (i - 8.0) + (j - 8.0) * (j - 8.0) + (k - cz) * (k - cz)) - 5.0;
        f[at] = (float)std::fmax(-1.0, std::fmin(1.0, d / 3.0));
        if (color) c[at] = (float)((i + j + k) % 7) / 6.f;
        if (holes && (i * 7 + j * 3 + k) % 11 == 0) w[at] = 0;
      }
  int64_t counts[3] = {-1, -1, -1};
  int rc = icpk_tsdf_mesh_host(&p, 1, f.data(), w.data(), color ? c.data() : nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, counts);
  const size_t nv = (size_t)counts[0], nt = (size_t)counts[1];
  if (counts[0] < 0 || (rc != ICPK_OK) != (nv + nt > 0)) return 1;  // (no room: refused exactly when there is a mesh)
  float* x[7];
  for (float*& q : x) q = (float*)std::malloc(nv * sizeof(float) + 1);  // (+ 1: malloc(0) may give NULL)
  int32_t* voxel = (int32_t*)std::malloc(nv * sizeof(int32_t) + 1);
  uint8_t* edge = (uint8_t*)std::malloc(nv + 1);
  int32_t* tri = (int32_t*)std::malloc(3 * nt * sizeof(int32_t) + 1);
  rc = icpk_tsdf_mesh_host(&p, 1, f.data(), w.data(), color ? c.data() : nullptr, counts[0], counts[1], x[0], x[1], x[2], x[3], x[4],
                           x[5], x[6], voxel, edge, tri, counts);
  int bad = rc != ICPK_OK || (size_t)counts[0] != nv || (size_t)counts[1] != nt;
  for (size_t t = 0; t < 3 * nt && !bad; ++t) bad = tri[t] < 0 || (size_t)tri[t] >= nv;
  for (size_t v = 1; v < nv && !bad; ++v) bad = (int64_t)voxel[v] * 8 + edge[v] <= (int64_t)voxel[v - 1] * 8 + edge[v - 1];
  if (nv > 0 && !bad) {  // one entry short: refused, the counts filled all the same
    int64_t again[3] = {-1, -1, -1};
    bad = icpk_tsdf_mesh_host(&p, 1, f.data(), w.data(), color ? c.data() : nullptr, counts[0] - 1, counts[1], x[0], x[1], x[2], x[3],
                              x[4], x[5], x[6], voxel, edge, tri, again) != ICPK_E_ARG ||
          again[0] != counts[0] || again[1] != counts[1] || again[2] != counts[2];
  }
  std::printf("%d x %d x %d%s%s: %lld vertices, %lld triangles, %lld without a normal%s\n", dims[0], dims[1], dims[2],
              color ? " colour" : "", holes ? " holes" : "", (long long)counts[0], (long long)counts[1], (long long)counts[2],
              bad ? "  FAILED" : "");
  for (float* q : x) std::free(q);
  std::free(voxel), std::free(edge), std::free(tri);
  return bad;
}

int main() {
  const int cube[3] = {16, 16, 16}, odd[3] = {17, 16, 5}, flat[3] = {16, 16, 1}, line[3] = {1, 1, 16};
  int bad = 0;
  bad |= run(cube, false, false, 8.0);  // a closed sphere with 30 exact zeros
  bad |= run(cube, true, true, 8.0);    // colour, and cells that are not known
  bad |= run(cube, false, false, 2.2);  // cut by the volume's border
  bad |= run(odd, true, false, 2.0);
  bad |= run(flat, false, false, 0.0);  // no cells
  bad |= run(line, false, false, 8.0);
  return bad;
}
