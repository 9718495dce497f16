// tests/cpp/test_tsdf_esdf.cpp -- icp::TsdfVolume::computeEsdf / esdfPlanes / esdfBox / queryEsdf (icp_tsdf.hpp, K31) over
// planes handed in; the Python test (tests/test_gpu_esdf_cpp.py) compares what it writes with the same calls made
// through the binding, byte for byte.
//
//   test_tsdf_esdf <in.bin> <out.bin>
// in : int32 dims[3], min_weight, flags, n_points, box_lo[3], box_hi[3]; float voxel, origin[3], trunc, max_distance;
//      float tsdf[n]; uint16 weight[n]; float x[n_points], y[n_points], z[n_points]
// out: int64 counts[4]; int32 sq[n]; uint8 cls[n]; float dist[n]; the box's int32 sq[m], uint8 cls[m], float dist[m];
//      float dist[n_points], gx, gy, gz; uint8 status[n_points]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_tsdf.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[12];
  float geo[6];
  if (std::fread(head, 4, 12, f) != 12 || std::fread(geo, 4, 6, f) != 6) return 4;
  icpk_tsdf_params p = icp::TsdfVolume::defaults();
  for (int a = 0; a < 3; ++a) p.dims[a] = head[a], p.origin[a] = geo[1 + a];
  p.voxel = geo[0], p.trunc = geo[4];
  icpk_esdf_params e = icp::TsdfVolume::esdfDefaults();
  e.min_weight = head[3], e.flags = head[4], e.max_distance = geo[5];
  const int npts = head[5];
  const int32_t* lo = head + 6;
  const int32_t* hi = head + 9;
  if (p.dims[0] < 1 || p.dims[1] < 1 || p.dims[2] < 1 || npts < 0) return 4;
  const size_t n = (size_t)p.dims[0] * p.dims[1] * p.dims[2];
  std::vector<float> tsdf(n), x(npts), y(npts), z(npts);
  std::vector<uint16_t> weight(n);
  if (std::fread(tsdf.data(), 4, n, f) != n || std::fread(weight.data(), 2, n, f) != n) return 4;
  for (std::vector<float>* v : {&x, &y, &z})
    if (std::fread(v->data(), 4, (size_t)npts, f) != (size_t)npts) return 4;
  std::fclose(f);
  try {
    icp::Engine eng(0);
    icp::TsdfVolume vol(eng, p, 468.60f, 318.27f);
    // before a compute there is nothing to get
    if (vol.esdfPlanes(nullptr, nullptr, nullptr) != ICPK_E_NOT_SET) return 8;
    int rc = vol.setPlanes(tsdf.data(), weight.data());
    int64_t counts[4] = {-1, -1, -1, -1};
    if (!rc) rc = vol.computeEsdf(e, counts);
    std::vector<int32_t> sq(n);
    std::vector<uint8_t> cls(n);
    std::vector<float> dist(n);
    if (!rc) rc = vol.esdfPlanes(sq.data(), cls.data(), dist.data());
    size_t m = 1;
    for (int a = 0; a < 3; ++a) m *= hi[a] > lo[a] ? (size_t)(hi[a] - lo[a]) : 1;
    std::vector<int32_t> bsq(m);
    std::vector<uint8_t> bcls(m);
    std::vector<float> bdist(m);
    if (!rc) rc = vol.esdfBox(lo, hi, bsq.data(), bcls.data(), bdist.data());
    std::vector<float> qd, gx, gy, gz;
    std::vector<uint8_t> st;
    if (!rc) rc = vol.queryEsdf(x, y, z, qd, gx, gy, gz, st);
    if (rc) {
      std::fprintf(stderr, "a call failed: %d %s\n", rc, eng.last_error());
      return 5;
    }
    // the refusals come through the mirror as statuses, and setPlanes drops the map
    icpk_esdf_params bad = e;
    bad.max_distance = 0.f;
    if (vol.computeEsdf(bad) != ICPK_E_ARG || vol.esdfPlanes(sq.data(), nullptr, nullptr) != ICPK_OK) return 8;
    if (vol.setPlanes(tsdf.data(), weight.data()) != ICPK_OK || vol.esdfPlanes(sq.data(), nullptr, nullptr) != ICPK_E_NOT_SET) return 8;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    std::fwrite(counts, 8, 4, o);
    std::fwrite(sq.data(), 4, n, o);
    std::fwrite(cls.data(), 1, n, o);
    std::fwrite(dist.data(), 4, n, o);
    std::fwrite(bsq.data(), 4, m, o);
    std::fwrite(bcls.data(), 1, m, o);
    std::fwrite(bdist.data(), 4, m, o);
    for (const std::vector<float>* v : {&qd, &gx, &gy, &gz}) std::fwrite(v->data(), 4, v->size(), o);
    std::fwrite(st.data(), 1, st.size(), o);
    std::fclose(o);
    std::printf("esdf of %d x %d x %d: %lld unknown, %lld free, %lld occupied, %lld far; %d points\n", p.dims[0], p.dims[1],
                p.dims[2], (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3], npts);
  } catch (const std::exception& ex) {
    std::fprintf(stderr, "%s\n", ex.what());
    return 7;
  }
  return 0;
}
