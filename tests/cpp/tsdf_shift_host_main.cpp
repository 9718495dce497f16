// tests/cpp/tsdf_shift_host_main.cpp -- the shift rule's host-callable half (csrc/tsdf_rule.h: tsdf_keep_box,
// tsdf_ends_stay, tsdf_crossing_kept, tsdf_leaving_status, tsdf_shifted_origin) with a main of its own and no GPU, meant
// to be compiled under -fsanitize=address,undefined (build.program("tsdf_shift_host_sanitized")) and run directly.  The box
// tests are held against the rule as include/icpk.h words it -- stays(v) asked of V, of N and of the six axis
// neighbours of each, one voxel at a time -- for every voxel, axis and shift of a small volume, the extreme shifts an
// int32 can hold among them; the origin goes there and back.
#include <climits>
#include <cstdio>
#include <cstring>

#include "tsdf_rule.h"

using namespace icpk;

static bool stays(const int dims[3], const long long s[3], const long long v[3]) {
  for (int a = 0; a < 3; ++a)
    if (!(s[a] <= v[a] && v[a] < dims[a] + s[a])) return false;
  return true;
}

int main() {
  const int dims[3] = {7, 5, 3};
  const int values[] = {INT_MIN, -1000, -8, -7, -6, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7, 8, 1000, INT_MAX};
  const int nv = (int)(sizeof(values) / sizeof(values[0]));
  long long checked = 0, kept_total = 0;
  for (int ix = 0; ix < nv; ++ix)
    for (int iy = 0; iy < nv; ++iy)
      for (int iz = 0; iz < nv; ++iz) {
        const int s[3] = {values[ix], values[iy], values[iz]};
        const long long sl[3] = {s[0], s[1], s[2]};
        const TsdfKeep box = tsdf_keep_box(dims, s);
        for (int k = 0; k < dims[2]; ++k)
          for (int j = 0; j < dims[1]; ++j)
            for (int i = 0; i < dims[0]; ++i)
              for (int axis = 0; axis < 3; ++axis) {
                const int c[3] = {i, j, k};
                long long V[3] = {i, j, k}, N[3] = {i, j, k};
                N[axis] += 1;
                const bool ends = stays(dims, sl, V) && stays(dims, sl, N);
                bool kept = ends;
                for (int a = 0; a < 3 && kept; ++a)
                  for (int d = -1; d <= 1; d += 2) {
                    long long p[3] = {V[0], V[1], V[2]}, q[3] = {N[0], N[1], N[2]};
                    p[a] += d, q[a] += d;
                    kept = kept && stays(dims, sl, p) && stays(dims, sl, q);
                  }
                if (tsdf_ends_stay(box, c, axis) != ends || tsdf_crossing_kept(box, c, axis) != kept) {
                  std::printf("box test differs at (%d %d %d) axis %d shift (%d %d %d)\n", i, j, k, axis, s[0], s[1], s[2]);
                  return 1;
                }
                const int want_listed = kept ? TSDF_NO_CROSSING : TSDF_CROSSING;
                const int want_dropped = ends ? TSDF_NO_CROSSING : TSDF_NO_NORMAL;
                if (tsdf_leaving_status(box, c, axis, TSDF_CROSSING) != want_listed ||
                    tsdf_leaving_status(box, c, axis, TSDF_NO_NORMAL) != want_dropped ||
                    tsdf_leaving_status(box, c, axis, TSDF_NO_CROSSING) != TSDF_NO_CROSSING) {
                  std::printf("leaving status differs at (%d %d %d) axis %d\n", i, j, k, axis);
                  return 1;
                }
                checked += 1, kept_total += kept;
              }
      }
  // the origin: always from the creation origin and the cumulative shift, so there and back is the same bits
  const float origins[] = {-2.3f, -2.56f, 0.4f, 1e-3f, -1000.1f}, voxels[] = {0.0625f, 0.02f, 0.11f, 0.01f};
  for (float o : origins)
    for (float vx : voxels) {
      long long total = 0;
      const long long steps[] = {1, 1, 1, -3, 4000, -4000, -7, 7, (long long)INT_MAX, -(long long)INT_MAX};
      for (long long st : steps) {
        total += st;
        const float now = tsdf_shifted_origin(o, total, vx);
        if (total == 0 && std::memcmp(&now, &o, sizeof(float)) != 0) {
          std::printf("the origin did not come back: %a against %a\n", (double)now, (double)o);
          return 1;
        }
      }
      if (!(tsdf_shifted_origin(o, 3, vx) > o)) return 1;
    }
  std::printf("tsdf shift host: %lld box tests (%lld kept), origins there and back: clean\n", checked, kept_total);
  return 0;
}
