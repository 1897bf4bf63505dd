// Posed resident clouds merged on the device and read back, through the C++ veneer: CvoGPU::merge / CvoGPU::download
// against CvoPointCloud::transform + operator+ on the host.
//   cvo_merge_check cvo_params.yaml
// Two tiny colour clouds (9 and 5 points).  Prints one line per check - "download", "concat", "voxel" - with the largest
// coordinate difference in ulp and whether the attributes are equal; exit code 0 when every check holds (coordinates within
// 1 ulp, attributes exactly).  The poses' entries are multiples of 2^-8 and the coordinates multiples of 2^-6, so every
// product and sum of a transform is exact in float whichever way it is associated or fused: the host's and the device's
// statement of the pose may differ in form, not in value.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cvo/CvoGPU.hpp"

static int ulps(float a, float b) {
  if (a == b) return 0;
  int ia, ib;
  std::memcpy(&ia, &a, 4);
  std::memcpy(&ib, &b, 4);
  if (ia < 0) ia = (int)0x80000000 - ia;
  if (ib < 0) ib = (int)0x80000000 - ib;
  return std::abs(ia - ib);
}

static cvo::CvoPointCloud tiny(int n, int seed) {
  std::vector<float> xyz(3 * (size_t)n);
  std::vector<unsigned char> rgb(3 * (size_t)n);
  unsigned s = 12345u + 977u * (unsigned)seed;
  for (size_t i = 0; i < xyz.size(); i++) {
    s = s * 1664525u + 1013904223u;
    xyz[i] = (float)((int)((s >> 16) % 512u) - 256) / 64.f;
    rgb[i] = (unsigned char)(s >> 8);
  }
  return cvo::CvoPointCloud::from_xyzrgb(xyz.data(), rgb.data(), n);
}

// largest coordinate difference in ulp; *same: features, labels and geometric types equal
static int compare(const cvo::CvoPointCloud& a, const cvo::CvoPointCloud& b, bool* same) {
  *same = a.num_points() == b.num_points() && a.features().cols() == b.features().cols() && a.labels().cols() == b.labels().cols() &&
          a.geometric_types() == b.geometric_types();
  if (!*same) return -1;
  int worst = 0;
  for (int i = 0; i < a.num_points(); i++) {
    for (int c = 0; c < 3; c++) worst = std::max(worst, ulps(a.positions()[i][c], b.positions()[i][c]));
    for (int c = 0; c < a.features().cols(); c++) *same = *same && a.features()(i, c) == b.features()(i, c);
    for (int c = 0; c < a.labels().cols(); c++) *same = *same && a.labels()(i, c) == b.labels()(i, c);
  }
  return worst;
}

static bool report(const char* name, const cvo::CvoPointCloud& got, const cvo::CvoPointCloud& want) {
  bool same = false;
  const int u = compare(got, want, &same);
  std::printf("%s points %d max_ulp %d attributes %s\n", name, got.num_points(), u, same ? "equal" : "DIFFER");
  return same && u >= 0 && u <= 1;
}

int main(int argc, char* argv[]) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s cvo_params.yaml\n", argv[0]);
    return 2;
  }
  cvo::CvoGPU gpu(argv[1]);
  const cvo::CvoPointCloud a = tiny(9, 1), b = tiny(5, 2);
  // 3x4 row-major: a general matrix in 1 / 256 steps (close to a rotation by 0.3 rad about z, tilted), and a quarter turn
  const std::vector<double> poses = {245 / 256., -75 / 256., 10 / 256., 0.5,   76 / 256., 244 / 256., -21 / 256., -1.25,
                                     -3 / 256.,  23 / 256.,  255 / 256., 2.0,  0, -1, 0, 3.5,   1, 0, 0, -0.75,   0, 0, 1, 0.125};
  auto resident = gpu.upload_clouds({&a, &b});
  bool ok = report("download", gpu.download(*resident, 0), a);
  cvo::CvoPointCloud moved[2];
  for (int k = 0; k < 2; k++) {
    cvo::Mat4f T = cvo::Mat4f::Identity();
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 4; c++) T(r, c) = (float)poses[12 * (size_t)k + 4 * r + c];
    cvo::CvoPointCloud::transform(T, k == 0 ? a : b, moved[k]);
  }
  const cvo::CvoPointCloud want = moved[0] + moved[1];
  auto merged = gpu.merge(*resident, &poses, 0.f);
  ok = report("concat", gpu.download(*merged, 0), want) && ok;
  ok = ok && (int)merged->kept(0).size() == 14;
  // one voxel of side 64 holds every moved point: the first row alone is kept
  auto one = gpu.merge(*resident, &poses, 64.f);
  ok = report("voxel", gpu.download(*one, 0), want.select({0})) && ok;
  ok = ok && one->kept(0) == std::vector<int>{0};
  std::printf("%s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
