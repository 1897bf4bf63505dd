// Keyframe depth filtering through the C++ veneer: CvoGPU::depth_filter (clouds in, kf_filtered out; and the resident form)
// against the last loops of upstream's driver main_depth_filtering.cpp (245-294) written out on the host over
// compute_association_gpu(kf, frame, T_t2s, kernel, association).
//   cvo_depth_filter_check cvo_params.yaml
// A keyframe of 60 colour points and three frames of noisy copies of them: frame 0 holds every point twice, frame 1 the points
// 10 .. 59 twice, frame 2 the points 0 .. 29 once - so rows 0 .. 9 see 3 observations (dropped: the comparison is count > 3),
// rows 10 .. 29 five and rows 30 .. 59 four, when each copy is associated with its own row alone (the kernel is narrow against
// the grid the keyframe sits on).  Prints one line per check - "clouds", "resident" - with the number of points, the largest
// coordinate difference in ulp and whether indices and attributes are equal; exit code 0 when every check holds (coordinates
// bit for bit: the host loop below rounds every product and sum on its own, as the library states it).
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

struct Rows {
  std::vector<float> xyz;
  std::vector<unsigned char> rgb;
  int n() const { return (int)(xyz.size() / 3); }
  cvo::CvoPointCloud cloud() const { return cvo::CvoPointCloud::from_xyzrgb(xyz.data(), rgb.data(), n()); }
};

int main(int argc, char* argv[]) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s cvo_params.yaml\n", argv[0]);
    return 2;
  }
  cvo::CvoGPU gpu(argv[1]);
  // the keyframe: a 10 x 6 grid of spacing 1 at depths 3 .. 5
  Rows kf;
  unsigned s = 2024u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (float)((int)((s >> 16) % 1024u) - 512) / 512.f;  // [-1, 1)
  };
  for (int i = 0; i < 60; i++) {
    const float p[3] = {(float)(i % 10) - 4.5f + 0.1f * rnd(), (float)(i / 10) - 2.5f + 0.1f * rnd(), 4.f + rnd()};
    kf.xyz.insert(kf.xyz.end(), p, p + 3);
    for (int c = 0; c < 3; c++) kf.rgb.push_back((unsigned char)(40 * (i % 5) + 10 * c));
  }
  auto copies = [&](int lo, int hi, int times) {
    Rows f;
    for (int t = 0; t < times; t++)
      for (int i = lo; i < hi; i++) {
        for (int c = 0; c < 3; c++) f.xyz.push_back(kf.xyz[3 * (size_t)i + c] + (c == 2 ? 0.05f : 0.01f) * rnd());
        for (int c = 0; c < 3; c++) f.rgb.push_back(kf.rgb[3 * (size_t)i + c]);
      }
    return f;
  };
  const Rows fr[3] = {copies(0, 60, 2), copies(10, 60, 2), copies(0, 30, 1)};
  const cvo::CvoPointCloud kfc = kf.cloud();
  const cvo::CvoPointCloud fc[3] = {fr[0].cloud(), fr[1].cloud(), fr[2].cloud()};
  cvo::Mat3f kernel = cvo::Mat3f::Identity();  // the driver's diag(n, n, d), d >> n
  kernel(0, 0) = kernel(1, 1) = 0.01f;
  kernel(2, 2) = 0.25f;
  std::vector<cvo::Mat4f> T(3, cvo::Mat4f::Identity()), Td(3, cvo::Mat4f::Identity());
  for (int k = 0; k < 3; k++) {  // depth matrices: a small tilt and a shift along z
    Td[k](2, 0) = 0.01f * (float)(k + 1);
    Td[k](2, 1) = -0.02f;
    Td[k](2, 2) = 0.999f;
    Td[k](2, 3) = 0.03f * (float)k;
  }
  // ---- the driver's loops on the host ----
  const int n = kfc.num_points();
  std::vector<float> depth(n, 0.f), weight(n, 0.f);
  std::vector<int> count(n, 0);
  for (int k = 0; k < 3; k++) {
    cvo::Association as;
    gpu.compute_association_gpu(kfc, fc[k], T[k], kernel, as);
    for (int i = 0; i < n; i++)
      for (int q = as.pairs.row_ptr[i]; q < as.pairs.row_ptr[i + 1]; q++) {
        const float* y = &fr[k].xyz[3 * (size_t)as.pairs.col[q]];
        volatile float px = Td[k](2, 0) * y[0], py = Td[k](2, 1) * y[1], pz = Td[k](2, 2) * y[2];
        volatile float z = px + py;
        z = z + pz;
        z = z + Td[k](2, 3);
        volatile float zw = z * as.pairs.val[q];
        depth[i] = depth[i] + zw;
        weight[i] = weight[i] + as.pairs.val[q];
        count[i]++;
      }
  }
  std::vector<int> want_idx;
  std::vector<float> want_xyz;
  for (int i = 0; i < n; i++) {
    if (!(count[i] > 3)) continue;
    const float z0 = kf.xyz[3 * (size_t)i + 2];
    volatile float wbar = weight[i] / (float)count[i];
    volatile float zw = z0 * wbar;
    volatile float d = depth[i] + zw;
    volatile float w = weight[i] + wbar;
    d = d / w;
    want_idx.push_back(i);
    for (int c = 0; c < 3; c++) {
      volatile float q = kf.xyz[3 * (size_t)i + c] / z0;
      want_xyz.push_back(q * d);
    }
  }
  bool ok = true;
  auto report = [&](const char* name, const cvo::CvoPointCloud& got, const std::vector<int>* kept) {
    bool same = got.num_points() == (int)want_idx.size() && (!kept || *kept == want_idx);
    int worst = same ? 0 : -1;
    for (int r = 0; same && r < got.num_points(); r++) {
      const int i = want_idx[(size_t)r];
      for (int c = 0; c < 3; c++) worst = std::max(worst, ulps(got.positions()[r][c], want_xyz[3 * (size_t)r + c]));
      for (int c = 0; c < got.features().cols(); c++) same = same && got.features()(r, c) == kfc.features()(i, c);
      for (int c = 0; c < 2; c++) same = same && got.geometric_types()[2 * (size_t)r + c] == kfc.geometric_types()[2 * (size_t)i + c];
    }
    std::printf("%s points %d max_ulp %d rows %s\n", name, got.num_points(), worst, same ? "equal" : "DIFFER");
    ok = ok && same && worst == 0;
  };
  report("clouds", gpu.depth_filter(kfc, {&fc[0], &fc[1], &fc[2]}, T, Td, kernel), nullptr);
  auto rk = gpu.upload_clouds({&kfc});
  auto rf = gpu.upload_clouds({&fc[0], &fc[1], &fc[2]});
  auto res = gpu.depth_filter(*rk, 0, *rf, T, Td, kernel);
  report("resident", gpu.download(*res, 0), &res->kept(0));
  ok = ok && !want_idx.empty() && (int)want_idx.size() < n;  // (the threshold drops some rows and keeps some)
  std::printf("%s\n", ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
