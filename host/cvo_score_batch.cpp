// Batched scoring through the C++ veneer: one frame pair under a sweep of poses, the way the reference's
// main_evaluate_indicator.cpp scores a pair over a range of poses, but as three calls (inner products, approximate and
// exact function_angle) instead of three per pose.
//   cvo_score_batch source.pcd target.pcd cvo_params.yaml ell [n_poses=8]
// Prints every pose (16 floats, column-major) and the three scores of every pose.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "cvo/CvoGPU.hpp"

int main(int argc, char* argv[]) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s source.pcd target.pcd cvo_params.yaml ell [n_poses=8]\n", argv[0]);
    return 2;
  }
  cvo::CvoPointCloud source(argv[1]), target(argv[2]);
  cvo::CvoGPU gpu(argv[3]);
  const float ell = std::strtof(argv[4], nullptr);
  const int n = argc > 5 ? std::atoi(argv[5]) : 8;
  // pose k: a turn of 0.02 k rad about z and a shift of (0.05 k, -0.02 k, 0.01 k)
  std::vector<cvo::Mat4f> T((size_t)n, cvo::Mat4f::Identity());
  for (int k = 0; k < n; k++) {
    const double a = 0.02 * k;
    T[k](0, 0) = (float)std::cos(a);
    T[k](0, 1) = (float)-std::sin(a);
    T[k](1, 0) = (float)std::sin(a);
    T[k](1, 1) = (float)std::cos(a);
    T[k](0, 3) = (float)(0.05 * k);
    T[k](1, 3) = (float)(-0.02 * k);
    T[k](2, 3) = (float)(0.01 * k);
  }
  auto clouds = gpu.upload_clouds({&source, &target});
  const std::vector<std::pair<int, int>> pairs((size_t)n, std::make_pair(0, 1));
  const std::vector<float> ells{ell};
  const std::vector<float> ip = gpu.inner_product_batch(*clouds, *clouds, pairs, T, ells);
  const std::vector<float> fa = gpu.function_angle_batch(*clouds, *clouds, pairs, T, ells, true);
  const std::vector<float> fe = gpu.function_angle_batch(*clouds, *clouds, pairs, T, ells, false);
  for (int k = 0; k < n; k++) {
    std::printf("pose %d", k);
    for (int i = 0; i < 16; i++) std::printf(" %.9g", T[k].data()[i]);
    std::printf("\nscore %d %.9g %.9g %.9g\n", k, ip[k], fa[k], fe[k]);
  }
  return 0;
}
