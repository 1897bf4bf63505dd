// Clouds from rows that are already on the device, through the C++ veneer: CvoGPU::upload_device (strided arrays) and
// CvoGPU::upload_device_aos192 (CvoPoint records) against the pcl overload of inner_product_gpu, which uploads the same
// records from host memory.
//   cvo_device_rows_check source.pcd target.pcd cvo_params.yaml ell
// Prints "host", "aos192" and "strided": <source, target> at the identity as a float and as its bit pattern.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "utils/CvoPoint.hpp"

static void* to_device(const std::vector<cvo::CvoPoint>& recs) {
  void* d = nullptr;
  if (hipMalloc(&d, sizeof(cvo::CvoPoint) * recs.size()) != hipSuccess ||
      hipMemcpy(d, recs.data(), sizeof(cvo::CvoPoint) * recs.size(), hipMemcpyHostToDevice) != hipSuccess) {
    std::fprintf(stderr, "device copy failed\n");
    std::exit(1);
  }
  return d;
}

static void print(const char* name, float v) {
  unsigned b;
  std::memcpy(&b, &v, 4);
  std::printf("%s %.9g %08x\n", name, v, b);
}

int main(int argc, char* argv[]) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s source.pcd target.pcd cvo_params.yaml ell\n", argv[0]);
    return 2;
  }
  cvo::CvoPointCloud source(argv[1]), target(argv[2]);
  cvo::CvoGPU gpu(argv[3]);
  const float ell = std::strtof(argv[4], nullptr);
  const std::vector<cvo::CvoPoint> s = cvo::CvoPointCloud_to_cvo_points(source), t = cvo::CvoPointCloud_to_cvo_points(target);
  const int n = (int)s.size(), m = (int)t.size();
  const cvo::Mat4f I = cvo::Mat4f::Identity();
  print("host", gpu.inner_product_gpu(s.data(), n, t.data(), m, I, ell));
  char* ds = (char*)to_device(s);
  char* dt = (char*)to_device(t);
  const std::vector<std::pair<int, int>> pair{{0, 0}};
  const std::vector<cvo::Mat4f> T{I};
  const std::vector<float> ells{ell};
  {
    auto a = gpu.upload_device_aos192((const cvo::CvoPoint*)ds, n), b = gpu.upload_device_aos192((const cvo::CvoPoint*)dt, m);
    print("aos192", gpu.inner_product_batch(*a, *b, pair, T, ells)[0]);
  }
  auto rows = [](const char* d, int k) {  // the same records as four strided arrays
    cvo_device_rows_t r{};
    r.n = r.n_records = k;
    r.xyz = d;
    r.feat = d + offsetof(cvo::CvoPoint, features);
    r.label = d + offsetof(cvo::CvoPoint, label_distribution);
    r.geotype = d + offsetof(cvo::CvoPoint, geometric_type);
    r.xyz_stride = r.feat_stride = r.label_stride = r.geotype_stride = sizeof(cvo::CvoPoint);
    return r;
  };
  {
    auto a = gpu.upload_device(rows(ds, n)), b = gpu.upload_device(rows(dt, m));
    (void)hipFree(ds);  // the clouds own copies
    (void)hipFree(dt);
    print("strided", gpu.inner_product_batch(*a, *b, pair, T, ells)[0]);
  }
  return 0;
}
