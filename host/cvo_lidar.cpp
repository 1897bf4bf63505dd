// The LiDAR constructors of cvo::CvoPointCloud and cvo::CvoGPU::upload_lidar over the C-ABI (cvo_lidar_select_host /
// cvo_cloud_upload_lidar, include/cvo_hip.h).
#include <mutex>
#include <stdexcept>
#include <string>

#include "cvo/CvoGPU.hpp"

namespace cvo {
namespace {

// upstream draws from std::rand(): one stream per process, never seeded by the library
std::mutex process_rand_mutex;
cvo_lidar_rand_t* process_rand() {
  static cvo_lidar_rand_t state = [] {
    cvo_lidar_rand_t s;
    cvo_lidar_rand_seed(&s, 1);
    return s;
  }();
  return &state;
}

cvo_lidar_config_t config_of(bool semantic, int beam_num) {
  cvo_lidar_config_t c;
  cvo_lidar_config_default(&c, semantic ? 1 : 0);
  c.beam_num = beam_num;
  return c;
}

void check_method(CvoPointCloud::PointSelectionMethod m) {
  if (m != CvoPointCloud::LOAM) throw std::invalid_argument("CvoPointCloud(lidar): only the LOAM point selection is built");
}

void construct(CvoPointCloud& out, const float* xyzi, int n, const std::vector<int>* semantic, int num_classes, int beam_num, std::vector<int>* index,
               cvo_lidar_rand_t* rand) {
  if (semantic && (int)semantic->size() != n) throw std::invalid_argument("CvoPointCloud(lidar): semantic needs one class id per point");
  const cvo_lidar_scan_t scan{n, xyzi, semantic ? semantic->data() : nullptr, semantic ? num_classes : 0};
  const cvo_lidar_config_t cfg = config_of(semantic != nullptr, beam_num);
  std::vector<int> idx(2 * (size_t)(n > 0 ? n : 1));
  int k = 0;
  std::unique_lock<std::mutex> lk;
  if (!rand) {
    lk = std::unique_lock<std::mutex>(process_rand_mutex);
    rand = process_rand();
  }
  const int rc = cvo_lidar_select_host(&scan, &cfg, rand, idx.data(), nullptr, &k);
  if (rc != CVO_OK) throw std::invalid_argument("CvoPointCloud(lidar): cvo_lidar_select_host refused the scan (" + std::to_string(rc) + ")");
  const int C = semantic ? num_classes : 0;
  out.reserve(k, 1, C);
  for (int i = 0; i < k; i++) {
    const float* p = xyzi + 4 * (size_t)idx[(size_t)i];
    std::vector<float> label((size_t)C, 0.f);
    if (C) label[(size_t)(*semantic)[(size_t)idx[(size_t)i]]] = 1.f;
    out.add_point(i, Vec3f{{p[0], p[1], p[2]}}, std::vector<float>{p[3]}, label, std::vector<float>{1.f, 0.f});
  }
  if (index) index->assign(idx.begin(), idx.begin() + k);
}

}  // namespace

CvoPointCloud::CvoPointCloud(const float* xyzi, int n, int target_num_points, int beam_num, PointSelectionMethod method, std::vector<int>* index,
                             cvo_lidar_rand_t* rand) {
  (void)target_num_points;
  check_method(method);
  construct(*this, xyzi, n, nullptr, 0, beam_num, index, rand);
}

CvoPointCloud::CvoPointCloud(const float* xyzi, int n, const std::vector<int>& semantic, int num_classes, int target_num_points, int beam_num,
                             PointSelectionMethod method, std::vector<int>* index, cvo_lidar_rand_t* rand) {
  (void)target_num_points;
  check_method(method);
  construct(*this, xyzi, n, &semantic, num_classes, beam_num, index, rand);
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_lidar(const float* xyzi, int n, const std::vector<int>* semantic, int num_classes, int beam_num,
                                                             std::vector<int>* index, cvo_lidar_rand_t* rand) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  if (semantic && (int)semantic->size() != n) throw std::invalid_argument("upload_lidar: semantic needs one class id per point");
  const cvo_lidar_scan_t scan{n, xyzi, semantic ? semantic->data() : nullptr, semantic ? num_classes : 0};
  const cvo_lidar_config_t cfg = config_of(semantic != nullptr, beam_num);
  std::vector<int> idx(2 * (size_t)(n > 0 ? n : 1));
  int k = 0;
  std::unique_lock<std::mutex> rl;
  if (!rand) {
    rl = std::unique_lock<std::mutex>(process_rand_mutex);
    rand = process_rand();
  }
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  const int rc = cvo_cloud_upload_lidar(ctx, &scan, &cfg, rand, &out->handles[0], idx.data(), &k);
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_cloud_upload_lidar: ") + cvo_last_error(ctx));
  if (index) index->assign(idx.begin(), idx.begin() + k);
  return out;
}

}  // namespace cvo
