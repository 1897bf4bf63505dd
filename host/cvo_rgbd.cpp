// The RGB-D image constructor of cvo::CvoPointCloud and cvo::CvoGPU::rgbd_points / upload_rgbd over the C-ABI
// (cvo_rgbd_points_host / cvo_rgbd_points / cvo_cloud_upload_rgbd, include/cvo_hip.h).
#include <stdexcept>
#include <string>
#include <type_traits>

#include "cvo/CvoGPU.hpp"

namespace cvo {
namespace {

template <typename DepthType>
cvo_rgbd_frame_t frame_of(const ImageRGBD<DepthType>& im, const Calibration& calib) {
  static_assert(std::is_same<DepthType, uint16_t>::value || std::is_same<DepthType, float>::value, "depth is uint16_t or float");
  cvo_rgbd_frame_t f{};
  f.rows = im.rows();
  f.cols = im.cols();
  f.channels = im.channels();
  f.image = im.image().data();
  f.gray = im.gray().empty() ? nullptr : im.gray().data();
  f.depth = im.depth_image().data();
  f.depth_type = std::is_same<DepthType, uint16_t>::value ? CVO_DEPTH_U16 : CVO_DEPTH_F32;
  const Mat3f& K = calib.intrinsic();
  f.fx = K(0, 0);
  f.fy = K(1, 1);
  f.cx = K(0, 2);
  f.cy = K(1, 2);
  f.scaling_factor = calib.scaling_factor();
  f.num_classes = im.num_classes();
  f.semantic = im.num_classes() > 0 ? im.semantic_image().data() : nullptr;
  return f;
}

// row buffers of one cvo_rgbd_points call
struct PointRows {
  int F, C;
  std::vector<int> pixel;
  std::vector<float> xyz, feat, label, geo;
  explicit PointRows(const cvo_rgbd_frame_t& f) : F(f.channels + 2), C(f.num_classes) {
    const size_t cap = (size_t)f.rows * f.cols;
    pixel.resize(cap);
    xyz.resize(3 * cap);
    feat.resize((size_t)F * cap);
    label.resize((size_t)C * cap);
    geo.resize(2 * cap);
  }
};

}  // namespace

template <typename DepthType>
CvoPointCloud::CvoPointCloud(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, PointSelectionMethod method, std::vector<int>* pixel) {
  const cvo_rgbd_frame_t f = frame_of(raw_image, calib);
  PointRows r(f);
  int n = 0;
  const int rc = cvo_rgbd_points_host(&f, (int)method, r.pixel.data(), &n, r.xyz.data(), r.feat.data(), r.C ? r.label.data() : nullptr, r.geo.data());
  if (rc != CVO_OK) throw std::invalid_argument("CvoPointCloud(ImageRGBD): cvo_rgbd_points_host refused the frame or the method (" + std::to_string(rc) + ")");
  reserve(n, r.F, r.C);
  for (int i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) positions_[(size_t)i][c] = r.xyz[3 * (size_t)i + c];
    for (int c = 0; c < r.F; c++) features_(i, c) = r.feat[(size_t)r.F * i + c];
    for (int c = 0; c < r.C; c++) labels_(i, c) = r.label[(size_t)r.C * i + c];
    geometric_types_[2 * (size_t)i] = r.geo[2 * (size_t)i];
    geometric_types_[2 * (size_t)i + 1] = r.geo[2 * (size_t)i + 1];
  }
  if (pixel) pixel->assign(r.pixel.begin(), r.pixel.begin() + n);
}
template CvoPointCloud::CvoPointCloud(const ImageRGBD<uint16_t>&, const Calibration&, PointSelectionMethod, std::vector<int>*);
template CvoPointCloud::CvoPointCloud(const ImageRGBD<float>&, const Calibration&, PointSelectionMethod, std::vector<int>*);

template <typename DepthType>
CvoPointCloud CvoGPU::rgbd_points(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, CvoPointCloud::PointSelectionMethod method,
                                  std::vector<int>* pixel) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_rgbd_frame_t f = frame_of(raw_image, calib);
  PointRows r(f);
  int n = 0;
  const int rc = cvo_rgbd_points(ctx, &f, (int)method, r.pixel.data(), &n, r.xyz.data(), r.feat.data(), r.C ? r.label.data() : nullptr, r.geo.data());
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_rgbd_points: ") + cvo_last_error(ctx));
  CvoPointCloud out;
  out.reserve(n, r.F, r.C);
  for (int i = 0; i < n; i++) {
    const Vec3f p{{r.xyz[3 * (size_t)i], r.xyz[3 * (size_t)i + 1], r.xyz[3 * (size_t)i + 2]}};
    out.add_point(i, p, std::vector<float>(r.feat.begin() + (size_t)r.F * i, r.feat.begin() + (size_t)r.F * (i + 1)),
                  std::vector<float>(r.label.begin() + (size_t)r.C * i, r.label.begin() + (size_t)r.C * (i + 1)),
                  std::vector<float>{r.geo[2 * (size_t)i], r.geo[2 * (size_t)i + 1]});
  }
  if (pixel) pixel->assign(r.pixel.begin(), r.pixel.begin() + n);
  return out;
}
template CvoPointCloud CvoGPU::rgbd_points(const ImageRGBD<uint16_t>&, const Calibration&, CvoPointCloud::PointSelectionMethod, std::vector<int>*) const;
template CvoPointCloud CvoGPU::rgbd_points(const ImageRGBD<float>&, const Calibration&, CvoPointCloud::PointSelectionMethod, std::vector<int>*) const;

template <typename DepthType>
std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_rgbd(const ImageRGBD<DepthType>& raw_image, const Calibration& calib, float leaf,
                                                            float edge_divisor, std::vector<int>* pixel, std::vector<unsigned char>* is_edge) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_rgbd_frame_t f = frame_of(raw_image, calib);
  const size_t cap = 2 * (size_t)f.rows * f.cols;
  std::vector<int> px(cap);
  std::vector<unsigned char> edge(cap);
  int n = 0;
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  const int rc = cvo_cloud_upload_rgbd(ctx, &f, leaf > 0.f ? leaf : params.multiframe_downsample_voxel_size, edge_divisor, &out->handles[0], px.data(),
                                       edge.data(), &n);
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_cloud_upload_rgbd: ") + cvo_last_error(ctx));
  if (pixel) pixel->assign(px.begin(), px.begin() + n);
  if (is_edge) is_edge->assign(edge.begin(), edge.begin() + n);
  return out;
}
template std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_rgbd(const ImageRGBD<uint16_t>&, const Calibration&, float, float, std::vector<int>*,
                                                                     std::vector<unsigned char>*) const;
template std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_rgbd(const ImageRGBD<float>&, const Calibration&, float, float, std::vector<int>*,
                                                                     std::vector<unsigned char>*) const;

}  // namespace cvo
