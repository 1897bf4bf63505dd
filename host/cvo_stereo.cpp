// The stereo image constructor of cvo::CvoPointCloud and cvo::CvoGPU::stereo_points / upload_stereo / upload_stereo_recipe
// over the C-ABI (cvo_stereo_points_host / cvo_stereo_points / cvo_cloud_upload_stereo / _recipe, include/cvo_hip.h).
#include <stdexcept>
#include <string>

#include "cvo/CvoGPU.hpp"

namespace cvo {
namespace {

cvo_stereo_frame_t frame_of(const ImageStereo& im, const Calibration& calib) {
  cvo_stereo_frame_t f{};
  f.rows = im.rows();
  f.cols = im.cols();
  f.channels = im.channels();
  f.image = im.image().data();
  f.gray = im.gray().empty() ? nullptr : im.gray().data();
  f.disparity = im.disparity().data();
  const Mat3f& K = calib.intrinsic();
  f.fx = K(0, 0);
  f.fy = K(1, 1);
  f.cx = K(0, 2);
  f.cy = K(1, 2);
  f.baseline = calib.baseline();
  f.num_classes = im.num_classes();
  f.semantic = im.num_classes() > 0 ? im.semantic_image().data() : nullptr;
  return f;
}

// row buffers of one cvo_stereo_points call, and the cloud they make
struct PointRows {
  int F, C;
  std::vector<int> pixel;
  std::vector<float> xyz, feat, label, geo;
  explicit PointRows(const cvo_stereo_frame_t& f) : F(f.channels + 2), C(f.num_classes) {
    const size_t cap = (size_t)f.rows * f.cols;
    pixel.resize(cap);
    xyz.resize(3 * cap);
    feat.resize((size_t)F * cap);
    label.resize((size_t)C * cap);
    geo.resize(2 * cap);
  }
  void fill(CvoPointCloud& out, int n) const {
    out.reserve(n, F, C);
    for (int i = 0; i < n; i++) {
      const Vec3f p{{xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]}};
      out.add_point(i, p, std::vector<float>(feat.begin() + (size_t)F * i, feat.begin() + (size_t)F * (i + 1)),
                    std::vector<float>(label.begin() + (size_t)C * i, label.begin() + (size_t)C * (i + 1)),
                    std::vector<float>{geo[2 * (size_t)i], geo[2 * (size_t)i + 1]});
    }
  }
};

}  // namespace

CvoPointCloud::CvoPointCloud(const ImageStereo& raw_image, const Calibration& calib, PointSelectionMethod method, std::vector<int>* pixel) {
  const cvo_stereo_frame_t f = frame_of(raw_image, calib);
  PointRows r(f);
  int n = 0;
  const int rc = cvo_stereo_points_host(&f, (int)method, r.pixel.data(), &n, r.xyz.data(), r.feat.data(), r.C ? r.label.data() : nullptr, r.geo.data());
  if (rc != CVO_OK) throw std::invalid_argument("CvoPointCloud(ImageStereo): cvo_stereo_points_host refused the frame or the method (" + std::to_string(rc) + ")");
  r.fill(*this, n);
  if (pixel) pixel->assign(r.pixel.begin(), r.pixel.begin() + n);
}

CvoPointCloud CvoGPU::stereo_points(const ImageStereo& raw_image, const Calibration& calib, CvoPointCloud::PointSelectionMethod method,
                                    std::vector<int>* pixel) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_stereo_frame_t f = frame_of(raw_image, calib);
  PointRows r(f);
  int n = 0;
  const int rc = cvo_stereo_points(ctx, &f, (int)method, r.pixel.data(), &n, r.xyz.data(), r.feat.data(), r.C ? r.label.data() : nullptr, r.geo.data());
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_stereo_points: ") + cvo_last_error(ctx));
  CvoPointCloud out;
  r.fill(out, n);
  if (pixel) pixel->assign(r.pixel.begin(), r.pixel.begin() + n);
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_stereo(const ImageStereo& raw_image, const Calibration& calib,
                                                              CvoPointCloud::PointSelectionMethod method, std::vector<int>* pixel) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_stereo_frame_t f = frame_of(raw_image, calib);
  std::vector<int> px((size_t)f.rows * f.cols);
  int n = 0;
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  const int rc = cvo_cloud_upload_stereo(ctx, &f, (int)method, &out->handles[0], px.data(), &n);
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_cloud_upload_stereo: ") + cvo_last_error(ctx));
  if (pixel) pixel->assign(px.begin(), px.begin() + n);
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_stereo_recipe(const ImageStereo& raw_image, const Calibration& calib, float leaf,
                                                                     float edge_divisor, std::vector<int>* pixel,
                                                                     std::vector<unsigned char>* is_edge) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_stereo_frame_t f = frame_of(raw_image, calib);
  const size_t cap = 2 * (size_t)f.rows * f.cols;
  std::vector<int> px(cap);
  std::vector<unsigned char> edge(cap);
  int n = 0;
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  const int rc = cvo_cloud_upload_stereo_recipe(ctx, &f, leaf > 0.f ? leaf : params.multiframe_downsample_voxel_size, edge_divisor, &out->handles[0],
                                                px.data(), edge.data(), &n);
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string("cvo_cloud_upload_stereo_recipe: ") + cvo_last_error(ctx));
  if (pixel) pixel->assign(px.begin(), px.begin() + n);
  if (is_edge) is_edge->assign(edge.begin(), edge.begin() + n);
  return out;
}

}  // namespace cvo
