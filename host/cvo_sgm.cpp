// cvo::CvoGPU::stereo_disparity, cvo::CvoGPU::disparity_filter and cvo::ImageStereo's (left, right) constructor over the C-ABI
// (cvo_stereo_disparity(_filtered / _host), cvo_disparity_filter(_host), include/cvo_hip.h): the library's own stereo matcher,
// not upstream's libelas, and libelas's three post-passes on its map.
#include <mutex>
#include <stdexcept>
#include <string>

#include "cvo/CvoGPU.hpp"

namespace cvo {
namespace {

cvo_sgm_config_t config_or_default(const cvo_sgm_config_t* config) {
  cvo_sgm_config_t c;
  cvo_sgm_config_default(&c);
  return config ? *config : c;
}

// the gray plane of a 1-channel or BGR image, by RawImage's formula
std::vector<uint8_t> gray_plane(const uint8_t* image, int rows, int cols, int channels) {
  if (!image || rows < 1 || cols < 1 || (channels != 1 && channels != 3)) throw std::invalid_argument("ImageStereo: images are rows x cols x 1 or 3 bytes");
  const size_t np = (size_t)rows * cols;
  std::vector<uint8_t> g(np);
  for (size_t p = 0; p < np; p++)
    g[p] = channels == 1 ? image[p] : (uint8_t)((1868 * (int)image[3 * p] + 9617 * (int)image[3 * p + 1] + 4899 * (int)image[3 * p + 2] + 8192) >> 14);
  return g;
}

}  // namespace

std::vector<float> CvoGPU::stereo_disparity(int rows, int cols, const unsigned char* left, const unsigned char* right,
                                            const cvo_sgm_config_t* config, const cvo_dfilter_config_t* dfilter) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_sgm_config_t cfg = config_or_default(config);
  std::vector<float> out(rows > 0 && cols > 0 ? (size_t)rows * cols : 0);
  float none = 0.f;
  float* map = out.empty() ? &none : out.data();
  const int rc = dfilter ? cvo_stereo_disparity_filtered(ctx, rows, cols, left, right, &cfg, dfilter, map) : cvo_stereo_disparity(ctx, rows, cols, left, right, &cfg, map);
  if (rc == CVO_E_INVALID || rc == CVO_E_UNSUPPORTED) throw std::invalid_argument(std::string("cvo_stereo_disparity: ") + cvo_last_error(ctx));
  if (rc != CVO_OK) throw std::runtime_error(std::string("cvo_stereo_disparity: ") + cvo_last_error(ctx));
  return out;
}

std::vector<float> CvoGPU::disparity_filter(int rows, int cols, const float* disparity, const cvo_dfilter_config_t* config) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  cvo_dfilter_config_t cfg;
  cvo_dfilter_config_default(&cfg);
  if (config) cfg = *config;
  std::vector<float> out(rows > 0 && cols > 0 ? (size_t)rows * cols : 0);
  float none = 0.f;
  const int rc = cvo_disparity_filter(ctx, rows, cols, disparity, &cfg, out.empty() ? &none : out.data());
  if (rc == CVO_E_INVALID || rc == CVO_E_UNSUPPORTED) throw std::invalid_argument(std::string("cvo_disparity_filter: ") + cvo_last_error(ctx));
  if (rc != CVO_OK) throw std::runtime_error(std::string("cvo_disparity_filter: ") + cvo_last_error(ctx));
  return out;
}

ImageStereo::ImageStereo(const uint8_t* left_image, const uint8_t* right_image, int rows, int cols, int channels, const CvoGPU* gpu,
                         const cvo_sgm_config_t* config, const cvo_dfilter_config_t* dfilter)
    : RawImage(left_image, rows, cols, channels) {
  const std::vector<uint8_t> left = gray_plane(left_image, rows, cols, channels), right = gray_plane(right_image, rows, cols, channels);
  if (gpu) {
    disparity_ = gpu->stereo_disparity(rows, cols, left.data(), right.data(), config, dfilter);
  } else {
    const cvo_sgm_config_t cfg = config_or_default(config);
    disparity_.resize((size_t)rows * cols);
    int rc = cvo_stereo_disparity_host(rows, cols, left.data(), right.data(), &cfg, disparity_.data());
    if (rc != CVO_OK) throw std::invalid_argument("ImageStereo: cvo_stereo_disparity_host refused the images or the configuration (" + std::to_string(rc) + ")");
    if (dfilter && (rc = cvo_disparity_filter_host(rows, cols, disparity_.data(), dfilter, disparity_.data())) != CVO_OK)
      throw std::invalid_argument("ImageStereo: cvo_disparity_filter_host refused the configuration (" + std::to_string(rc) + ")");
  }
  check();
}

}  // namespace cvo
