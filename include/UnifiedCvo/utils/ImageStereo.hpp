// cvo::ImageStereo (upstream utils/ImageStereo.hpp): the left RawImage with its left disparity map, in pixels.
// Raw buffers in place of cv::Mat; no denoising inside the class: CvoGPU::nlm_denoise(_lab) first (see RawImage.hpp).
//
// Upstream's ImageStereo(left, right) constructor computes the disparity with libelas (StaticStereo::disparity,
// StaticStereo.cpp:20-64).  libelas is not part of this library.  The (left, right, ...) constructor below computes it with
// the library's OWN matcher (cvo_stereo_disparity, include/cvo_hip.h: semi-global matching over a census cost, stated in
// tests/np_sgm.py) - another algorithm, so its map, and the poses that follow from it, differ from upstream's; the three
// passes libelas runs on its map afterwards (speckle, gap, adaptive mean) are built and optional (cvo_disparity_filter).  A caller who
// wants libelas's (or any other matcher's) map runs that matcher and hands the RESULT to the other constructors (invalid
// pixels are coded -10 by both; every disparity below 0.05 is rejected).
#pragma once
#include <vector>

#include "cvo_hip.h"
#include "utils/RawImage.hpp"

namespace cvo {

class CvoGPU;

class ImageStereo : public RawImage {
 public:
  // New: upstream's missing constructor over raw buffers.  left / right: rows x cols x channels bytes (1 channel, or BGR, which
  // goes to gray by RawImage's formula); the disparity is cvo_stereo_disparity's on gpu's context (CvoGPU::stereo_disparity),
  // or - gpu == nullptr - the CPU twin's (cvo_stereo_disparity_host, one thread).  config == nullptr: cvo_sgm_config_default.
  // dfilter given: the map then goes through libelas's three post-passes (cvo_disparity_filter: speckle, gap, adaptive mean),
  // as upstream's does inside libelas; nullptr: the raw map, as before.
  // Refusals throw std::invalid_argument.  Defined in host/cvo_sgm.cpp.
  ImageStereo(const uint8_t* left_image, const uint8_t* right_image, int rows, int cols, int channels, const CvoGPU* gpu = nullptr,
              const cvo_sgm_config_t* config = nullptr, const cvo_dfilter_config_t* dfilter = nullptr);
  ImageStereo(const uint8_t* left_image, int rows, int cols, int channels, const std::vector<float>& left_disparity)
      : RawImage(left_image, rows, cols, channels), disparity_(left_disparity) {
    check();
  }
  ImageStereo(const uint8_t* left_image, int rows, int cols, int channels, const std::vector<float>& left_disparity, int num_classes,
              const std::vector<float>& semantics)
      : RawImage(left_image, rows, cols, channels, num_classes, semantics), disparity_(left_disparity) {
    check();
  }
  const std::vector<float>& disparity() const { return disparity_; }

 private:
  void check() const {
    if (disparity_.size() != (size_t)rows() * cols()) throw std::invalid_argument("ImageStereo: disparity needs rows x cols entries");
  }
  std::vector<float> disparity_;
};

}  // namespace cvo
