// cvo::ImageStereo (upstream utils/ImageStereo.hpp): the left RawImage with its left disparity map, in pixels.
// Raw buffers in place of cv::Mat; no denoising inside the class: CvoGPU::nlm_denoise(_lab) first (see RawImage.hpp).
//
// NOT here: upstream's ImageStereo(left, right) constructor computes the disparity with libelas
// (StaticStereo::disparity, StaticStereo.cpp:20-64).  libelas is not part of this library: the caller runs its own matcher
// and hands the RESULT to this class (libelas codes invalid pixels as -10; every disparity below 0.05 is rejected).
#pragma once
#include <vector>

#include "utils/RawImage.hpp"

namespace cvo {

class ImageStereo : public RawImage {
 public:
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
