// cvo::ImageRGBD<DepthType> (upstream utils/ImageRGBD.hpp): a RawImage with its depth image, DepthType uint16_t or float.
// Raw buffers in place of cv::Mat; no denoising inside the class: CvoGPU::nlm_denoise(_lab) first (see RawImage.hpp).
#pragma once
#include <vector>

#include "utils/RawImage.hpp"

namespace cvo {

template <typename DepthType>
class ImageRGBD : public RawImage {
 public:
  ImageRGBD(const uint8_t* image, int rows, int cols, int channels, const std::vector<DepthType>& depth_image)
      : RawImage(image, rows, cols, channels), depth_image_(depth_image) {
    check();
  }
  ImageRGBD(const uint8_t* image, int rows, int cols, int channels, const std::vector<DepthType>& depth_image, int num_classes,
            const std::vector<float>& semantics)
      : RawImage(image, rows, cols, channels, num_classes, semantics), depth_image_(depth_image) {
    check();
  }
  const std::vector<DepthType>& depth_image() const { return depth_image_; }

 private:
  void check() const {
    if (depth_image_.size() != (size_t)rows() * cols()) throw std::invalid_argument("ImageRGBD: depth needs rows x cols entries");
  }
  std::vector<DepthType> depth_image_;
};

}  // namespace cvo
