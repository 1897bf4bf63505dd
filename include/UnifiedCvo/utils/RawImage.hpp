// cvo::RawImage (upstream utils/RawImage.hpp, RawImage.cpp) over raw buffers in place of cv::Mat: the colour image, the
// float gray plane, its central-difference gradient and - optionally - a per-pixel class distribution.
//
// NOT in this class: upstream's constructor first runs cv::fastNlMeansDenoising(Colored) on the image (RawImage.cpp:21-24).
// The library has that step as a call of its own - cvo_nlm_denoise / cvo_nlm_denoise_lab (include/cvo_hip.h),
// CvoGPU::nlm_denoise / nlm_denoise_lab - and a caller who wants upstream's numbers hands its RESULT to this class (colour
// frames: BGR -> Lab with the caller's OpenCV, nlm_denoise_lab, Lab -> BGR).
// The gray plane of a 3-channel (BGR) image is OpenCV 3's 8-bit COLOR_BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14;
// OpenCV 4 differs by one level at rare pixels, so set_gray() takes the plane of the caller's own OpenCV.
// Header-only, host compiler only.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace cvo {

class RawImage {
 public:
  RawImage() = default;
  // image: rows x cols x channels bytes (channels 1 or 3, BGR order), copied
  RawImage(const uint8_t* image, int rows, int cols, int channels) : rows_(rows), cols_(cols), channels_(channels) {
    if (rows < 1 || cols < 1 || (channels != 1 && channels != 3) || !image) throw std::invalid_argument("RawImage: rows, cols >= 1, channels 1 or 3");
    image_.assign(image, image + (size_t)rows * cols * channels);
  }
  RawImage(const uint8_t* image, int rows, int cols, int channels, int num_classes, const std::vector<float>& semantic)
      : RawImage(image, rows, cols, channels) {
    if (num_classes < 0 || semantic.size() != (size_t)rows * cols * (size_t)num_classes) throw std::invalid_argument("RawImage: semantic needs rows x cols x num_classes floats");
    num_class_ = num_classes;
    semantic_image_ = semantic;
  }
  // the 8-bit gray plane the gradient is taken of, in place of the BGR -> gray formula (rows x cols bytes, copied)
  void set_gray(const uint8_t* gray) {
    gray_.assign(gray, gray + (size_t)rows_ * cols_);
    intensity_.clear();
  }

  const std::vector<uint8_t>& image() const { return image_; }
  const std::vector<uint8_t>& gray() const { return gray_; }  // empty unless set_gray was called
  int rows() const { return rows_; }
  int cols() const { return cols_; }
  int channels() const { return channels_; }
  int num_classes() const { return num_class_; }
  const std::vector<float>& semantic_image() const { return semantic_image_; }
  // the float gray plane; gradient_: (dx, dy) interleaved per pixel, 0.5 x central differences, zero on the border rows
  // and columns; gradient_square: dx^2 + dy^2 (RawImage.cpp:55-82).  Computed on first use.
  const std::vector<float>& intensity() const { return ensure(), intensity_; }
  const std::vector<float>& gradient() const { return ensure(), gradient_; }
  const std::vector<float>& gradient_square() const { return ensure(), gradient_square_; }

 private:
  void ensure() const {
    if (!intensity_.empty() || image_.empty()) return;
    const size_t n = (size_t)rows_ * cols_;
    intensity_.resize(n);
    for (size_t p = 0; p < n; p++) {
      if (!gray_.empty())
        intensity_[p] = (float)gray_[p];
      else if (channels_ == 1)
        intensity_[p] = (float)image_[p];
      else
        intensity_[p] = (float)((1868 * (int)image_[3 * p] + 9617 * (int)image_[3 * p + 1] + 4899 * (int)image_[3 * p + 2] + 8192) >> 14);
    }
    gradient_.assign(2 * n, 0.f);
    gradient_square_.assign(n, 0.f);
    for (int y = 1; y + 1 < rows_; y++)
      for (int x = 1; x + 1 < cols_; x++) {
        const size_t p = (size_t)y * cols_ + x;
        const float dx = 0.5f * (intensity_[p + 1] - intensity_[p - 1]), dy = 0.5f * (intensity_[p + cols_] - intensity_[p - cols_]);
        gradient_[2 * p] = dx;
        gradient_[2 * p + 1] = dy;
        gradient_square_[p] = dx * dx + dy * dy;
      }
  }

  int rows_ = 0, cols_ = 0, channels_ = 0, num_class_ = 0;
  std::vector<uint8_t> image_, gray_;
  std::vector<float> semantic_image_;
  mutable std::vector<float> intensity_, gradient_, gradient_square_;
};

}  // namespace cvo
