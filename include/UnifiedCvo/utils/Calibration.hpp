// cvo::Calibration (upstream utils/Calibration.hpp): pinhole intrinsics + stereo baseline or RGB-D depth scaling factor,
// read from upstream's text files: "fx fy cx cy baseline [cols rows]" (STEREO, scaling factor 1) or
// "fx fy cx cy scaling_factor [cols rows]" (RGBD).  A file that cannot be opened leaves the identity, as upstream.
#pragma once
#include <fstream>
#include <string>

#include "utils/data_type.hpp"

namespace cvo {

class Calibration {
 public:
  enum PointCloudType { STEREO, RGBD };

  Calibration() = default;
  explicit Calibration(const std::string& file, PointCloudType data_type = STEREO) {
    if (data_type == STEREO) scaling_factor_ = 1.f;
    std::ifstream in(file);
    if (!in.is_open()) return;
    float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f, last = 0.f;
    in >> fx >> fy >> cx >> cy >> last;
    set_intrinsic(fx, fy, cx, cy);
    (data_type == STEREO ? baseline_ : scaling_factor_) = last;
    int c = 0, r = 0;
    if (in >> c >> r) {
      cols_ = c;
      rows_ = r;
    }
  }
  const Mat3f& intrinsic() const { return intrinsic_; }
  float baseline() const { return baseline_; }
  float scaling_factor() const { return scaling_factor_; }
  int image_cols() const { return cols_; }
  int image_rows() const { return rows_; }

 private:
  void set_intrinsic(float fx, float fy, float cx, float cy) {
    intrinsic_(0, 0) = fx;
    intrinsic_(1, 1) = fy;
    intrinsic_(0, 2) = cx;
    intrinsic_(1, 2) = cy;
  }
  Mat3f intrinsic_ = Mat3f::Identity();
  float baseline_ = 0.f, scaling_factor_ = 0.f;
  int cols_ = 0, rows_ = 0;
};

}  // namespace cvo
