// Compiles the RGB-D veneer headers (utils/RawImage.hpp, utils/ImageRGBD.hpp, utils/Calibration.hpp) on their own, host
// compiler only, and executes them: the gray formula, the gradient layout, the calibration file reader.
//   rgbd_headers_check rgbd_calib.txt stereo_calib.txt
#include <cstdio>
#include <vector>

#include "utils/Calibration.hpp"
#include "utils/ImageRGBD.hpp"

int main(int argc, char* argv[]) {
  if (argc < 3) return 2;
  const int rows = 5, cols = 6;
  std::vector<uint8_t> bgr((size_t)rows * cols * 3);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++)
      for (int c = 0; c < 3; c++) bgr[((size_t)y * cols + x) * 3 + c] = (uint8_t)(10 + 6 * x + 8 * y);  // gray = the same value
  std::vector<uint16_t> depth((size_t)rows * cols, 5000);
  cvo::ImageRGBD<uint16_t> im(bgr.data(), rows, cols, 3, depth);
  const size_t p = 2 * cols + 3;
  if (im.intensity()[p] != 10.f + 18.f + 16.f || im.gradient()[2 * p] != 6.f || im.gradient()[2 * p + 1] != 8.f || im.gradient_square()[p] != 100.f) return 1;
  if (im.gradient_square()[3] != 0.f || im.gradient_square()[(size_t)cols] != 0.f || im.depth_image().size() != 30 || im.channels() != 3) return 1;
  std::vector<uint8_t> gray((size_t)rows * cols, 7);
  im.set_gray(gray.data());
  if (im.intensity()[p] != 7.f || im.gradient_square()[p] != 0.f) return 1;
  std::vector<float> sem((size_t)rows * cols * 2, 0.5f), fdepth((size_t)rows * cols, 1.f);
  cvo::ImageRGBD<float> fim(gray.data(), rows, cols, 1, fdepth, 2, sem);
  if (fim.num_classes() != 2 || fim.semantic_image().size() != 60 || fim.intensity()[0] != 7.f) return 1;
  bool threw = false;
  try {
    cvo::RawImage bad(bgr.data(), rows, cols, 2);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw) return 1;
  const cvo::Calibration rgbd(argv[1], cvo::Calibration::RGBD), stereo(argv[2]);
  std::printf("rgbd %g %g %g %g %g %d %d\n", rgbd.intrinsic()(0, 0), rgbd.intrinsic()(1, 1), rgbd.intrinsic()(0, 2), rgbd.intrinsic()(1, 2),
              rgbd.scaling_factor(), rgbd.image_cols(), rgbd.image_rows());
  std::printf("stereo %g %g %g %g %g %g %d\n", stereo.intrinsic()(0, 0), stereo.intrinsic()(1, 1), stereo.intrinsic()(0, 2), stereo.intrinsic()(1, 2),
              stereo.baseline(), stereo.scaling_factor(), stereo.image_cols());
  const cvo::Calibration none(std::string("/nonexistent/calib.txt"), cvo::Calibration::RGBD);
  if (none.intrinsic()(0, 0) != 1.f || none.intrinsic()(2, 2) != 1.f || none.scaling_factor() != 0.f) return 1;
  std::printf("headers ok\n");
  return 0;
}
