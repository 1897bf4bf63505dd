// Compiles the stereo veneer header (utils/ImageStereo.hpp, with utils/RawImage.hpp and utils/Calibration.hpp) on its own,
// host compiler only, and executes it: the disparity is held as given, sizes are checked, the stereo calibration is read.
//   stereo_headers_check stereo_calib.txt
#include <cstdio>
#include <vector>

#include "utils/Calibration.hpp"
#include "utils/ImageStereo.hpp"

int main(int argc, char* argv[]) {
  if (argc < 2) return 2;
  const int rows = 5, cols = 6;
  std::vector<uint8_t> gray((size_t)rows * cols);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) gray[(size_t)y * cols + x] = (uint8_t)(10 + 6 * x + 8 * y);
  std::vector<float> disp((size_t)rows * cols, -10.f);
  disp[7] = 0.05f;
  const cvo::ImageStereo im(gray.data(), rows, cols, 1, disp);
  const size_t p = 2 * cols + 3;
  if (im.disparity().size() != 30 || im.disparity()[7] != 0.05f || im.disparity()[8] != -10.f || im.channels() != 1) return 1;
  if (im.gradient()[2 * p] != 6.f || im.gradient()[2 * p + 1] != 8.f || im.num_classes() != 0) return 1;
  std::vector<float> sem((size_t)rows * cols * 3, 0.25f);
  const cvo::ImageStereo with_classes(gray.data(), rows, cols, 1, disp, 3, sem);
  if (with_classes.num_classes() != 3 || with_classes.semantic_image().size() != 90) return 1;
  bool threw = false;
  try {
    cvo::ImageStereo bad(gray.data(), rows, cols, 1, std::vector<float>(7));
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  if (!threw) return 1;
  const cvo::Calibration stereo(argv[1]);
  std::printf("stereo %g %g %g %g %g %g\n", stereo.intrinsic()(0, 0), stereo.intrinsic()(1, 1), stereo.intrinsic()(0, 2), stereo.intrinsic()(1, 2),
              stereo.baseline(), stereo.scaling_factor());
  std::printf("headers ok\n");
  return 0;
}
