// The stereo front end through the C++ veneer (utils/ImageStereo.hpp, utils/Calibration.hpp, CvoPointCloud's stereo
// constructor, CvoGPU::stereo_points / upload_stereo / upload_stereo_recipe).
//   cvo_stereo_check image disparity calib.txt METHOD [--device params.yaml] [--leaf L] [--divisor D] [--gray gray]
// image / gray: .npy of uint8, (rows, cols) or (rows, cols, 3); disparity: .npy of float32, (rows, cols); or raw files given
// as name:rows:cols[:channels] (disparity raw: name:rows:cols:f32).  calib.txt: upstream's stereo calibration file
// ("fx fy cx cy baseline").  METHOD: CV_FAST | DSO_EDGES | FULL (the constructor; host unless --device), UPLOAD (upload_stereo
// with CV_FAST; needs --device) or RECIPE (upload_stereo_recipe; needs --device).
// Prints "n <points>", the pixel index of every point on one line, for RECIPE a line of 0 / 1 (is_edge), and for the
// constructor "rows <hash>": FNV-1a over the bytes of xyz, features and geometric types, point by point.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"

int main(int argc, char* argv[]) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s image disparity calib.txt CV_FAST|DSO_EDGES|FULL|UPLOAD|RECIPE [--device params.yaml] [--leaf L] [--divisor D] [--gray gray]\n",
                 argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array img = cvo_check::load(argv[1]), disp = cvo_check::load(argv[2]);
    const cvo::Calibration calib(std::string(argv[3]), cvo::Calibration::STEREO);
    const std::string method = argv[4];
    const char* yaml = nullptr;
    float leaf = 0.f, divisor = 5.f;
    cvo_check::Array gray;
    bool has_gray = false;
    for (int i = 5; i + 1 < argc; i += 2) {
      if (!std::strcmp(argv[i], "--device")) yaml = argv[i + 1];
      else if (!std::strcmp(argv[i], "--leaf")) leaf = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--divisor")) divisor = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--gray")) gray = cvo_check::load(argv[i + 1]), has_gray = true;
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    if (img.shape.size() < 2 || disp.shape.size() != 2 || disp.descr != "<f4") throw std::runtime_error("image is (rows, cols[, 3]), disparity (rows, cols) float32");
    const int rows = img.shape[0], cols = img.shape[1], ch = img.shape.size() > 2 ? img.shape[2] : 1;
    if (disp.bytes.size() != sizeof(float) * (size_t)rows * cols || img.bytes.size() != (size_t)rows * cols * ch) throw std::runtime_error("image / disparity sizes disagree");
    const float* d = (const float*)disp.bytes.data();
    cvo::ImageStereo frame((const uint8_t*)img.bytes.data(), rows, cols, ch, std::vector<float>(d, d + (size_t)rows * cols));
    if (has_gray) frame.set_gray((const uint8_t*)gray.bytes.data());
    std::vector<int> pixel;
    if (method == "RECIPE" || method == "UPLOAD") {
      if (!yaml) throw std::runtime_error(method + " needs --device params.yaml");
      cvo::CvoGPU gpu(yaml);
      std::vector<unsigned char> edge;
      auto cloud = method == "RECIPE" ? gpu.upload_stereo_recipe(frame, calib, leaf, divisor, &pixel, &edge)
                                      : gpu.upload_stereo(frame, calib, cvo::CvoPointCloud::CV_FAST, &pixel);
      std::printf("n %d\n", cloud->num_points(0));
      for (int p : pixel) std::printf("%d ", p);
      std::printf("\n");
      for (unsigned char e : edge) std::printf("%d ", (int)e);
      std::printf("\n");
      return 0;
    }
    cvo::CvoPointCloud::PointSelectionMethod m;
    if (method == "CV_FAST") m = cvo::CvoPointCloud::CV_FAST;
    else if (method == "DSO_EDGES") m = cvo::CvoPointCloud::DSO_EDGES;
    else if (method == "FULL") m = cvo::CvoPointCloud::FULL;
    else throw std::runtime_error("METHOD is CV_FAST, DSO_EDGES, FULL, UPLOAD or RECIPE");
    const cvo::CvoPointCloud pc = yaml ? cvo::CvoGPU(yaml).stereo_points(frame, calib, m, &pixel) : cvo::CvoPointCloud(frame, calib, m, &pixel);
    std::printf("n %d\n", pc.num_points());
    for (int p : pixel) std::printf("%d ", p);
    std::printf("\nrows %016llx\n", cvo_check::rows_hash(pc));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_stereo_check: %s\n", e.what());
    return 1;
  }
}
