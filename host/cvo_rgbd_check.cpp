// The RGB-D front end through the C++ veneer (utils/ImageRGBD.hpp, utils/Calibration.hpp, CvoPointCloud's image
// constructor, CvoGPU::rgbd_points / upload_rgbd).
//   cvo_rgbd_check image depth calib.txt METHOD [--device params.yaml] [--leaf L] [--divisor D] [--gray gray]
// image / gray: .npy of uint8, (rows, cols) or (rows, cols, 3); depth: .npy of uint16 or float32, (rows, cols); or raw
// files given as name:rows:cols[:channels] (depth raw: name:rows:cols:u16 | f32).  calib.txt: upstream's RGBD calibration
// file.  METHOD: FULL | DSO_EDGES (the constructor; host unless --device) or RECIPE (upload_rgbd; needs --device).
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

namespace {

using cvo_check::Array;
using cvo_check::load;

template <typename DepthType>
int run(const Array& img, const Array& dep, const Array* gray, const cvo::Calibration& calib, const std::string& method, const char* yaml, float leaf,
        float divisor) {
  const int rows = img.shape[0], cols = img.shape[1], ch = img.shape.size() > 2 ? img.shape[2] : 1;
  if (dep.bytes.size() != sizeof(DepthType) * (size_t)rows * cols || img.bytes.size() != (size_t)rows * cols * ch) throw std::runtime_error("image / depth sizes disagree");
  const DepthType* d = (const DepthType*)dep.bytes.data();
  cvo::ImageRGBD<DepthType> frame((const uint8_t*)img.bytes.data(), rows, cols, ch, std::vector<DepthType>(d, d + (size_t)rows * cols));
  if (gray) frame.set_gray((const uint8_t*)gray->bytes.data());
  std::vector<int> pixel;
  if (method == "RECIPE") {
    if (!yaml) throw std::runtime_error("RECIPE needs --device params.yaml");
    cvo::CvoGPU gpu(yaml);
    std::vector<unsigned char> edge;
    auto cloud = gpu.upload_rgbd(frame, calib, leaf, divisor, &pixel, &edge);
    std::printf("n %d\n", cloud->num_points(0));
    for (int p : pixel) std::printf("%d ", p);
    std::printf("\n");
    for (unsigned char e : edge) std::printf("%d ", (int)e);
    std::printf("\n");
    return 0;
  }
  const auto m = method == "FULL" ? cvo::CvoPointCloud::FULL : cvo::CvoPointCloud::DSO_EDGES;
  if (method != "FULL" && method != "DSO_EDGES") throw std::runtime_error("METHOD is FULL, DSO_EDGES or RECIPE");
  cvo::CvoPointCloud pc = yaml ? cvo::CvoGPU(yaml).rgbd_points(frame, calib, m, &pixel) : cvo::CvoPointCloud(frame, calib, m, &pixel);
  std::printf("n %d\n", pc.num_points());
  for (int p : pixel) std::printf("%d ", p);
  std::printf("\n");
  std::printf("rows %016llx\n", cvo_check::rows_hash(pc));
  return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s image depth calib.txt FULL|DSO_EDGES|RECIPE [--device params.yaml] [--leaf L] [--divisor D] [--gray gray]\n", argv[0]);
    return 2;
  }
  try {
    const Array img = load(argv[1]), dep = load(argv[2]);
    const cvo::Calibration calib(std::string(argv[3]), cvo::Calibration::RGBD);
    const char* yaml = nullptr;
    float leaf = 0.f, divisor = 4.f;
    Array gray;
    bool has_gray = false;
    for (int i = 5; i + 1 < argc; i += 2) {
      if (!std::strcmp(argv[i], "--device")) yaml = argv[i + 1];
      else if (!std::strcmp(argv[i], "--leaf")) leaf = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--divisor")) divisor = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--gray")) gray = load(argv[i + 1]), has_gray = true;
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    if (img.shape.size() < 2 || dep.shape.size() != 2) throw std::runtime_error("image is (rows, cols[, 3]), depth (rows, cols)");
    if (dep.descr == "<u2") return run<uint16_t>(img, dep, has_gray ? &gray : nullptr, calib, argv[4], yaml, leaf, divisor);
    if (dep.descr == "<f4") return run<float>(img, dep, has_gray ? &gray : nullptr, calib, argv[4], yaml, leaf, divisor);
    throw std::runtime_error("depth is uint16 or float32");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_rgbd_check: %s\n", e.what());
    return 1;
  }
}
