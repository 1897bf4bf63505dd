// The stereo matcher through the C-ABI's CPU twin and the C++ veneer (CvoGPU::stereo_disparity, ImageStereo's (left, right)
// constructor).
//   cvo_sgm_check left.npy right.npy [--config D P1 P2 UNIQUENESS LR_MAX_DIFF PATHS] [--device params.yaml] [--points calib.txt METHOD]
// left / right: .npy of uint8, (rows, cols) or (rows, cols, 3) (BGR: to gray by RawImage's formula), or raw files given as
// name:rows:cols[:channels].  Without --device the CPU twin runs (cvo_stereo_disparity_host); with it, the kernels on a CvoGPU.
// Without --points: gray planes only; prints "shape <rows> <cols>" and "disparity <hash>", FNV-1a over the map's bytes.
// With --points: builds cvo::ImageStereo(left, right, ...) and prints what cvo_stereo_check prints of
// CvoPointCloud(frame, calib, METHOD) (CV_FAST | DSO_EDGES | FULL; on the host), after the same two lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"

int main(int argc, char* argv[]) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s left right [--config D P1 P2 UNIQUENESS LR_MAX_DIFF PATHS] [--device params.yaml] [--points calib.txt METHOD]\n", argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array left = cvo_check::load(argv[1]), right = cvo_check::load(argv[2]);
    if (left.descr != "|u1" || right.descr != "|u1" || left.shape.size() < 2 || left.shape.size() > 3 || left.shape != right.shape)
      throw std::runtime_error("left and right are uint8 images of one shape, (rows, cols) or (rows, cols, 3)");
    const int rows = left.shape[0], cols = left.shape[1], ch = left.shape.size() > 2 ? left.shape[2] : 1;
    if (left.bytes.size() != (size_t)rows * cols * ch || right.bytes.size() != left.bytes.size()) throw std::runtime_error("a file's size does not match its shape");
    cvo_sgm_config_t cfg;
    cvo_sgm_config_default(&cfg);
    const char *yaml = nullptr, *calib_file = nullptr;
    std::string method;
    for (int i = 3; i < argc; i++) {
      const std::string o = argv[i];
      if (o == "--config" && i + 6 < argc) {
        int* field[6] = {&cfg.max_disparity, &cfg.p1, &cfg.p2, &cfg.uniqueness, &cfg.lr_max_diff, &cfg.paths};
        for (int k = 0; k < 6; k++) *field[k] = std::atoi(argv[++i]);
      } else if (o == "--device" && i + 1 < argc) {
        yaml = argv[++i];
      } else if (o == "--points" && i + 2 < argc) {
        calib_file = argv[++i];
        method = argv[++i];
      } else {
        throw std::runtime_error("unknown option " + o);
      }
    }
    const uint8_t *l = (const uint8_t*)left.bytes.data(), *r = (const uint8_t*)right.bytes.data();
    std::unique_ptr<cvo::CvoGPU> gpu(yaml ? new cvo::CvoGPU(yaml) : nullptr);
    const size_t np = (size_t)rows * cols;
    if (!calib_file) {
      if (ch != 1) throw std::runtime_error("without --points the images are gray planes");
      std::vector<float> disparity(np);
      if (gpu) {
        disparity = gpu->stereo_disparity(rows, cols, l, r, &cfg);
      } else {
        const int rc = cvo_stereo_disparity_host(rows, cols, l, r, &cfg, disparity.data());
        if (rc != CVO_OK) throw std::runtime_error("the library refused the images or the configuration (" + std::to_string(rc) + ")");
      }
      std::printf("shape %d %d\ndisparity %016llx\n", rows, cols, cvo_check::fnv(14695981039346656037ull, disparity.data(), sizeof(float) * np));
      return 0;
    }
    cvo::CvoPointCloud::PointSelectionMethod m;
    if (method == "CV_FAST") m = cvo::CvoPointCloud::CV_FAST;
    else if (method == "DSO_EDGES") m = cvo::CvoPointCloud::DSO_EDGES;
    else if (method == "FULL") m = cvo::CvoPointCloud::FULL;
    else throw std::runtime_error("METHOD is CV_FAST, DSO_EDGES or FULL");
    const cvo::Calibration calib(std::string(calib_file), cvo::Calibration::STEREO);
    const cvo::ImageStereo frame(l, r, rows, cols, ch, gpu.get(), &cfg);
    std::printf("shape %d %d\ndisparity %016llx\n", rows, cols, cvo_check::fnv(14695981039346656037ull, frame.disparity().data(), sizeof(float) * np));
    std::vector<int> pixel;
    const cvo::CvoPointCloud pc(frame, calib, m, &pixel);
    std::printf("n %d\n", pc.num_points());
    for (int p : pixel) std::printf("%d ", p);
    std::printf("\nrows %016llx\n", cvo_check::rows_hash(pc));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_sgm_check: %s\n", e.what());
    return 1;
  }
}
