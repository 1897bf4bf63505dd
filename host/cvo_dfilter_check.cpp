// The disparity post-filter through the C-ABI's CPU twin and the C++ veneer (CvoGPU::disparity_filter, CvoGPU::stereo_disparity
// with a filter, ImageStereo's (left, right, ..., dfilter) constructor).
//   cvo_dfilter_check map.npy [--config SIM SPECKLE_SIZE GAP_WIDTH MEAN] [--device params.yaml]
//   cvo_dfilter_check --pair left.npy right.npy MAX_DISPARITY [--config ...] [--device params.yaml]
// map: .npy of float32 (rows, cols), or a raw file given as name:rows:cols:f32; invalid pixels are negative.  Without --device
// the CPU twin runs (cvo_disparity_filter_host, in place: out == in); with it, the kernels on a CvoGPU.
// --pair: left / right are uint8 gray planes; builds cvo::ImageStereo(left, right, ..., dfilter) - the matcher at MAX_DISPARITY,
// then the filter - and, with --device, also runs CvoGPU::stereo_disparity with the filter, which must give the same map.
// Prints "shape <rows> <cols>" and "filtered <hash>", FNV-1a over the filtered map's bytes.
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
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s map.npy | --pair left.npy right.npy MAX_DISPARITY  [--config SIM SPECKLE_SIZE GAP_WIDTH MEAN] [--device params.yaml]\n", argv[0]);
    return 2;
  }
  try {
    cvo_dfilter_config_t cfg;
    cvo_dfilter_config_default(&cfg);
    const char* yaml = nullptr;
    std::vector<std::string> files;
    int max_disparity = 0;
    for (int i = 1; i < argc; i++) {
      const std::string o = argv[i];
      if (o == "--config" && i + 4 < argc) {
        cfg.speckle_sim_threshold = (float)std::atof(argv[++i]);
        cfg.speckle_size = std::atoi(argv[++i]);
        cfg.ipol_gap_width = std::atoi(argv[++i]);
        cfg.adaptive_mean = std::atoi(argv[++i]);
      } else if (o == "--device" && i + 1 < argc) {
        yaml = argv[++i];
      } else if (o == "--pair" && i + 3 < argc && files.empty()) {
        files = {argv[i + 1], argv[i + 2]};
        max_disparity = std::atoi(argv[i + 3]);
        i += 3;
      } else if (o.rfind("--", 0) != 0 && files.empty()) {
        files = {o};
      } else {
        throw std::runtime_error("unknown option " + o);
      }
    }
    if (files.empty()) throw std::runtime_error("no map and no pair given");
    std::unique_ptr<cvo::CvoGPU> gpu(yaml ? new cvo::CvoGPU(yaml) : nullptr);
    std::vector<float> out;
    int rows, cols;
    if (files.size() == 1) {
      const cvo_check::Array map = cvo_check::load(files[0]);
      if (map.descr != "<f4" || map.shape.size() != 2) throw std::runtime_error("the map is float32, (rows, cols)");
      rows = map.shape[0], cols = map.shape[1];
      if (map.bytes.size() != sizeof(float) * (size_t)rows * cols) throw std::runtime_error("the file's size does not match its shape");
      if (gpu) {
        out = gpu->disparity_filter(rows, cols, (const float*)map.bytes.data(), &cfg);
      } else {
        out.resize((size_t)rows * cols);
        std::memcpy(out.data(), map.bytes.data(), map.bytes.size());
        const int rc = cvo_disparity_filter_host(rows, cols, out.data(), &cfg, out.data());
        if (rc != CVO_OK) throw std::runtime_error("the library refused the map or the configuration (" + std::to_string(rc) + ")");
      }
    } else {
      const cvo_check::Array left = cvo_check::load(files[0]), right = cvo_check::load(files[1]);
      if (left.descr != "|u1" || right.descr != "|u1" || left.shape.size() != 2 || left.shape != right.shape)
        throw std::runtime_error("left and right are uint8 gray planes of one shape");
      rows = left.shape[0], cols = left.shape[1];
      if (left.bytes.size() != (size_t)rows * cols || right.bytes.size() != left.bytes.size()) throw std::runtime_error("a file's size does not match its shape");
      cvo_sgm_config_t sgm;
      cvo_sgm_config_default(&sgm);
      sgm.max_disparity = max_disparity;
      const uint8_t *l = (const uint8_t*)left.bytes.data(), *r = (const uint8_t*)right.bytes.data();
      const cvo::ImageStereo frame(l, r, rows, cols, 1, gpu.get(), &sgm, &cfg);
      out = frame.disparity();
      if (gpu && gpu->disparity_filter(rows, cols, gpu->stereo_disparity(rows, cols, l, r, &sgm).data(), &cfg) != out)
        throw std::runtime_error("the matcher followed by the filter differs from the filtered matcher");
    }
    std::printf("shape %d %d\nfiltered %016llx\n", rows, cols, cvo_check::fnv(14695981039346656037ull, out.data(), sizeof(float) * out.size()));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_dfilter_check: %s\n", e.what());
    return 1;
  }
}
