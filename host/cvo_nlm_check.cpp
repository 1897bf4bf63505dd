// The denoising through the C-ABI's CPU twin and the C++ veneer (CvoGPU::nlm_denoise / nlm_denoise_lab).
//   cvo_nlm_check image.npy [--lab H_COLOR] [--h H] [--windows T S] [--in-place] [--device params.yaml]
// image.npy: uint8 (rows, cols) or (rows, cols, channels).  Without --device cvo_nlm_denoise_host (with --lab:
// cvo_nlm_denoise_lab_host) runs; with it, the veneer's call on a CvoGPU.  Prints "shape <rows> <cols> <channels>" and
// "bytes <hash>", FNV-1a over the denoised image.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"

int main(int argc, char* argv[]) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s image.npy [--lab H_COLOR] [--h H] [--windows T S] [--in-place] [--device params.yaml]\n", argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array img = cvo_check::load(argv[1]);
    if (img.descr != "|u1" || img.shape.size() < 2 || img.shape.size() > 3) throw std::runtime_error("image is (rows, cols[, channels]) uint8");
    const int rows = img.shape[0], cols = img.shape[1], channels = img.shape.size() == 3 ? img.shape[2] : 1;
    if (img.bytes.size() != (size_t)rows * cols * channels) throw std::runtime_error("image: the file's size does not match its shape");
    cvo_nlm_config_t cfg;
    cvo_nlm_config_default(&cfg);
    bool lab = false, in_place = false;
    float h_color = 10.f;
    const char* yaml = nullptr;
    for (int i = 2; i < argc; i++) {
      const std::string o = argv[i];
      if (o == "--lab" && i + 1 < argc) {
        lab = true;
        h_color = (float)std::atof(argv[++i]);
      } else if (o == "--h" && i + 1 < argc) {
        cfg.h = (float)std::atof(argv[++i]);
      } else if (o == "--windows" && i + 2 < argc) {
        cfg.template_window = std::atoi(argv[i + 1]);
        cfg.search_window = std::atoi(argv[i + 2]);
        i += 2;
      } else if (o == "--in-place") {
        in_place = true;
      } else if (o == "--device" && i + 1 < argc) {
        yaml = argv[++i];
      } else {
        throw std::runtime_error("unknown option " + o);
      }
    }
    if (lab && channels != 3) throw std::runtime_error("--lab needs a 3-channel image");
    std::vector<unsigned char> src((const unsigned char*)img.bytes.data(), (const unsigned char*)img.bytes.data() + img.bytes.size());
    std::vector<unsigned char> out(src.size());
    unsigned char* dst = in_place ? src.data() : out.data();
    if (yaml) {
      cvo::CvoGPU gpu(yaml);
      if (lab)
        gpu.nlm_denoise_lab(rows, cols, src.data(), dst, cfg.h, h_color, cfg.template_window, cfg.search_window);
      else
        gpu.nlm_denoise(rows, cols, channels, src.data(), dst, cfg.h, cfg.template_window, cfg.search_window);
    } else {
      const int rc = lab ? cvo_nlm_denoise_lab_host(rows, cols, src.data(), &cfg, h_color, dst) : cvo_nlm_denoise_host(rows, cols, channels, src.data(), &cfg, dst);
      if (rc != CVO_OK) throw std::runtime_error("the library refused the image or the configuration (" + std::to_string(rc) + ")");
    }
    std::printf("shape %d %d %d\nbytes %016llx\n", rows, cols, channels, cvo_check::fnv(14695981039346656037ull, dst, src.size()));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_nlm_check: %s\n", e.what());
    return 1;
  }
}
