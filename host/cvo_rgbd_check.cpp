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
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"

namespace {

struct Array {
  std::vector<char> bytes;
  std::vector<int> shape;
  std::string descr;  // "|u1", "<u2", "<f4"
};

std::vector<std::string> split(const std::string& s, char c) {
  std::vector<std::string> out(1);
  for (char ch : s) {
    if (ch == c)
      out.emplace_back();
    else
      out.back() += ch;
  }
  return out;
}

Array load(const std::string& arg) {
  Array a;
  const std::vector<std::string> parts = split(arg, ':');
  std::ifstream in(parts[0], std::ios::binary);
  if (!in) throw std::runtime_error("cannot open " + parts[0]);
  std::vector<char> all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (parts.size() > 1) {  // raw
    for (size_t k = 1; k < parts.size(); k++) {
      if (parts[k] == "u16") a.descr = "<u2";
      else if (parts[k] == "f32") a.descr = "<f4";
      else a.shape.push_back(std::atoi(parts[k].c_str()));
    }
    if (a.descr.empty()) a.descr = "|u1";
    a.bytes = std::move(all);
    return a;
  }
  if (all.size() < 10 || std::memcmp(all.data(), "\x93NUMPY", 6) != 0) throw std::runtime_error(parts[0] + ": neither .npy nor name:rows:cols");
  const size_t hlen = (unsigned char)all[6] == 1 ? (unsigned char)all[8] | ((size_t)(unsigned char)all[9] << 8)
                                                 : (unsigned char)all[8] | ((size_t)(unsigned char)all[9] << 8) | ((size_t)(unsigned char)all[10] << 16) | ((size_t)(unsigned char)all[11] << 24);
  const size_t hoff = (unsigned char)all[6] == 1 ? 10 : 12;
  const std::string head(all.data() + hoff, hlen);
  const size_t d = head.find("'descr'"), s = head.find("'shape'");
  if (d == std::string::npos || s == std::string::npos || head.find("'fortran_order': False") == std::string::npos) throw std::runtime_error(parts[0] + ": unsupported .npy header");
  const size_t q0 = head.find('\'', d + 7), q1 = head.find('\'', q0 + 1);
  a.descr = head.substr(q0 + 1, q1 - q0 - 1);
  const size_t p0 = head.find('(', s), p1 = head.find(')', p0);
  for (const std::string& t : split(head.substr(p0 + 1, p1 - p0 - 1), ','))
    if (t.find_first_of("0123456789") != std::string::npos) a.shape.push_back(std::atoi(t.c_str()));
  a.bytes.assign(all.begin() + (long)(hoff + hlen), all.end());
  return a;
}

unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

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
  unsigned long long h = 14695981039346656037ull;
  for (int i = 0; i < pc.num_points(); i++) {
    h = fnv(h, pc.positions()[(size_t)i].v, 12);
    for (int c = 0; c < pc.num_features(); c++) {
      const float f = pc.features()(i, c);
      h = fnv(h, &f, 4);
    }
    h = fnv(h, &pc.geometric_types()[2 * (size_t)i], 8);
  }
  std::printf("rows %016llx\n", h);
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
