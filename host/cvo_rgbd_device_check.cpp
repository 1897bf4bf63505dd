// RGB-D frames that are already in device memory, through the C++ veneer (CvoGPU::upload_rgbd_points_device /
// upload_rgbd_device), and the CPU twin of their rows (cvo_rgbd_frame_rows_host) on its own.
//   cvo_rgbd_device_check image depth calib.txt METHOD [--semantic scores] [--device params.yaml] [--leaf L] [--divisor D]
// image: .npy of uint8, (rows, cols) or (rows, cols, 3); depth: .npy of uint16 or float32; scores: .npy of float32, (rows, cols,
// classes); or raw files as cvo_rgbd_check takes them.  calib.txt: upstream's RGBD calibration file.  METHOD: FULL | DSO_EDGES
// | RECIPE.  The scores are handed over as C x H x W, the layout a network leaves them in.
// Without --device no GPU is touched: the pixels come from cvo_rgbd_points_host (RECIPE: DSO_EDGES' as edges, then FULL's) and
// the rows from the twin - the program a host sanitizer is run on.  With --device the planes are copied into device memory
// and the veneer builds the resident cloud from them; its rows are read back with CvoGPU::download.
// Prints "n <points>", the pixel index of every point on one line, and "rows <hash>": FNV-1a over the bytes of xyz, 5
// features, the class scores the cloud holds (19, or none) and the geometric type, point by point.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"

namespace {

using cvo_check::Array;
using cvo_check::fnv;
using cvo_check::load;

struct DevicePlane {
  void* p = nullptr;
  DevicePlane(const void* host, size_t bytes) {
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("device copy failed");
  }
  ~DevicePlane() { (void)hipFree(p); }
  DevicePlane(const DevicePlane&) = delete;
  DevicePlane& operator=(const DevicePlane&) = delete;
};

void print(int n, const std::vector<int>& pixel, unsigned long long hash) {
  std::printf("n %d\n", n);
  for (int p : pixel) std::printf("%d ", p);
  std::printf("\nrows %016llx\n", hash);
}

int run(const Array& img, const Array& dep, const Array* sem, const cvo::Calibration& calib, const std::string& method, const char* yaml, float leaf,
        float divisor) {
  const int rows = img.shape[0], cols = img.shape[1], ch = img.shape.size() > 2 ? img.shape[2] : 1;
  const size_t np = (size_t)rows * cols, depth_size = dep.descr == "<u2" ? 2 : 4;
  if (dep.bytes.size() != depth_size * np || img.bytes.size() != np * (size_t)ch) throw std::runtime_error("image / depth sizes disagree");
  const int classes = sem ? sem->shape[2] : 0;
  std::vector<float> chw(np * (size_t)classes);  // C x H x W
  for (size_t p = 0; sem && p < np; p++)
    for (int c = 0; c < classes; c++) chw[(size_t)c * np + p] = ((const float*)sem->bytes.data())[p * (size_t)classes + c];
  const bool recipe = method == "RECIPE";
  if (!recipe && method != "FULL" && method != "DSO_EDGES") throw std::runtime_error("METHOD is FULL, DSO_EDGES or RECIPE");
  const int m = method == "FULL" ? CVO_SELECT_FULL : CVO_SELECT_DSO_EDGES;
  cvo_rgbd_device_frame_t f{};
  f.rows = rows;
  f.cols = cols;
  f.channels = ch;
  f.image = img.bytes.data();
  f.depth = dep.bytes.data();
  f.depth_type = depth_size == 2 ? CVO_DEPTH_U16 : CVO_DEPTH_F32;
  f.fx = calib.intrinsic()(0, 0);
  f.fy = calib.intrinsic()(1, 1);
  f.cx = calib.intrinsic()(0, 2);
  f.cy = calib.intrinsic()(1, 2);
  f.scaling_factor = calib.scaling_factor();
  f.num_classes = classes;
  f.semantic = classes ? chw.data() : nullptr;
  f.semantic_row_stride = sizeof(float) * (size_t)cols;
  f.semantic_pixel_stride = sizeof(float);
  f.semantic_class_stride = sizeof(float) * np;
  if (!yaml) {  // the twin alone
    cvo_rgbd_frame_t h{};
    h.rows = rows, h.cols = cols, h.channels = ch;
    h.image = (const uint8_t*)f.image, h.depth = f.depth, h.depth_type = f.depth_type;
    h.fx = f.fx, h.fy = f.fy, h.cx = f.cx, h.cy = f.cy, h.scaling_factor = f.scaling_factor;
    h.num_classes = classes;
    h.semantic = classes ? (const float*)sem->bytes.data() : nullptr;
    std::vector<int> pixel, part(np);
    std::vector<unsigned char> edge;
    for (int pass = recipe ? 0 : 1; pass < 2; pass++) {
      int n = 0;
      const int pm = recipe ? (pass == 0 ? CVO_SELECT_DSO_EDGES : CVO_SELECT_FULL) : m;
      if (cvo_rgbd_points_host(&h, pm, part.data(), &n, nullptr, nullptr, nullptr, nullptr) != CVO_OK) throw std::runtime_error("cvo_rgbd_points_host refused the frame");
      pixel.insert(pixel.end(), part.begin(), part.begin() + n);
      edge.insert(edge.end(), (size_t)n, (unsigned char)(recipe && pass == 0));
    }
    const size_t n = pixel.size();
    std::vector<float> xyz(3 * n), feat(5 * n), label(19 * n), geo(2 * n);
    std::vector<unsigned char> excluded(n);
    if (cvo_rgbd_frame_rows_host(&f, recipe, m, (int)n, pixel.data(), edge.data(), xyz.data(), feat.data(), label.data(), geo.data(), excluded.data()) != CVO_OK)
      throw std::runtime_error("cvo_rgbd_frame_rows_host refused the frame");
    unsigned long long hash = 14695981039346656037ull;
    for (size_t i = 0; i < n; i++) {
      if (excluded[i]) throw std::runtime_error("the twin excludes a pixel cvo_rgbd_points_host kept");
      hash = fnv(hash, &xyz[3 * i], 12);
      hash = fnv(hash, &feat[5 * i], 20);
      if (classes && !recipe) hash = fnv(hash, &label[19 * i], 76);
      hash = fnv(hash, &geo[2 * i], 8);
    }
    print((int)n, pixel, hash);
    return 0;
  }
  cvo::CvoGPU gpu(yaml);
  const DevicePlane d_img(f.image, img.bytes.size()), d_dep(f.depth, dep.bytes.size());
  std::unique_ptr<DevicePlane> d_sem;
  if (classes) d_sem.reset(new DevicePlane(chw.data(), sizeof(float) * chw.size()));
  f.image = d_img.p;
  f.depth = d_dep.p;
  f.semantic = classes ? d_sem->p : nullptr;
  auto cloud = recipe ? gpu.upload_rgbd_device(f, leaf, divisor) : gpu.upload_rgbd_points_device(f, (cvo::CvoPointCloud::PointSelectionMethod)m);
  const cvo::CvoPointCloud pc = gpu.download(*cloud, 0);
  unsigned long long hash = 14695981039346656037ull;
  for (int i = 0; i < pc.num_points(); i++) {
    hash = fnv(hash, pc.positions()[(size_t)i].v, 12);
    for (int c = 0; c < 5; c++) {
      const float v = c < pc.num_features() ? pc.features()(i, c) : 0.f;
      hash = fnv(hash, &v, 4);
    }
    for (int c = 0; c < 19 && pc.num_classes() > 0; c++) {
      const float v = c < pc.num_classes() ? pc.labels()(i, c) : 0.f;
      hash = fnv(hash, &v, 4);
    }
    hash = fnv(hash, &pc.geometric_types()[2 * (size_t)i], 8);
  }
  print(cloud->num_points(0), cloud->kept(0), hash);
  return 0;
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s image depth calib.txt FULL|DSO_EDGES|RECIPE [--semantic scores] [--device params.yaml] [--leaf L] [--divisor D]\n", argv[0]);
    return 2;
  }
  try {
    const Array img = load(argv[1]), dep = load(argv[2]);
    const cvo::Calibration calib(std::string(argv[3]), cvo::Calibration::RGBD);
    const char* yaml = nullptr;
    float leaf = 0.f, divisor = 4.f;
    Array sem;
    bool has_sem = false;
    for (int i = 5; i + 1 < argc; i += 2) {
      if (!std::strcmp(argv[i], "--device")) yaml = argv[i + 1];
      else if (!std::strcmp(argv[i], "--leaf")) leaf = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--divisor")) divisor = (float)std::atof(argv[i + 1]);
      else if (!std::strcmp(argv[i], "--semantic")) sem = load(argv[i + 1]), has_sem = true;
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    if (img.shape.size() < 2 || dep.shape.size() != 2) throw std::runtime_error("image is (rows, cols[, 3]), depth (rows, cols)");
    if (dep.descr != "<u2" && dep.descr != "<f4") throw std::runtime_error("depth is uint16 or float32");
    if (has_sem && (sem.descr != "<f4" || sem.shape.size() != 3 || sem.shape[0] != img.shape[0] || sem.shape[1] != img.shape[1]))
      throw std::runtime_error("scores are float32 (rows, cols, classes)");
    return run(img, dep, has_sem ? &sem : nullptr, calib, argv[4], yaml, leaf, divisor);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_rgbd_device_check: %s\n", e.what());
    return 1;
  }
}
