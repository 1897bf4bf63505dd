// The semantic voxel map through the C++ veneer (mapping/bkioctomap.h), with the statements of upstream's driver.
//   cvo_bki_check case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE [--device params.yaml]
// case.npy: float32 (rows, 4 + 3 + 5 + NUM_CLASS): per row the frame's number, the frame's origin, then a hit - x y z, five
// features, NUM_CLASS label values -, frames in ascending order, hits already in the map frame.  Without --device the CPU twin.
// Prints "cloud <n>", "rows <hash>" - FNV-1a over the bytes of xyz, features and labels of the cloud read out, row by row - and
// "on_device <0|1>": where the map's last insert ran (cvo_debug_map_stats).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"
#include "cvo_hip_debug.h"
#include "mapping/bkioctomap.h"

int main(int argc, char* argv[]) {
  if (argc < 9) {
    std::fprintf(stderr, "usage: %s case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE [--device params.yaml]\n", argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array in = cvo_check::load(argv[1]);
    const int num_class = std::atoi(argv[2]);
    const float resolution = (float)std::atof(argv[3]), prior = (float)std::atof(argv[4]), free_thresh = (float)std::atof(argv[5]),
                occupied_thresh = (float)std::atof(argv[6]), free_resolution = (float)std::atof(argv[7]), max_range = (float)std::atof(argv[8]);
    const char* yaml = nullptr;
    for (int i = 9; i < argc; i++) {
      if (std::string(argv[i]) == "--device" && i + 1 < argc) yaml = argv[++i];
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    const int width = 12 + num_class;
    if (in.descr != "<f4" || in.shape.size() != 2 || in.shape[1] != width) throw std::runtime_error("the case is float32, (rows, 12 + NUM_CLASS)");
    const float* row = (const float*)in.bytes.data();
    const int rows = in.shape[0];
    std::unique_ptr<cvo::CvoGPU> gpu(yaml ? new cvo::CvoGPU(yaml) : nullptr);
    // ---- the driver's statements ----
    const int block_depth = 1;
    const double sf2 = 1.0, ell = 1.0;
    const float var_thresh = 1.0f;
    const double ds_resolution = -1;
    std::unique_ptr<semantic_bki::SemanticBKIOctoMap> map_csm(
        gpu ? new semantic_bki::SemanticBKIOctoMap(*gpu, resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh)
            : new semantic_bki::SemanticBKIOctoMap(resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh));
    for (int r = 0; r < rows;) {
      int end = r;
      while (end < rows && row[(size_t)end * width] == row[(size_t)r * width]) end++;
      cvo::CvoPointCloud transformed_pc(5, num_class);
      transformed_pc.reserve(end - r, 5, num_class);
      for (int i = r; i < end; i++) {
        const float* p = row + (size_t)i * width;
        transformed_pc.add_point(i - r, cvo::Vec3f{{p[4], p[5], p[6]}}, std::vector<float>(p + 7, p + 12), std::vector<float>(p + 12, p + 12 + num_class), {0.f, 0.f});
      }
      semantic_bki::point3f origin(row[(size_t)r * width + 1], row[(size_t)r * width + 2], row[(size_t)r * width + 3]);
      map_csm->insert_pointcloud_csm(&transformed_pc, origin, ds_resolution, free_resolution, max_range);
      r = end;
    }
    cvo::CvoPointCloud cloud_out(map_csm.get(), num_class);
    // ---- ----
    unsigned long long h = 14695981039346656037ull;
    for (int i = 0; i < cloud_out.num_points(); i++) {
      const cvo::Vec3f p = cloud_out.positions()[(size_t)i];
      h = cvo_check::fnv(h, p.v, sizeof p.v);
      for (int c = 0; c < 5; c++) {
        const float f = cloud_out.features()(i, c);
        h = cvo_check::fnv(h, &f, sizeof f);
      }
      for (int c = 0; c < num_class; c++) {
        const float l = cloud_out.labels()(i, c);
        h = cvo_check::fnv(h, &l, sizeof l);
      }
    }
    int on_device = 0;
    if (map_csm->handle() && cvo_debug_map_stats(map_csm->handle(), &on_device, nullptr, nullptr, nullptr, nullptr) != CVO_OK) throw std::runtime_error("cvo_debug_map_stats failed");
    std::printf("cloud %d\nrows %016llx\non_device %d\n", cloud_out.num_points(), h, on_device);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_bki_check: %s\n", e.what());
    return 1;
  }
}
