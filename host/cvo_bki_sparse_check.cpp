// The semantic voxel map's two kernels through the C++ veneer (mapping/bkioctomap.h): insert_pointcloud - the sparse kernel,
// the signature upstream's header keeps commented out - and insert_pointcloud_csm, frame by frame into one map.
//   cvo_bki_sparse_check case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE SF2 ELL KERNELS [--device params.yaml]
// case.npy: as cvo_bki_check's - float32 (rows, 4 + 3 + 5 + NUM_CLASS): per row the frame's number, the frame's origin, then a
// hit.  KERNELS: one letter per frame, 's' (sparse) or 'c' (counting).  Without --device the CPU twin.
// Prints "cloud <n>", "rows <hash>" - FNV-1a over the rows of the cloud read out -, "table <voxels> <hash>" - the same over key,
// ms and fs of every stored voxel in ascending key order - and "on_device <0|1>".
#include <algorithm>
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
  if (argc < 12) {
    std::fprintf(stderr,
                 "usage: %s case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE SF2 ELL KERNELS [--device params.yaml]\n",
                 argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array in = cvo_check::load(argv[1]);
    const int num_class = std::atoi(argv[2]);
    const float resolution = (float)std::atof(argv[3]), prior = (float)std::atof(argv[4]), free_thresh = (float)std::atof(argv[5]),
                occupied_thresh = (float)std::atof(argv[6]), free_resolution = (float)std::atof(argv[7]), max_range = (float)std::atof(argv[8]),
                sf2 = (float)std::atof(argv[9]), ell = (float)std::atof(argv[10]);
    const std::string kernels = argv[11];
    const char* yaml = nullptr;
    for (int i = 12; i < argc; i++) {
      if (std::string(argv[i]) == "--device" && i + 1 < argc) yaml = argv[++i];
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    const int width = 12 + num_class;
    if (num_class < 0 || num_class > 19 || in.descr != "<f4" || in.shape.size() != 2 || in.shape[1] != width)
      throw std::runtime_error("the case is float32, (rows, 12 + NUM_CLASS)");
    if (kernels.find_first_not_of("sc") != std::string::npos) throw std::runtime_error("KERNELS holds 's' and 'c' only");
    const float* row = (const float*)in.bytes.data();
    const int rows = in.shape[0];
    std::unique_ptr<cvo::CvoGPU> gpu(yaml ? new cvo::CvoGPU(yaml) : nullptr);
    std::unique_ptr<semantic_bki::SemanticBKIOctoMap> map(
        gpu ? new semantic_bki::SemanticBKIOctoMap(*gpu, resolution, 1, num_class + 1, sf2, ell, prior, 1.0f, free_thresh, occupied_thresh)
            : new semantic_bki::SemanticBKIOctoMap(resolution, 1, num_class + 1, sf2, ell, prior, 1.0f, free_thresh, occupied_thresh));
    size_t frame = 0;
    for (int r = 0; r < rows; frame++) {
      int end = r;
      while (end < rows && row[(size_t)end * width] == row[(size_t)r * width]) end++;
      if (frame >= kernels.size()) throw std::runtime_error("KERNELS names fewer frames than the case holds");
      cvo::CvoPointCloud pc(5, num_class);
      pc.reserve(end - r, 5, num_class);
      for (int i = r; i < end; i++) {
        const float* p = row + (size_t)i * width;
        pc.add_point(i - r, cvo::Vec3f{{p[4], p[5], p[6]}}, std::vector<float>(p + 7, p + 12), std::vector<float>(p + 12, p + 12 + num_class), {0.f, 0.f});
      }
      semantic_bki::point3f origin(row[(size_t)r * width + 1], row[(size_t)r * width + 2], row[(size_t)r * width + 3]);
      if (kernels[frame] == 's') map->insert_pointcloud(&pc, origin, -1.f, free_resolution, max_range);
      else map->insert_pointcloud_csm(&pc, origin, -1.f, free_resolution, max_range);
      r = end;
    }
    cvo::CvoPointCloud out(map.get(), num_class);
    unsigned long long h = 14695981039346656037ull;
    for (int i = 0; i < out.num_points(); i++) {
      h = cvo_check::fnv(h, out.positions()[(size_t)i].v, 12);
      for (int c = 0; c < 5; c++) {
        const float f = out.features()(i, c);
        h = cvo_check::fnv(h, &f, sizeof f);
      }
      for (int c = 0; c < num_class; c++) {
        const float l = out.labels()(i, c);
        h = cvo_check::fnv(h, &l, sizeof l);
      }
    }
    int on_device = 0;
    unsigned long long counts[8] = {};
    unsigned long long t = 14695981039346656037ull;
    size_t voxels = 0;
    if (map->handle()) {
      if (cvo_debug_map_stats(map->handle(), &on_device, counts, nullptr, nullptr, nullptr) != CVO_OK) throw std::runtime_error("cvo_debug_map_stats failed");
      const size_t cap = std::max<size_t>(counts[3], 1), nc = counts[7];
      std::vector<unsigned long long> keys(cap, ~0ull);
      std::vector<float> ms(cap * nc), fs(cap * 5);
      if (cvo_debug_map_stats(map->handle(), nullptr, nullptr, keys.data(), ms.data(), fs.data()) != CVO_OK) throw std::runtime_error("cvo_debug_map_stats failed");
      std::vector<size_t> live;
      for (size_t s = 0; s < cap; s++)
        if (keys[s] != ~0ull) live.push_back(s);
      std::sort(live.begin(), live.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
      for (size_t s : live) {
        t = cvo_check::fnv(t, &keys[s], 8);
        t = cvo_check::fnv(t, &ms[s * nc], 4 * nc);
        t = cvo_check::fnv(t, &fs[s * 5], 20);
      }
      voxels = live.size();
    }
    std::printf("cloud %d\nrows %016llx\ntable %zu %016llx\non_device %d\n", out.num_points(), h, voxels, t, on_device);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_bki_sparse_check: %s\n", e.what());
    return 1;
  }
}
