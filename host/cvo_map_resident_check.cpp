// The semantic voxel map fed from and read out into resident clouds, through the C++ veneer (mapping/bkioctomap.h):
// SemanticBKIOctoMap::insert_pointcloud_csm(const ResidentClouds&, k, pose12, ...) and SemanticBKIOctoMap::resident_cloud().
//   cvo_map_resident_check case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE params.yaml
// case.npy: float32 (rows, 1 + 12 + 3 + 5 + NUM_CLASS): per row the frame's number, the frame's pose (3x4 row-major), then a
// hit in the frame's own coordinates - x y z, five features, NUM_CLASS label values -, frames in ascending order.  Every frame
// is uploaded (CvoGPU::upload_clouds) and inserted from where it is, under its pose.
// Prints "cloud <n>", "rows <hash>" - FNV-1a over the bytes of xyz, features and labels of the resident cloud read out and
// downloaded, row by row -, "table <voxels> <hash>" - the same over key, ms and fs of every stored voxel in ascending key
// order - and "on_device <0|1>": where the map's last insert ran (cvo_debug_map_stats).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"
#include "cvo_hip_debug.h"
#include "mapping/bkioctomap.h"

int main(int argc, char* argv[]) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: %s case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE params.yaml\n", argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array in = cvo_check::load(argv[1]);
    const int num_class = std::atoi(argv[2]);
    const float resolution = (float)std::atof(argv[3]), prior = (float)std::atof(argv[4]), free_thresh = (float)std::atof(argv[5]),
                occupied_thresh = (float)std::atof(argv[6]), free_resolution = (float)std::atof(argv[7]), max_range = (float)std::atof(argv[8]);
    const int width = 21 + num_class;
    if (num_class < 0 || num_class > 19 || in.descr != "<f4" || in.shape.size() != 2 || in.shape[1] != width)
      throw std::runtime_error("the case is float32, (rows, 21 + NUM_CLASS)");
    const float* row = (const float*)in.bytes.data();
    const int rows = in.shape[0];
    cvo::CvoGPU gpu(argv[9]);
    semantic_bki::SemanticBKIOctoMap map_csm(gpu, resolution, 1, num_class + 1, 1.0f, 1.0f, prior, 1.0f, free_thresh, occupied_thresh);
    for (int r = 0; r < rows;) {
      int end = r;
      while (end < rows && row[(size_t)end * width] == row[(size_t)r * width]) end++;
      cvo::CvoPointCloud frame(5, num_class);
      frame.reserve(end - r, 5, num_class);
      for (int i = r; i < end; i++) {
        const float* p = row + (size_t)i * width + 13;
        frame.add_point(i - r, cvo::Vec3f{{p[0], p[1], p[2]}}, std::vector<float>(p + 3, p + 8), std::vector<float>(p + 8, p + 8 + num_class), {0.f, 0.f});
      }
      const auto resident = gpu.upload_clouds({&frame});
      map_csm.insert_pointcloud_csm(*resident, 0, row + (size_t)r * width + 1, -1.f, free_resolution, max_range);
      r = end;
    }
    const auto map_cloud = map_csm.resident_cloud();
    const cvo::CvoPointCloud out = gpu.download(*map_cloud, 0);
    unsigned long long h = 14695981039346656037ull;
    for (int i = 0; i < out.num_points(); i++) {
      h = cvo_check::fnv(h, out.positions()[(size_t)i].v, 12);
      for (int c = 0; c < out.features().cols(); c++) {
        const float f = out.features()(i, c);
        h = cvo_check::fnv(h, &f, sizeof f);
      }
      for (int c = 0; c < out.labels().cols(); c++) {
        const float l = out.labels()(i, c);
        h = cvo_check::fnv(h, &l, sizeof l);
      }
    }
    // the table: every stored voxel, ascending key
    int on_device = 0;
    unsigned long long counts[8] = {};
    unsigned long long t = 14695981039346656037ull;
    size_t voxels = 0;
    if (map_csm.handle()) {
      if (cvo_debug_map_stats(map_csm.handle(), &on_device, counts, nullptr, nullptr, nullptr) != CVO_OK) throw std::runtime_error("cvo_debug_map_stats failed");
      const size_t cap = std::max<size_t>(counts[3], 1), nc = counts[7];
      std::vector<unsigned long long> keys(cap, ~0ull);
      std::vector<float> ms(cap * nc), fs(cap * 5);
      if (cvo_debug_map_stats(map_csm.handle(), nullptr, nullptr, keys.data(), ms.data(), fs.data()) != CVO_OK) throw std::runtime_error("cvo_debug_map_stats failed");
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
    std::fprintf(stderr, "cvo_map_resident_check: %s\n", e.what());
    return 1;
  }
}
