// The LiDAR front end through the C++ veneer (CvoPointCloud's LiDAR constructors, CvoGPU::upload_lidar).
//   cvo_lidar_check scan.npy [--semantic labels.npy CLASSES] [--beams B] [--seed S] [--frames K] [--device params.yaml]
// scan.npy: float32 (n, 4) - x, y, z, intensity in upstream's axes, scan order; labels.npy: int32 (n).  Without --device the
// constructor runs K times on one stream of draws (seed S; without --seed: the process's own stream) and prints, per frame,
// "n <points>", the point index of every row on one line and "rows <hash>" (FNV-1a over xyz, features and geometric types,
// point by point); with --device, upload_lidar: "n <points>" and the indices.
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
    std::fprintf(stderr, "usage: %s scan.npy [--semantic labels.npy CLASSES] [--beams B] [--seed S] [--frames K] [--device params.yaml]\n", argv[0]);
    return 2;
  }
  try {
    const cvo_check::Array scan = cvo_check::load(argv[1]);
    if (scan.shape.size() != 2 || scan.shape[1] != 4 || scan.descr != "<f4" || scan.bytes.size() != sizeof(float) * 4 * (size_t)scan.shape[0])
      throw std::runtime_error("scan is (n, 4) float32");
    const int n = scan.shape[0];
    const float* xyzi = (const float*)scan.bytes.data();
    std::vector<int> semantic;
    int classes = 0, beams = 64, frames = 1;
    const char* yaml = nullptr;
    cvo_lidar_rand_t state;
    cvo_lidar_rand_t* rand = nullptr;
    for (int i = 2; i < argc; i++) {
      const std::string o = argv[i];
      if (o == "--semantic" && i + 2 < argc) {
        const cvo_check::Array lab = cvo_check::load(argv[i + 1]);
        if (lab.descr != "<i4" || lab.bytes.size() != sizeof(int) * (size_t)n) throw std::runtime_error("labels are (n) int32");
        semantic.assign((const int*)lab.bytes.data(), (const int*)lab.bytes.data() + n);
        classes = std::atoi(argv[i + 2]);
        i += 2;
      } else if (o == "--beams" && i + 1 < argc) {
        beams = std::atoi(argv[++i]);
      } else if (o == "--seed" && i + 1 < argc) {
        cvo_lidar_rand_seed(&state, (unsigned)std::strtoul(argv[++i], nullptr, 10));
        rand = &state;
      } else if (o == "--frames" && i + 1 < argc) {
        frames = std::atoi(argv[++i]);
      } else if (o == "--device" && i + 1 < argc) {
        yaml = argv[++i];
      } else {
        throw std::runtime_error("unknown option " + o);
      }
    }
    for (int f = 0; f < frames; f++) {
      std::vector<int> index;
      if (yaml) {
        cvo::CvoGPU gpu(yaml);
        auto cloud = gpu.upload_lidar(xyzi, n, classes ? &semantic : nullptr, classes, beams, &index, rand);
        std::printf("n %d\n", cloud->num_points(0));
        for (int p : index) std::printf("%d ", p);
        std::printf("\n");
        continue;
      }
      const cvo::CvoPointCloud pc = classes ? cvo::CvoPointCloud(xyzi, n, semantic, classes, 5000, beams, cvo::CvoPointCloud::LOAM, &index, rand)
                                            : cvo::CvoPointCloud(xyzi, n, 5000, beams, cvo::CvoPointCloud::LOAM, &index, rand);
      std::printf("n %d\n", pc.num_points());
      for (int p : index) std::printf("%d ", p);
      std::printf("\nrows %016llx\n", cvo_check::rows_hash(pc));
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_lidar_check: %s\n", e.what());
    return 1;
  }
}
