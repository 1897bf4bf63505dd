// Multi-frame registration on the MI355X backend, in the style of the reference's multi-frame drivers
// (src/experiments/main_multi_frame_irls_*.cpp): N clouds and their initial poses in, N poses out.
//   cvo_multiframe_align params.yaml frames.txt edges.txt [--voxel [size]]
// frames.txt: one line per frame, "<cloud.pcd> <hold_const 0|1> p0 ... p11" (3x4 row-major pose);
// edges.txt: one line per edge, "<frame1> <frame2>" (indices into frames.txt).  Prints "pose <k> p0 ... p11" per frame
// (%.17g) and the registration time.  --voxel: the frames are thinned to one point per voxel of side `size` (default: the
// yaml's multiframe_downsample_voxel_size) on the device as they are uploaded, as the reference's drivers do with
// cvo::VoxelMap (main_multi_frame_irls_tum.cpp:290-335); prints "kept <k> <points>" per frame before the poses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <list>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"

int main(int argc, char* argv[]) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s params.yaml frames.txt edges.txt [--voxel [size]]\n", argv[0]);
    return 2;
  }
  const bool voxel = argc > 4 && !std::strcmp(argv[4], "--voxel");
  const float voxel_size = voxel && argc > 5 ? (float)std::atof(argv[5]) : 0.f;  // 0: the yaml's value
  cvo::CvoGPU cvo_align(argv[1]);
  std::vector<std::unique_ptr<cvo::CvoPointCloud>> clouds;
  std::vector<cvo::CvoFrame::Ptr> frames;
  std::vector<bool> hold;
  std::vector<double> poses;  // 12 per frame (--voxel: the solve runs on resident clouds, not on frames)
  std::ifstream ff(argv[2]);
  for (std::string line; std::getline(ff, line);) {
    std::istringstream is(line);
    std::string path;
    int h = 0;
    double pose[12];
    if (!(is >> path >> h)) continue;
    for (double& v : pose) is >> v;
    if (!is) {
      std::fprintf(stderr, "bad frame line: %s\n", line.c_str());
      return 2;
    }
    clouds.emplace_back(new cvo::CvoPointCloud(path));
    if (!voxel) frames.push_back(std::make_shared<cvo::CvoFrameGPU>(clouds.back().get(), pose));
    poses.insert(poses.end(), pose, pose + 12);
    hold.push_back(h != 0);
  }
  if (voxel) {
    std::vector<const cvo::CvoPointCloud*> raw;
    for (const auto& c : clouds) raw.push_back(c.get());
    const auto resident = cvo_align.upload_clouds_voxel(raw, voxel_size);
    std::vector<std::pair<int, int>> ed;
    std::ifstream fe(argv[3]);
    for (int a, b; fe >> a >> b;) ed.emplace_back(a, b);
    std::printf("Start multi-frame align: %d voxel-thinned frames, %zu edges\n", resident->size(), ed.size());
    for (int k = 0; k < resident->size(); k++) std::printf("kept %d %d\n", k, resident->num_points(k));
    double seconds = 0;
    const int ret = cvo_align.align(*resident, poses, hold, ed, &seconds);
    for (int k = 0; k < resident->size(); k++) {
      std::printf("pose %d", k);
      for (int q = 0; q < 12; q++) std::printf(" %.17g", poses[12 * (size_t)k + q]);
      std::printf("\n");
    }
    std::printf("ret %d\nregistration_seconds %f\n", ret, seconds);
    return ret;
  }
  std::list<std::pair<cvo::CvoFrame::Ptr, cvo::CvoFrame::Ptr>> edges;
  std::ifstream fe(argv[3]);
  for (int a, b; fe >> a >> b;) {
    if (a < 0 || b < 0 || a >= (int)frames.size() || b >= (int)frames.size()) {
      std::fprintf(stderr, "edge %d %d: frame index out of range\n", a, b);
      return 2;
    }
    edges.emplace_back(frames[a], frames[b]);
  }
  std::printf("Start multi-frame align: %zu frames, %zu edges\n", frames.size(), edges.size());
  double seconds = 0;
  const int ret = cvo_align.align(frames, hold, edges, &seconds);
  for (size_t k = 0; k < frames.size(); k++) {
    std::printf("pose %zu", k);
    for (double v : frames[k]->pose_vec) std::printf(" %.17g", v);
    std::printf("\n");
  }
  std::printf("ret %d\nregistration_seconds %f\n", ret, seconds);
  return ret;
}
