// Multi-frame registration on the MI355X backend, in the style of the reference's multi-frame drivers
// (src/experiments/main_multi_frame_irls_*.cpp): N clouds and their initial poses in, N poses out.
//   cvo_multiframe_align params.yaml frames.txt edges.txt
// frames.txt: one line per frame, "<cloud.pcd> <hold_const 0|1> p0 ... p11" (3x4 row-major pose);
// edges.txt: one line per edge, "<frame1> <frame2>" (indices into frames.txt).  Prints "pose <k> p0 ... p11" per frame
// (%.17g) and the registration time.
#include <cstdio>
#include <fstream>
#include <list>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"

int main(int argc, char* argv[]) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s params.yaml frames.txt edges.txt\n", argv[0]);
    return 2;
  }
  cvo::CvoGPU cvo_align(argv[1]);
  std::vector<std::unique_ptr<cvo::CvoPointCloud>> clouds;
  std::vector<cvo::CvoFrame::Ptr> frames;
  std::vector<bool> hold;
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
    frames.push_back(std::make_shared<cvo::CvoFrameGPU>(clouds.back().get(), pose));
    hold.push_back(h != 0);
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
