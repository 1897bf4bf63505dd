// The read side of the semantic voxel map through the C++ veneer (mapping/bkioctomap.h): search, raycast, render.
//   cvo_bki_query_check case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE KERNEL SF2 ELL
//                       points.npy rays.npy STOP_MASK MAX_STEPS view.npy [--device params.yaml]
// case.npy as cvo_bki_check's: float32 (rows, 4 + 3 + 5 + NUM_CLASS), per row the frame's number, the frame's origin, a hit.
// KERNEL 0: insert_pointcloud_csm, 1: insert_pointcloud (the sparse kernel).  points.npy float32 (n, 3); rays.npy float32
// (m, 6): origin, end; view.npy float32 (1, 20): pose12, fx, fy, cx, cy, z_far, rows, cols, stop mask.  "-" leaves one out.
// Without --device the CPU twin.  Prints FNV-1a hashes:
//   "query <n> <hash>"   per point: found and state (a byte each), semantics (int32), get_probs, get_vars, get_features, get_center
//   "single <hash>"      the same over search(x, y, z) of the first point alone
//   "rays <m> <hash>"    per ray: status, steps (int32), key (8 bytes), centre, t, state and semantics (int32)
//   "view <rows> <cols> <hash>"  depth, semantics, feat, label, plane after plane
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_check_io.hpp"
#include "mapping/bkioctomap.h"

namespace {

const float* floats(const cvo_check::Array& a, int width, const char* what) {
  if (a.descr != "<f4" || a.shape.size() != 2 || a.shape[1] != width) throw std::runtime_error(std::string(what) + " is float32 with " + std::to_string(width) + " columns");
  return (const float*)a.bytes.data();
}

unsigned long long node_hash(unsigned long long h, const semantic_bki::SemanticOcTreeNode& node) {
  const std::uint8_t found = (std::uint8_t)node.found(), state = (std::uint8_t)node.get_state();
  const std::int32_t sem = node.get_semantics();
  h = cvo_check::fnv(h, &found, 1);
  h = cvo_check::fnv(h, &state, 1);
  h = cvo_check::fnv(h, &sem, 4);
  std::vector<float> v;
  node.get_probs(v);
  h = cvo_check::fnv(h, v.data(), 4 * v.size());
  node.get_vars(v);
  h = cvo_check::fnv(h, v.data(), 4 * v.size());
  node.get_features(v);
  h = cvo_check::fnv(h, v.data(), 4 * v.size());
  const semantic_bki::point3f c = node.get_center();
  return cvo_check::fnv(h, c.data(), 12);
}

}  // namespace

int main(int argc, char* argv[]) {
  if (argc < 17) {
    std::fprintf(stderr, "usage: %s case.npy NUM_CLASS RESOLUTION PRIOR FREE_THRESH OCCUPIED_THRESH FREE_RESOLUTION MAX_RANGE KERNEL SF2 ELL points.npy rays.npy STOP_MASK MAX_STEPS view.npy [--device params.yaml]\n", argv[0]);
    return 2;
  }
  try {
    const int num_class = std::atoi(argv[2]);
    const float resolution = (float)std::atof(argv[3]), prior = (float)std::atof(argv[4]), free_thresh = (float)std::atof(argv[5]),
                occupied_thresh = (float)std::atof(argv[6]), free_resolution = (float)std::atof(argv[7]), max_range = (float)std::atof(argv[8]);
    const int kernel = std::atoi(argv[9]);
    const float sf2 = (float)std::atof(argv[10]), ell = (float)std::atof(argv[11]);
    const std::string points_file = argv[12], rays_file = argv[13], view_file = argv[16];
    const unsigned stop_mask = (unsigned)std::atoi(argv[14]);
    const int max_steps = std::atoi(argv[15]);
    const char* yaml = nullptr;
    for (int i = 17; i < argc; i++) {
      if (std::string(argv[i]) == "--device" && i + 1 < argc) yaml = argv[++i];
      else throw std::runtime_error(std::string("unknown option ") + argv[i]);
    }
    std::unique_ptr<cvo::CvoGPU> gpu(yaml ? new cvo::CvoGPU(yaml) : nullptr);
    const int block_depth = 1;
    const float var_thresh = 1.0f, ds_resolution = -1.f;
    std::unique_ptr<semantic_bki::SemanticBKIOctoMap> map(
        gpu ? new semantic_bki::SemanticBKIOctoMap(*gpu, resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh)
            : new semantic_bki::SemanticBKIOctoMap(resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh));
    if (std::string(argv[1]) != "-") {
      const cvo_check::Array in = cvo_check::load(argv[1]);
      const int width = 12 + num_class;
      const float* row = floats(in, width, "the case");
      const int rows = in.shape[0];
      for (int r = 0; r < rows;) {
        int end = r;
        while (end < rows && row[(size_t)end * width] == row[(size_t)r * width]) end++;
        cvo::CvoPointCloud pc(5, num_class);
        pc.reserve(end - r, 5, num_class);
        for (int i = r; i < end; i++) {
          const float* p = row + (size_t)i * width;
          pc.add_point(i - r, cvo::Vec3f{{p[4], p[5], p[6]}}, std::vector<float>(p + 7, p + 12), std::vector<float>(p + 12, p + 12 + num_class), {0.f, 0.f});
        }
        const semantic_bki::point3f origin(row[(size_t)r * width + 1], row[(size_t)r * width + 2], row[(size_t)r * width + 3]);
        if (kernel) map->insert_pointcloud(&pc, origin, ds_resolution, free_resolution, max_range);
        else map->insert_pointcloud_csm(&pc, origin, ds_resolution, free_resolution, max_range);
        r = end;
      }
    }
    const unsigned long long seed = 14695981039346656037ull;
    if (points_file != "-") {
      const cvo_check::Array in = cvo_check::load(points_file);
      const float* p = floats(in, 3, "points");
      std::vector<semantic_bki::point3f> pts;
      for (int i = 0; i < in.shape[0]; i++) pts.emplace_back(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
      unsigned long long h = seed;
      for (const semantic_bki::SemanticOcTreeNode& node : map->search(pts)) h = node_hash(h, node);
      std::printf("query %d %016llx\n", in.shape[0], h);
      if (!pts.empty()) std::printf("single %016llx\n", node_hash(seed, map->search(pts[0].x(), pts[0].y(), pts[0].z())));
    }
    if (rays_file != "-") {
      const cvo_check::Array in = cvo_check::load(rays_file);
      const float* p = floats(in, 6, "rays");
      std::vector<semantic_bki::point3f> o, e;
      for (int i = 0; i < in.shape[0]; i++) {
        o.emplace_back(p[6 * i], p[6 * i + 1], p[6 * i + 2]);
        e.emplace_back(p[6 * i + 3], p[6 * i + 4], p[6 * i + 5]);
      }
      unsigned long long h = seed;
      for (const semantic_bki::RayHit& r : map->raycast(o, e, stop_mask, max_steps)) {
        const std::int32_t head[2] = {r.status, r.steps}, tail[2] = {(std::int32_t)r.state, r.semantics};
        h = cvo_check::fnv(h, head, 8);
        h = cvo_check::fnv(h, &r.key, 8);
        h = cvo_check::fnv(h, r.centre.data(), 12);
        h = cvo_check::fnv(h, &r.t, 4);
        h = cvo_check::fnv(h, tail, 8);
      }
      std::printf("rays %d %016llx\n", in.shape[0], h);
    }
    if (view_file != "-") {
      const cvo_check::Array in = cvo_check::load(view_file);
      const float* v = floats(in, 20, "the view");
      const semantic_bki::MapView view = map->render(v, v[12], v[13], v[14], v[15], (int)v[17], (int)v[18], v[16], (unsigned)v[19]);
      unsigned long long h = seed;
      h = cvo_check::fnv(h, view.depth.data(), 4 * view.depth.size());
      h = cvo_check::fnv(h, view.semantics.data(), 4 * view.semantics.size());
      h = cvo_check::fnv(h, view.feat.data(), 4 * view.feat.size());
      h = cvo_check::fnv(h, view.label.data(), 4 * view.label.size());
      std::printf("view %d %d %016llx\n", view.rows, view.cols, h);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cvo_bki_query_check: %s\n", e.what());
    return 1;
  }
}
