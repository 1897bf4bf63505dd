// cvo::VoxelMap (include/UnifiedCvo/utils/VoxelMap.hpp) without a device: host compiler only.
//   cvo_voxel_check points.f32 voxel_size
// points.f32: n x 3 raw floats.  Inserts every point, prints "points=<n> voxels=<size()>", the indices of
// sample_points() on one line, then one line per check of query_point, a second insert of the same pointer, and
// delete_point (tests/test_voxel_cpu.py compares the first two lines with numpy).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "utils/VoxelMap.hpp"

struct P {
  float x, y, z;
  int index;
};

int main(int argc, char* argv[]) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s points.f32 voxel_size\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<float> raw;
  float buf[3072];
  for (size_t got; (got = std::fread(buf, sizeof(float), 3072, f)) > 0;) raw.insert(raw.end(), buf, buf + got);
  std::fclose(f);
  const int n = (int)(raw.size() / 3);
  const float s = (float)std::atof(argv[2]);
  std::vector<P> pts((size_t)n);
  for (int i = 0; i < n; i++) pts[i] = P{raw[3 * (size_t)i], raw[3 * (size_t)i + 1], raw[3 * (size_t)i + 2], i};

  cvo::VoxelMap<P> map(s);
  for (P& p : pts)
    if (!map.insert_point(&p)) {
      std::printf("insert of point %d refused\n", p.index);
      return 1;
    }
  const std::vector<P*> sample = map.sample_points();
  std::printf("points=%d voxels=%zu\n", n, map.size());
  for (const P* p : sample) std::printf("%d ", p->index);
  std::printf("\n");
  if (sample.size() != map.size()) return 1;

  // every point's voxel is found by pointer and by position, holds the point, and its first member is a sampled one
  std::vector<char> sampled((size_t)n, 0);
  for (const P* p : sample) sampled[p->index] = 1;
  for (P& p : pts) {
    const cvo::Voxel<P>* v = map.query_point(&p);
    if (!v || v != map.query_point(p.x, p.y, p.z) || v->voxPoints.empty() || !sampled[v->voxPoints[0]->index] ||
        v->voxPoints[0]->index > p.index) {
      std::printf("query of point %d failed\n", p.index);
      return 1;
    }
  }
  P far{1.0e6f, -1.0e6f, 1.0e6f, -1};
  if (map.query_point(&far)) return 1;
  std::printf("queries ok\n");

  if (n > 0 && (map.insert_point(&pts[0]) || map.size() != sample.size())) return 1;
  std::printf("double insert refused\n");

  // deleting every member of the first sampled point's voxel removes the voxel; a point that is not in the map is refused
  if (n > 0) {
    const size_t before = map.size();
    const std::vector<P*> members = map.query_point(sample[0])->voxPoints;  // (a copy: the voxel goes away)
    for (size_t k = 0; k < members.size(); k++) {
      if (!map.delete_point(members[k])) return 1;
      if (map.size() != (k + 1 == members.size() ? before - 1 : before)) return 1;
    }
    if (map.query_point(sample[0]) || map.delete_point(members[0]) || map.delete_point(&far)) return 1;
    if (members.size() > 1) {  // with its first member gone, a voxel hands out its next one
      map.insert_point(members[0]);
      map.insert_point(members[1]);
      map.delete_point(members[0]);
      const std::vector<P*> again = map.sample_points();
      if (again.empty() || again.back() != members[1]) return 1;
    }
  }
  std::printf("delete ok\n");
  return 0;
}
