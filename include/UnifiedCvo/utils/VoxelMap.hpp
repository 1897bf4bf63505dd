// cvo::VoxelMap<PointT>: the voxel grid upstream's drivers thin a raw frame with before align()
// (upstream include/UnifiedCvo/utils/VoxelMap.hpp; main_multi_frame_irls_tum.cpp:290-335), host only, header only, for
// any PointT with float members x, y, z.  Same interface - insert_point, delete_point, query_point, size,
// sample_points - so driver code compiles against it unchanged.  Two differences, both towards reproducibility
// (DESIGN.md section 4):
//   * a voxel is the integer triple (lrint(x / s), lrint(y / s), lrint(z / s)) for every leaf size; upstream compares voxel
//     centres rounded to centimetres, which merges voxels below a 1 cm leaf depending on the hash-bucket layout;
//   * sample_points() returns the FIRST-inserted member of every voxel, voxels in the order their first member was
//     inserted; upstream draws a member at random and walks the hash map's order.
// The device form of the same selection is cvo_voxel_select / cvo_cloud_upload_voxel (include/cvo_hip.h), which also
// refuses what this class silently accepts (non-finite coordinates, |k| >= 2^20).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <utility>
#include <vector>

namespace cvo {

template <typename PointType>
class Voxel {
 public:
  Voxel() {}
  Voxel(float x, float y, float z) : xc(x), yc(y), zc(z) {}

  float xc = 0.f, yc = 0.f, zc = 0.f;  // voxel centre
  std::vector<PointType*> voxPoints;   // members, in insertion order
};

template <typename PointType>
class VoxelMap {
 public:
  explicit VoxelMap(float voxelSize) : voxelSize_(voxelSize) {}

  // true if the point went in; false if this pointer already is a member of its voxel
  bool insert_point(PointType* pt) {
    const Key k = key_of(pt->x, pt->y, pt->z);
    auto it = vmap_.find(k);
    if (it == vmap_.end()) {
      Cell c;
      c.voxel = Voxel<PointType>(k.i[0] * voxelSize_, k.i[1] * voxelSize_, k.i[2] * voxelSize_);
      it = vmap_.emplace(k, std::move(c)).first;
    }
    Cell& c = it->second;
    if (std::find(c.voxel.voxPoints.begin(), c.voxel.voxPoints.end(), pt) != c.voxel.voxPoints.end()) return false;
    c.voxel.voxPoints.push_back(pt);
    c.seq.push_back(next_seq_++);
    return true;
  }

  // true if the point was a member of its voxel; a voxel that loses its last member is removed
  bool delete_point(PointType* pt) {
    const auto it = vmap_.find(key_of(pt->x, pt->y, pt->z));
    if (it == vmap_.end()) return false;
    Cell& c = it->second;
    const auto at = std::find(c.voxel.voxPoints.begin(), c.voxel.voxPoints.end(), pt);
    if (at == c.voxel.voxPoints.end()) return false;
    c.seq.erase(c.seq.begin() + (at - c.voxel.voxPoints.begin()));
    c.voxel.voxPoints.erase(at);
    if (c.voxel.voxPoints.empty()) vmap_.erase(it);
    return true;
  }

  // the voxel that holds the point / the position, or nullptr
  const Voxel<PointType>* query_point(const PointType* pt) const { return query_point(pt->x, pt->y, pt->z); }
  const Voxel<PointType>* query_point(float globalX, float globalY, float globalZ) const {
    const auto it = vmap_.find(key_of(globalX, globalY, globalZ));
    return it == vmap_.end() ? nullptr : &it->second.voxel;
  }

  size_t size() { return vmap_.size(); }  // (non-const upstream)
  size_t size() const { return vmap_.size(); }

  // one point of every voxel: its first-inserted member, voxels ordered by that member's insertion
  const std::vector<PointType*> sample_points() const {
    std::vector<std::pair<std::uint64_t, PointType*>> firsts;
    firsts.reserve(vmap_.size());
    for (const auto& kv : vmap_) firsts.emplace_back(kv.second.seq.front(), kv.second.voxel.voxPoints.front());
    std::sort(firsts.begin(), firsts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<PointType*> res;
    res.reserve(firsts.size());
    for (const auto& f : firsts) res.push_back(f.second);
    return res;
  }

 private:
  struct Key {
    long i[3];
    bool operator==(const Key& o) const { return i[0] == o.i[0] && i[1] == o.i[1] && i[2] == o.i[2]; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const {
      std::uint64_t h = 0x9e3779b97f4a7c15ull;
      for (long v : k.i) {
        h ^= (std::uint64_t)v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
        h *= 0xbf58476d1ce4e5b9ull;
        h ^= h >> 31;
      }
      return (size_t)h;
    }
  };
  struct Cell {
    Voxel<PointType> voxel;
    std::vector<std::uint64_t> seq;  // insertion numbers of voxPoints
  };
  Key key_of(float x, float y, float z) const {
    return Key{{std::lrint(x / voxelSize_), std::lrint(y / voxelSize_), std::lrint(z / voxelSize_)}};
  }

  float voxelSize_ = 0.1f;
  std::uint64_t next_seq_ = 0;
  std::unordered_map<Key, Cell, KeyHash> vmap_;
};

}  // namespace cvo
