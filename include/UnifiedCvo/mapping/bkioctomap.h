// The semantic voxel map behind upstream's names (mapping/bkioctomap.h, mapping/point3f.h), written afresh over the C-ABI of
// include/cvo_hip.h (cvo_map_*): what the body of upstream's driver main_local_mapping.cpp uses -
//   semantic_bki::SemanticBKIOctoMap map(resolution, block_depth, num_class + 1, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh);
//   map.insert_pointcloud_csm(&transformed_pc, origin, ds_resolution, free_resolution, max_range);
//   cvo::CvoPointCloud cloud_out(&map, num_class);
// block_depth 1 only (std::invalid_argument otherwise); tests/np_bki.py states what is computed.  insert_pointcloud, whose
// declaration upstream's header keeps commented out, is the same insert under the sparse kernel (cvo_map_set_kernel,
// tests/np_bki_sparse.py); a map takes inserts of either kind in any order.  The read side (tests/np_bki_query.py): search with
// upstream's node getters, and - new, the library's own, NOT upstream's RayCaster - raycast and render.  Defined in host/cvo_bki.cpp.
#pragma once
#include <cstdint>
#include <memory>
#include <ostream>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "cvo_hip.h"
#include "utils/CvoPointCloud.hpp"

namespace semantic_bki {

// the subset of upstream's point3f the driver uses
class point3f {
 public:
  point3f() : v_{0.f, 0.f, 0.f} {}
  point3f(float x, float y, float z) : v_{x, y, z} {}
  float& x() { return v_[0]; }
  float& y() { return v_[1]; }
  float& z() { return v_[2]; }
  const float& x() const { return v_[0]; }
  const float& y() const { return v_[1]; }
  const float& z() const { return v_[2]; }
  const float* data() const { return v_; }

 private:
  float v_[3];
};
inline std::ostream& operator<<(std::ostream& out, const point3f& p) { return out << "(" << p.x() << " " << p.y() << " " << p.z() << ")"; }

typedef cvo::CvoPointCloud CVOPointCloud;

// upstream's occupancy states (bkioctree_node.h); PRUNED never occurs at block_depth 1
enum class State : char { FREE, OCCUPIED, UNKNOWN, PRUNED };

// What search() returns: a VALUE with upstream's getter names (Semantics, bkioctree_node.h), computed by the library
// (cvo_map_query) - not a reference into the map.  A point without a stored voxel yields upstream's default node: UNKNOWN,
// ms = prior pushed through the same expressions; its get_semantics() is -1 (upstream leaves it uninitialised).
class Semantics {
  friend class SemanticBKIOctoMap;

 public:
  State get_state() const { return state_; }
  int get_semantics() const { return semantics_; }
  void get_probs(std::vector<float>& probs) const { probs = probs_; }
  void get_occupied_probs(std::vector<float>& probs) const { probs.assign(probs_.begin() + 1, probs_.end()); }
  void get_vars(std::vector<float>& vars) const { vars = vars_; }
  void get_features(std::vector<float>& features) const { features.assign(feat_, feat_ + 5); }
  // New: 1 a stored voxel answered, 0 the default node, 2 the point lies outside the map's key range or is not finite
  int found() const { return found_; }
  point3f get_center() const { return centre_; }  // of the point's voxel (NaN when found() == 2)

 private:
  State state_ = State::UNKNOWN;
  int semantics_ = -1, found_ = 0;
  std::vector<float> probs_, vars_;
  float feat_[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  point3f centre_;
};
typedef Semantics SemanticOcTreeNode;

// one ray of raycast(): cvo_map_raycast's outputs (include/cvo_hip.h)
struct RayHit {
  int status = 0, steps = 0, semantics = -1;  // status: 0 reached the end, 1 stopped, 2 more than max_steps voxels, 3 outside
  State state = State::UNKNOWN;
  std::uint64_t key = ~0ull;
  point3f centre;
  float t = 0.f;
};

// what render() returns: rows x cols planes, row-major (cvo_map_render)
struct MapView {
  int rows = 0, cols = 0, num_classes = 0;
  std::vector<float> depth;      // z-depth, 0: no stop
  std::vector<int> semantics;    // -1: no stop
  std::vector<float> feat;       // x 5: get_features
  std::vector<float> label;      // x num_classes: get_occupied_probs, cvo_rgbd_frame_t::semantic's layout
};

class SemanticBKIOctoMap {
 public:
  // num_class counts the free class, as upstream: a cloud's label rows have num_class - 1 entries (num_class 1: clouds without labels).
  // The map is the CPU twin's (one thread) ...
  SemanticBKIOctoMap(float resolution, unsigned short block_depth, int num_class, float sf2, float ell, float prior, float var_thresh,
                     float free_thresh, float occupied_thresh);
  // ... or, new, lives on gpu's context (the switch BKI_HOST decides its side at the first insert)
  SemanticBKIOctoMap(const cvo::CvoGPU& gpu, float resolution, unsigned short block_depth, int num_class, float sf2, float ell, float prior,
                     float var_thresh, float free_thresh, float occupied_thresh);
  ~SemanticBKIOctoMap();
  SemanticBKIOctoMap(const SemanticBKIOctoMap&) = delete;
  SemanticBKIOctoMap& operator=(const SemanticBKIOctoMap&) = delete;

  // The cloud's points are in the map frame.  free_res and max_range belong to the map here: the first insert fixes them, a
  // later insert with other values throws std::invalid_argument, as does anything the library refuses.  ds_resolution is
  // accepted and unused, as upstream.
  void insert_pointcloud_csm(const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res, float max_range);
  // New: cloud k of `clouds`, resident on the map's context, as the hits of one insert without a host copy
  // (cvo_map_insert_cloud): its rows in original order, moved by pose12 (3x4 row-major, what align() leaves) and seen from the
  // pose's translation.  The first insert fixes free_res and max_range, as above.  A map of the CPU twin throws.
  void insert_pointcloud_csm(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12], float ds_resolution, float free_res,
                             float max_range);
  // The same two inserts under the sparse kernel (SemanticBKInference::predict with covSparse over a block and its face
  // neighbours; sf2 and ell are the constructor's): upstream's commented-out insert_pointcloud.  sf2 or ell not finite and > 0 throws.
  void insert_pointcloud(const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res, float max_range);
  void insert_pointcloud(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12], float ds_resolution, float free_res,
                         float max_range);
  // New: the occupied voxels as one resident cloud built on the device (cvo_map_cloud_resident), to align the next frame
  // against; what CvoPointCloud(&map, num_classes) uploaded would be.  Before the first insert: an empty cloud.
  std::unique_ptr<cvo::CvoGPU::ResidentClouds> resident_cloud() const;

  // upstream's search: the node of the voxel the point's key names (block_to_hash_key; ONE voxel, not the closed boxes of an
  // insert), batched over points (cvo_map_query) and - new - over the rows of a resident cloud moved by pose12 (nullptr: as
  // stored) without a host copy (cvo_map_query_cloud).  Before the first insert every point gets the default node.
  SemanticOcTreeNode search(point3f p) const;
  SemanticOcTreeNode search(float x, float y, float z) const;
  std::vector<SemanticOcTreeNode> search(const std::vector<point3f>& points) const;
  std::vector<SemanticOcTreeNode> search(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12]) const;
  // New, the library's own walk (NOT upstream's RayCaster, which has no caller upstream): the voxels each segment
  // origins[i] -> ends[i] passes through, face by face, to the first one whose state bit (CVO_MAP_STOP_*) is in stop_mask.
  std::vector<RayHit> raycast(const std::vector<point3f>& origins, const std::vector<point3f>& ends, unsigned stop_mask = CVO_MAP_STOP_OCCUPIED,
                              int max_steps = 1 << 20) const;
  // New: the map seen by a pinhole camera at pose12 (3x4 row-major, camera to map), one ray per pixel out to camera z = z_far.
  MapView render(const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far,
                 unsigned stop_mask = CVO_MAP_STOP_OCCUPIED) const;

  float get_resolution() const { return cfg_.resolution; }
  int num_classes() const { return cfg_.num_classes; }  // of a label row
  cvo_map* handle() const { return map_; }              // nullptr before the first insert
  bool on_host() const { return gpu_ == nullptr; }

 private:
  const cvo::CvoGPU* gpu_ = nullptr;
  cvo_map_config_t cfg_;
  cvo_map* map_ = nullptr;
  void open_or_check(const char* who, int kernel, float ds_resolution, float free_res, float max_range);
  // the map the read side asks: this one, or - before the first insert - an empty map of the twin with the same configuration
  struct Reader;
  std::vector<SemanticOcTreeNode> nodes_of(const char* who, int n, const float* xyz, const cvo::CvoGPU::ResidentClouds* clouds, int k,
                                           const float* pose12) const;
  void insert_host(const char* who, int kernel, const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res, float max_range);
  void insert_resident(const char* who, int kernel, const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12], float ds_resolution,
                       float free_res, float max_range);
};

}  // namespace semantic_bki
