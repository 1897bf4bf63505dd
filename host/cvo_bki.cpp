// semantic_bki::SemanticBKIOctoMap and cvo::CvoPointCloud(const SemanticBKIOctoMap*, num_classes) over cvo_map_* (include/cvo_hip.h),
// and CvoGPU::map_open.
#include <stdexcept>
#include <string>
#include <vector>

#include "cvo/CvoGPU.hpp"
#include "mapping/bkioctomap.h"

namespace cvo {

cvo_map* CvoGPU::map_open(const cvo_map_config_t& cfg, long long initial_voxels) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  cvo_map* m = nullptr;
  const int rc = cvo_map_open(ctx, &cfg, initial_voxels, &m);
  if (rc != CVO_OK) throw std::invalid_argument(std::string("cvo_map_open: ") + cvo_last_error(ctx));
  return m;
}

std::string CvoGPU::last_error() const { return cvo_last_error(ctx); }

void CvoGPU::map_insert_cloud(cvo_map* map, const ResidentClouds& clouds, int k, const float* pose12, const float* origin) const {
  if (k < 0 || k >= clouds.size()) throw std::invalid_argument("map_insert_cloud: no such cloud");
  std::lock_guard<std::mutex> lk(call_mutex);
  if (cvo_map_insert_cloud(map, clouds.handles[(size_t)k], pose12, origin) != CVO_OK) throw std::invalid_argument(cvo_last_error(ctx));
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::map_resident_cloud(cvo_map* map) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  if (cvo_map_cloud_resident(map, out->handles.data(), nullptr) != CVO_OK) throw std::invalid_argument(cvo_last_error(ctx));
  return out;
}

void CvoGPU::map_query_cloud(cvo_map* map, const ResidentClouds& clouds, int k, const float* pose12, const cvo_map_query_out_t& out) const {
  if (k < 0 || k >= clouds.size()) throw std::invalid_argument("map_query_cloud: no such cloud");
  std::lock_guard<std::mutex> lk(call_mutex);
  if (cvo_map_query_cloud(map, clouds.handles[(size_t)k], pose12, &out) != CVO_OK) throw std::invalid_argument(cvo_last_error(ctx));
}

CvoPointCloud::CvoPointCloud(const semantic_bki::SemanticBKIOctoMap* map, const int num_classes) {
  if (!map || num_classes != map->num_classes()) throw std::invalid_argument("CvoPointCloud(map, num_classes): the map has another number of classes");
  num_classes_ = num_classes;
  feature_dimensions_ = 5;
  if (!map->handle()) return;  // (nothing inserted yet)
  long long n = 0, occupied = 0;  // (the size is one counting pass over the table; the voxels are collected and sorted once, below)
  if (cvo_map_size(map->handle(), nullptr, &occupied) != CVO_OK) throw std::runtime_error("cvo_map_size failed");
  std::vector<float> xyz(3 * (size_t)occupied), feat(5 * (size_t)occupied), label((size_t)num_classes * occupied);
  const int rc = map->on_host() ? cvo_map_cloud_host(map->handle(), occupied, xyz.data(), feat.data(), label.data(), &n)
                                : cvo_map_cloud(map->handle(), occupied, xyz.data(), feat.data(), label.data(), &n, nullptr);
  if (rc != CVO_OK) throw std::runtime_error("cvo_map_cloud failed (" + std::to_string(rc) + ")");
  num_points_ = (int)n;
  positions_.resize((size_t)n);
  features_.resize((int)n, 5);
  labels_.resize((int)n, num_classes);
  geometric_types_.assign(2 * (size_t)n, 0.f);
  for (long long i = 0; i < n; i++) {
    positions_[(size_t)i] = Vec3f{{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}};
    for (int c = 0; c < 5; c++) features_((int)i, c) = feat[5 * i + c];
    for (int c = 0; c < num_classes; c++) labels_((int)i, c) = label[(size_t)num_classes * i + c];
  }
}

}  // namespace cvo

namespace semantic_bki {

static cvo_map_config_t make_config(float resolution, unsigned short block_depth, int num_class, float sf2, float ell, float prior, float var_thresh,
                                    float free_thresh, float occupied_thresh) {
  cvo_map_config_t c;
  cvo_map_config_default(&c);
  c.resolution = resolution;
  c.block_depth = block_depth;
  c.num_classes = num_class - 1;
  c.sf2 = sf2;
  c.ell = ell;
  c.prior = prior;
  c.var_thresh = var_thresh;
  c.free_thresh = free_thresh;
  c.occupied_thresh = occupied_thresh;
  if (block_depth != 1) throw std::invalid_argument("SemanticBKIOctoMap: only block_depth 1 is built");
  if (num_class < 1 || num_class > 20) throw std::invalid_argument("SemanticBKIOctoMap: num_class lies in 1 .. 20");
  return c;
}

SemanticBKIOctoMap::SemanticBKIOctoMap(float resolution, unsigned short block_depth, int num_class, float sf2, float ell, float prior, float var_thresh,
                                       float free_thresh, float occupied_thresh)
    : cfg_(make_config(resolution, block_depth, num_class, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh)) {}

SemanticBKIOctoMap::SemanticBKIOctoMap(const cvo::CvoGPU& gpu, float resolution, unsigned short block_depth, int num_class, float sf2, float ell,
                                       float prior, float var_thresh, float free_thresh, float occupied_thresh)
    : gpu_(&gpu), cfg_(make_config(resolution, block_depth, num_class, sf2, ell, prior, var_thresh, free_thresh, occupied_thresh)) {}

SemanticBKIOctoMap::~SemanticBKIOctoMap() {
  if (map_) cvo_map_close(map_);
}

// the first insert opens the map with its free_res and max_range; a later one must name the same.  Every insert names its kernel.
void SemanticBKIOctoMap::open_or_check(const char* who, int kernel, float ds_resolution, float free_res, float max_range) {
  const std::string w(who);
  if (!map_) {
    cfg_.ds_resolution = ds_resolution;
    cfg_.free_resolution = free_res;
    cfg_.max_range = max_range;
    if (gpu_) {
      map_ = gpu_->map_open(cfg_);
    } else if (cvo_map_open_host(&cfg_, &map_) != CVO_OK) {
      throw std::invalid_argument(w + ": the library refused the map's configuration");
    }
  } else if (free_res != cfg_.free_resolution || max_range != cfg_.max_range) {
    throw std::invalid_argument(w + ": free_res and max_range are fixed by the map's first insert");
  }
  if (cvo_map_set_kernel(map_, kernel) != CVO_OK)
    throw std::invalid_argument(w + ": " + (gpu_ ? gpu_->last_error() : std::string("the sparse kernel needs sf2 and ell finite and > 0")));
}

void SemanticBKIOctoMap::insert_resident(const char* who, int kernel, const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12],
                                         float ds_resolution, float free_res, float max_range) {
  const std::string w(who);
  if (!gpu_) throw std::invalid_argument(w + ": a map of the CPU twin takes host clouds");
  if (!pose12) throw std::invalid_argument(w + ": no pose");
  open_or_check(who, kernel, ds_resolution, free_res, max_range);
  try {
    gpu_->map_insert_cloud(map_, clouds, k, pose12, nullptr);
  } catch (const std::invalid_argument& e) {
    throw std::invalid_argument(w + ": " + e.what());
  }
}

void SemanticBKIOctoMap::insert_pointcloud_csm(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12], float ds_resolution,
                                               float free_res, float max_range) {
  insert_resident("insert_pointcloud_csm", CVO_MAP_KERNEL_CSM, clouds, k, pose12, ds_resolution, free_res, max_range);
}

void SemanticBKIOctoMap::insert_pointcloud(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12], float ds_resolution,
                                           float free_res, float max_range) {
  insert_resident("insert_pointcloud", CVO_MAP_KERNEL_SPARSE, clouds, k, pose12, ds_resolution, free_res, max_range);
}

std::unique_ptr<cvo::CvoGPU::ResidentClouds> SemanticBKIOctoMap::resident_cloud() const {
  if (!gpu_) throw std::invalid_argument("resident_cloud: a map of the CPU twin has no resident cloud");
  if (!map_) {  // (nothing inserted yet: the upload of no rows)
    const cvo::CvoPointCloud none(5, cfg_.num_classes);
    return gpu_->upload_clouds({&none});
  }
  return gpu_->map_resident_cloud(map_);
}

// ---- the read side ----
struct SemanticBKIOctoMap::Reader {
  cvo_map* map = nullptr;
  bool host = true, temporary = false;
  explicit Reader(const SemanticBKIOctoMap& m) : map(m.map_), host(m.gpu_ == nullptr) {
    if (map) return;
    cvo_map_config_t c = m.cfg_;
    if (!(c.free_resolution > 0.f)) c.free_resolution = 1.f;
    if (cvo_map_open_host(&c, &map) != CVO_OK) throw std::invalid_argument("SemanticBKIOctoMap: the library refused the map's configuration");
    host = temporary = true;
  }
  ~Reader() {
    if (temporary) cvo_map_close_host(map);
  }
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;
};

static void refused(const char* who, const cvo::CvoGPU* gpu, bool host, int rc) {
  throw std::invalid_argument(std::string(who) + ": " + (gpu && !host ? gpu->last_error() : "the library refused the call (" + std::to_string(rc) + ")"));
}

std::vector<SemanticOcTreeNode> SemanticBKIOctoMap::nodes_of(const char* who, int n, const float* xyz, const cvo::CvoGPU::ResidentClouds* clouds,
                                                             int k, const float* pose12) const {
  const Reader r(*this);
  const size_t nn = (size_t)n, nc = (size_t)(cfg_.num_classes > 1 ? cfg_.num_classes : 1) + 1;
  std::vector<std::uint8_t> found(nn), state(nn);
  std::vector<std::int32_t> sem(nn);
  std::vector<float> probs(nc * nn), vars(nc * nn), feat(5 * nn), centre(3 * nn);
  const cvo_map_query_out_t out{found.data(), state.data(), sem.data(), probs.data(), vars.data(), feat.data(), centre.data()};
  if (clouds) {
    if (r.host) throw std::invalid_argument(std::string(who) + (gpu_ ? ": nothing is inserted yet" : ": a map of the CPU twin takes points, not a resident cloud"));
    try {
      gpu_->map_query_cloud(r.map, *clouds, k, pose12, out);
    } catch (const std::invalid_argument& e) {
      throw std::invalid_argument(std::string(who) + ": " + e.what());
    }
  } else {
    const int rc = r.host ? cvo_map_query_host(r.map, n, xyz, &out) : cvo_map_query(r.map, n, xyz, &out);
    if (rc != CVO_OK) refused(who, gpu_, r.host, rc);
  }
  std::vector<SemanticOcTreeNode> nodes(nn);
  for (size_t i = 0; i < nn; i++) {
    SemanticOcTreeNode& s = nodes[i];
    s.state_ = (State)state[i];
    s.semantics_ = sem[i];
    s.found_ = found[i];
    s.probs_.assign(probs.begin() + (long)(nc * i), probs.begin() + (long)(nc * (i + 1)));
    s.vars_.assign(vars.begin() + (long)(nc * i), vars.begin() + (long)(nc * (i + 1)));
    for (int c = 0; c < 5; c++) s.feat_[c] = feat[5 * i + c];
    s.centre_ = point3f(centre[3 * i], centre[3 * i + 1], centre[3 * i + 2]);
  }
  return nodes;
}

SemanticOcTreeNode SemanticBKIOctoMap::search(point3f p) const { return nodes_of("search", 1, p.data(), nullptr, 0, nullptr)[0]; }

SemanticOcTreeNode SemanticBKIOctoMap::search(float x, float y, float z) const { return search(point3f(x, y, z)); }

static std::vector<float> packed(const std::vector<point3f>& pts) {
  std::vector<float> xyz(3 * pts.size());
  for (size_t i = 0; i < pts.size(); i++)
    for (int a = 0; a < 3; a++) xyz[3 * i + a] = pts[i].data()[a];
  return xyz;
}

std::vector<SemanticOcTreeNode> SemanticBKIOctoMap::search(const std::vector<point3f>& points) const {
  const std::vector<float> xyz = packed(points);
  return nodes_of("search", (int)points.size(), xyz.data(), nullptr, 0, nullptr);
}

std::vector<SemanticOcTreeNode> SemanticBKIOctoMap::search(const cvo::CvoGPU::ResidentClouds& clouds, int k, const float pose12[12]) const {
  if (k < 0 || k >= clouds.size()) throw std::invalid_argument("search: no such cloud");
  return nodes_of("search", clouds.num_points(k), nullptr, &clouds, k, pose12);
}

std::vector<RayHit> SemanticBKIOctoMap::raycast(const std::vector<point3f>& origins, const std::vector<point3f>& ends, unsigned stop_mask,
                                                int max_steps) const {
  if (origins.size() != ends.size()) throw std::invalid_argument("raycast: origins and ends differ in number");
  const Reader r(*this);
  const size_t n = ends.size();
  const std::vector<float> o = packed(origins), e = packed(ends);
  std::vector<std::uint8_t> status(n), state(n);
  std::vector<std::uint64_t> key(n);
  std::vector<std::int32_t> steps(n), sem(n);
  std::vector<float> centre(3 * n), t(n);
  const cvo_map_ray_out_t out{status.data(), key.data(), centre.data(), t.data(), steps.data(), state.data(), sem.data()};
  const int rc = r.host ? cvo_map_raycast_host(r.map, (int)n, o.data(), e.data(), stop_mask, max_steps, &out)
                        : cvo_map_raycast(r.map, (int)n, o.data(), e.data(), stop_mask, max_steps, &out);
  if (rc != CVO_OK) refused("raycast", gpu_, r.host, rc);
  std::vector<RayHit> hits(n);
  for (size_t i = 0; i < n; i++) {
    hits[i].status = status[i];
    hits[i].steps = steps[i];
    hits[i].semantics = sem[i];
    hits[i].state = (State)state[i];
    hits[i].key = key[i];
    hits[i].centre = point3f(centre[3 * i], centre[3 * i + 1], centre[3 * i + 2]);
    hits[i].t = t[i];
  }
  return hits;
}

MapView SemanticBKIOctoMap::render(const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far,
                                   unsigned stop_mask) const {
  if (rows < 1 || cols < 1 || (long long)rows * cols > (1ll << 24)) throw std::invalid_argument("render: rows and cols are at least 1, at most 2^24 pixels");
  const Reader r(*this);
  MapView v;
  v.rows = rows, v.cols = cols, v.num_classes = cfg_.num_classes;
  const size_t px = (size_t)rows * cols;
  v.depth.resize(px);
  v.semantics.resize(px);
  v.feat.resize(5 * px);
  v.label.resize((size_t)cfg_.num_classes * px);
  static_assert(sizeof(int) == sizeof(std::int32_t), "MapView::semantics holds the library's int32");
  const cvo_map_render_out_t out{v.depth.data(), (std::int32_t*)v.semantics.data(), v.feat.data(), v.label.empty() ? nullptr : v.label.data()};
  const int rc = r.host ? cvo_map_render_host(r.map, pose12, fx, fy, cx, cy, rows, cols, z_far, stop_mask, &out)
                        : cvo_map_render(r.map, pose12, fx, fy, cx, cy, rows, cols, z_far, stop_mask, &out);
  if (rc != CVO_OK) refused("render", gpu_, r.host, rc);
  return v;
}

void SemanticBKIOctoMap::insert_pointcloud_csm(const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res, float max_range) {
  insert_host("insert_pointcloud_csm", CVO_MAP_KERNEL_CSM, cloud, origin, ds_resolution, free_res, max_range);
}

void SemanticBKIOctoMap::insert_pointcloud(const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res, float max_range) {
  insert_host("insert_pointcloud", CVO_MAP_KERNEL_SPARSE, cloud, origin, ds_resolution, free_res, max_range);
}

void SemanticBKIOctoMap::insert_host(const char* who, int kernel, const CVOPointCloud* cloud, const point3f& origin, float ds_resolution, float free_res,
                                     float max_range) {
  const std::string w(who);
  if (!cloud) throw std::invalid_argument(w + ": no cloud");
  open_or_check(who, kernel, ds_resolution, free_res, max_range);
  const int n = cloud->num_points(), C = cfg_.num_classes;
  if (C > 0 && cloud->num_classes() != C) throw std::invalid_argument(w + ": the cloud's label rows do not have the map's classes");
  std::vector<float> xyz(3 * (size_t)n), feat, label((size_t)C * n);
  if (cloud->feature_dimensions() == 5) feat.resize(5 * (size_t)n);
  for (int i = 0; i < n; i++) {
    for (int a = 0; a < 3; a++) xyz[3 * (size_t)i + a] = cloud->positions()[(size_t)i][a];
    if (!feat.empty())
      for (int c = 0; c < 5; c++) feat[5 * (size_t)i + c] = cloud->features()(i, c);
    for (int c = 0; c < C; c++) label[(size_t)C * i + c] = cloud->labels()(i, c);
  }
  const float* f = feat.empty() ? nullptr : feat.data();
  const float* l = C > 0 ? label.data() : nullptr;
  const int rc = gpu_ ? cvo_map_insert(map_, n, xyz.data(), f, l, origin.data()) : cvo_map_insert_host(map_, n, xyz.data(), f, l, origin.data());
  if (rc != CVO_OK) throw std::invalid_argument(w + ": " + (gpu_ ? gpu_->last_error() : "the library refused the cloud (" + std::to_string(rc) + ")"));
}

}  // namespace semantic_bki
