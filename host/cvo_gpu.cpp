// cvo::CvoGPU over the C-ABI (see include/UnifiedCvo/cvo/CvoGPU.hpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "cvo/CvoGPU.hpp"

namespace cvo {
namespace {

struct DeviceCloud {
  cvo_cloud* h = nullptr;
  ~DeviceCloud() {
    if (h) cvo_cloud_free(h);
  }
};

void check(cvo_ctx* ctx, int rc, const char* what) {
  if (rc <= CVO_E_INVALID) throw std::runtime_error(std::string(what) + ": " + cvo_last_error(ctx));
}

// What CvoPointCloud_to_gpu builds per point (upstream CvoGPU_impl.cu:206-263).
void upload(cvo_ctx* ctx, const CvoPointCloud& pc, DeviceCloud& out) {
  const int n = pc.num_points();
  std::vector<float> xyz(3 * (size_t)n), feat, label, geo(2 * (size_t)n, 0.f);
  for (int i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) xyz[3 * (size_t)i + c] = pc.positions()[i][c];
  const MatXf& F = pc.features();
  if (F.rows() == n && F.cols() > 0) {
    feat.assign(CVO_FEATURE_DIMENSIONS * (size_t)n, 0.f);
    for (int i = 0; i < n; i++)
      for (int c = 0; c < CVO_FEATURE_DIMENSIONS && c < F.cols(); c++) feat[CVO_FEATURE_DIMENSIONS * (size_t)i + c] = F(i, c);
  }
  const MatXf& L = pc.labels();
  if (pc.num_classes() > 0 && L.rows() == n) {
    label.assign(CVO_NUM_CLASSES * (size_t)n, 0.f);
    for (int i = 0; i < n; i++)
      for (int c = 0; c < pc.num_classes() && c < CVO_NUM_CLASSES; c++) label[CVO_NUM_CLASSES * (size_t)i + c] = L(i, c);
  }
  const std::vector<float>& g = pc.geometric_types();
  for (size_t i = 0; i < geo.size() && i < g.size(); i++) geo[i] = g[i];
  check(ctx, cvo_cloud_upload(ctx, n, xyz.data(), feat.empty() ? nullptr : feat.data(),
                              label.empty() ? nullptr : label.data(), geo.data(), &out.h),
        "cvo_cloud_upload");
}

// The same arrays without the upload (voxel selection: the library gathers the kept rows itself)
struct FlatCloud {
  int n = 0;
  std::vector<float> xyz, feat, label, geo;
  explicit FlatCloud(const CvoPointCloud& pc) : n(pc.num_points()), xyz(3 * (size_t)pc.num_points()), geo(2 * (size_t)pc.num_points(), 0.f) {
    for (int i = 0; i < n; i++)
      for (int c = 0; c < 3; c++) xyz[3 * (size_t)i + c] = pc.positions()[i][c];
    const MatXf& F = pc.features();
    if (F.rows() == n && F.cols() > 0) {
      feat.assign(CVO_FEATURE_DIMENSIONS * (size_t)n, 0.f);
      for (int i = 0; i < n; i++)
        for (int c = 0; c < CVO_FEATURE_DIMENSIONS && c < F.cols(); c++) feat[CVO_FEATURE_DIMENSIONS * (size_t)i + c] = F(i, c);
    }
    const MatXf& L = pc.labels();
    if (pc.num_classes() > 0 && L.rows() == n) {
      label.assign(CVO_NUM_CLASSES * (size_t)n, 0.f);
      for (int i = 0; i < n; i++)
        for (int c = 0; c < pc.num_classes() && c < CVO_NUM_CLASSES; c++) label[CVO_NUM_CLASSES * (size_t)i + c] = L(i, c);
    }
    const std::vector<float>& g = pc.geometric_types();
    for (size_t i = 0; i < geo.size() && i < g.size(); i++) geo[i] = g[i];
  }
};

void fill_association(cvo_ctx* ctx, const cvo_params_t& p, cvo_cloud* s, cvo_cloud* t, const Mat4f& T, float ell,
                      Association& a) {
  const int n = cvo_cloud_size(s);
  a.source_inliers.clear();
  a.target_inliers.clear();
  a.pairs.rows = n;
  a.pairs.cols = cvo_cloud_size(t);
  a.pairs.row_ptr.assign(n + 1, 0);
  size_t nnz = 0;
  int rc = cvo_association(ctx, &p, s, t, T.data(), ell, a.pairs.row_ptr.data(), nullptr, nullptr, 0, &nnz);
  if (rc != CVO_E_NOMEM) check(ctx, rc, "cvo_association");
  a.pairs.col.assign(nnz, 0);
  a.pairs.val.assign(nnz, 0.f);
  if (nnz)
    check(ctx, cvo_association(ctx, &p, s, t, T.data(), ell, a.pairs.row_ptr.data(), a.pairs.col.data(),
                               a.pairs.val.data(), nnz, &nnz),
          "cvo_association");
  for (int i = 0; i < n; i++)
    if (a.pairs.row_ptr[i + 1] > a.pairs.row_ptr[i]) a.source_inliers.push_back(i);
  a.target_inliers = a.pairs.col;
}

// The Association align() exports (upstream CvoGPU.cu:1552-1556 -> gpu_association_to_cpu, CvoGPU_impl.cu:366-427):
// the kernel matrix of the loop's LAST EXECUTED iteration, which is still resident in the context.
void fill_align_association(cvo_ctx* ctx, int n_source, int n_target, Association& a) {
  a.source_inliers.clear();
  a.target_inliers.clear();
  a.pairs.rows = n_source;
  a.pairs.cols = n_target;
  a.pairs.row_ptr.assign(n_source + 1, 0);
  size_t nnz = 0;
  int rc = cvo_align_association(ctx, 0, a.pairs.row_ptr.data(), nullptr, nullptr, 0, &nnz, nullptr, nullptr);
  if (rc != CVO_E_NOMEM) check(ctx, rc, "cvo_align_association");
  a.pairs.col.assign(nnz, 0);
  a.pairs.val.assign(nnz, 0.f);
  if (nnz)
    check(ctx, cvo_align_association(ctx, 0, a.pairs.row_ptr.data(), a.pairs.col.data(), a.pairs.val.data(), nnz, &nnz,
                                     nullptr, nullptr),
          "cvo_align_association");
  for (int i = 0; i < n_source; i++)
    if (a.pairs.row_ptr[i + 1] > a.pairs.row_ptr[i]) a.source_inliers.push_back(i);
  a.target_inliers = a.pairs.col;
}

}  // namespace

std::vector<CvoPoint> CvoPointCloud_to_cvo_points(const CvoPointCloud& pc) {
  const int n = pc.num_points();
  std::vector<CvoPoint> out((size_t)n);
  const MatXf& F = pc.features();
  const MatXf& L = pc.labels();
  const std::vector<float>& g = pc.geometric_types();
  for (int i = 0; i < n; i++) {
    CvoPoint p{};
    p.x = pc.positions()[i][0];
    p.y = pc.positions()[i][1];
    p.z = pc.positions()[i][2];
    p.data_w = 1.f;
    if (F.rows() == n)
      for (int c = 0; c < 5 && c < F.cols(); c++) p.features[c] = F(i, c);
    if (F.rows() == n && F.cols() >= 3) {  // r, g, b bytes (CvoGPU_impl.cu:229-234)
      const unsigned r = (unsigned)std::min(255.0, (double)F(i, 0) * 255.0), gg = (unsigned)std::min(255.0, (double)F(i, 1) * 255.0),
                     b = (unsigned)std::min(255.0, (double)F(i, 2) * 255.0);
      p.rgba = (r << 16) | (gg << 8) | b;
    }
    if (pc.num_classes() > 0 && L.rows() == n) {
      int best = 0;
      for (int c = 0; c < pc.num_classes() && c < 19; c++) {
        p.label_distribution[c] = L(i, c);
        if (L(i, c) > L(i, best)) best = c;
      }
      p.label = best;
    }
    if (g.size() >= 2 * (size_t)i + 2) {
      p.geometric_type[0] = g[2 * (size_t)i];
      p.geometric_type[1] = g[2 * (size_t)i + 1];
    }
    out[(size_t)i] = p;
  }
  return out;
}

CvoGPU::CvoGPU(const std::string& f, int device) {
  std::vector<std::string> warnings;
  read_CvoParams_yaml(f.c_str(), &params, &warnings);
  if (std::getenv("CVO_VERBOSE"))
    for (const std::string& w : warnings) std::fprintf(stderr, "[cvo] %s: %s\n", f.c_str(), w.c_str());
  int rc = cvo_ctx_create(device, &ctx);
  if (rc != CVO_OK) throw std::runtime_error("cvo_ctx_create failed: no usable HIP device " + std::to_string(device));
}

CvoGPU::~CvoGPU() {
  if (ctx) cvo_ctx_destroy(ctx);
}

void CvoGPU::write_params(const CvoParams* p_cpu) {
  if (p_cpu != &params) params = *p_cpu;
}

int CvoGPU::align(const CvoPointCloud& source_points, const CvoPointCloud& target_points, const Mat4f& init,
                  Mat4f& transform, Association* association, double* registration_seconds) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (source_points.num_points() == 0 || target_points.num_points() == 0) return 0;
  DeviceCloud s, t;
  upload(ctx, source_points, s);
  upload(ctx, target_points, t);
  cvo_align_info_t info;
  Mat4f out = transform;
  int rc = cvo_align(ctx, &params, s.h, t.h, init.data(), out.data(), &info);
  check(ctx, rc, "cvo_align");
  transform = out;
  if (registration_seconds) *registration_seconds = info.seconds;
  if (params.is_exporting_association && association)  // upstream CvoGPU.cu:1552-1556
    fill_align_association(ctx, source_points.num_points(), target_points.num_points(), *association);
  return rc;
}

int CvoGPU::align(const CvoPoint* src_pts, int n_source, const CvoPoint* tgt_pts, int n_target, const Mat4f& init,
                  Mat4f& transform, Association* association, double* registration_seconds) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (n_source == 0 || n_target == 0) return 0;
  DeviceCloud s, t;
  check(ctx, cvo_cloud_upload_aos192(ctx, n_source, src_pts, &s.h), "cvo_cloud_upload_aos192");
  check(ctx, cvo_cloud_upload_aos192(ctx, n_target, tgt_pts, &t.h), "cvo_cloud_upload_aos192");
  cvo_align_info_t info;
  Mat4f out = transform;
  int rc = cvo_align(ctx, &params, s.h, t.h, init.data(), out.data(), &info);
  check(ctx, rc, "cvo_align");
  transform = out;
  if (registration_seconds) *registration_seconds = info.seconds;
  if (params.is_exporting_association && association) fill_align_association(ctx, n_source, n_target, *association);
  return rc;
}

float CvoGPU::inner_product_gpu(const CvoPoint* src_pts, int n_source, const CvoPoint* tgt_pts, int n_target, const Mat4f& T,
                                float ell) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (n_source == 0 || n_target == 0) return 0.f;
  DeviceCloud s, t;
  check(ctx, cvo_cloud_upload_aos192(ctx, n_source, src_pts, &s.h), "cvo_cloud_upload_aos192");
  check(ctx, cvo_cloud_upload_aos192(ctx, n_target, tgt_pts, &t.h), "cvo_cloud_upload_aos192");
  float v = 0;
  check(ctx, cvo_inner_product(ctx, &params, s.h, t.h, T.data(), ell, &v), "cvo_inner_product");
  return v;
}

float CvoGPU::function_angle(const CvoPoint* src_pts, int n_source, const CvoPoint* tgt_pts, int n_target, const Mat4f& T,
                             float ell, bool is_approximate) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (n_source == 0 || n_target == 0) return 0.f;  // upstream CvoGPU.cu:1855-1857
  DeviceCloud s, t;
  check(ctx, cvo_cloud_upload_aos192(ctx, n_source, src_pts, &s.h), "cvo_cloud_upload_aos192");
  check(ctx, cvo_cloud_upload_aos192(ctx, n_target, tgt_pts, &t.h), "cvo_cloud_upload_aos192");
  float v = 0;
  check(ctx, cvo_function_angle(ctx, &params, s.h, t.h, T.data(), ell, is_approximate ? 1 : 0, &v), "cvo_function_angle");
  return v;
}

std::vector<int> CvoGPU::align_batch(const std::vector<const CvoPointCloud*>& sources,
                                     const std::vector<const CvoPointCloud*>& targets,
                                     const std::vector<Mat4f>& inits, std::vector<Mat4f>& transforms,
                                     double* seconds) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  const int n = (int)sources.size();
  if ((int)targets.size() != n || (int)inits.size() != n) throw std::runtime_error("align_batch: size mismatch");
  std::vector<DeviceCloud> s(n), t(n);
  std::vector<const cvo_cloud*> sh(n), th(n);
  std::vector<float> init(16 * (size_t)n), out(16 * (size_t)n);
  for (int i = 0; i < n; i++) {
    upload(ctx, *sources[i], s[i]);
    upload(ctx, *targets[i], t[i]);
    sh[i] = s[i].h;
    th[i] = t[i].h;
    std::copy(inits[i].data(), inits[i].data() + 16, &init[16 * (size_t)i]);
  }
  std::vector<cvo_align_info_t> infos(n);
  check(ctx, cvo_align_batch(ctx, &params, n, sh.data(), th.data(), init.data(), out.data(), infos.data(), nullptr),
        "cvo_align_batch");
  transforms.resize(n);
  std::vector<int> rets(n);
  for (int i = 0; i < n; i++) {
    std::copy(&out[16 * (size_t)i], &out[16 * (size_t)i] + 16, transforms[i].data());
    rets[i] = infos[i].ret;
  }
  if (seconds && n) *seconds = infos[0].seconds;
  return rets;
}

CvoGPU::ResidentClouds::~ResidentClouds() {
  for (cvo_cloud* h : handles)
    if (h) cvo_cloud_free(h);
}

int CvoGPU::align(std::vector<CvoFrame::Ptr>& frames, const std::vector<bool>& frames_to_hold_const,
                  const std::list<std::pair<CvoFrame::Ptr, CvoFrame::Ptr>>& edges, double* registration_seconds) const {
  const int F = (int)frames.size();
  if (frames_to_hold_const.size() != frames.size())
    throw std::invalid_argument("align: frames_to_hold_const needs one flag per frame");
  std::vector<int> ed;
  for (const auto& e : edges)
    for (const CvoFrame::Ptr& f : {e.first, e.second}) {
      const auto it = std::find(frames.begin(), frames.end(), f);
      if (!f || it == frames.end()) throw std::invalid_argument("align: an edge names a frame that is not in `frames`");
      ed.push_back((int)(it - frames.begin()));
    }
  std::lock_guard<std::mutex> lk(call_mutex);
  // the frames' resident clouds when they all are CvoFrameGPU of one context, else uploads on this object's context
  cvo_ctx* c = nullptr;
  std::vector<const cvo_cloud*> clouds(F, nullptr);
  for (int k = 0; k < F; k++) {
    const auto* g = dynamic_cast<const CvoFrameGPU*>(frames[k].get());
    if (!g || (c && g->context() != c)) {
      c = nullptr;
      break;
    }
    c = g->context();
    clouds[k] = g->points_gpu();
  }
  std::vector<DeviceCloud> own(c ? 0 : F);
  if (!c) {
    c = ctx;
    for (int k = 0; k < F; k++) {
      upload(c, *frames[k]->points, own[k]);
      clouds[k] = own[k].h;
    }
  }
  std::vector<double> poses(12 * (size_t)F);
  std::vector<int> hold(F);
  for (int k = 0; k < F; k++) {
    std::copy(frames[k]->pose_vec, frames[k]->pose_vec + 12, poses.begin() + 12 * (size_t)k);
    hold[k] = frames_to_hold_const[k] ? 1 : 0;
  }
  cvo_params_t p;
  static_assert(sizeof(cvo_params_t) == sizeof(CvoParams), "cvo_params_t must stay layout-identical to cvo::CvoParams");
  std::memcpy(&p, &params, sizeof(p));
  cvo_multiframe_info_t info{};
  check(c, cvo_multiframe_align(c, &p, F, clouds.data(), poses.data(), hold.data(), (int)edges.size(), ed.data(), &info,
                                nullptr, 0, nullptr),
        "cvo_multiframe_align");
  for (int k = 0; k < F; k++) {
    std::copy(poses.begin() + 12 * (size_t)k, poses.begin() + 12 * (size_t)k + 12, frames[k]->pose_vec);
    frames[k]->transform_pointcloud();
  }
  if (registration_seconds) *registration_seconds = info.seconds;
  return 0;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_clouds(const std::vector<const CvoPointCloud*>& clouds,
                                                              int host_threads) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const int k = (int)clouds.size();
  // what CvoPointCloud_to_gpu builds per point (upstream CvoGPU_impl.cu:206-263), for all clouds, then ONE parallel upload
  std::vector<std::vector<float>> xyz(k), feat(k), label(k), geo(k);
  std::vector<int> n(k);
  std::vector<const float*> px(k), pf(k), pl(k), pg(k);
  for (int c = 0; c < k; c++) {
    const CvoPointCloud& pc = *clouds[c];
    n[c] = pc.num_points();
    xyz[c].resize(3 * (size_t)n[c]);
    for (int i = 0; i < n[c]; i++)
      for (int d = 0; d < 3; d++) xyz[c][3 * (size_t)i + d] = pc.positions()[i][d];
    const MatXf& F = pc.features();
    if (F.rows() == n[c] && F.cols() > 0) {
      feat[c].assign(CVO_FEATURE_DIMENSIONS * (size_t)n[c], 0.f);
      for (int i = 0; i < n[c]; i++)
        for (int d = 0; d < CVO_FEATURE_DIMENSIONS && d < F.cols(); d++) feat[c][CVO_FEATURE_DIMENSIONS * (size_t)i + d] = F(i, d);
    }
    const MatXf& L = pc.labels();
    if (pc.num_classes() > 0 && L.rows() == n[c]) {
      label[c].assign(CVO_NUM_CLASSES * (size_t)n[c], 0.f);
      for (int i = 0; i < n[c]; i++)
        for (int d = 0; d < pc.num_classes() && d < CVO_NUM_CLASSES; d++) label[c][CVO_NUM_CLASSES * (size_t)i + d] = L(i, d);
    }
    const std::vector<float>& g = pc.geometric_types();
    if (!g.empty()) {
      geo[c].assign(2 * (size_t)n[c], 0.f);
      for (size_t i = 0; i < geo[c].size() && i < g.size(); i++) geo[c][i] = g[i];
    }
    px[c] = xyz[c].data();
    pf[c] = feat[c].empty() ? nullptr : feat[c].data();
    pl[c] = label[c].empty() ? nullptr : label[c].data();
    pg[c] = geo[c].empty() ? nullptr : geo[c].data();
  }
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(k, nullptr);
  if (k)
    check(ctx, cvo_cloud_upload_many(ctx, k, n.data(), px.data(), pf.data(), pl.data(), pg.data(), host_threads, out->handles.data()),
          "cvo_cloud_upload_many");
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_device(const cvo_device_rows_t& rows) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  check(ctx, cvo_cloud_from_device(ctx, &rows, out->handles.data()), "cvo_cloud_from_device");
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_device_aos192(const CvoPoint* d_pts, int n) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  check(ctx, cvo_cloud_from_device_aos192(ctx, n, d_pts, out->handles.data()), "cvo_cloud_from_device_aos192");
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_rgbd_points_device(const cvo_rgbd_device_frame_t& frame,
                                                                          CvoPointCloud::PointSelectionMethod method) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  std::vector<int>& pixel = out->kept_[0];
  pixel.resize((size_t)std::max(frame.rows, 1) * (size_t)std::max(frame.cols, 1));
  int n = 0;
  check(ctx, cvo_cloud_from_rgbd_device(ctx, &frame, (int)method, out->handles.data(), &n, pixel.data()), "cvo_cloud_from_rgbd_device");
  pixel.resize((size_t)n);
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_rgbd_device(const cvo_rgbd_device_frame_t& frame, float leaf, float edge_divisor) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  std::vector<int>& pixel = out->kept_[0];
  pixel.resize(2 * (size_t)std::max(frame.rows, 1) * (size_t)std::max(frame.cols, 1));
  int n = 0, n_edge = 0;
  check(ctx, cvo_cloud_from_rgbd_device_recipe(ctx, &frame, leaf > 0.f ? leaf : params.multiframe_downsample_voxel_size, edge_divisor,
                                               out->handles.data(), &n, &n_edge, pixel.data()),
        "cvo_cloud_from_rgbd_device_recipe");
  pixel.resize((size_t)n);
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::merge(const ResidentClouds& clouds, const std::vector<double>* poses, float voxel_size) const {
  if (poses && poses->size() != 12 * (size_t)clouds.size()) throw std::invalid_argument("merge: 12 pose entries per cloud");
  std::lock_guard<std::mutex> lk(call_mutex);
  const float s = voxel_size < 0.f ? params.multiframe_downsample_voxel_size / 2 : voxel_size;
  std::vector<const cvo_cloud*> h(clouds.handles.begin(), clouds.handles.end());
  size_t total = 0;
  for (const cvo_cloud* c : h) total += (size_t)cvo_cloud_size(c);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  std::vector<int>& k = out->kept_[0];
  k.resize(std::max<size_t>(total, 1));
  int nk = 0;
  check(ctx, cvo_cloud_merge(ctx, (int)h.size(), h.data(), poses ? poses->data() : nullptr, s, out->handles.data(), k.data(), &nk),
        "cvo_cloud_merge");
  k.resize((size_t)nk);
  return out;
}

CvoPointCloud CvoGPU::download(const ResidentClouds& clouds, int k) const {
  if (k < 0 || k >= clouds.size()) throw std::invalid_argument("download: no such cloud");
  std::lock_guard<std::mutex> lk(call_mutex);
  const cvo_cloud* c = clouds.handles[(size_t)k];
  const int n = cvo_cloud_size(c);
  const size_t nn = (size_t)n;
  std::vector<float> xyz(3 * nn + 1), feat(CVO_FEATURE_DIMENSIONS * nn + 1), label(CVO_NUM_CLASSES * nn + 1), geo(2 * nn + 1);
  int present = 0;
  check(ctx, cvo_cloud_download(ctx, c, xyz.data(), feat.data(), label.data(), geo.data(), &present), "cvo_cloud_download");
  const int F = present & CVO_CLOUD_HAS_FEAT ? CVO_FEATURE_DIMENSIONS : 0, Cn = present & CVO_CLOUD_HAS_LABEL ? CVO_NUM_CLASSES : 0;
  CvoPointCloud out(F, Cn);
  out.reserve(n, F, Cn);
  for (int i = 0; i < n; i++) {
    const float* f = &feat[CVO_FEATURE_DIMENSIONS * (size_t)i];
    const float* l = &label[CVO_NUM_CLASSES * (size_t)i];
    out.add_point(i, Vec3f{{xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]}}, std::vector<float>(f, f + F),
                  std::vector<float>(l, l + Cn), {geo[2 * (size_t)i], geo[2 * (size_t)i + 1]});
  }
  return out;
}

CvoPointCloud CvoGPU::voxel_downsample(const CvoPointCloud& cloud, float voxel_size, std::vector<int>* kept) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const int n = cloud.num_points();
  std::vector<float> xyz(3 * (size_t)n);
  for (int i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) xyz[3 * (size_t)i + c] = cloud.positions()[i][c];
  std::vector<int> k((size_t)std::max(n, 1));
  int nk = 0;
  check(ctx, cvo_voxel_select(ctx, n, xyz.data(), voxel_size > 0.f ? voxel_size : params.multiframe_downsample_voxel_size, k.data(), &nk),
        "cvo_voxel_select");
  k.resize((size_t)nk);
  CvoPointCloud out = cloud.select(k);
  if (kept) *kept = std::move(k);
  return out;
}

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::upload_clouds_voxel(const std::vector<const CvoPointCloud*>& clouds,
                                                                    float voxel_size) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const float s = voxel_size > 0.f ? voxel_size : params.multiframe_downsample_voxel_size;
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(clouds.size(), nullptr);
  out->kept_.resize(clouds.size());
  for (size_t c = 0; c < clouds.size(); c++) {  // (on a throw `out` releases the clouds already made)
    const FlatCloud f(*clouds[c]);
    std::vector<int>& k = out->kept_[c];
    k.resize((size_t)std::max(f.n, 1));
    int nk = 0;
    check(ctx, cvo_cloud_upload_voxel(ctx, f.n, f.xyz.data(), f.feat.empty() ? nullptr : f.feat.data(),
                                      f.label.empty() ? nullptr : f.label.data(), f.geo.data(), s, &out->handles[c], k.data(), &nk),
          "cvo_cloud_upload_voxel");
    k.resize((size_t)nk);
  }
  return out;
}

int CvoGPU::align(const ResidentClouds& clouds, std::vector<double>& poses, const std::vector<bool>& frames_to_hold_const,
                  const std::vector<std::pair<int, int>>& edges, double* registration_seconds) const {
  const int F = clouds.size();
  if ((int)frames_to_hold_const.size() != F || poses.size() != 12 * (size_t)F)
    throw std::invalid_argument("align: one hold flag and 12 pose entries per cloud");
  std::vector<int> ed, hold(F);
  for (const auto& e : edges) {
    ed.push_back(e.first);
    ed.push_back(e.second);
  }
  for (int k = 0; k < F; k++) hold[k] = frames_to_hold_const[k] ? 1 : 0;
  std::lock_guard<std::mutex> lk(call_mutex);
  std::vector<const cvo_cloud*> h(clouds.handles.begin(), clouds.handles.end());
  cvo_params_t p;
  std::memcpy(&p, &params, sizeof(p));
  cvo_multiframe_info_t info{};
  check(ctx, cvo_multiframe_align(ctx, &p, F, h.data(), poses.data(), hold.data(), (int)edges.size(), ed.data(), &info, nullptr, 0, nullptr),
        "cvo_multiframe_align");
  if (registration_seconds) *registration_seconds = info.seconds;
  return 0;
}

std::vector<int> CvoGPU::align_batch(const ResidentClouds& sources, const ResidentClouds& targets, const std::vector<Mat4f>& inits,
                                     std::vector<Mat4f>& transforms, double* seconds) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const int n = sources.size();
  if (targets.size() != n || (int)inits.size() != n) throw std::runtime_error("align_batch: size mismatch");
  std::vector<float> init(16 * (size_t)n), out(16 * (size_t)n);
  for (int i = 0; i < n; i++) std::copy(inits[i].data(), inits[i].data() + 16, &init[16 * (size_t)i]);
  std::vector<cvo_align_info_t> infos(n);
  transforms.resize(n);
  std::vector<int> rets(n);
  if (n == 0) return rets;
  check(ctx, cvo_align_batch(ctx, &params, n, sources.handles.data(), targets.handles.data(), init.data(), out.data(), infos.data(),
                             nullptr),
        "cvo_align_batch");
  for (int i = 0; i < n; i++) {
    std::copy(&out[16 * (size_t)i], &out[16 * (size_t)i] + 16, transforms[i].data());
    rets[i] = infos[i].ret;
  }
  if (seconds) *seconds = infos[0].seconds;
  return rets;
}

std::vector<int> CvoGPU::align_stream(const ResidentClouds& sources, const ResidentClouds& targets,
                                      const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& inits,
                                      std::vector<Mat4f>& transforms, int slots, const std::vector<int>* max_iterations,
                                      double* seconds) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const int n = (int)pairs.size();
  if ((int)inits.size() != n || (max_iterations && (int)max_iterations->size() != n)) throw std::runtime_error("align_stream: size mismatch");
  transforms.resize(n);
  std::vector<int> rets(n, 0);
  if (n == 0) return rets;
  int n_max = 0, n_min = 1 << 30, m_max = 0;
  for (const auto& pr : pairs) {
    if (pr.first < 0 || pr.first >= sources.size() || pr.second < 0 || pr.second >= targets.size())
      throw std::runtime_error("align_stream: pair index out of range");
    const int ns = cvo_cloud_size(sources.handles[pr.first]), nt = cvo_cloud_size(targets.handles[pr.second]);
    n_max = std::max(n_max, ns);
    n_min = std::min(n_min, ns);
    m_max = std::max(m_max, nt);
  }
  std::vector<cvo_batch_result_t> buf((size_t)n);  // (before the queue opens: nothing below may throw while it is open ...)
  struct QueueGuard {  // (... and if something does, the queue is closed on the way out: an open queue locks the context)
    cvo_batch_queue* q = nullptr;
    ~QueueGuard() {
      if (q) cvo_batch_close(q);
    }
  } guard;
  check(ctx, cvo_batch_open(ctx, &params, std::max(1, std::min(slots, n)), n_max, m_max, n_min, nullptr, &guard.q), "cvo_batch_open");
  cvo_batch_queue* const q = guard.q;
  const auto t0 = std::chrono::steady_clock::now();
  int got = 0, rc = CVO_OK;
  for (int k = 0; k < n && rc == CVO_OK; k++) {
    rc = cvo_batch_submit(q, sources.handles[pairs[k].first], targets.handles[pairs[k].second], inits[k].data(),
                          max_iterations ? (*max_iterations)[k] : 0, nullptr);
    int m = 0;
    if (rc == CVO_OK && (k & 15) == 15) rc = cvo_batch_poll(q, 0, n - got, buf.data() + got, &m);  // keep the device fed while submitting
    got += m;
  }
  while (rc == CVO_OK && got < n) {
    int m = 0;
    rc = cvo_batch_poll(q, 2, n - got, buf.data() + got, &m);
    got += m;
    if (rc == CVO_OK && m == 0 && cvo_batch_pending(q) == 0) break;
  }
  cvo_batch_close(q);
  guard.q = nullptr;
  check(ctx, rc, "cvo_batch_submit / cvo_batch_poll");
  if (got != n) throw std::runtime_error("align_stream: the queue delivered fewer results than pairs were submitted");
  for (int k = 0; k < n; k++) {  // (delivered in submission order: buf[k].ticket == k)
    std::copy(buf[k].transform, buf[k].transform + 16, transforms[k].data());
    rets[k] = buf[k].info.ret;
  }
  if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rets;
}

// function_angle: 0 = inner products, 1 = approximate function_angle, 2 = exact
std::vector<float> CvoGPU::score_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                       const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                       const std::vector<float>& ell, int function_angle) const {
  std::lock_guard<std::mutex> lk(call_mutex);
  const int n = (int)pairs.size();
  if ((int)T.size() != n || (ell.size() != 1 && (int)ell.size() != n)) throw std::runtime_error("score batch: size mismatch");
  std::vector<const cvo_cloud*> sh((size_t)n), th((size_t)n);
  std::vector<float> Tm(16 * (size_t)n), l((size_t)n), out((size_t)n, 0.f);
  for (int k = 0; k < n; k++) {
    const auto& pr = pairs[k];
    if (pr.first < 0 || pr.first >= sources.size() || pr.second < 0 || pr.second >= targets.size())
      throw std::runtime_error("score batch: pair index out of range");
    sh[k] = sources.handles[pr.first];
    th[k] = targets.handles[pr.second];
    std::copy(T[k].data(), T[k].data() + 16, &Tm[16 * (size_t)k]);
    l[k] = ell.size() == 1 ? ell[0] : ell[k];
  }
  if (function_angle == 0)
    check(ctx, cvo_inner_product_batch(ctx, &params, n, sh.data(), th.data(), Tm.data(), l.data(), out.data()),
          "cvo_inner_product_batch");
  else
    check(ctx, cvo_function_angle_batch(ctx, &params, n, sh.data(), th.data(), Tm.data(), l.data(), function_angle == 1 ? 1 : 0,
                                        out.data()),
          "cvo_function_angle_batch");
  return out;
}

std::vector<float> CvoGPU::inner_product_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                               const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                               const std::vector<float>& ell) const {
  return score_batch(sources, targets, pairs, T, ell, 0);
}

std::vector<float> CvoGPU::function_angle_batch(const ResidentClouds& sources, const ResidentClouds& targets,
                                                const std::vector<std::pair<int, int>>& pairs, const std::vector<Mat4f>& T,
                                                const std::vector<float>& ell, bool is_approximate) const {
  return score_batch(sources, targets, pairs, T, ell, is_approximate ? 1 : 2);
}

std::string CvoGPU::advice() const { return cvo_ctx_advice(ctx); }

float CvoGPU::inner_product_gpu(const CvoPointCloud& a, const CvoPointCloud& b, const Mat4f& T, float ell) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (a.num_points() == 0 || b.num_points() == 0) return 0.f;
  DeviceCloud s, t;
  upload(ctx, a, s);
  upload(ctx, b, t);
  float v = 0;
  check(ctx, cvo_inner_product(ctx, &params, s.h, t.h, T.data(), ell, &v), "cvo_inner_product");
  return v;
}

float CvoGPU::function_angle(const CvoPointCloud& a, const CvoPointCloud& b, const Mat4f& T, float ell,
                             bool is_approximate, bool is_gpu) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (a.num_points() == 0 || b.num_points() == 0) return 0.f;
  if (!is_gpu) {  // upstream CvoGPU.cu:1827-1843: the host inner product in all three places
    const float fxfz = inner_product_cpu(a, b, T, ell);
    float fx_norm, fz_norm;
    if (is_approximate) {
      fx_norm = std::sqrt((float)a.num_points());
      fz_norm = std::sqrt((float)b.num_points());
    } else {
      const Mat4f I = Mat4f::Identity();
      fx_norm = std::sqrt(inner_product_cpu(a, a, I, ell));
      fz_norm = std::sqrt(inner_product_cpu(b, b, I, ell));
    }
    return fxfz / (fx_norm * fz_norm);
  }
  DeviceCloud s, t;
  upload(ctx, a, s);
  upload(ctx, b, t);
  float v = 0;
  check(ctx, cvo_function_angle(ctx, &params, s.h, t.h, T.data(), ell, is_approximate ? 1 : 0, &v),
        "cvo_function_angle");
  return v;
}

void CvoGPU::compute_association_gpu(const CvoPointCloud& a, const CvoPointCloud& b, const Mat4f& T, float ell,
                                     Association& association) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (a.num_points() == 0 || b.num_points() == 0) return;
  DeviceCloud s, t;
  upload(ctx, a, s);
  upload(ctx, b, t);
  fill_association(ctx, params, s.h, t.h, T, ell, association);
}

void CvoGPU::compute_association_gpu(const CvoPointCloud& a, const CvoPointCloud& b, const Mat4f& T, const Mat3f& kernel,
                                     Association& association) const {
  std::lock_guard<std::mutex> lk(call_mutex);  // (see CvoGPU.hpp: the const entry points share one context)
  if (a.num_points() == 0 || b.num_points() == 0) return;
  DeviceCloud s, t;
  upload(ctx, a, s);
  upload(ctx, b, t);
  const int n = a.num_points();
  Association& as = association;
  as.source_inliers.clear();
  as.target_inliers.clear();
  as.pairs.rows = n;
  as.pairs.cols = b.num_points();
  as.pairs.row_ptr.assign(n + 1, 0);
  size_t nnz = 0;
  int rc = cvo_association_non_isotropic(ctx, &params, s.h, t.h, T.data(), kernel.data(), as.pairs.row_ptr.data(), nullptr,
                                         nullptr, 0, &nnz);
  if (rc != CVO_E_NOMEM) check(ctx, rc, "cvo_association_non_isotropic");
  as.pairs.col.assign(nnz, 0);
  as.pairs.val.assign(nnz, 0.f);
  if (nnz)
    check(ctx, cvo_association_non_isotropic(ctx, &params, s.h, t.h, T.data(), kernel.data(), as.pairs.row_ptr.data(),
                                             as.pairs.col.data(), as.pairs.val.data(), nnz, &nnz),
          "cvo_association_non_isotropic");
  for (int i = 0; i < n; i++)
    if (as.pairs.row_ptr[i + 1] > as.pairs.row_ptr[i]) as.source_inliers.push_back(i);
  as.target_inliers = as.pairs.col;
}

namespace {

// cvo_depth_filter over handles: the refined keyframe's handle and the original indices of its points
cvo_cloud* depth_filter_handles(cvo_ctx* ctx, const CvoParams& params, const cvo_cloud* kf, const std::vector<const cvo_cloud*>& frames,
                                const std::vector<Mat4f>& T_t2s, const std::vector<Mat4f>& T_s2t, const Mat3f& kernel, int min_count,
                                std::vector<int>& kept) {
  const size_t k = frames.size();
  if (T_t2s.size() != k || T_s2t.size() != k) throw std::invalid_argument("depth_filter: one T_t2s and one T_s2t per frame");
  std::vector<float> T(16 * k + 1), Td(16 * k + 1);
  for (size_t q = 0; q < k; q++) {
    std::copy(T_t2s[q].data(), T_t2s[q].data() + 16, T.begin() + 16 * q);
    std::copy(T_s2t[q].data(), T_s2t[q].data() + 16, Td.begin() + 16 * q);
  }
  cvo_params_t p;
  static_assert(sizeof(cvo_params_t) == sizeof(CvoParams), "cvo_params_t must stay layout-identical to cvo::CvoParams");
  std::memcpy(&p, &params, sizeof(p));
  kept.assign((size_t)std::max(cvo_cloud_size(kf), 1), 0);
  cvo_cloud* out = nullptr;
  int nk = 0;
  check(ctx, cvo_depth_filter(ctx, &p, kf, (int)k, frames.data(), T.data(), Td.data(), kernel.data(), min_count, &out, kept.data(), nullptr,
                              &nk, nullptr),
        "cvo_depth_filter");
  kept.resize((size_t)nk);
  return out;
}

}  // namespace

std::unique_ptr<CvoGPU::ResidentClouds> CvoGPU::depth_filter(const ResidentClouds& kf, int kf_index, const ResidentClouds& frames,
                                                             const std::vector<Mat4f>& T_t2s, const std::vector<Mat4f>& T_s2t,
                                                             const Mat3f& kernel, int min_count) const {
  if (kf_index < 0 || kf_index >= kf.size()) throw std::invalid_argument("depth_filter: no such keyframe");
  std::lock_guard<std::mutex> lk(call_mutex);
  std::unique_ptr<ResidentClouds> out(new ResidentClouds());
  out->handles.assign(1, nullptr);
  out->kept_.resize(1);
  const std::vector<const cvo_cloud*> h(frames.handles.begin(), frames.handles.end());
  out->handles[0] = depth_filter_handles(ctx, params, kf.handles[(size_t)kf_index], h, T_t2s, T_s2t, kernel, min_count, out->kept_[0]);
  return out;
}

CvoPointCloud CvoGPU::depth_filter(const CvoPointCloud& kf, const std::vector<const CvoPointCloud*>& frames, const std::vector<Mat4f>& T_t2s,
                                   const std::vector<Mat4f>& T_s2t, const Mat3f& kernel, int min_count) const {
  std::vector<const CvoPointCloud*> all{&kf};
  all.insert(all.end(), frames.begin(), frames.end());
  const std::unique_ptr<ResidentClouds> up = upload_clouds(all);
  std::unique_ptr<ResidentClouds> res(new ResidentClouds());
  res->handles.assign(1, nullptr);
  res->kept_.resize(1);
  {
    std::lock_guard<std::mutex> lk(call_mutex);
    const std::vector<const cvo_cloud*> h(up->handles.begin() + 1, up->handles.end());
    res->handles[0] = depth_filter_handles(ctx, params, up->handles[0], h, T_t2s, T_s2t, kernel, min_count, res->kept_[0]);
  }
  return download(*res, 0);
}

}  // namespace cvo
