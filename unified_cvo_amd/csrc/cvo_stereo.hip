// cvo_stereo.hip -- stereo front end: cvo_stereo_points (CvoPointCloud(ImageStereo, Calibration, CV_FAST / DSO_EDGES / FULL)
// from a GIVEN disparity map: libelas is not part of this library), cvo_stereo_points_host (the same on one CPU thread, no
// context), cvo_cloud_upload_stereo (the pairwise KITTI driver's cloud: those rows through the ordinary upload; its locked
// body, stereo_upload_locked, is also the last stage of the pair chain of cvo_stereo_pair.hip),
// cvo_cloud_upload_stereo_recipe (the multi-frame KITTI driver's per-frame block, main_multi_frame_irls_kitti.cpp:235-292),
// cvo_debug_stereo_stats.  The candidates come from cvo_fast.hip (CV_FAST) and the RGB-D section (DSO_EDGES, FULL), features,
// labels, recipe rows and the voxel passes are the RGB-D section's; what is new here is the keep predicate and the
// back-projection (cvo_k_stereo.h).  On the device only pixels, disparity and an exclusion byte go up and only pixel indices
// come back.  A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// map_given false: the pair chain (cvo_stereo_pair.hip), which makes the disparity itself
int stereo_validate(const cvo_stereo_frame_t* f, bool map_given, std::string* msg) {
  if (!f) {
    *msg = "frame is NULL";
    return CVO_E_INVALID;
  }
  auto usable = [](float v) { return std::isfinite(v) && v != 0.f; };
  return frame_validate(f->rows, f->cols, f->channels, f->image, f->num_classes, f->semantic, msg, [&]() -> std::string {
    if (map_given && !f->disparity) return "disparity is NULL";
    if (!usable(f->fx) || !usable(f->fy)) return "fx and fy must be finite and not 0, got " + std::to_string(f->fx) + ", " + std::to_string(f->fy);
    if (!usable(f->baseline)) return "baseline must be finite and not 0, got " + std::to_string(f->baseline);
    return "";
  });
}

int stereo_method(int method, std::string* msg) {
  if (method == CVO_SELECT_CV_FAST || method == CVO_SELECT_FULL || method == CVO_SELECT_DSO_EDGES) return CVO_OK;
  *msg = "point selection method " + std::to_string(method) + " is not supported (CV_FAST, DSO_EDGES and FULL are)";
  return method >= 0 && method <= CVO_SELECT_FULL ? CVO_E_UNSUPPORTED : CVO_E_INVALID;
}

// the frame as the RGB-D section reads it: the disparity in place of a float depth image (its gray plane, gradient,
// exclusion bytes, selector and staging do not look at the calibration)
cvo_rgbd_frame_t stereo_view(const cvo_stereo_frame_t& f) {
  cvo_rgbd_frame_t v{};
  v.rows = f.rows;
  v.cols = f.cols;
  v.channels = f.channels;
  v.image = f.image;
  v.gray = f.gray;
  v.depth = f.disparity;
  v.depth_type = CVO_DEPTH_F32;
  v.fx = v.fy = v.scaling_factor = 1.f;
  v.num_classes = f.num_classes;
  v.semantic = f.semantic;
  return v;
}

// the smallest float whose correctly rounded root is >= 55 (the host's sqrtf is IEEE)
float stereo_far2() {
  float t = 55.f * 55.f;
  for (float below = std::nextafterf(t, 0.f); std::sqrt(below) >= 55.f; below = std::nextafterf(t, 0.f)) t = below;
  return t;
}

// Eigen 3.3's compute_inverse_size3 on K, in float, every operation rounded on its own
StereoCalib stereo_calib(const cvo_stereo_frame_t& f) {
#pragma clang fp contract(off)
  static const float far2 = stereo_far2();
  const float invdet = 1.f / (f.fx * f.fy);
  StereoCalib k;
  k.k00 = f.fy * invdet;
  k.k11 = f.fx * invdet;
  k.k02 = -(f.cx * f.fy) * invdet;
  k.k12 = -(f.fx * f.cy) * invdet;
  k.k22 = (f.fx * f.fy) * invdet;
  k.bf = std::fabs(f.baseline) * f.fx;
  k.far2 = far2;
  return k;
}

cvo_fast_schedule_t stereo_schedule(const cvo_stereo_frame_t& f) {
  return f.num_classes > 0 ? cvo_fast_schedule_t CVO_FAST_STEREO_SEMANTIC : cvo_fast_schedule_t CVO_FAST_STEREO;
}

void stereo_copy_dso_schedule(const RgbdStatsAcc& r, StereoStatsAcc& st) {
  st.tried.assign(r.tried, r.tried + r.n_tried);
  st.count.assign(r.count, r.count + r.n_tried);
}

// ---- CPU twin: pixels the constructor keeps, in its order, and their coordinates ----
void stereo_points_cpu(const cvo_stereo_frame_t& f, int method, std::vector<int>& pix, std::vector<float>& xyz, StereoStatsAcc& st) {
  const int w = f.cols, h = f.rows;
  const cvo_rgbd_frame_t view = stereo_view(f);
  const StereoCalib k = stereo_calib(f);
  pix.clear();
  xyz.clear();
  float p3[3];
  auto consider = [&](int p) {
    st.candidates++;
    if (!stereo_point(k, p % w, p / w, w, h, f.disparity[p], p3) || rgbd_excluded(view, (size_t)p)) return;
    pix.push_back(p);
    xyz.insert(xyz.end(), p3, p3 + 3);
  };
  if (method == CVO_SELECT_FULL) {
    for (int u = 0; u < w; u++)
      for (int v = 0; v < h; v++) consider(v * w + u);
  } else {
    std::vector<int> cand;
    if (method == CVO_SELECT_CV_FAST) {
      fast_select_cpu(gray_view(view), w, h, stereo_schedule(f), cand, st);
    } else {
      RgbdStatsAcc r;
      rgbd_select_cpu(view, cand, r);
      stereo_copy_dso_schedule(r, st);
    }
    for (int p : cand) consider(p);
  }
  st.kept += pix.size();
}

// ---- device route ----
int stereo_device_backproject(cvo_ctx* ctx, const cvo_stereo_frame_t& f, RgbdDevice& d, const int* list, int n, int at, int* n_out) {
  return frame_device_backproject(ctx, "stereo back-projection", d,
                                  StereoKeep{list, d.w, d.h, (const float*)d.depth, d.excl, stereo_calib(f), nullptr, nullptr}, n, at, n_out);
}

// candidates of a method on the device: *list == nullptr is FULL's column-major order
int stereo_device_candidates(cvo_ctx* ctx, const cvo_stereo_frame_t& f, int method, RgbdDevice& d, StereoStatsAcc& st, const int** list, int* n) {
  *list = nullptr;
  *n = f.cols * f.rows;
  int rc = CVO_OK;
  if (method == CVO_SELECT_CV_FAST) {
    rc = fast_device_select(ctx, d, stereo_schedule(f), st, list, n);
  } else if (method == CVO_SELECT_DSO_EDGES) {
    RgbdStatsAcc r;
    rc = rgbd_device_select(ctx, d, r, list, n);
    stereo_copy_dso_schedule(r, st);
  }
  st.candidates += (unsigned long long)*n;
  return rc;
}

int stereo_points_device(cvo_ctx* ctx, const cvo_stereo_frame_t& f, int method, std::vector<int>& pix, std::vector<float>& xyz, StereoStatsAcc& st) {
  RgbdDevice d;
  int rc = rgbd_device_stage(ctx, stereo_view(f), method != CVO_SELECT_FULL, d, method == CVO_SELECT_CV_FAST);
  if (rc != CVO_OK) return rc;
  const int* list = nullptr;
  int n = 0, kept = 0;
  if ((rc = stereo_device_candidates(ctx, f, method, d, st, &list, &n)) != CVO_OK) return rc;
  if ((rc = stereo_device_backproject(ctx, f, d, list, n, 0, &kept)) != CVO_OK) return rc;
  st.kept = (unsigned long long)kept;
  if ((rc = rgbd_fetch(ctx, d.pix, kept, pix)) != CVO_OK) return rc;
  xyz.resize(3 * (size_t)kept);
  if (kept) {
    HIP_TRY(ctx, hipMemcpyAsync(xyz.data(), d.xyz, sizeof(float) * 3 * (size_t)kept, hipMemcpyDeviceToHost, ctx->upload_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  }
  return CVO_OK;
}

// the constructor's points by the context's route (ctx == nullptr: the twin)
int stereo_points_any(cvo_ctx* ctx, const cvo_stereo_frame_t& f, int method, std::vector<int>& pix, std::vector<float>& xyz, StereoStatsAcc& st) {
  if (!ctx || stereo_on_host(ctx, f.rows, f.cols)) {
    stereo_points_cpu(f, method, pix, xyz, st);
    return CVO_OK;
  }
  st.on_device = 1;
  return stereo_points_device(ctx, f, method, pix, xyz, st);
}

// the recipe of a stereo frame: pixel indices and coordinates of the survivors, edge first
int stereo_recipe_pixels(cvo_ctx* ctx, const char* who, const cvo_stereo_frame_t& f, float leaf, float divisor, std::vector<int>& pix,
                         std::vector<float>& xyz, int* n_edge, StereoStatsAcc& st) {
  const bool on_host = stereo_on_host(ctx, f.rows, f.cols, STEREO_RECIPE_HOST_BELOW);
  xyz.clear();
  const int rc = recipe_pixels(
      ctx, who, stereo_view(f), on_host, leaf, divisor, pix, &xyz, n_edge,
      [&](int method, std::vector<int>& cand, std::vector<float>& cxyz) { stereo_points_cpu(f, method, cand, cxyz, st); },
      [&](RgbdDevice& d, int* n_e, int* n_s) {
        st.on_device = 1;
        const int* list = nullptr;
        int n_sel = 0, rc;
        if ((rc = stereo_device_candidates(ctx, f, CVO_SELECT_DSO_EDGES, d, st, &list, &n_sel)) != CVO_OK) return rc;
        if ((rc = stereo_device_backproject(ctx, f, d, list, n_sel, 0, n_e)) != CVO_OK) return rc;
        st.candidates += (unsigned long long)f.cols * f.rows;
        if ((rc = stereo_device_backproject(ctx, f, d, nullptr, f.cols * f.rows, *n_e, n_s)) != CVO_OK) return rc;
        st.kept = (unsigned long long)*n_e + *n_s;
        return CVO_OK;
      });
  if (rc != CVO_OK || on_host) return rc;
  // the survivors' coordinates on the host: the same arithmetic (stereo_point is shared), a few thousand points
  const StereoCalib k = stereo_calib(f);
  xyz.resize(3 * pix.size());
  for (size_t i = 0; i < pix.size(); i++)
    if ((unsigned)pix[i] >= (unsigned)(f.cols * f.rows) || !stereo_point(k, pix[i] % f.cols, pix[i] / f.cols, f.cols, f.rows, f.disparity[pix[i]], &xyz[3 * i]))
      return fail(ctx, CVO_E_HIP, std::string(who) + ": the device kept a pixel the predicate rejects");
  return CVO_OK;
}

// the refusals every entry point shares (method nullptr: the recipe, which runs DSO_EDGES and FULL; a twin stores no text)
int stereo_check(cvo_ctx* ctx, const char* who, const cvo_stereo_frame_t* frame, const int* method, bool map_given = true) {
  const bool dso = !method || *method == CVO_SELECT_DSO_EDGES;
  std::string msg;
  int rc = stereo_validate(frame, map_given, &msg);
  if (rc == CVO_OK && method) rc = stereo_method(*method, &msg);
  if (rc == CVO_OK && dso) rc = rgbd_threshold_range(frame->cols, frame->rows, &msg);
  return rc != CVO_OK ? fail(ctx, rc, std::string(who) + ": " + msg) : rc;
}

// the body of cvo_stereo_points_host and cvo_stereo_points
int stereo_points_entry(cvo_ctx* ctx, const char* who, const cvo_stereo_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                        float* label, float* geotype) {
  const int rc = stereo_check(ctx, who, frame, &method);
  if (rc != CVO_OK) return rc;
  if (!pixel || !n) return fail(ctx, CVO_E_INVALID, std::string(who) + ": pixel and n are required");
  return frontend_call(ctx, who, [&] {
    std::vector<int> pix;
    std::vector<float> p3;
    StereoStatsAcc st;
    const int rc = stereo_points_any(ctx, *frame, method, pix, p3, st);
    if (rc != CVO_OK) return rc;
    rgbd_point_rows(stereo_view(*frame), method, pix, nullptr, feat, label, geotype);
    if (xyz && !p3.empty()) std::memcpy(xyz, p3.data(), sizeof(float) * p3.size());
    copy_kept(pix, pixel, n);
    if (ctx) ctx->stereo_last = st;
    return CVO_OK;
  });
}

// cvo_cloud_upload_stereo of a checked frame - and the last stage of the pair chain (cvo_stereo_pair.hip) -: the caller holds
// upload_mutex
int stereo_upload_locked(cvo_ctx* ctx, const cvo_stereo_frame_t& frame, int method, cvo_cloud** out, int* pixel, int* n) {
  std::vector<int> pix;
  std::vector<float> p3;
  StereoStatsAcc st;
  int rc = stereo_points_any(ctx, frame, method, pix, p3, st);
  if (rc != CVO_OK) return rc;
  // the rows as cvo_cloud_upload takes them: F = channels + 2 features zero-padded to FD, labels padded / cut to NC
  const size_t np = pix.size(), F = (size_t)frame.channels + 2, C = (size_t)frame.num_classes;
  std::vector<float> ft(F * np), lb(C * np), geo(2 * np), feat((size_t)FD * np, 0.f), label(C ? (size_t)NC * np : 0, 0.f);
  rgbd_point_rows(stereo_view(frame), method, pix, nullptr, ft.data(), C ? lb.data() : nullptr, geo.data());
  for (size_t i = 0; i < np; i++) {
    std::memcpy(&feat[(size_t)FD * i], &ft[F * i], sizeof(float) * std::min(F, (size_t)FD));
    if (C) std::memcpy(&label[(size_t)NC * i], &lb[C * i], sizeof(float) * std::min(C, (size_t)NC));
  }
  const HostCloud h{(int)np, (const char*)p3.data(), 12, (const char*)feat.data(), sizeof(float) * FD, C ? (const char*)label.data() : nullptr,
                    sizeof(float) * NC, (const char*)geo.data(), 8};
  if ((rc = upload_one_locked(ctx, h, out)) != CVO_OK) return rc;
  copy_kept(pix, pixel, n);
  ctx->stereo_last = st;
  return CVO_OK;
}

}  // namespace

extern "C" {

int cvo_stereo_points_host(const cvo_stereo_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label, float* geotype) {
  return stereo_points_entry(nullptr, "cvo_stereo_points_host", frame, method, pixel, n, xyz, feat, label, geotype);
}

int cvo_stereo_points(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label,
                      float* geotype) {
  if (!ctx) return CVO_E_INVALID;
  return stereo_points_entry(ctx, "cvo_stereo_points", frame, method, pixel, n, xyz, feat, label, geotype);
}

int cvo_cloud_upload_stereo(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, int method, cvo_cloud** out, int* pixel, int* n) {
  if (!ctx) return CVO_E_INVALID;
  const int rc = stereo_check(ctx, "cvo_cloud_upload_stereo", frame, &method);
  if (rc != CVO_OK) return rc;
  if (!out) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_stereo: out is NULL");
  return frontend_call(ctx, "cvo_cloud_upload_stereo", [&] { return stereo_upload_locked(ctx, *frame, method, out, pixel, n); });
}

int cvo_cloud_upload_stereo_recipe(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, float leaf, float edge_divisor, cvo_cloud** out, int* pixel,
                                   unsigned char* is_edge, int* n) {
  if (!ctx) return CVO_E_INVALID;
  const int rc = stereo_check(ctx, "cvo_cloud_upload_stereo_recipe", frame, nullptr);
  if (rc != CVO_OK) return rc;
  if (!out) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_stereo_recipe: out is NULL");
  std::string msg;
  if (voxel_validate(0, nullptr, leaf, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_stereo_recipe: leaf: " + msg);
  if (!std::isfinite(edge_divisor) || !(edge_divisor > 0.f))
    return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_stereo_recipe: edge_divisor must be finite and > 0, got " + std::to_string(edge_divisor));
  return frontend_call(ctx, "cvo_cloud_upload_stereo_recipe", [&] {
    std::vector<int> pix;
    std::vector<float> xyz;
    StereoStatsAcc st;
    int n_edge = 0, rc;
    if ((rc = stereo_recipe_pixels(ctx, "cvo_cloud_upload_stereo_recipe", *frame, leaf, edge_divisor, pix, xyz, &n_edge, st)) != CVO_OK) return rc;
    const size_t np = pix.size();
    std::vector<float> feat((size_t)FD * np), geo(2 * np);
    const cvo_rgbd_frame_t view = stereo_view(*frame);
    const GrayView g = gray_view(view);
    float unused[3];
    for (size_t i = 0; i < np; i++) rgbd_recipe_row(view, g, pix[i], (int)i < n_edge, unused, &feat[(size_t)FD * i], &geo[2 * i]);
    const HostCloud h{(int)np, (const char*)xyz.data(), 12, (const char*)feat.data(), sizeof(float) * FD, nullptr, 0, (const char*)geo.data(), 8};
    if ((rc = upload_one_locked(ctx, h, out)) != CVO_OK) return rc;
    copy_kept(pix, pixel, n, is_edge, n_edge);
    ctx->stereo_last = st;
    return CVO_OK;
  });
}

int cvo_debug_stereo_stats(cvo_ctx* ctx, int capacity, int* n_tried, int* thresholds, int* counts, int* threshold_used, unsigned* histogram,
                           unsigned long long* candidates, unsigned long long* kept, int* on_device) {
  if (!ctx || capacity < 0) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const StereoStatsAcc& s = ctx->stereo_last;
  if (n_tried) *n_tried = (int)s.tried.size();
  for (int i = 0; i < (int)s.tried.size() && i < capacity; i++) {
    if (thresholds) thresholds[i] = s.tried[(size_t)i];
    if (counts) counts[i] = s.count[(size_t)i];
  }
  if (threshold_used) *threshold_used = s.threshold_used;
  if (histogram) std::memcpy(histogram, s.hist, sizeof s.hist);
  if (candidates) *candidates = s.candidates;
  if (kept) *kept = s.kept;
  if (on_device) *on_device = s.on_device;
  return CVO_OK;
}

}  // extern "C"
