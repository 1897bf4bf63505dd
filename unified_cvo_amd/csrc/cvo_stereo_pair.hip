// cvo_stereo_pair.hip -- the entry points that chain the matcher (cvo_sgm.hip), the disparity filter (cvo_dfilter.hip) and the
// stereo front end (cvo_stereo.hip): cvo_stereo_disparity(_host), cvo_stereo_disparity_filtered, cvo_cloud_upload_stereo_pair
// and cvo_cloud_upload_stereo_pair_filtered.  Each validates every stage's arguments once, in the order matcher, filter,
// front end, and runs the stages' locked bodies under ONE frontend_call: the context stays locked from the matcher to the
// upload, so no other thread's call can replace ctx->err or a stage's stats in between.  The map is handed over resident: it
// stays in the matcher's region and is downloaded only for a caller or a stage that reads it on the host.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// the matcher's refusals - its `planes` first -, then - filtered - the filter's
int pair_validate(int rows, int cols, std::initializer_list<const void*> planes, const cvo_sgm_config_t* sgm_cfg, bool filtered,
                  const cvo_dfilter_config_t* dfilter_cfg, std::string* msg) {
  int rc = sgm_validate_pointers(planes, msg);
  if (rc == CVO_OK) rc = sgm_validate_config(rows, cols, sgm_cfg, msg);
  if (rc == CVO_OK && filtered) rc = dfilter_validate_for_matcher(rows, cols, dfilter_cfg, msg);
  return rc;
}

// The matcher and - dfilter_cfg != nullptr - the filter of its map, each by the context's route (ctx == nullptr: the twin);
// arguments checked, the caller holds upload_mutex.  Each stage commits its own stats.
int stereo_disparity_run(cvo_ctx* ctx, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t& sgm_cfg,
                         const cvo_dfilter_config_t* dfilter_cfg, float* disparity) {
  const SgmConst k = sgm_const(rows, cols, sgm_cfg);
  const size_t np = (size_t)rows * cols;
  SgmStatsAcc stats(k);
  std::vector<float> raw;  // the raw map on the host: the twin's, or the kernels' for a filter that takes the CPU twin
  const float* resident = nullptr;
  if (!ctx || sgm_on_host(ctx, (long long)np)) {
    raw.resize(np);
    sgm_cpu(k, left, right, raw.data());
  } else {
    // the map stays in the matcher's region; it is downloaded to the caller, or to `raw` for a filter on the host, or not at all
    stats.on_device = 1;
    const bool filter_on_host = dfilter_cfg && dfilter_on_host(ctx, (long long)np);
    if (filter_on_host) raw.resize(np);
    const int rc = sgm_device(ctx, k, left, right, dfilter_cfg ? (filter_on_host ? raw.data() : nullptr) : disparity, stats);
    if (rc != CVO_OK) return rc;
    resident = (const float*)(ctx->sgm_scratch.p + stats.o_disparity);
  }
  if (ctx) ctx->sgm_last = stats;
  if (dfilter_cfg) return dfilter_run(ctx, dfilter_const(rows, cols, *dfilter_cfg), raw.data(), resident, disparity);
  if (!resident) std::memcpy(disparity, raw.data(), sizeof(float) * np);  // (nothing is written unless the call succeeds)
  return CVO_OK;
}

// the body of cvo_stereo_disparity_host, cvo_stereo_disparity and cvo_stereo_disparity_filtered
int stereo_disparity_entry(cvo_ctx* ctx, const char* who, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* sgm_cfg,
                           bool filtered, const cvo_dfilter_config_t* dfilter_cfg, float* disparity) {
  std::string msg;
  const int rc = pair_validate(rows, cols, {left, right, disparity}, sgm_cfg, filtered, dfilter_cfg, &msg);
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] { return stereo_disparity_run(ctx, rows, cols, left, right, *sgm_cfg, dfilter_cfg, disparity); });
}

// the body of cvo_cloud_upload_stereo_pair and its _filtered form: the frame's disparity pointer is not looked at
int upload_stereo_pair(cvo_ctx* ctx, const char* who, const cvo_stereo_frame_t* frame, const uint8_t* right_gray, const cvo_sgm_config_t* sgm_cfg,
                       bool filtered, const cvo_dfilter_config_t* dfilter_cfg, int method, cvo_cloud** out, int* pixel, int* n) {
  if (!frame || !out) return fail(ctx, CVO_E_INVALID, std::string(who) + ": frame and out are required");
  std::string msg;
  int rc = pair_validate(frame->rows, frame->cols, {frame->image, right_gray}, sgm_cfg, filtered, dfilter_cfg, &msg);
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  if ((rc = stereo_check(ctx, who, frame, &method, false)) != CVO_OK) return rc;
  return frontend_call(ctx, who, [&] {
    const size_t np = (size_t)frame->rows * frame->cols;
    std::vector<float> disparity(np);
    cvo_stereo_frame_t f = *frame;
    f.disparity = disparity.data();
    // the left plane: the frame's gray plane, or the gray the front end itself takes of the image
    std::vector<uint8_t> gray;
    const uint8_t* left = f.gray ? f.gray : f.image;
    if (!f.gray && f.channels != 1) {
      gray.resize(np);
      for (size_t p = 0; p < np; p++) gray[p] = (uint8_t)rgbd_gray(f.image, f.channels, p);
      left = gray.data();
    }
    const int rc = stereo_disparity_run(ctx, f.rows, f.cols, left, right_gray, *sgm_cfg, dfilter_cfg, disparity.data());
    return rc != CVO_OK ? rc : stereo_upload_locked(ctx, f, method, out, pixel, n);
  });
}

}  // namespace

extern "C" {

int cvo_stereo_disparity_host(int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* cfg, float* disparity) {
  return stereo_disparity_entry(nullptr, "cvo_stereo_disparity_host", rows, cols, left, right, cfg, false, nullptr, disparity);
}

int cvo_stereo_disparity(cvo_ctx* ctx, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* cfg,
                         float* disparity) {
  if (!ctx) return CVO_E_INVALID;
  return stereo_disparity_entry(ctx, "cvo_stereo_disparity", rows, cols, left, right, cfg, false, nullptr, disparity);
}

int cvo_stereo_disparity_filtered(cvo_ctx* ctx, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* sgm_cfg,
                                  const cvo_dfilter_config_t* dfilter_cfg, float* disparity) {
  if (!ctx) return CVO_E_INVALID;
  return stereo_disparity_entry(ctx, "cvo_stereo_disparity_filtered", rows, cols, left, right, sgm_cfg, true, dfilter_cfg, disparity);
}

int cvo_cloud_upload_stereo_pair(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, const uint8_t* right_gray, const cvo_sgm_config_t* cfg, int method,
                                 cvo_cloud** out, int* pixel, int* n) {
  if (!ctx) return CVO_E_INVALID;
  return upload_stereo_pair(ctx, "cvo_cloud_upload_stereo_pair", frame, right_gray, cfg, false, nullptr, method, out, pixel, n);
}

int cvo_cloud_upload_stereo_pair_filtered(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, const uint8_t* right_gray, const cvo_sgm_config_t* sgm_cfg,
                                          const cvo_dfilter_config_t* dfilter_cfg, int method, cvo_cloud** out, int* pixel, int* n) {
  if (!ctx) return CVO_E_INVALID;
  return upload_stereo_pair(ctx, "cvo_cloud_upload_stereo_pair_filtered", frame, right_gray, sgm_cfg, true, dfilter_cfg, method, out, pixel, n);
}

}  // extern "C"
