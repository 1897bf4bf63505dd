// cvo_fast.hip -- the CV_FAST point selection (select_points_from_image, CvoPointCloud.cpp:273-312): cv::FAST(gray, kp, t,
// false) re-run under the reference's adaptive threshold schedule.  One pass gives every pixel's score and the score
// histogram (cvo_k_fast.h), the schedule is replayed on the histogram's suffix sums - on the device route that is one 1 KB
// read-back and one synchronisation per frame, however many thresholds the schedule tries -, and the pixels above the
// standing threshold are compacted in row-major order.  cvo_fast_select / cvo_fast_select_host expose the selector on its
// own; cvo_stereo.hip uses it for CV_FAST clouds.  A SECTION of the one translation unit cvo_hip.hip.
namespace {

// Below this many pixels the CPU twin is the default route; STEREO_HOST=0 / 1 forces one route for every size.  Measured on
// the MI355X (scripts/stereo_probe.py --crossover, profiles/stereo/crossover.txt).  The points, the
// pairwise upload and cvo_fast_select: the kernels win at every size measured, down to 72 x 140 (0.15 ms against the twin's
// 0.27); smaller frames were not measured and take the twin.  The recipe has more launches and synchronisations of fixed
// cost: the twin wins at 140 x 140 (0.41 ms against 0.44), the kernels at 200 x 160 (0.60 against 0.77).
constexpr int STEREO_HOST_BELOW = 10000, STEREO_RECIPE_HOST_BELOW = 24000;

bool stereo_on_host(const cvo_ctx* ctx, int rows, int cols, int below = STEREO_HOST_BELOW) {
  return route_on_host(ctx->opt.stereo_host, (long long)rows * cols, below);
}

int fast_validate_schedule(const cvo_fast_schedule_t* s, std::string* msg) {
  if (!s) {
    *msg = "schedule is NULL";
    return CVO_E_INVALID;
  }
  if (s->thresh < 0 || s->num_want < 0 || s->num_min < 0 || s->break_thresh < 0 || s->thresh > 255 || s->num_min > s->num_want) {
    *msg = "schedule needs 0 <= thresh <= 255, 0 <= num_min <= num_want, break_thresh >= 0, got {" + std::to_string(s->thresh) + ", " +
           std::to_string(s->num_want) + ", " + std::to_string(s->num_min) + ", " + std::to_string(s->break_thresh) + "}";
    return CVO_E_INVALID;
  }
  return CVO_OK;
}

int fast_validate_plane(int rows, int cols, const unsigned char* gray, std::string* msg) {
  if (rows < 1 || cols < 1) {
    *msg = "rows and cols must be >= 1, got " + std::to_string(rows) + " x " + std::to_string(cols);
    return CVO_E_INVALID;
  }
  if (!gray) {
    *msg = "gray is NULL";
    return CVO_E_INVALID;
  }
  if ((long long)rows * cols > COMPACT_MAX_ELEMENTS) {
    *msg = "more than 2^24 pixels";
    return CVO_E_UNSUPPORTED;
  }
  return CVO_OK;
}

// The reference's loop, literally (CvoPointCloud.cpp:278-302), over count(t) = keypoints of cv::FAST at threshold t (t
// clamped to 0 .. 255 as OpenCV does): the first call is always at 5; the keypoints that stand are those of the LAST call.
// Returns that call's threshold.  The one departure: the lowering loop also ends below 0 (upstream's would not end).
template <class Count>
int fast_schedule(const cvo_fast_schedule_t& s, Count count, StereoStatsAcc& st) {
  st.tried.clear();
  st.count.clear();
  auto run = [&](int t) {
    const int c = count(std::min(std::max(t, 0), 255));
    st.tried.push_back(t);
    st.count.push_back(c);
    return c;
  };
  int thresh = s.thresh, used = 5, n = run(5);
  while (n > s.num_want) {
    n = run(used = ++thresh);
    if (thresh == s.break_thresh) break;
  }
  while (n < s.num_min) {
    n = run(used = --thresh);
    if (thresh <= 0) break;
  }
  st.threshold_used = std::min(std::max(used, 0), 255);
  return st.threshold_used;
}

// keypoint count at every threshold from the histogram of clamp(s, -1, 255): s > t <=> bin >= t + 2
void fast_counts(const unsigned* hist, int* count /* 256 */) {
  long long run = 0;
  for (int t = 255; t >= 0; t--) {
    run += t + 2 < FAST_BINS ? hist[t + 2] : 0;
    count[t] = (int)run;
  }
}

// ---- CPU twin ----
void fast_select_cpu(const GrayView& g, int w, int h, const cvo_fast_schedule_t& s, std::vector<int>& pix, StereoStatsAcc& st) {
  const size_t np = (size_t)w * h;
  std::vector<unsigned char> code(np);
  unsigned hist[FAST_BINS] = {};
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const int sc = fast_score_at(w, h, x, y, [&](int xx, int yy) { return rgbd_gray(g.p, g.channels, (size_t)yy * w + xx); });
      code[(size_t)y * w + x] = (unsigned char)std::max(sc, 0);
      hist[sc + 1]++;
    }
  int count[256];
  fast_counts(hist, count);
  const int t = fast_schedule(s, [&](int tt) { return count[tt]; }, st);
  std::memcpy(st.hist, hist, sizeof hist);
  pix.clear();
  pix.reserve((size_t)count[t]);
  for (size_t p = 0; p < np; p++)
    if ((int)code[p] > t) pix.push_back((int)p);
}

// ---- device route: the selection stays on the device (*list, *n), in d.out ----
int fast_device_select(cvo_ctx* ctx, RgbdDevice& d, const cvo_fast_schedule_t& s, StereoStatsAcc& stats, const int** list, int* n) {
  hipStream_t st = ctx->upload_stream;
  const int w = d.w, h = d.h, np = w * h;
  const int nb_score = ((w + FAST_TILE_W - 1) / FAST_TILE_W) * ((h + FAST_TILE_H - 1) / FAST_TILE_H);
  HIP_TRY(ctx, hipMemsetAsync(d.fast_hist, 0, sizeof(unsigned) * FAST_BINS, st));
  if (ctx->opt.fast_tile)
    hipLaunchKernelGGL(k_fast_score<true>, dim3(nb_score), dim3(RGBD_THREADS), 0, st, w, h, d.img_channels, (const unsigned char*)d.img, d.score, d.fast_hist);
  else
    hipLaunchKernelGGL(k_fast_score<false>, dim3(nb_score), dim3(RGBD_THREADS), 0, st, w, h, d.img_channels, (const unsigned char*)d.img, d.score, d.fast_hist);
  HIP_TRY(ctx, hipGetLastError());
  unsigned hist[FAST_BINS];
  HIP_TRY(ctx, hipMemcpyAsync(hist, d.fast_hist, sizeof hist, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  unsigned long long total = 0;
  for (unsigned c : hist) total += c;
  if (total != (unsigned long long)np) return fail(ctx, CVO_E_HIP, "FAST selection: the device's histogram does not count every pixel once");
  int count[256];
  fast_counts(hist, count);
  const int t = fast_schedule(s, [&](int tt) { return count[tt]; }, stats);
  std::memcpy(stats.hist, hist, sizeof hist);
  *list = d.out;
  *n = count[t];
  if (*n == 0) return CVO_OK;
  return compact(ctx, np, FastAbove{d.score, t, d.out}, d.blocks, scan_into(ctx, d.ctl));  // (no synchronisation: the selection stays on the device)
}

// a gray plane as the frame the RGB-D staging lays out: one channel, no depth, no classes
cvo_rgbd_frame_t fast_plane_frame(int rows, int cols, const unsigned char* gray) {
  cvo_rgbd_frame_t f{};
  f.rows = rows;
  f.cols = cols;
  f.channels = 1;
  f.image = gray;
  f.depth_type = CVO_DEPTH_F32;
  f.fx = f.fy = f.scaling_factor = 1.f;
  return f;
}

// the body of cvo_fast_select_host and cvo_fast_select
int fast_select_entry(cvo_ctx* ctx, const char* who, int rows, int cols, const uint8_t* gray, const cvo_fast_schedule_t* schedule, int* pixel, int* n,
                      int* threshold_used) {
  std::string msg;
  int rc = fast_validate_plane(rows, cols, gray, &msg);
  if (rc == CVO_OK) rc = fast_validate_schedule(schedule, &msg);
  if (rc == CVO_OK && (!pixel || !n)) {
    rc = CVO_E_INVALID;
    msg = "pixel and n are required";
  }
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] {
    std::vector<int> pix;
    StereoStatsAcc st;
    if (!ctx || stereo_on_host(ctx, rows, cols)) {
      fast_select_cpu(GrayView{gray, 1}, cols, rows, *schedule, pix, st);
    } else {
      st.on_device = 1;
      RgbdDevice d;
      const int* list = nullptr;
      int k = 0, rc;
      if ((rc = rgbd_device_stage(ctx, fast_plane_frame(rows, cols, gray), true, d, true)) != CVO_OK) return rc;
      if ((rc = fast_device_select(ctx, d, *schedule, st, &list, &k)) != CVO_OK) return rc;
      if ((rc = rgbd_fetch(ctx, list, k, pix)) != CVO_OK) return rc;
    }
    st.candidates = st.kept = pix.size();
    copy_kept(pix, pixel, n);
    if (threshold_used) *threshold_used = st.threshold_used;
    if (ctx) ctx->stereo_last = st;
    return CVO_OK;
  });
}

}  // namespace

extern "C" {

int cvo_fast_select_host(int rows, int cols, const uint8_t* gray, const cvo_fast_schedule_t* schedule, int* pixel, int* n, int* threshold_used) {
  return fast_select_entry(nullptr, "cvo_fast_select_host", rows, cols, gray, schedule, pixel, n, threshold_used);
}

int cvo_fast_select(cvo_ctx* ctx, int rows, int cols, const uint8_t* gray, const cvo_fast_schedule_t* schedule, int* pixel, int* n,
                    int* threshold_used) {
  if (!ctx) return CVO_E_INVALID;
  return fast_select_entry(ctx, "cvo_fast_select", rows, cols, gray, schedule, pixel, n, threshold_used);
}

}  // extern "C"
