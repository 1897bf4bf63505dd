// cvo_rgbd.hip -- RGB-D front end: cvo_rgbd_points (CvoPointCloud(ImageRGBD, Calibration, FULL / DSO_EDGES)),
// cvo_rgbd_points_host (the same on one CPU thread, no context), cvo_cloud_upload_rgbd (the multi-frame drivers' per-frame
// recipe: both candidate sets, voxel selection, edge rows then surface rows, the ordinary upload), cvo_debug_rgbd_stats,
// cvo_debug_rgbd_readback (the stages of the last selection on the device, for the tests).
// On the device (kernels of cvo_k_rgbd.h on upload_stream, under upload_mutex) only pixels, depth and an exclusion byte
// go up and only pixel indices come back; the survivors' rows are built on the host, as the voxel path does.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// Below this many pixels the CPU twin is the default route; RGBD_HOST=0 / 1 forces one route for every size.
constexpr int RGBD_HOST_BELOW = 32768;
constexpr int RGBD_NUM_WANT = 10000;  // dso_select_pixels' num_want (CvoPointCloud.cpp:327)

// The refusals the frame types share, in the order the entry points report them: shape, image, then `calibration()` - the
// type's own depth / disparity and calibration checks: what is wrong, or "" -, classes, 2^24 pixels.
template <class Calibration>
int frame_validate(int rows, int cols, int channels, const unsigned char* image, int num_classes, const float* semantic, std::string* msg,
                   Calibration calibration) {
  auto bad = [&](const std::string& m) {
    *msg = m;
    return CVO_E_INVALID;
  };
  if (rows < 1 || cols < 1) return bad("rows and cols must be >= 1, got " + std::to_string(rows) + " x " + std::to_string(cols));
  if (channels != 1 && channels != 3) return bad("channels must be 1 or 3, got " + std::to_string(channels));
  if (!image) return bad("image is NULL");
  const std::string wrong = calibration();
  if (!wrong.empty()) return bad(wrong);
  if (num_classes < 0 || (num_classes > 0 && !semantic)) return bad("num_classes > 0 needs the semantic image");
  if ((long long)rows * cols > COMPACT_MAX_ELEMENTS) {
    *msg = "more than 2^24 pixels";
    return CVO_E_UNSUPPORTED;
  }
  return CVO_OK;
}

int rgbd_validate(const cvo_rgbd_frame_t* f, std::string* msg) {
  if (!f) {
    *msg = "frame is NULL";
    return CVO_E_INVALID;
  }
  auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  return frame_validate(f->rows, f->cols, f->channels, f->image, f->num_classes, f->semantic, msg, [&]() -> std::string {
    if (!f->depth) return "depth is NULL";
    if (f->depth_type != CVO_DEPTH_U16 && f->depth_type != CVO_DEPTH_F32) return "depth_type must be CVO_DEPTH_U16 or CVO_DEPTH_F32";
    if (!positive(f->fx) || !positive(f->fy)) return "fx and fy must be finite and > 0, got " + std::to_string(f->fx) + ", " + std::to_string(f->fy);
    if (!positive(f->scaling_factor)) return "scaling_factor must be finite and > 0, got " + std::to_string(f->scaling_factor);
    return "";
  });
}

int rgbd_method(int method, std::string* msg) {
  if (method == CVO_SELECT_FULL || method == CVO_SELECT_DSO_EDGES) return CVO_OK;
  *msg = "point selection method " + std::to_string(method) + " is not supported (FULL and DSO_EDGES are)";
  return method >= 0 && method <= CVO_SELECT_FULL ? CVO_E_UNSUPPORTED : CVO_E_INVALID;
}

// The literal thsSmoothed index of every pixel select() considers must stay inside (w/32)(h/32) + 100 entries
int rgbd_threshold_range(int w, int h, std::string* msg) {
  if (w < 10 || h < 8) return CVO_OK;  // (no pixel is considered)
  const long long last = ((w - 6) >> 5) + (long long)((h - 4) >> 5) * (w / 32), size = (long long)(w / 32) * (h / 32) + RGBD_THS_SLACK;
  if (last < size) return CVO_OK;
  *msg = "the selector's threshold index (x >> 5) + (y >> 5) * (cols / 32) reaches " + std::to_string(last) + " of " + std::to_string(size) +
         " entries for a " + std::to_string(w) + " x " + std::to_string(h) + " image";
  return CVO_E_UNSUPPORTED;
}

// the plane the gradient is taken of: the caller's gray plane, a 1-channel image, or the BGR image (gray per access)
struct GrayView {
  const unsigned char* p;
  int channels;
};
GrayView gray_view(const cvo_rgbd_frame_t& f) { return f.gray ? GrayView{f.gray, 1} : GrayView{f.image, f.channels}; }

// gradient_[j] of the interleaved (dx, dy) array (RawImage.cpp:55-82), computed where it is asked for
float rgbd_gradient_at(const GrayView& g, int w, int h, size_t j) {
  const size_t p = j >> 1;
  const int x = (int)(p % w), y = (int)(p / w);
  if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return 0.f;
  const size_t d = (j & 1) ? (size_t)w : 1;
  return 0.5f * ((float)rgbd_gray(g.p, g.channels, p + d) - (float)rgbd_gray(g.p, g.channels, p - d));
}

bool rgbd_excluded(const cvo_rgbd_frame_t& f, size_t p) {  // first maximum is class 10 (CvoPointCloud.cpp:501-507)
  if (f.num_classes <= 0) return false;
  const float* row = f.semantic + p * (size_t)f.num_classes;
  int best = 0;
  for (int c = 1; c < f.num_classes; c++)
    if (row[c] > row[best]) best = c;
  return best == 10;
}

// dso_select_pixels' schedule (CvoPixelSelector.cpp:430-453) over count(pot): returns the potential whose selection stands
template <class Count>
int rgbd_schedule(Count count, RgbdStatsAcc& st) {
  st.n_tried = 0;
  auto run = [&](int pot) {
    const int c = count(pot);
    st.tried[st.n_tried] = pot;
    st.count[st.n_tried++] = c;
    return c;
  };
  int pot = 3, have = run(3), times = 1;
  while (have > RGBD_NUM_WANT) {
    pot = 3 + times;
    have = run(pot);
    times++;
    if (times == 5) break;
  }
  if (have < RGBD_NUM_WANT / 3 * 2) {
    pot = 3 + times - 2;
    have = run(pot);
  }
  st.edge_selected = (unsigned long long)have;
  return pot;
}

// ---- CPU twin ------------------------------------------------------------------------------------------------------

void rgbd_select_cpu(const cvo_rgbd_frame_t& f, std::vector<int>& uv, RgbdStatsAcc& st) {
  const int w = f.cols, h = f.rows, w32 = w / 32, h32 = h / 32;
  const GrayView g = gray_view(f);
  std::vector<float> g2((size_t)w * h);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) g2[(size_t)y * w + x] = rgbd_g2(g.p, g.channels, w, h, x, y);
  std::vector<float> ths((size_t)w32 * h32 + RGBD_THS_SLACK, 0.f), sm(ths.size(), 0.f);
  for (int by = 0; by < h32; by++)
    for (int bx = 0; bx < w32; bx++) {
      unsigned bins[50] = {};
      for (int j = 0; j < 32; j++)
        for (int i = 0; i < 32; i++) {
          const int it = i + 32 * bx, jt = j + 32 * by;
          if (it > w - 2 || jt > h - 2 || it < 1 || jt < 1) continue;
          bins[std::min(48, rgbd_root(g2[(size_t)jt * w + it]))]++;
          bins[49]++;
        }
      ths[bx + by * w32] = (float)(rgbd_quantile(bins, bins[49]) + 7);
    }
  for (int by = 0; by < h32; by++)
    for (int bx = 0; bx < w32; bx++) sm[bx + by * w32] = rgbd_smooth_one(ths.data(), w32, h32, bx, by);
  std::vector<int> lists[RGBD_POTS];
  bool done[RGBD_POTS] = {};
  const int pot = rgbd_schedule(
      [&](int p) {
        std::vector<int>& l = lists[p - RGBD_POT_MIN];
        if (!done[p - RGBD_POT_MIN]) {
          const int nc = rgbd_cells(p, w, h);
          for (int c = 0; c < nc; c++) {
            const int best = rgbd_cell_best(c, p, w, h, g2.data(), sm.data());
            if (best >= 0) l.push_back(best);
          }
          done[p - RGBD_POT_MIN] = true;
        }
        return (int)l.size();
      },
      st);
  uv.swap(lists[pot - RGBD_POT_MIN]);
}

// candidates of a method with a depth that are not excluded, in the reference's order
void rgbd_candidates_cpu(const cvo_rgbd_frame_t& f, int method, std::vector<int>& pix, RgbdStatsAcc& st) {
  const int w = f.cols, h = f.rows;
  pix.clear();
  float dep;
  if (method == CVO_SELECT_FULL) {
    unsigned long long with_depth = 0;
    for (int u = 0; u < w; u++)
      for (int v = 0; v < h; v++) {
        const size_t p = (size_t)v * w + u;
        if (!rgbd_depth(f.depth, f.depth_type, p, &dep)) continue;
        with_depth++;
        if (!rgbd_excluded(f, p)) pix.push_back((int)p);
      }
    st.with_depth = with_depth;
    st.surface_points = pix.size();
    return;
  }
  std::vector<int> uv;
  rgbd_select_cpu(f, uv, st);
  for (int p : uv)
    if (rgbd_depth(f.depth, f.depth_type, (size_t)p, &dep) && !rgbd_excluded(f, (size_t)p)) pix.push_back(p);
  st.edge_points = pix.size();
}

// ---- rows of kept pixels (host, both routes) -------------------------------------------------------------------------

RgbdCalib rgbd_calib(const cvo_rgbd_frame_t& f) { return RgbdCalib{f.fx, f.fy, f.cx, f.cy, f.scaling_factor}; }

void rgbd_xyz(const cvo_rgbd_frame_t& f, int p, float* xyz) {
  float dep = 0.f;
  (void)rgbd_depth(f.depth, f.depth_type, (size_t)p, &dep);
  rgbd_backproject(rgbd_calib(f), p % f.cols, p / f.cols, dep, xyz);
}

// the channels + 2 features of the image constructor (CvoPointCloud.cpp:527-545).  The reference reads the interleaved
// gradient array at the PIXEL index (v w + u, v w + u + 1): reproduced.
void rgbd_features(const cvo_rgbd_frame_t& f, const GrayView& g, int p, float* out) {
  const int ch = f.channels;
  for (int c = 0; c < ch; c++) out[c] = (float)((double)(float)f.image[(size_t)p * ch + c] / 255.0);
  out[ch] = (float)((double)rgbd_gradient_at(g, f.cols, f.rows, (size_t)p) / 500.0 + 0.5);
  out[ch + 1] = (float)((double)rgbd_gradient_at(g, f.cols, f.rows, (size_t)p + 1) / 500.0 + 0.5);
}

// the rows of the kept pixels that are asked for (a stereo frame comes as its stereo_view and has its xyz already)
void rgbd_point_rows(const cvo_rgbd_frame_t& f, int method, const std::vector<int>& pix, float* xyz, float* feat, float* label, float* geotype) {
  const GrayView g = gray_view(f);
  const int F = f.channels + 2;
  const float t0 = method == CVO_SELECT_FULL ? 0.5f : (method == CVO_SELECT_CV_FAST ? 1.f : 0.9f);  // (CV_FAST: the stereo constructor's pure edges)
  const float t1 = method == CVO_SELECT_FULL ? 0.5f : (method == CVO_SELECT_CV_FAST ? 0.f : 0.1f);
  for (size_t i = 0; i < pix.size(); i++) {
    if (xyz) rgbd_xyz(f, pix[i], xyz + 3 * i);
    if (feat) rgbd_features(f, g, pix[i], feat + F * i);
    if (label && f.num_classes > 0)
      std::memcpy(label + i * (size_t)f.num_classes, f.semantic + (size_t)pix[i] * f.num_classes, sizeof(float) * (size_t)f.num_classes);
    if (geotype) {
      geotype[2 * i] = t0;
      geotype[2 * i + 1] = t1;
    }
  }
}

// a row of the drivers' recipe: the first three image-constructor features through export_to_pcd's bytes
// (min(255, int(f * 255)), CvoPointCloud.cpp:1237-1239) and back through the (XYZRGB, GeometryType) constructor (:614-618)
void rgbd_recipe_row(const cvo_rgbd_frame_t& f, const GrayView& g, int p, bool edge, float* xyz, float* feat5, float* geo) {
  float ft[5] = {};
  rgbd_features(f, g, p, ft);
  rgbd_xyz(f, p, xyz);
  for (int c = 0; c < 3; c++) {
    const int byte = std::min(255, (int)(ft[c] * 255));
    feat5[c] = (float)((double)(float)byte / 255.0);
  }
  feat5[3] = feat5[4] = 0.f;
  geo[0] = edge ? 1.f : 0.f;
  geo[1] = edge ? 0.f : 1.f;
}

// ---- device route --------------------------------------------------------------------------------------------------------

struct RgbdDevice {
  int w = 0, h = 0;
  unsigned char *img = nullptr, *excl = nullptr;
  void* depth = nullptr;
  float *g2 = nullptr, *ths = nullptr, *sm = nullptr, *xyz = nullptr;
  int *hit = nullptr, *sel = nullptr, *pix = nullptr, *out = nullptr;
  unsigned* blocks = nullptr;
  unsigned* ctl = nullptr;  // the total of the last compaction
  unsigned char* score = nullptr;  // FAST score bytes and the frame's 257-bin histogram (cvo_fast.hip), when asked for
  unsigned* fast_hist = nullptr;
  int img_channels = 1;
  RgbdCells cells{};
  int n_cells = 0, nb_cells = 0;
  std::vector<unsigned> sel_offset;  // exclusive offsets of the selection's blocks, after rgbd_device_select
};

// lays the frame's buffers out in the context's RGB-D scratch region and copies image, depth and exclusion bytes up
// (need_fast: room for the FAST detector's score bytes and histogram as well; a frame without a depth image copies none)
int rgbd_device_stage(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, bool need_select, RgbdDevice& d, bool need_fast = false) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->rgbd_sel.valid = false;  // (the region is about to be laid out anew: the last selection's stages end here)
  const int w = f.cols, h = f.rows;
  const size_t np = (size_t)w * h;
  d.w = w;
  d.h = h;
  d.n_cells = 0;
  for (int k = 0; k < RGBD_POTS; k++) {
    d.cells.start[k] = d.n_cells;
    d.n_cells += (int)align_up((size_t)rgbd_cells(RGBD_POT_MIN + k, w, h), RGBD_THREADS);
  }
  d.cells.start[RGBD_POTS] = d.n_cells;
  d.nb_cells = d.n_cells / RGBD_THREADS;
  const GrayView g = gray_view(f);
  d.img_channels = g.channels;
  const size_t img_bytes = np * (size_t)g.channels, depth_bytes = f.depth ? np * (f.depth_type == CVO_DEPTH_U16 ? 2 : 4) : 0;
  const size_t n_ths = (size_t)(w / 32) * (h / 32) + RGBD_THS_SLACK, nb = std::max((np + RGBD_THREADS - 1) / RGBD_THREADS, (size_t)d.nb_cells);
  size_t cap = 0;  // candidates of both sets: every pixel (FULL) + the largest selection
  for (int k = 0; k < RGBD_POTS; k++) cap = std::max(cap, (size_t)rgbd_cells(RGBD_POT_MIN + k, w, h));
  cap += np;
  const int rc = ctx->rgbd_scratch.lay_out(ctx, "RGB-D scratch", [&](ScratchLayout& l) {
    l.take(d.ctl, 1);
    l.take(d.img, need_select ? img_bytes : 0);
    l.take_as<char>(d.depth, depth_bytes);
    if (f.num_classes > 0) l.take(d.excl, np);
    l.take(d.g2, need_select ? np : 0);
    l.take(d.ths, 2 * n_ths);  // (thresholds, then their smoothed copy)
    d.sm = d.ths + n_ths;
    l.take(d.hit, (size_t)d.n_cells);
    l.take(d.sel, (size_t)d.n_cells);
    l.take(d.blocks, nb);
    l.take(d.pix, cap);
    l.take(d.out, cap);
    l.take(d.xyz, 3 * cap);
    l.take(d.score, need_fast ? np : 0);
    l.take(d.fast_hist, need_fast ? (size_t)FAST_BINS : 0);
  });
  if (rc != CVO_OK) return rc;
  hipStream_t st = ctx->upload_stream;
  if (need_select) HIP_TRY(ctx, hipMemcpyAsync(d.img, g.p, img_bytes, hipMemcpyHostToDevice, st));
  if (depth_bytes) HIP_TRY(ctx, hipMemcpyAsync(d.depth, f.depth, depth_bytes, hipMemcpyHostToDevice, st));
  if (d.excl) {
    ctx->rgbd_excl.resize(np);  // (lives until the stream has been synchronised: a member, not a local)
    for (size_t p = 0; p < np; p++) ctx->rgbd_excl[p] = rgbd_excluded(f, p) ? 1 : 0;
    HIP_TRY(ctx, hipMemcpyAsync(d.excl, ctx->rgbd_excl.data(), np, hipMemcpyHostToDevice, st));
  }
  return CVO_OK;
}

// the selector on the device: all six potentials in one launch chain, ONE synchronisation, then the schedule on the host.
// *list / *n: the standing selection, on the device.
int rgbd_device_select(cvo_ctx* ctx, RgbdDevice& d, RgbdStatsAcc& stats, const int** list, int* n) {
  hipStream_t st = ctx->upload_stream;
  const int w = d.w, h = d.h, w32 = w / 32, h32 = h / 32, np = w * h;
  const size_t n_ths = (size_t)w32 * h32 + RGBD_THS_SLACK;
  HIP_TRY(ctx, hipMemsetAsync(d.ths, 0, 2 * sizeof(float) * n_ths, st));
  hipLaunchKernelGGL(k_rgbd_gray_grad, dim3((np + RGBD_THREADS - 1) / RGBD_THREADS), dim3(RGBD_THREADS), 0, st, w, h, d.img_channels,
                     (const unsigned char*)d.img, d.g2);
  if (w32 * h32 > 0) {
    hipLaunchKernelGGL(k_rgbd_hist, dim3(w32 * h32), dim3(RGBD_THREADS), 0, st, w, h, (const float*)d.g2, d.ths);
    hipLaunchKernelGGL(k_rgbd_smooth, dim3(1), dim3(RGBD_THREADS), 0, st, w32, h32, (const float*)d.ths, d.sm);
  }
  hipLaunchKernelGGL(k_rgbd_select, dim3(d.nb_cells), dim3(RGBD_THREADS), 0, st, w, h, d.cells, (const float*)d.g2, (const float*)d.sm, d.hit,
                     d.blocks);
  const int rc = compact_counted(ctx, d.n_cells, RgbdCellHit{d.hit, d.sel}, d.blocks, scan_into(ctx, d.ctl));
  if (rc != CVO_OK) return rc;
  d.sel_offset.assign((size_t)d.nb_cells + 1, 0u);
  unsigned c = 0;
  HIP_TRY(ctx, hipMemcpyAsync(d.sel_offset.data(), d.blocks, sizeof(unsigned) * (size_t)d.nb_cells, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&c, d.ctl, sizeof c, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  d.sel_offset[d.nb_cells] = c;
  auto first = [&](int pot) { return d.sel_offset[(size_t)d.cells.start[pot - RGBD_POT_MIN] / RGBD_THREADS]; };
  auto count = [&](int pot) { return (int)(d.sel_offset[(size_t)d.cells.start[pot - RGBD_POT_MIN + 1] / RGBD_THREADS] - first(pot)); };
  const int pot = rgbd_schedule(count, stats);
  *list = d.sel + first(pot);
  *n = count(pot);
  if (*n < 0 || *n > rgbd_cells(pot, w, h)) return fail(ctx, CVO_E_HIP, "RGB-D selection: the device selected more pixels than there are cells");
  RgbdSelectionAcc& s = ctx->rgbd_sel;  // (for cvo_debug_rgbd_readback: nothing is launched or copied for it)
  s.w = w;
  s.h = h;
  s.cells = d.cells;
  s.sel_offset = d.sel_offset;
  s.g2 = d.g2;
  s.ths = d.ths;
  s.sm = d.sm;
  s.sel = d.sel;
  s.valid = true;
  return CVO_OK;
}

// a frame type's keep predicate and back-projection (RgbdKeep, StereoKeep) over the n candidates of pred.list (nullptr:
// FULL) into d.pix / d.xyz from `at` on; *n_out survivors.  One synchronisation.
template <class P>
int frame_device_backproject(cvo_ctx* ctx, const char* who, RgbdDevice& d, P pred, int n, int at, int* n_out) {
  *n_out = 0;
  if (n == 0) return CVO_OK;
  pred.pix_out = d.pix + at;
  pred.xyz = d.xyz + 3 * (size_t)at;
  int rc = compact(ctx, n, pred, d.blocks, scan_into(ctx, d.ctl));
  if (rc != CVO_OK) return rc;
  unsigned c = 0;
  if ((rc = compact_total(ctx, d.ctl, n, who, "pixels", &c)) != CVO_OK) return rc;
  *n_out = (int)c;
  return CVO_OK;
}

int rgbd_device_backproject(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, RgbdDevice& d, const int* list, int n, int at, int* n_out) {
  return frame_device_backproject(ctx, "RGB-D back-projection", d, RgbdKeep{list, d.w, d.h, d.depth, f.depth_type, d.excl, rgbd_calib(f), nullptr, nullptr},
                                  n, at, n_out);
}

int rgbd_fetch(cvo_ctx* ctx, const int* d_src, int n, std::vector<int>& out) {
  out.resize((size_t)n);
  if (n) {
    HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_src, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->upload_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  }
  return CVO_OK;
}

// pixels with a depth when an exclusion byte hides some of them from the FULL pass's count (semantic frames only)
unsigned long long rgbd_count_depth(const cvo_rgbd_frame_t& f) {
  unsigned long long c = 0;
  float dep;
  for (size_t p = 0, np = (size_t)f.cols * f.rows; p < np; p++) c += rgbd_depth(f.depth, f.depth_type, p, &dep) ? 1 : 0;
  return c;
}

int rgbd_points_device(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, int method, std::vector<int>& pix, RgbdStatsAcc& st) {
  RgbdDevice d;
  int rc = rgbd_device_stage(ctx, f, method == CVO_SELECT_DSO_EDGES, d);
  if (rc != CVO_OK) return rc;
  const int* list = nullptr;
  int n = f.cols * f.rows, kept = 0;
  if (method == CVO_SELECT_DSO_EDGES && (rc = rgbd_device_select(ctx, d, st, &list, &n)) != CVO_OK) return rc;
  if ((rc = rgbd_device_backproject(ctx, f, d, list, n, 0, &kept)) != CVO_OK) return rc;
  if (method == CVO_SELECT_FULL) {
    st.surface_points = (unsigned long long)kept;
    st.with_depth = d.excl ? rgbd_count_depth(f) : (unsigned long long)kept;
  } else {
    st.edge_points = (unsigned long long)kept;
  }
  return rgbd_fetch(ctx, d.pix, kept, pix);
}

bool rgbd_on_host(const cvo_ctx* ctx, const cvo_rgbd_frame_t& f) { return route_on_host(ctx->opt.rgbd_host, (long long)f.cols * f.rows, RGBD_HOST_BELOW); }

// The drivers' per-frame recipe for either frame type: both candidate sets - edges, then FULL - through the voxel grid
// (leaf / divisor for the edges); pixel indices of the survivors, edge first, n_edge of them edges, and - xyz != nullptr, host
// route only - their coordinates.  `view`: the frame as rgbd_device_stage reads it.
//   host_pass(method, cand, cxyz)   host route: a pass's candidates and their coordinates (the CPU twins)
//   device_pass(d, &n_e, &n_s)      device route: selection and both back-projections into d.pix / d.xyz, edges from 0, FULL from n_e
template <class HostPass, class DevicePass>
int recipe_pixels(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t& view, bool on_host, float leaf, float divisor, std::vector<int>& pix,
                  std::vector<float>* xyz, int* n_edge, HostPass host_pass, DevicePass device_pass) {
  const float s_edge = leaf / divisor;
  std::string msg;
  if (voxel_validate(0, nullptr, s_edge, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": leaf / edge_divisor: " + msg);
  pix.clear();
  *n_edge = 0;
  if (on_host) {
    for (int pass = 0; pass < 2; pass++) {
      std::vector<int> cand, kept;
      std::vector<float> cxyz;
      host_pass(pass == 0 ? CVO_SELECT_DSO_EDGES : CVO_SELECT_FULL, cand, cxyz);
      const float s = pass == 0 ? s_edge : leaf;
      if (voxel_validate((int)cand.size(), cxyz.data(), s, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + msg);
      voxel_select_cpu((int)cand.size(), cxyz.data(), s, kept);
      for (int k : kept) {
        pix.push_back(cand[(size_t)k]);
        if (xyz) xyz->insert(xyz->end(), &cxyz[3 * (size_t)k], &cxyz[3 * (size_t)k] + 3);
      }
      if (pass == 0) *n_edge = (int)kept.size();
    }
    return CVO_OK;
  }
  RgbdDevice d;
  int rc = rgbd_device_stage(ctx, view, true, d);
  if (rc != CVO_OK) return rc;
  int n_e = 0, n_s = 0;
  if ((rc = device_pass(d, &n_e, &n_s)) != CVO_OK) return rc;
  int total = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int n = pass == 0 ? n_e : n_s, at = pass == 0 ? 0 : n_e;
    if (n == 0) continue;
    const int* d_kept = nullptr;
    rc = voxel_run_device(ctx, n, nullptr, d.xyz + 3 * (size_t)at, pass == 0 ? s_edge : leaf, nullptr, &d_kept);
    if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + ctx->err);
    const int nk = (int)ctx->vox_last.n_kept;
    hipLaunchKernelGGL(k_rgbd_gather, dim3((nk + RGBD_THREADS - 1) / RGBD_THREADS), dim3(RGBD_THREADS), 0, ctx->upload_stream, nk, n, d_kept,
                       (const int*)(d.pix + at), d.out + total);
    HIP_TRY(ctx, hipGetLastError());
    total += nk;
    if (pass == 0) *n_edge = nk;
  }
  return rgbd_fetch(ctx, d.out, total, pix);
}

// the recipe of an RGB-D frame
int rgbd_recipe_pixels(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t& f, float leaf, float divisor, std::vector<int>& pix, int* n_edge,
                       RgbdStatsAcc& st) {
  st.on_device = rgbd_on_host(ctx, f) ? 0 : 1;
  return recipe_pixels(
      ctx, who, f, !st.on_device, leaf, divisor, pix, nullptr, n_edge,
      [&](int method, std::vector<int>& cand, std::vector<float>& cxyz) {
        rgbd_candidates_cpu(f, method, cand, st);
        cxyz.resize(3 * cand.size());
        for (size_t i = 0; i < cand.size(); i++) rgbd_xyz(f, cand[i], &cxyz[3 * i]);
      },
      [&](RgbdDevice& d, int* n_e, int* n_s) {
        const int* list = nullptr;
        int n_sel = 0, rc;
        if ((rc = rgbd_device_select(ctx, d, st, &list, &n_sel)) != CVO_OK) return rc;
        if ((rc = rgbd_device_backproject(ctx, f, d, list, n_sel, 0, n_e)) != CVO_OK) return rc;
        if ((rc = rgbd_device_backproject(ctx, f, d, nullptr, f.cols * f.rows, *n_e, n_s)) != CVO_OK) return rc;
        st.edge_points = (unsigned long long)*n_e;
        st.surface_points = (unsigned long long)*n_s;
        st.with_depth = d.excl ? rgbd_count_depth(f) : (unsigned long long)*n_s;
        return CVO_OK;
      });
}

// a successful RGB-D call's last statement: its stats stand, and one that took the host route leaves no stages to read back
void rgbd_commit(cvo_ctx* ctx, const RgbdStatsAcc& st) {
  ctx->rgbd_last = st;
  if (!st.on_device) ctx->rgbd_sel.valid = false;
}

// the body of cvo_rgbd_points_host and cvo_rgbd_points
int rgbd_points_entry(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                      float* label, float* geotype) {
  std::string msg;
  int rc = rgbd_validate(frame, &msg);
  if (rc == CVO_OK) rc = rgbd_method(method, &msg);
  if (rc == CVO_OK && method == CVO_SELECT_DSO_EDGES) rc = rgbd_threshold_range(frame->cols, frame->rows, &msg);
  if (rc == CVO_OK && (!pixel || !n)) {
    rc = CVO_E_INVALID;
    msg = "pixel and n are required";
  }
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] {
    std::vector<int> pix;
    RgbdStatsAcc st;
    if (!ctx || rgbd_on_host(ctx, *frame)) {
      rgbd_candidates_cpu(*frame, method, pix, st);
    } else {
      st.on_device = 1;
      const int rc = rgbd_points_device(ctx, *frame, method, pix, st);
      if (rc != CVO_OK) return rc;
    }
    rgbd_point_rows(*frame, method, pix, xyz, feat, label, geotype);
    copy_kept(pix, pixel, n);
    if (ctx) rgbd_commit(ctx, st);
    return CVO_OK;
  });
}

}  // namespace

extern "C" {

int cvo_rgbd_points_host(const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label, float* geotype) {
  return rgbd_points_entry(nullptr, "cvo_rgbd_points_host", frame, method, pixel, n, xyz, feat, label, geotype);
}

int cvo_rgbd_points(cvo_ctx* ctx, const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label,
                    float* geotype) {
  if (!ctx) return CVO_E_INVALID;
  return rgbd_points_entry(ctx, "cvo_rgbd_points", frame, method, pixel, n, xyz, feat, label, geotype);
}

int cvo_cloud_upload_rgbd(cvo_ctx* ctx, const cvo_rgbd_frame_t* frame, float leaf, float edge_divisor, cvo_cloud** out, int* pixel,
                          unsigned char* is_edge, int* n) {
  if (!ctx) return CVO_E_INVALID;
  std::string msg;
  int rc = rgbd_validate(frame, &msg);
  if (rc == CVO_OK) rc = rgbd_threshold_range(frame->cols, frame->rows, &msg);
  if (rc == CVO_OK && !out) {
    rc = CVO_E_INVALID;
    msg = "out is NULL";
  }
  if (rc == CVO_OK && voxel_validate(0, nullptr, leaf, &msg) != CVO_OK) {
    rc = CVO_E_INVALID;
    msg = "leaf: " + msg;
  }
  if (rc == CVO_OK && (!std::isfinite(edge_divisor) || !(edge_divisor > 0.f))) {
    rc = CVO_E_INVALID;
    msg = "edge_divisor must be finite and > 0, got " + std::to_string(edge_divisor);
  }
  if (rc != CVO_OK) return fail(ctx, rc, "cvo_cloud_upload_rgbd: " + msg);
  return frontend_call(ctx, "cvo_cloud_upload_rgbd", [&] {
    std::vector<int> pix;
    RgbdStatsAcc st;
    int n_edge = 0, rc;
    if ((rc = rgbd_recipe_pixels(ctx, "cvo_cloud_upload_rgbd", *frame, leaf, edge_divisor, pix, &n_edge, st)) != CVO_OK) return rc;
    const size_t np = pix.size();
    std::vector<float> xyz(3 * np), feat((size_t)FD * np), geo(2 * np);
    const GrayView g = gray_view(*frame);
    for (size_t i = 0; i < np; i++) rgbd_recipe_row(*frame, g, pix[i], (int)i < n_edge, &xyz[3 * i], &feat[(size_t)FD * i], &geo[2 * i]);
    const HostCloud h{(int)np, (const char*)xyz.data(), 12, (const char*)feat.data(), sizeof(float) * FD, nullptr, 0, (const char*)geo.data(), 8};
    if ((rc = upload_one_locked(ctx, h, out)) != CVO_OK) return rc;
    copy_kept(pix, pixel, n, is_edge, n_edge);
    rgbd_commit(ctx, st);
    return CVO_OK;
  });
}

int cvo_debug_rgbd_stats(cvo_ctx* ctx, int* n_tried, int* potentials, int* counts, unsigned long long* edge_selected,
                         unsigned long long* edge_points, unsigned long long* surface_points, unsigned long long* with_depth, int* on_device) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const RgbdStatsAcc& s = ctx->rgbd_last;
  if (n_tried) *n_tried = s.n_tried;
  for (int i = 0; i < s.n_tried; i++) {
    if (potentials) potentials[i] = s.tried[i];
    if (counts) counts[i] = s.count[i];
  }
  if (edge_selected) *edge_selected = s.edge_selected;
  if (edge_points) *edge_points = s.edge_points;
  if (surface_points) *surface_points = s.surface_points;
  if (with_depth) *with_depth = s.with_depth;
  if (on_device) *on_device = s.on_device;
  return CVO_OK;
}

int cvo_debug_rgbd_readback(cvo_ctx* ctx, int* rows, int* cols, int* counts, float* g2, float* ths, float* sm, int* selected) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const RgbdSelectionAcc& s = ctx->rgbd_sel;
  if (!s.valid || !ctx->rgbd_scratch.p)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_rgbd_readback: the context's last RGB-D call ran no selection on the device");
  if (rows) *rows = s.h;
  if (cols) *cols = s.w;
  auto first = [&](int k) { return s.sel_offset[(size_t)s.cells.start[k] / RGBD_THREADS]; };
  for (int k = 0; counts && k < RGBD_POTS; k++) counts[k] = (int)(first(k + 1) - first(k));
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)s.w * s.h, n_ths = (size_t)(s.w / 32) * (s.h / 32) + RGBD_THS_SLACK, n_sel = first(RGBD_POTS);
  if (g2) HIP_TRY(ctx, hipMemcpyAsync(g2, s.g2, sizeof(float) * np, hipMemcpyDeviceToHost, st));
  if (ths) HIP_TRY(ctx, hipMemcpyAsync(ths, s.ths, sizeof(float) * n_ths, hipMemcpyDeviceToHost, st));
  if (sm) HIP_TRY(ctx, hipMemcpyAsync(sm, s.sm, sizeof(float) * n_ths, hipMemcpyDeviceToHost, st));
  if (selected && n_sel) HIP_TRY(ctx, hipMemcpyAsync(selected, s.sel, sizeof(int) * n_sel, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

}  // extern "C"
