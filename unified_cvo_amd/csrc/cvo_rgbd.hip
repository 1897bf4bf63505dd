// cvo_rgbd.hip -- RGB-D front end: cvo_rgbd_points (CvoPointCloud(ImageRGBD, Calibration, FULL / DSO_EDGES)),
// cvo_rgbd_points_host (the same on one CPU thread, no context), cvo_cloud_upload_rgbd (the multi-frame drivers' per-frame
// recipe: both candidate sets, voxel selection, edge rows then surface rows, the ordinary upload), cvo_debug_rgbd_stats,
// cvo_debug_rgbd_readback (the stages of the last selection on the device, for the tests).
// On the device (kernels of cvo_k_rgbd.h on upload_stream, under upload_mutex) only pixels, depth and an exclusion byte
// go up and only pixel indices come back; the survivors' rows are built on the host, as the voxel path does.
// cvo_cloud_from_rgbd_device / _recipe: the same two clouds of a frame whose planes are ALREADY in device memory - the planes
// read in place, the class rule in the keep predicate, the rows by k_rgbd_rows (cvo_k_rgbd_rows.h), the cloud by the ingest of
// cvo_ingest.hip: no plane and no row crosses to the host.  cvo_rgbd_frame_rows_host: the CPU twin of that row arithmetic.
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

// the plane the gradient is taken of (GrayView, cvo_k_rgbd_rows.h): the caller's gray plane, a 1-channel image, or the BGR image
GrayView gray_view(const cvo_rgbd_frame_t& f) { return f.gray ? GrayView{f.gray, 1} : GrayView{f.image, f.channels}; }

// a host frame's dense rows x cols x num_classes scores as the strided view the shared arithmetic reads
RgbdScores rgbd_scores(const cvo_rgbd_frame_t& f) {
  const size_t c = (size_t)std::max(f.num_classes, 0);
  return RgbdScores{(const char*)f.semantic, sizeof(float) * c * (size_t)f.cols, sizeof(float) * c, sizeof(float), f.semantic ? f.num_classes : 0, f.cols};
}

bool rgbd_excluded(const cvo_rgbd_frame_t& f, size_t p) { return rgbd_excluded(rgbd_scores(f), p); }

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

// a host frame as the shared row arithmetic (rgbd_xyz, rgbd_features, rgbd_recipe_row of cvo_k_rgbd_rows.h) reads it
RgbdRowFrame rgbd_row_frame(const cvo_rgbd_frame_t& f, const GrayView& g) {
  return RgbdRowFrame{f.cols, f.rows, f.channels, f.image, g, f.depth, f.depth_type, rgbd_calib(f), rgbd_scores(f)};
}

void rgbd_xyz(const cvo_rgbd_frame_t& f, int p, float* xyz) { rgbd_xyz(rgbd_row_frame(f, gray_view(f)), p, xyz); }

// the geometric type of the image constructor's points (CV_FAST: the stereo constructor's pure edges)
RgbdRowKind rgbd_constructor_rows(int method) {
  return RgbdRowKind{0, method == CVO_SELECT_FULL ? 0.5f : (method == CVO_SELECT_CV_FAST ? 1.f : 0.9f),
                     method == CVO_SELECT_FULL ? 0.5f : (method == CVO_SELECT_CV_FAST ? 0.f : 0.1f)};
}

// the rows of the kept pixels that are asked for (a stereo frame comes as its stereo_view and has its xyz already)
void rgbd_point_rows(const cvo_rgbd_frame_t& f, int method, const std::vector<int>& pix, float* xyz, float* feat, float* label, float* geotype) {
  const RgbdRowFrame rf = rgbd_row_frame(f, gray_view(f));
  const int F = f.channels + 2;
  const RgbdRowKind kind = rgbd_constructor_rows(method);
  for (size_t i = 0; i < pix.size(); i++) {
    if (xyz) rgbd_xyz(rf, pix[i], xyz + 3 * i);
    if (feat) rgbd_features(rf, pix[i], feat + F * i);
    if (label && f.num_classes > 0)
      std::memcpy(label + i * (size_t)f.num_classes, f.semantic + (size_t)pix[i] * f.num_classes, sizeof(float) * (size_t)f.num_classes);
    if (geotype) {
      geotype[2 * i] = kind.t0;
      geotype[2 * i + 1] = kind.t1;
    }
  }
}

// a row of the drivers' recipe (rgbd_recipe_row of cvo_k_rgbd_rows.h) of a host frame
void rgbd_recipe_row(const cvo_rgbd_frame_t& f, const GrayView& g, int p, bool edge, float* xyz, float* feat5, float* geo) {
  rgbd_recipe_row(rgbd_row_frame(f, g), p, edge, xyz, feat5, geo);
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
// (need_fast: room for the FAST detector's score bytes and histogram as well; a frame without a depth image copies none).
// planes_on_device: f.image / gray / depth are the CALLER'S device memory (a checked cvo_rgbd_device_frame_t): the kernels
// read them where they are - nothing is copied, no room is taken for them, and there is no exclusion plane (RgbdKeepScores).
int rgbd_device_stage(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, bool need_select, RgbdDevice& d, bool need_fast = false, bool planes_on_device = false) {
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
  const size_t img_bytes = planes_on_device ? 0 : np * (size_t)g.channels;
  const size_t depth_bytes = f.depth && !planes_on_device ? np * (f.depth_type == CVO_DEPTH_U16 ? 2 : 4) : 0;
  const size_t n_ths = (size_t)(w / 32) * (h / 32) + RGBD_THS_SLACK, nb = std::max((np + RGBD_THREADS - 1) / RGBD_THREADS, (size_t)d.nb_cells);
  size_t cap = 0;  // candidates of both sets: every pixel (FULL) + the largest selection
  for (int k = 0; k < RGBD_POTS; k++) cap = std::max(cap, (size_t)rgbd_cells(RGBD_POT_MIN + k, w, h));
  cap += np;
  const int rc = ctx->rgbd_scratch.lay_out(ctx, "RGB-D scratch", [&](ScratchLayout& l) {
    l.take(d.ctl, 2);  // (the compaction's total; the pixels with a depth of a device frame with classes)
    l.take(d.img, need_select ? img_bytes : 0);
    l.take_as<char>(d.depth, depth_bytes);
    if (f.num_classes > 0 && !planes_on_device) l.take(d.excl, np);
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
  if (planes_on_device) {  // (only ever read: the kernels take them as pointers to const)
    d.img = const_cast<unsigned char*>(g.p);
    d.depth = const_cast<void*>(f.depth);
    return CVO_OK;
  }
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

// A device frame's back-projection: the class scores' rule in keep() (RgbdKeepScores) where the frame has classes, RgbdKeep
// as it is where it has none.  with_depth (optional): the pixels of the whole frame with a depth, counted by the ordered
// compaction's count and scan (RgbdHasDepth) ahead of the pass and read back with its total: still one synchronisation.
int rgbd_device_backproject_scores(cvo_ctx* ctx, const cvo_rgbd_frame_t& view, const RgbdScores& scores, RgbdDevice& d, const int* list, int n, int at,
                                   int* n_out, unsigned long long* with_depth) {
  const char* who = "RGB-D back-projection";
  RgbdKeep keep{list, d.w, d.h, d.depth, view.depth_type, nullptr, rgbd_calib(view), d.pix + at, d.xyz + 3 * (size_t)at};
  *n_out = 0;
  if (n == 0) return CVO_OK;
  hipStream_t st = ctx->upload_stream;
  if (with_depth) {
    const int np = d.w * d.h;
    const RgbdHasDepth has{d.depth, view.depth_type};
    hipLaunchKernelGGL(k_compact_count<RgbdHasDepth>, dim3((np + COMPACT_THREADS - 1) / COMPACT_THREADS), dim3(COMPACT_THREADS), 0, st, np, has, d.blocks);
    scan_into(ctx, d.ctl + 1)((np + COMPACT_THREADS - 1) / COMPACT_THREADS, d.blocks);
    HIP_TRY(ctx, hipGetLastError());
  }
  int rc = scores.classes > 0 ? compact(ctx, n, RgbdKeepScores{keep, scores}, d.blocks, scan_into(ctx, d.ctl))
                              : compact(ctx, n, keep, d.blocks, scan_into(ctx, d.ctl));
  if (rc != CVO_OK) return rc;
  unsigned c[2] = {0u, 0u};
  HIP_TRY(ctx, hipMemcpyAsync(c, d.ctl, sizeof(unsigned) * (with_depth ? 2 : 1), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if ((rc = compact_check(ctx, c[0], n, who, "pixels")) != CVO_OK) return rc;
  if (with_depth && (rc = compact_check(ctx, c[1], d.w * d.h, who, "pixels with a depth")) != CVO_OK) return rc;
  *n_out = (int)c[0];
  if (with_depth) *with_depth = c[1];
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

// ---- THE device candidate chain of both RGB-D routes, over a back-projection policy with two operations:
//   run(d, list, n, at, n_out, full)   the candidates list[0 .. n) (nullptr: every pixel) into d.pix / d.xyz from `at`; full: the FULL pass
//   with_depth(d, n_full)              the pixels of the frame with a depth, asked once the FULL pass has kept n_full

// a host frame (staged by rgbd_device_stage): the exclusion plane the host made hides pixels from the pass, and then from its count
struct RgbdHostFramePolicy {
  cvo_ctx* ctx;
  const cvo_rgbd_frame_t& f;
  int run(RgbdDevice& d, const int* list, int n, int at, int* n_out, bool) { return rgbd_device_backproject(ctx, f, d, list, n, at, n_out); }
  unsigned long long with_depth(const RgbdDevice& d, int n_full) const { return d.excl ? rgbd_count_depth(f) : (unsigned long long)n_full; }
};

// a device frame (read in place): the class scores' rule runs in keep(), and the FULL pass of a frame with classes counts the depths itself
struct RgbdDeviceFramePolicy {
  cvo_ctx* ctx;
  const cvo_rgbd_frame_t& view;
  const RgbdScores& scores;
  unsigned long long counted = 0;
  int run(RgbdDevice& d, const int* list, int n, int at, int* n_out, bool full) {
    return rgbd_device_backproject_scores(ctx, view, scores, d, list, n, at, n_out, full && scores.classes > 0 ? &counted : nullptr);
  }
  unsigned long long with_depth(const RgbdDevice&, int n_full) const { return scores.classes > 0 ? counted : (unsigned long long)n_full; }
};

// the stats of a call that ran the chain: n_edge edge candidates and n_full FULL ones kept (-1: that pass did not run)
template <class Policy>
void rgbd_chain_stats(RgbdStatsAcc& st, const Policy& bp, const RgbdDevice& d, int n_edge, int n_full) {
  st.on_device = 1;
  if (n_edge >= 0) st.edge_points = (unsigned long long)n_edge;
  if (n_full < 0) return;
  st.surface_points = (unsigned long long)n_full;
  st.with_depth = bp.with_depth(d, n_full);
}

// the points of a method: stage -> select (the DSO edges) -> back-project -> stats; *kept pixel indices are in d.pix
template <class Policy>
int rgbd_points_chain(cvo_ctx* ctx, const cvo_rgbd_frame_t& view, bool planes_on_device, int method, Policy bp, RgbdDevice& d, RgbdStatsAcc& st,
                      int* kept) {
  const bool full = method == CVO_SELECT_FULL;
  int rc = rgbd_device_stage(ctx, view, method == CVO_SELECT_DSO_EDGES, d, false, planes_on_device);
  if (rc != CVO_OK) return rc;
  const int* list = nullptr;
  int n = view.cols * view.rows;
  if (method == CVO_SELECT_DSO_EDGES && (rc = rgbd_device_select(ctx, d, st, &list, &n)) != CVO_OK) return rc;
  if ((rc = bp.run(d, list, n, 0, kept, full)) != CVO_OK) return rc;
  rgbd_chain_stats(st, bp, d, full ? -1 : *kept, full ? *kept : -1);
  return CVO_OK;
}

// the recipe's device_pass (recipe_pixels): the selection, then both back-projections - edges from 0, FULL from *n_e - and the stats
template <class Policy>
auto rgbd_device_pass(cvo_ctx* ctx, int n_pixels, Policy bp, RgbdStatsAcc& st) {
  return [ctx, n_pixels, bp, &st](RgbdDevice& d, int* n_e, int* n_s) mutable {
    const int* list = nullptr;
    int n_sel = 0, rc;
    if ((rc = rgbd_device_select(ctx, d, st, &list, &n_sel)) != CVO_OK) return rc;
    if ((rc = bp.run(d, list, n_sel, 0, n_e, false)) != CVO_OK) return rc;
    if ((rc = bp.run(d, nullptr, n_pixels, *n_e, n_s, true)) != CVO_OK) return rc;
    rgbd_chain_stats(st, bp, d, *n_e, *n_s);
    return (int)CVO_OK;
  };
}

int rgbd_points_device(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, int method, std::vector<int>& pix, RgbdStatsAcc& st) {
  RgbdDevice d;
  int kept = 0;
  const int rc = rgbd_points_chain(ctx, f, false, method, RgbdHostFramePolicy{ctx, f}, d, st, &kept);
  if (rc != CVO_OK) return rc;
  return rgbd_fetch(ctx, d.pix, kept, pix);
}

bool rgbd_on_host(const cvo_ctx* ctx, const cvo_rgbd_frame_t& f) { return route_on_host(ctx->opt.rgbd_host, (long long)f.cols * f.rows, RGBD_HOST_BELOW); }

// The device route of the recipe below, up to where the survivors' pixel indices are in d.out (*total of them, the first
// *n_edge the edges): staging (planes_on_device: of a device frame, rgbd_device_stage), device_pass, the two voxel selections.
template <class DevicePass>
int recipe_pixels_device(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t& view, bool planes_on_device, float leaf, float s_edge, RgbdDevice& d,
                         int* n_edge, int* total, DevicePass device_pass) {
  *total = 0;
  int rc = rgbd_device_stage(ctx, view, true, d, false, planes_on_device);
  if (rc != CVO_OK) return rc;
  int n_e = 0, n_s = 0;
  if ((rc = device_pass(d, &n_e, &n_s)) != CVO_OK) return rc;
  for (int pass = 0; pass < 2; pass++) {
    const int n = pass == 0 ? n_e : n_s, at = pass == 0 ? 0 : n_e;
    if (n == 0) continue;
    const int* d_kept = nullptr;
    rc = voxel_run_device(ctx, n, nullptr, d.xyz + 3 * (size_t)at, pass == 0 ? s_edge : leaf, nullptr, &d_kept);
    if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + ctx->err);
    const int nk = (int)ctx->vox_last.n_kept;
    hipLaunchKernelGGL(k_rgbd_gather, dim3((nk + RGBD_THREADS - 1) / RGBD_THREADS), dim3(RGBD_THREADS), 0, ctx->upload_stream, nk, n, d_kept,
                       (const int*)(d.pix + at), d.out + *total);
    HIP_TRY(ctx, hipGetLastError());
    *total += nk;
    if (pass == 0) *n_edge = nk;
  }
  return CVO_OK;
}

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
  int total = 0;
  const int rc = recipe_pixels_device(ctx, who, view, false, leaf, s_edge, d, n_edge, &total, device_pass);
  if (rc != CVO_OK) return rc;
  return rgbd_fetch(ctx, d.out, total, pix);
}

// the recipe of an RGB-D frame
int rgbd_recipe_pixels(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t& f, float leaf, float divisor, std::vector<int>& pix, int* n_edge,
                       RgbdStatsAcc& st) {
  return recipe_pixels(
      ctx, who, f, rgbd_on_host(ctx, f), leaf, divisor, pix, nullptr, n_edge,
      [&](int method, std::vector<int>& cand, std::vector<float>& cxyz) {
        rgbd_candidates_cpu(f, method, cand, st);
        cxyz.resize(3 * cand.size());
        for (size_t i = 0; i < cand.size(); i++) rgbd_xyz(f, cand[i], &cxyz[3 * i]);
      },
      rgbd_device_pass(ctx, f.cols * f.rows, RgbdHostFramePolicy{ctx, f}, st));
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
      const int rc = rgbd_points_device(ctx, *frame, method, pix, st);
      if (rc != CVO_OK) return rc;
    }
    rgbd_point_rows(*frame, method, pix, xyz, feat, label, geotype);
    copy_kept(pix, pixel, n);
    if (ctx) rgbd_commit(ctx, st);
    return CVO_OK;
  });
}

// ---- frames whose planes are already in device memory (cvo_rgbd_device_frame_t) ---------------------------------------------
// The planes are read IN PLACE: the selection, the back-projection and k_rgbd_rows take the caller's pointers, nothing is
// copied into the scratch region (the call synchronises before it returns, so the planes need not outlive it).  RGBD_HOST does
// not apply.  The same struct with HOST pointers is what the twin cvo_rgbd_frame_rows_host reads.

// the frame as the selection and the stage read it: the planes' pointers; the class scores go their own way (RgbdScores)
cvo_rgbd_frame_t rgbd_device_view(const cvo_rgbd_device_frame_t& f) {
  cvo_rgbd_frame_t v{};
  v.rows = f.rows;
  v.cols = f.cols;
  v.channels = f.channels;
  v.image = (const uint8_t*)f.image;
  v.gray = (const uint8_t*)f.gray;
  v.depth = f.depth;
  v.depth_type = f.depth_type;
  v.fx = f.fx;
  v.fy = f.fy;
  v.cx = f.cx;
  v.cy = f.cy;
  v.scaling_factor = f.scaling_factor;
  return v;
}

RgbdScores rgbd_device_scores(const cvo_rgbd_device_frame_t& f) {
  if (f.num_classes <= 0) return RgbdScores{nullptr, 0, 0, 0, 0, f.cols};
  return RgbdScores{(const char*)f.semantic, f.semantic_row_stride, f.semantic_pixel_stride, f.semantic_class_stride, f.num_classes, f.cols};
}

RgbdRowFrame rgbd_device_row_frame(const cvo_rgbd_device_frame_t& f) {
  const cvo_rgbd_frame_t v = rgbd_device_view(f);
  RgbdRowFrame rf = rgbd_row_frame(v, gray_view(v));
  rf.scores = rgbd_device_scores(f);
  return rf;
}

// what the host can say of a device frame's FIELDS without classifying a pointer: cvo_rgbd_points' refusals in its words, then
// the class count and the strides
int rgbd_device_fields(const cvo_rgbd_device_frame_t* f, std::string* msg) {
  if (!f) {
    *msg = "frame is NULL";
    return CVO_E_INVALID;
  }
  cvo_rgbd_frame_t v = rgbd_device_view(*f);
  v.num_classes = f->num_classes;
  v.semantic = (const float*)f->semantic;
  const int rc = rgbd_validate(&v, msg);
  if (rc != CVO_OK) return rc;
  if (f->num_classes > NC) {
    *msg = "num_classes " + std::to_string(f->num_classes) + ": a resident cloud holds " + std::to_string(NC) + " class columns";
    return CVO_E_UNSUPPORTED;
  }
  const size_t stride[3] = {f->semantic_row_stride, f->semantic_pixel_stride, f->semantic_class_stride};
  const char* name[3] = {"semantic_row_stride", "semantic_pixel_stride", "semantic_class_stride"};
  for (int k = 0; f->num_classes > 0 && k < 3; k++)
    if (stride[k] == 0 || (stride[k] & 3u) != 0 || stride[k] > 0xffffffffull) {
      *msg = std::string(name[k]) + ": a stride of " + std::to_string(stride[k]) + " bytes (strides are > 0 and multiples of 4)";
      return CVO_E_INVALID;
    }
  return CVO_OK;
}

// every plane classified (device_extent_ok, cvo_ingest.hip) before anything reads through it; the caller holds upload_mutex
int rgbd_device_planes(cvo_ctx* ctx, const cvo_rgbd_device_frame_t& f, std::string* why) {
  const size_t np = (size_t)f.rows * f.cols, depth_size = f.depth_type == CVO_DEPTH_U16 ? 2 : 4;
  const std::string shape = std::to_string(f.rows) + " x " + std::to_string(f.cols);
  if (!device_extent_ok(ctx, "image", f.image, 1, np * (size_t)f.channels, shape + " x " + std::to_string(f.channels) + " bytes", why)) return CVO_E_INVALID;
  if (f.gray && !device_extent_ok(ctx, "gray", f.gray, 1, np, shape + " bytes", why)) return CVO_E_INVALID;
  if (!device_extent_ok(ctx, "depth", f.depth, depth_size, np * depth_size, shape + (depth_size == 2 ? " uint16 depths" : " float depths"), why)) return CVO_E_INVALID;
  if (f.num_classes > 0) {
    const size_t need = (size_t)(f.rows - 1) * f.semantic_row_stride + (size_t)(f.cols - 1) * f.semantic_pixel_stride +
                        (size_t)(f.num_classes - 1) * f.semantic_class_stride + sizeof(float);
    if (!device_extent_ok(ctx, "semantic", f.semantic, 4, need, shape + " x " + std::to_string(f.num_classes) + " strided scores", why)) return CVO_E_INVALID;
  }
  return CVO_OK;
}

// the rows of the pixels d_pix[0 .. n) (the first n_edge a recipe's edges) by k_rgbd_rows, where k_cloud_ingest reads them, and
// the ingest; the pixel list comes down only when the caller asked for it, ahead of the ingest's synchronisation.  staged: the cloud.
int rgbd_device_cloud(cvo_ctx* ctx, const char* who, const RgbdRowFrame& rf, const RgbdRowKind& kind, const int* d_pix, int n, int n_edge, int* pixel,
                      std::vector<StagedCloud>& staged) {
  hipStream_t st = ctx->upload_stream;
  RgbdRowsOut o{};
  const bool labels = rf.scores.classes > 0 && !kind.recipe;  // (a recipe's cloud carries none, as cvo_cloud_upload_rgbd's)
  if (n > 0) {
    const size_t nn = (size_t)n;
    const int rc = ctx->rgbd_rows.lay_out(ctx, "RGB-D rows", [&](ScratchLayout& l) {
      l.take(o.xyz, 3 * nn);
      l.take(o.feat, FD * nn);
      if (labels) l.take(o.label, NC * nn);
      l.take(o.geo, 2 * nn);
    });
    if (rc != CVO_OK) return rc;
    hipLaunchKernelGGL(k_rgbd_rows, dim3((unsigned)((n + RGBD_ROW_THREADS - 1) / RGBD_ROW_THREADS)), dim3(RGBD_ROW_THREADS), 0, st, n, n_edge, d_pix, rf, kind, o);
    HIP_TRY(ctx, hipGetLastError());
    if (pixel) HIP_TRY(ctx, hipMemcpyAsync(pixel, d_pix, sizeof(int) * nn, hipMemcpyDeviceToHost, st));
  }
  const cvo_device_rows_t r = device_rows(n, n, o.xyz, o.feat, FD, o.label, NC, o.geo);
  const int rc = ingest_device_clouds(ctx, 1, &r, staged, who);  // (synchronises upload_stream; on error the cloud is released)
  if (rc != CVO_OK || n == 0) (void)hipStreamSynchronize(st);     // (nothing of this call is in flight when it returns)
  return rc;
}

// the arguments every device-frame entry point refuses before it takes the lock
int rgbd_device_check(const cvo_rgbd_device_frame_t* frame, int method, bool select, std::string* msg) {
  int rc = rgbd_device_fields(frame, msg);
  if (rc == CVO_OK) rc = rgbd_method(method, msg);
  if (rc == CVO_OK && select) rc = rgbd_threshold_range(frame->cols, frame->rows, msg);
  return rc;
}

int rgbd_from_device_points(cvo_ctx* ctx, const char* who, const cvo_rgbd_device_frame_t& f, int method, int* pixel, int* n_out,
                            std::vector<StagedCloud>& staged) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::string why;
  if (rgbd_device_planes(ctx, f, &why) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + why);
  const cvo_rgbd_frame_t view = rgbd_device_view(f);
  const RgbdRowFrame rf = rgbd_device_row_frame(f);
  RgbdStatsAcc st;
  RgbdDevice d;
  int kept = 0;
  int rc = rgbd_points_chain(ctx, view, true, method, RgbdDeviceFramePolicy{ctx, view, rf.scores}, d, st, &kept);
  if (rc != CVO_OK) return rc;
  if ((rc = rgbd_device_cloud(ctx, who, rf, rgbd_constructor_rows(method), d.pix, kept, 0, pixel, staged)) != CVO_OK) return rc;
  if (n_out) *n_out = kept;
  rgbd_commit(ctx, st);
  return CVO_OK;
}

int rgbd_from_device_recipe(cvo_ctx* ctx, const char* who, const cvo_rgbd_device_frame_t& f, float leaf, float divisor, int* pixel, int* n_out,
                            int* n_edge_out, std::vector<StagedCloud>& staged) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::string why;
  if (rgbd_device_planes(ctx, f, &why) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + why);
  const cvo_rgbd_frame_t view = rgbd_device_view(f);
  const RgbdRowFrame rf = rgbd_device_row_frame(f);
  RgbdStatsAcc st;
  RgbdDevice d;
  int n_edge = 0, total = 0;
  int rc = recipe_pixels_device(ctx, who, view, true, leaf, leaf / divisor, d, &n_edge, &total,
                                rgbd_device_pass(ctx, f.cols * f.rows, RgbdDeviceFramePolicy{ctx, view, rf.scores}, st));
  if (rc != CVO_OK) return rc;
  if ((rc = rgbd_device_cloud(ctx, who, rf, RgbdRowKind{1, 0.f, 0.f}, d.out, total, n_edge, pixel, staged)) != CVO_OK) return rc;
  if (n_out) *n_out = total;
  if (n_edge_out) *n_edge_out = n_edge;
  rgbd_commit(ctx, st);
  return CVO_OK;
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

int cvo_cloud_from_rgbd_device(cvo_ctx* ctx, const cvo_rgbd_device_frame_t* frame, int method, cvo_cloud** out, int* n, int* pixel) {
  const char* who = "cvo_cloud_from_rgbd_device";
  if (out) *out = nullptr;
  if (n) *n = 0;
  if (!ctx) return CVO_E_INVALID;
  std::string msg;
  int rc = rgbd_device_check(frame, method, method == CVO_SELECT_DSO_EDGES, &msg);
  if (rc == CVO_OK && !out) {
    rc = CVO_E_INVALID;
    msg = "out is NULL";
  }
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) { return rgbd_from_device_points(ctx, who, *frame, method, pixel, n, staged); });
}

int cvo_cloud_from_rgbd_device_recipe(cvo_ctx* ctx, const cvo_rgbd_device_frame_t* frame, float leaf, float edge_divisor, cvo_cloud** out, int* n,
                                      int* n_edge, int* pixel) {
  const char* who = "cvo_cloud_from_rgbd_device_recipe";
  if (out) *out = nullptr;
  if (n) *n = 0;
  if (n_edge) *n_edge = 0;
  if (!ctx) return CVO_E_INVALID;
  std::string msg;
  int rc = rgbd_device_check(frame, CVO_SELECT_DSO_EDGES, true, &msg);
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
  if (rc == CVO_OK && voxel_validate(0, nullptr, leaf / edge_divisor, &msg) != CVO_OK) {
    rc = CVO_E_INVALID;
    msg = "leaf / edge_divisor: " + msg;
  }
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) {
    return rgbd_from_device_recipe(ctx, who, *frame, leaf, edge_divisor, pixel, n, n_edge, staged);
  });
}

int cvo_rgbd_frame_rows_host(const cvo_rgbd_device_frame_t* frame, int recipe, int method, int n, const int* pixel, const unsigned char* is_edge,
                             float* xyz, float* feat, float* label, float* geotype, unsigned char* excluded) {
  std::string msg;
  int rc = rgbd_device_fields(frame, &msg);
  if (rc == CVO_OK && !recipe) rc = rgbd_method(method, &msg);
  if (rc != CVO_OK) return rc;
  if (n < 0 || (n > 0 && !pixel) || (n > 0 && recipe && !is_edge)) return CVO_E_INVALID;
  const int np = frame->rows * frame->cols;
  for (int i = 0; i < n; i++)
    if ((unsigned)pixel[i] >= (unsigned)np) return CVO_E_INVALID;
  const RgbdRowFrame rf = rgbd_device_row_frame(*frame);
  const RgbdRowKind kind = recipe ? RgbdRowKind{1, 0.f, 0.f} : rgbd_constructor_rows(method);
  for (int i = 0; i < n; i++) {
    const int p = pixel[i];
    float row_xyz[3], row_feat[FD], row_geo[2];
    rgbd_row5(rf, kind, p, recipe && is_edge[i] != 0, row_xyz, row_feat, row_geo);
    if (xyz) std::memcpy(xyz + 3 * (size_t)i, row_xyz, sizeof row_xyz);
    if (feat) std::memcpy(feat + (size_t)FD * i, row_feat, sizeof row_feat);
    if (geotype) std::memcpy(geotype + 2 * (size_t)i, row_geo, sizeof row_geo);
    if (label) {
      const char* at = rf.scores.classes > 0 ? rgbd_scores_at(rf.scores, (size_t)p) : nullptr;
      for (int c = 0; c < NC; c++) label[(size_t)NC * i + c] = c < rf.scores.classes ? rgbd_score(at, rf.scores, c) : 0.f;
    }
    if (excluded) excluded[i] = rgbd_excluded(rf.scores, (size_t)p) ? 1 : 0;
  }
  return CVO_OK;
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
