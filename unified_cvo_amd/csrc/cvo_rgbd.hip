// cvo_rgbd.hip -- RGB-D front end: cvo_rgbd_points (CvoPointCloud(ImageRGBD, Calibration, FULL / DSO_EDGES)),
// cvo_rgbd_points_host (the same on one CPU thread, no context), cvo_cloud_upload_rgbd (the multi-frame drivers' per-frame
// recipe: both candidate sets, voxel selection, edge rows then surface rows, the ordinary upload), cvo_debug_rgbd_stats.
// On the device (kernels of cvo_k_rgbd.h on upload_stream, under upload_mutex) only pixels, depth and an exclusion byte
// go up and only pixel indices come back; the survivors' rows are built on the host, as the voxel path does.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// Below this many pixels the CPU twin is the default route; RGBD_HOST=0 / 1 forces one route for every size.
constexpr int RGBD_HOST_BELOW = 32768;
constexpr int RGBD_NUM_WANT = 10000;  // dso_select_pixels' num_want (CvoPointCloud.cpp:327)

int rgbd_validate(const cvo_rgbd_frame_t* f, std::string* msg) {
  auto bad = [&](const std::string& m) {
    *msg = m;
    return CVO_E_INVALID;
  };
  auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  if (!f) return bad("frame is NULL");
  if (f->rows < 1 || f->cols < 1) return bad("rows and cols must be >= 1, got " + std::to_string(f->rows) + " x " + std::to_string(f->cols));
  if (f->channels != 1 && f->channels != 3) return bad("channels must be 1 or 3, got " + std::to_string(f->channels));
  if (!f->image) return bad("image is NULL");
  if (!f->depth) return bad("depth is NULL");
  if (f->depth_type != CVO_DEPTH_U16 && f->depth_type != CVO_DEPTH_F32) return bad("depth_type must be CVO_DEPTH_U16 or CVO_DEPTH_F32");
  if (!positive(f->fx) || !positive(f->fy)) return bad("fx and fy must be finite and > 0, got " + std::to_string(f->fx) + ", " + std::to_string(f->fy));
  if (!positive(f->scaling_factor)) return bad("scaling_factor must be finite and > 0, got " + std::to_string(f->scaling_factor));
  if (f->num_classes < 0 || (f->num_classes > 0 && !f->semantic)) return bad("num_classes > 0 needs the semantic image");
  if ((long long)f->rows * f->cols > VOX_MAX_POINTS) {
    *msg = "more than 2^24 pixels";
    return CVO_E_UNSUPPORTED;
  }
  return CVO_OK;
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

void rgbd_point_rows(const cvo_rgbd_frame_t& f, int method, const std::vector<int>& pix, float* xyz, float* feat, float* label, float* geotype) {
  const GrayView g = gray_view(f);
  const int F = f.channels + 2;
  const float t0 = method == CVO_SELECT_FULL ? 0.5f : 0.9f, t1 = method == CVO_SELECT_FULL ? 0.5f : 0.1f;
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
  VoxelCtl* ctl = nullptr;
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
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
  };
  const size_t o_ctl = take(sizeof(VoxelCtl)), o_img = take(need_select ? img_bytes : 0), o_depth = take(depth_bytes),
               o_excl = take(f.num_classes > 0 ? np : 0), o_g2 = take(need_select ? sizeof(float) * np : 0), o_ths = take(2 * sizeof(float) * n_ths),
               o_hit = take(sizeof(int) * (size_t)d.n_cells), o_sel = take(sizeof(int) * (size_t)d.n_cells), o_blocks = take(sizeof(unsigned) * nb),
               o_pix = take(sizeof(int) * cap), o_out = take(sizeof(int) * cap), o_xyz = take(sizeof(float) * 3 * cap),
               o_score = take(need_fast ? np : 0), o_fhist = take(need_fast ? sizeof(unsigned) * FAST_BINS : 0);
  if (off > ctx->rgbd_scratch_bytes) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
    if (ctx->rgbd_scratch) (void)hipFree(ctx->rgbd_scratch);
    ctx->rgbd_scratch = nullptr;
    ctx->rgbd_scratch_bytes = 0;
    const hipError_t e = hipMalloc(&ctx->rgbd_scratch, off);
    if (e != hipSuccess) return fail(ctx, CVO_E_NOMEM, std::string("RGB-D scratch hipMalloc: ") + hipGetErrorString(e));
    ctx->rgbd_scratch_bytes = off;
  }
  char* b = ctx->rgbd_scratch;
  d.ctl = (VoxelCtl*)(b + o_ctl);
  d.img = (unsigned char*)(b + o_img);
  d.depth = b + o_depth;
  d.excl = f.num_classes > 0 ? (unsigned char*)(b + o_excl) : nullptr;
  d.g2 = (float*)(b + o_g2);
  d.ths = (float*)(b + o_ths);
  d.sm = d.ths + n_ths;
  d.hit = (int*)(b + o_hit);
  d.sel = (int*)(b + o_sel);
  d.blocks = (unsigned*)(b + o_blocks);
  d.pix = (int*)(b + o_pix);
  d.out = (int*)(b + o_out);
  d.xyz = (float*)(b + o_xyz);
  d.score = (unsigned char*)(b + o_score);
  d.fast_hist = (unsigned*)(b + o_fhist);
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
  hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(VOX_THREADS), 0, st, d.nb_cells, d.blocks, d.ctl, 0, (const VoxelBlockStats*)nullptr);
  hipLaunchKernelGGL(k_rgbd_compact, dim3(d.nb_cells), dim3(RGBD_THREADS), 0, st, d.n_cells, (const int*)d.hit, (const unsigned*)d.blocks, d.sel);
  HIP_TRY(ctx, hipGetLastError());
  d.sel_offset.assign((size_t)d.nb_cells + 1, 0u);
  VoxelCtl c{};
  HIP_TRY(ctx, hipMemcpyAsync(d.sel_offset.data(), d.blocks, sizeof(unsigned) * (size_t)d.nb_cells, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&c, d.ctl, sizeof c, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  d.sel_offset[d.nb_cells] = c.n_kept;
  auto first = [&](int pot) { return d.sel_offset[(size_t)d.cells.start[pot - RGBD_POT_MIN] / RGBD_THREADS]; };
  auto count = [&](int pot) { return (int)(d.sel_offset[(size_t)d.cells.start[pot - RGBD_POT_MIN + 1] / RGBD_THREADS] - first(pot)); };
  const int pot = rgbd_schedule(count, stats);
  *list = d.sel + first(pot);
  *n = count(pot);
  if (*n < 0 || *n > rgbd_cells(pot, w, h)) return fail(ctx, CVO_E_HIP, "RGB-D selection: the device selected more pixels than there are cells");
  return CVO_OK;
}

// depth test + exclusion + back-projection of a candidate list (nullptr: FULL) into d.pix / d.xyz from `at` on; *n_out
// survivors.  One synchronisation.
int rgbd_device_backproject(cvo_ctx* ctx, const cvo_rgbd_frame_t& f, RgbdDevice& d, const int* list, int n, int at, int* n_out) {
  *n_out = 0;
  if (n == 0) return CVO_OK;
  hipStream_t st = ctx->upload_stream;
  const int nb = (n + RGBD_THREADS - 1) / RGBD_THREADS;
  hipLaunchKernelGGL(k_rgbd_bp_flag, dim3(nb), dim3(RGBD_THREADS), 0, st, n, list, d.w, d.h, (const void*)d.depth, f.depth_type,
                     (const unsigned char*)d.excl, d.blocks);
  hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(VOX_THREADS), 0, st, nb, d.blocks, d.ctl, 0, (const VoxelBlockStats*)nullptr);
  hipLaunchKernelGGL(k_rgbd_bp_write, dim3(nb), dim3(RGBD_THREADS), 0, st, n, list, d.w, d.h, (const void*)d.depth, f.depth_type,
                     (const unsigned char*)d.excl, rgbd_calib(f), (const unsigned*)d.blocks, d.pix + at, d.xyz + 3 * (size_t)at);
  HIP_TRY(ctx, hipGetLastError());
  VoxelCtl c{};
  HIP_TRY(ctx, hipMemcpyAsync(&c, d.ctl, sizeof c, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (c.n_kept > (unsigned)n) return fail(ctx, CVO_E_HIP, "RGB-D back-projection: the device kept more pixels than it was given");
  *n_out = (int)c.n_kept;
  return CVO_OK;
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

bool rgbd_on_host(const cvo_ctx* ctx, const cvo_rgbd_frame_t& f) {
  return ctx->opt.rgbd_host > 0 || (ctx->opt.rgbd_host < 0 && (long long)f.cols * f.rows < RGBD_HOST_BELOW);
}

// both candidate sets through the voxel grid: pixel indices of the survivors, edge first; n_edge of them are edges
int rgbd_recipe_pixels(cvo_ctx* ctx, const char* who, const cvo_rgbd_frame_t& f, float leaf, float divisor, std::vector<int>& pix, int* n_edge,
                       RgbdStatsAcc& st) {
  const float s_edge = leaf / divisor;
  std::string msg;
  if (voxel_validate(0, nullptr, s_edge, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": leaf / edge_divisor: " + msg);
  pix.clear();
  if (rgbd_on_host(ctx, f)) {
    st.on_device = 0;
    for (int pass = 0; pass < 2; pass++) {
      std::vector<int> cand, kept;
      rgbd_candidates_cpu(f, pass == 0 ? CVO_SELECT_DSO_EDGES : CVO_SELECT_FULL, cand, st);
      std::vector<float> xyz(3 * cand.size());
      for (size_t i = 0; i < cand.size(); i++) rgbd_xyz(f, cand[i], &xyz[3 * i]);
      const float s = pass == 0 ? s_edge : leaf;
      if (voxel_validate((int)cand.size(), xyz.data(), s, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + msg);
      voxel_select_cpu((int)cand.size(), xyz.data(), s, kept);
      for (int k : kept) pix.push_back(cand[(size_t)k]);
      if (pass == 0) *n_edge = (int)kept.size();
    }
    return CVO_OK;
  }
  st.on_device = 1;
  RgbdDevice d;
  int rc = rgbd_device_stage(ctx, f, true, d);
  if (rc != CVO_OK) return rc;
  const int* list = nullptr;
  int n_sel = 0, n_e = 0, n_s = 0;
  if ((rc = rgbd_device_select(ctx, d, st, &list, &n_sel)) != CVO_OK) return rc;
  if ((rc = rgbd_device_backproject(ctx, f, d, list, n_sel, 0, &n_e)) != CVO_OK) return rc;
  if ((rc = rgbd_device_backproject(ctx, f, d, nullptr, f.cols * f.rows, n_e, &n_s)) != CVO_OK) return rc;
  st.edge_points = (unsigned long long)n_e;
  st.surface_points = (unsigned long long)n_s;
  st.with_depth = d.excl ? rgbd_count_depth(f) : (unsigned long long)n_s;
  hipStream_t stream = ctx->upload_stream;
  int total = 0;
  *n_edge = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int n = pass == 0 ? n_e : n_s, at = pass == 0 ? 0 : n_e;
    if (n == 0) continue;
    const int* d_kept = nullptr;
    rc = voxel_run_device(ctx, n, nullptr, d.xyz + 3 * (size_t)at, pass == 0 ? s_edge : leaf, nullptr, &d_kept);
    if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + ctx->err);
    const int nk = (int)ctx->vox_last.n_kept;
    hipLaunchKernelGGL(k_rgbd_gather, dim3((nk + RGBD_THREADS - 1) / RGBD_THREADS), dim3(RGBD_THREADS), 0, stream, nk, n, d_kept,
                       (const int*)(d.pix + at), d.out + total);
    HIP_TRY(ctx, hipGetLastError());
    total += nk;
    if (pass == 0) *n_edge = nk;
  }
  return rgbd_fetch(ctx, d.out, total, pix);
}

}  // namespace

extern "C" {

int cvo_rgbd_points_host(const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label, float* geotype) {
  std::string msg;
  int rc = rgbd_validate(frame, &msg);
  if (rc == CVO_OK) rc = rgbd_method(method, &msg);
  if (rc == CVO_OK && method == CVO_SELECT_DSO_EDGES) rc = rgbd_threshold_range(frame->cols, frame->rows, &msg);
  if (rc != CVO_OK) return rc;
  if (!pixel || !n) return CVO_E_INVALID;
  try {
    std::vector<int> pix;
    RgbdStatsAcc st;
    rgbd_candidates_cpu(*frame, method, pix, st);
    rgbd_point_rows(*frame, method, pix, xyz, feat, label, geotype);
    if (!pix.empty()) std::memcpy(pixel, pix.data(), sizeof(int) * pix.size());
    *n = (int)pix.size();
  } catch (const std::exception&) {
    return CVO_E_NOMEM;
  }
  return CVO_OK;
}

int cvo_rgbd_points(cvo_ctx* ctx, const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat, float* label,
                    float* geotype) {
  if (!ctx) return CVO_E_INVALID;
  std::string msg;
  int rc = rgbd_validate(frame, &msg);
  if (rc == CVO_OK) rc = rgbd_method(method, &msg);
  if (rc == CVO_OK && method == CVO_SELECT_DSO_EDGES) rc = rgbd_threshold_range(frame->cols, frame->rows, &msg);
  if (rc == CVO_OK && (!pixel || !n)) {
    rc = CVO_E_INVALID;
    msg = "pixel and n are required";
  }
  if (rc != CVO_OK) return fail(ctx, rc, "cvo_rgbd_points: " + msg);
  try {
    std::lock_guard<std::mutex> lk(ctx->upload_mutex);
    std::vector<int> pix;
    RgbdStatsAcc st;
    if (rgbd_on_host(ctx, *frame)) {
      rgbd_candidates_cpu(*frame, method, pix, st);
    } else {
      st.on_device = 1;
      if ((rc = rgbd_points_device(ctx, *frame, method, pix, st)) != CVO_OK) return rc;
    }
    rgbd_point_rows(*frame, method, pix, xyz, feat, label, geotype);
    if (!pix.empty()) std::memcpy(pixel, pix.data(), sizeof(int) * pix.size());
    *n = (int)pix.size();
    ctx->rgbd_last = st;
  } catch (const std::exception& e) {
    return fail(ctx, CVO_E_NOMEM, std::string("cvo_rgbd_points: ") + e.what());
  }
  return CVO_OK;
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
  try {
    std::lock_guard<std::mutex> lk(ctx->upload_mutex);
    std::vector<int> pix;
    RgbdStatsAcc st;
    int n_edge = 0;
    if ((rc = rgbd_recipe_pixels(ctx, "cvo_cloud_upload_rgbd", *frame, leaf, edge_divisor, pix, &n_edge, st)) != CVO_OK) return rc;
    const size_t np = pix.size();
    std::vector<float> xyz(3 * np), feat((size_t)FD * np), geo(2 * np);
    const GrayView g = gray_view(*frame);
    for (size_t i = 0; i < np; i++) rgbd_recipe_row(*frame, g, pix[i], (int)i < n_edge, &xyz[3 * i], &feat[(size_t)FD * i], &geo[2 * i]);
    HostCloud h{(int)np, (const char*)xyz.data(), 12, (const char*)feat.data(), sizeof(float) * FD, nullptr, 0, (const char*)geo.data(), 8};
    std::vector<StagedCloud> one(1);
    if ((rc = upload_host_cloud(ctx, h, ctx->upload_stream, &one[0])) != CVO_OK) return rc;
    if ((rc = finish_uploads(ctx, one)) != CVO_OK) return rc;
    *out = one[0].c;
    if (pixel && np) std::memcpy(pixel, pix.data(), sizeof(int) * np);
    if (is_edge)
      for (size_t i = 0; i < np; i++) is_edge[i] = (int)i < n_edge ? 1 : 0;
    if (n) *n = (int)np;
    ctx->rgbd_last = st;
  } catch (const std::exception& e) {
    return fail(ctx, CVO_E_NOMEM, std::string("cvo_cloud_upload_rgbd: ") + e.what());
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

}  // extern "C"
