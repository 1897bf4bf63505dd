// cvo_dfilter.hip -- the disparity post-filter: cvo_disparity_filter(_host) (libelas's removeSmallSegments, gapInterpolation
// and adaptiveMean, full-resolution branch, on a float map whose invalid pixels are negative), dfilter_run for the chains of
// cvo_stereo_pair.hip (the matcher of cvo_sgm.hip, then the filter, the map resident in between), and
// cvo_debug_dfilter_stats.  tests/np_dfilter.py states what is computed; the CPU twin (dfilter_cpu) uses the same arithmetic
// (cvo_dfilter_math.h) as the kernels of cvo_k_dfilter.h.  A SECTION of the one translation unit cvo_hip.hip; not compiled on
// its own.
namespace {

// pixels; below, the CPU twin is the default route (profiles/dfilter/crossover.txt)
constexpr int DFILTER_HOST_BELOW = 32768;
constexpr long long DFILTER_MAX_PIXELS = 1ll << 24;

bool dfilter_on_host(const cvo_ctx* ctx, long long np) { return route_on_host(ctx->opt.dfilter_host, np, DFILTER_HOST_BELOW); }

int dfilter_validate_config(int rows, int cols, const cvo_dfilter_config_t* cfg, std::string* msg) {
  if (!cfg) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (rows < 1 || cols < 1) return *msg = "rows and cols start at 1", CVO_E_INVALID;
  if (!std::isfinite(cfg->speckle_sim_threshold) || cfg->speckle_sim_threshold < 0.f) return *msg = "speckle_sim_threshold must be finite and >= 0", CVO_E_INVALID;
  if (cfg->speckle_size < 0 || cfg->ipol_gap_width < 0) return *msg = "speckle_size and ipol_gap_width start at 0", CVO_E_INVALID;
  return CVO_OK;
}

// the map: finite, and no negative value within `sim` of a valid one (libelas's flood fill would depend on its seed order)
int dfilter_validate_map(int rows, int cols, const float* in, float sim, std::string* msg) {
  const size_t np = (size_t)rows * cols;
  bool finite = true, apart = true;
  for (size_t p = 0; p < np; p++) {
    const float v = in[p];
    finite &= std::isfinite(v);
    apart &= v >= 0.f || v < -sim;
  }
  if (!finite) return *msg = "the map holds a value that is not finite", CVO_E_INVALID;
  if (!apart) return *msg = "the map holds a negative value that is not below -speckle_sim_threshold", CVO_E_INVALID;
  return CVO_OK;
}

int dfilter_validate(int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, const float* out, std::string* msg) {
  if (!in || !out) return *msg = "a required pointer is missing", CVO_E_INVALID;
  const int rc = dfilter_validate_config(rows, cols, cfg, msg);
  if (rc != CVO_OK) return rc;
  if ((long long)rows * cols > DFILTER_MAX_PIXELS) return *msg = "more than 2^24 pixels", CVO_E_UNSUPPORTED;
  return dfilter_validate_map(rows, cols, in, cfg->speckle_sim_threshold, msg);
}

DFilterConst dfilter_const(int rows, int cols, const cvo_dfilter_config_t& c) {
  return DFilterConst{rows, cols, c.speckle_sim_threshold, c.speckle_size, c.ipol_gap_width, c.adaptive_mean};
}

// ---- CPU twin: one thread; d is filtered in place ----
void dfilter_speckle_cpu(const DFilterConst& k, float* d, DFilterStatsAcc& stats) {
  if (k.speckle_size <= 1) return;
  const int W = k.cols, H = k.rows;
  const size_t np = (size_t)W * H;
  std::vector<unsigned char> done(np, 0);
  std::vector<int> seg;
  for (size_t s = 0; s < np; s++) {
    if (done[s]) continue;
    done[s] = 1;
    if (!dfilter_valid(d[s])) {
      d[s] = DFILTER_INVALID;  // a segment of its own, below any speckle_size > 1
      continue;
    }
    seg.assign(1, (int)s);
    for (size_t i = 0; i < seg.size(); i++) {
      const int c = seg[i], y = c / W, x = c - y * W;
      const int nb[4] = {x > 0 ? c - 1 : -1, x + 1 < W ? c + 1 : -1, y > 0 ? c - W : -1, y + 1 < H ? c + W : -1};
      for (int n : nb)
        if (n >= 0 && !done[(size_t)n] && dfilter_valid(d[n]) && dfilter_similar(d[c], d[n], k.sim)) done[(size_t)n] = 1, seg.push_back(n);
    }
    stats.segments++;
    if ((long long)seg.size() < k.speckle_size) {
      for (int c : seg) d[c] = DFILTER_INVALID;  // (no later segment reads them: an invalid pixel joins nothing)
      stats.removed += seg.size();
    }
  }
}

// libelas's loop over one line, as it is
void dfilter_gap_line_cpu(float* d, int len, size_t es, int width, DFilterStatsAcc& stats) {
  int count = 0;
  for (int j = 0; j < len; j++) {
    if (dfilter_valid(d[(size_t)j * es])) {
      if (count >= 1 && count <= width && j - count > 0) {
        const float v = dfilter_fill(d[(size_t)(j - count - 1) * es], d[(size_t)j * es]);
        for (int i = j - count; i < j; i++) d[(size_t)i * es] = v;
        stats.filled += (unsigned long long)count;
      }
      count = 0;
    } else {
      count++;
    }
  }
}

void dfilter_gap_cpu(const DFilterConst& k, float* d, DFilterStatsAcc& stats) {
  if (k.gap_width < 1) return;
  for (int v = 0; v < k.rows; v++) dfilter_gap_line_cpu(d + (size_t)v * k.cols, k.cols, 1, k.gap_width, stats);
  for (int u = 0; u < k.cols; u++) dfilter_gap_line_cpu(d + u, k.rows, (size_t)k.cols, k.gap_width, stats);
}

void dfilter_mean_cpu(const DFilterConst& k, float* d) {
  if (!k.mean) return;
  const int W = k.cols, H = k.rows;
  const size_t np = (size_t)W * H;
  std::vector<float> copy(np);
  for (size_t p = 0; p < np; p++) copy[p] = dfilter_valid(d[p]) ? d[p] : DFILTER_INVALID;
  std::vector<float> tmp(copy);  // (libelas leaves the valid pixels of D_tmp unset: the one departure)
  float q;
  for (int v = 3; v <= H - 4; v++)
    for (int u = 4; u <= W - 4; u++) {
      const float* win = &copy[(size_t)v * W + (size_t)(u - DFILTER_MEAN_BEFORE)];
      if (dfilter_mean(win, 1, u - DFILTER_MEAN_BEFORE, win[DFILTER_MEAN_BEFORE], &q)) tmp[(size_t)v * W + u] = q;
    }
  for (int v = 4; v <= H - 4; v++)
    for (int u = 3; u <= W - 4; u++) {
      const float* win = &tmp[(size_t)(v - DFILTER_MEAN_BEFORE) * W + (size_t)u];
      if (dfilter_mean(win, W, v - DFILTER_MEAN_BEFORE, win[(size_t)DFILTER_MEAN_BEFORE * W], &q)) d[(size_t)v * W + u] = q;
    }
}

void dfilter_cpu(const DFilterConst& k, float* d, DFilterStatsAcc& stats) {
  dfilter_speckle_cpu(k, d, stats);
  dfilter_gap_cpu(k, d, stats);
  dfilter_mean_cpu(k, d);
}

// ---- device route ----
// Enqueues the filter of the resident map d_in (nullptr: `in`, uploaded first) on upload_stream, then one download of the
// result with its counters and one synchronisation; both copies go through the context's pinned staging buffer.  The maps after each stage stay in the region for
// cvo_debug_dfilter_stats until the next call.
int dfilter_device(cvo_ctx* ctx, const DFilterConst& k, const float* in, const float* d_in, float* out, DFilterStatsAcc& stats) {
  hipStream_t st = ctx->upload_stream;
  const size_t np = (size_t)k.rows * k.cols, map = 4 * np;
  float *d_map = nullptr, *d_speckle = nullptr, *d_gap_rows = nullptr, *d_gap = nullptr, *d_tmp = nullptr, *d_out = nullptr;
  DFilterSpeckleArgs a;
  DFilterGapArgs g;
  const int rc = ctx->dfilter_scratch.lay_out(ctx, "disparity filter scratch", [&](ScratchLayout& l) {
    l.take(d_map, np);
    l.take(a.parent, np);
    l.take(a.root, np);
    l.take(a.size, np);
    l.take(g.prev, np);
    l.take(d_speckle, np);
    l.take(d_gap_rows, np);
    l.take(d_gap, np);
    l.take(d_tmp, np);
    l.take_as<char>(d_out, map + sizeof(DFilterCounters));  // the counters behind the map: one download
  });
  if (rc != CVO_OK) return rc;
  // (the read-back keeps offsets, not pointers: a later refused call may move the region while this call's record stands)
  auto offset_of = [&](const float* p) { return (size_t)((const char*)p - ctx->dfilter_scratch.p); };
  // pinned staging: [the map going up | the result and its counters coming down]
  char *h_up = nullptr, *h_down = nullptr;
  const int rc_staging = ctx->dfilter_staging.lay_out(ctx, "disparity filter staging", [&](ScratchLayout& l) {
    l.take(h_up, map);
    l.take(h_down, map + sizeof(DFilterCounters));
  });
  if (rc_staging != CVO_OK) return rc_staging;
  DFilterCounters* counters = (DFilterCounters*)(d_out + np);
  HIP_TRY(ctx, hipMemsetAsync(counters, 0, sizeof *counters, st));
  if (!d_in) {
    std::memcpy(h_up, in, map);
    HIP_TRY(ctx, hipMemcpyAsync(d_map, h_up, map, hipMemcpyHostToDevice, st));
    d_in = d_map;
  }
  const int tiles_x = (k.cols + DFILTER_TILE_W - 1) / DFILTER_TILE_W;
  const dim3 grid((unsigned)tiles_x * (unsigned)((k.rows + DFILTER_TILE_H - 1) / DFILTER_TILE_H)), block(DFILTER_THREADS);  // (at most 2^24 pixels)
  const bool speckle = k.speckle_size > 1, gap = k.gap_width >= 1, mean = k.mean != 0;
  // the last stage that runs writes the result; a stage that does not run passes its input on
  const float* cur = d_in;
  float *const speckle_out = gap || mean ? d_speckle : d_out, *const gap_out = mean ? d_gap : d_out;
  if (speckle) {
    a.src = cur;
    a.out = speckle_out;
    a.counters = counters;
    a.rows = k.rows;
    a.cols = k.cols;
    a.tiles_x = tiles_x;
    a.speckle_size = k.speckle_size;
    a.sim = k.sim;
    hipLaunchKernelGGL(k_dfilter_label, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_dfilter_unite, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_dfilter_roots, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_dfilter_mask, grid, block, 0, st, a);
    cur = a.out;
  }
  stats.o_speckle = speckle ? offset_of(speckle_out) : 0;
  stats.speckle_resident = speckle;
  if (gap) {
    g.in = cur;
    g.out = d_gap_rows;
    g.filled = &counters->filled_rows;
    g.n_lines = k.rows;
    g.len = k.cols;
    g.line_stride = k.cols;
    g.elem_stride = 1;
    g.width = k.gap_width;
    hipLaunchKernelGGL(k_dfilter_gap, dim3((unsigned)g.n_lines), dim3(64), 0, st, g);
    g.in = g.out;
    g.out = gap_out;
    g.filled = &counters->filled_cols;
    g.n_lines = k.cols;
    g.len = k.rows;
    g.line_stride = 1;
    g.elem_stride = k.cols;
    hipLaunchKernelGGL(k_dfilter_gap, dim3((unsigned)g.n_lines), dim3(64), 0, st, g);
    cur = g.out;
  }
  stats.o_gap = gap ? offset_of(gap_out) : stats.o_speckle;
  stats.gap_resident = speckle || gap;
  if (mean) {
    DFilterMeanArgs m;
    m.in = cur;
    m.tmp = nullptr;
    m.out = d_tmp;
    m.rows = k.rows;
    m.cols = k.cols;
    m.tiles_x = tiles_x;
    hipLaunchKernelGGL(k_dfilter_mean_h, grid, block, 0, st, m);
    m.tmp = m.out;
    m.out = d_out;
    hipLaunchKernelGGL(k_dfilter_mean_v, grid, block, 0, st, m);
    cur = m.out;
  }
  stats.o_tmp = offset_of(d_tmp);
  stats.tmp_resident = mean;
  if (cur != d_out) HIP_TRY(ctx, hipMemcpyAsync(d_out, cur, map, hipMemcpyDeviceToDevice, st));  // (every stage off)
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h_down, d_out, map + sizeof(DFilterCounters), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memcpy(out, h_down, map);  // (nothing is written unless the call succeeds)
  DFilterCounters c;
  std::memcpy(&c, h_down + map, sizeof c);
  stats.segments = c.segments;
  stats.removed = c.removed;
  stats.filled = (unsigned long long)c.filled_rows + c.filled_cols;
  stats.tile_w = DFILTER_TILE_W;
  stats.tile_h = DFILTER_TILE_H;
  return CVO_OK;
}

// the filter of a checked map, by the context's route; the caller holds upload_mutex.  in: on the host; d_in: the same map
// resident, or nullptr
int dfilter_run(cvo_ctx* ctx, const DFilterConst& k, const float* in, const float* d_in, float* out) {
  DFilterStatsAcc stats(k);
  const size_t np = (size_t)k.rows * k.cols;
  if (!ctx || dfilter_on_host(ctx, (long long)np)) {
    std::vector<float> d(in, in + np);
    dfilter_cpu(k, d.data(), stats);
    std::memcpy(out, d.data(), sizeof(float) * np);
  } else {
    stats.on_device = 1;
    const int rc = dfilter_device(ctx, k, in, d_in, out, stats);
    if (rc != CVO_OK) return rc;
  }
  if (ctx) ctx->dfilter_last = stats;
  return CVO_OK;
}

int dfilter_entry(cvo_ctx* ctx, const char* who, int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, float* out) {
  std::string msg;
  const int rc = dfilter_validate(rows, cols, in, cfg, out, &msg);
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] { return dfilter_run(ctx, dfilter_const(rows, cols, *cfg), in, nullptr, out); });
}

// what the two _filtered entry points refuse of the filter's configuration before the matcher runs: the matcher's map is
// finite and its only negative value is -10, which has to lie below -speckle_sim_threshold
int dfilter_validate_for_matcher(int rows, int cols, const cvo_dfilter_config_t* cfg, std::string* msg) {
  const int rc = dfilter_validate_config(rows, cols, cfg, msg);
  if (rc != CVO_OK) return rc;
  if (!(SGM_INVALID < -cfg->speckle_sim_threshold)) return *msg = "the matcher's invalid marker -10 is not below -speckle_sim_threshold", CVO_E_INVALID;
  return CVO_OK;
}

}  // namespace

extern "C" {

void cvo_dfilter_config_default(cvo_dfilter_config_t* cfg) {
  if (!cfg) return;
  cfg->speckle_sim_threshold = 1.f;
  cfg->speckle_size = 200;
  cfg->ipol_gap_width = 3;
  cfg->adaptive_mean = 1;
}

int cvo_disparity_filter_host(int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, float* out) {
  return dfilter_entry(nullptr, "cvo_disparity_filter_host", rows, cols, in, cfg, out);
}

int cvo_disparity_filter(cvo_ctx* ctx, int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, float* out) {
  if (!ctx) return CVO_E_INVALID;
  return dfilter_entry(ctx, "cvo_disparity_filter", rows, cols, in, cfg, out);
}

int cvo_debug_dfilter_stats(cvo_ctx* ctx, int* on_device, int* rows, int* cols, int* tile_w, int* tile_h, unsigned long long* counts,
                            float* after_speckle, float* after_gap, float* mean_tmp) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const DFilterStatsAcc& s = ctx->dfilter_last;
  if (on_device) *on_device = s.on_device;
  if (rows) *rows = s.rows;
  if (cols) *cols = s.cols;
  if (tile_w) *tile_w = s.tile_w;
  if (tile_h) *tile_h = s.tile_h;
  if (counts) counts[0] = s.segments, counts[1] = s.removed, counts[2] = s.filled;
  if (!after_speckle && !after_gap && !mean_tmp) return CVO_OK;
  if (!s.on_device || !ctx->dfilter_scratch.p) return fail(ctx, CVO_E_INVALID, "cvo_debug_dfilter_stats: the context's last disparity filter did not run on the device");
  if ((after_speckle && !s.speckle_resident) || (after_gap && !s.gap_resident) || (mean_tmp && !s.tmp_resident))
    return fail(ctx, CVO_E_INVALID, "cvo_debug_dfilter_stats: a stage that did not run left no map");
  const size_t map = 4 * (size_t)s.rows * s.cols;
  const char* base = ctx->dfilter_scratch.p;
  if (after_speckle) HIP_TRY(ctx, hipMemcpyAsync(after_speckle, base + s.o_speckle, map, hipMemcpyDeviceToHost, ctx->upload_stream));
  if (after_gap) HIP_TRY(ctx, hipMemcpyAsync(after_gap, base + s.o_gap, map, hipMemcpyDeviceToHost, ctx->upload_stream));
  if (mean_tmp) HIP_TRY(ctx, hipMemcpyAsync(mean_tmp, base + s.o_tmp, map, hipMemcpyDeviceToHost, ctx->upload_stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  return CVO_OK;
}

}  // extern "C"
