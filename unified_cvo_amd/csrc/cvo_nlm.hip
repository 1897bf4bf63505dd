// cvo_nlm.hip -- non-local-means denoising, RawImage's first statement (RawImage.cpp:21-24): cvo_nlm_weights,
// cvo_nlm_denoise(_host), cvo_nlm_denoise_lab(_host) and cvo_debug_nlm_stats.  OpenCV's FastNlMeansDenoisingInvoker for
// 8-bit images with the squared distance, restated from its published algorithm; tests/np_nlm.py states what is computed.
// The weight table is built in ONE place (nlm_table: double, the host's exp) for both routes.  The CPU twin (nlm_cpu) keeps
// OpenCV's organisation per offset - a plane of squared differences, column sums, a sliding row window - and shares no code
// with the kernel (cvo_k_nlm.h).  A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// pixels; below, the CPU twin is the default route (profiles/nlm/crossover.txt)
constexpr int NLM_HOST_BELOW = 256;

bool nlm_on_host(const cvo_ctx* ctx, long long np) { return route_on_host(ctx->opt.nlm_host, np, NLM_HOST_BELOW); }

struct NlmTable {
  int th = 0, sh = 0, mult = 0, shift = 0, n_table = 0, n_nonzero = 0;
  std::vector<int> weight;  // the nonzero leading part
};

int nlm_validate_config(const cvo_nlm_config_t* cfg, std::string* msg) {
  if (!cfg) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (!std::isfinite(cfg->h) || !(cfg->h > 0.f)) return *msg = "h must be finite and > 0", CVO_E_INVALID;
  if (cfg->template_window < 1 || cfg->search_window < 1) return *msg = "window sizes start at 1", CVO_E_INVALID;
  if (cfg->template_window / 2 > NLM_MAX_TH || cfg->search_window / 2 > NLM_MAX_SH)
    return *msg = "template windows above 7 and search windows above 21 are not built", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

int nlm_validate_image(int rows, int cols, int channels, const void* src, const void* dst, std::string* msg) {
  if (!src || !dst) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (rows < 1 || cols < 1) return *msg = "rows and cols start at 1", CVO_E_INVALID;
  if (channels < 1 || channels > 3) return *msg = "channels must be 1, 2 or 3", CVO_E_INVALID;
  if ((long long)rows * cols > (1ll << 24)) return *msg = "more than 2^24 pixels", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

// The constants and the table of FastNlMeansDenoisingInvoker<uchar, int, unsigned, DistSquared>: hh in float as
// OpenCV's `h * h * channels`, the exponent and the product in double, lrint to even, entries under 0.001 mult cut to 0.
// The weights fall with d, so the nonzero entries are a leading run; only that run is kept.
void nlm_table(float h, int template_window, int search_window, int channels, NlmTable& t) {
  t.th = template_window / 2;
  t.sh = search_window / 2;
  const int tw = 2 * t.th + 1, sw = 2 * t.sh + 1;
  t.mult = INT_MAX / (sw * sw * 255);
  t.shift = 0;
  while ((1 << t.shift) < tw * tw) t.shift++;
  const double m = (double)(1 << t.shift) / (double)(tw * tw);
  t.n_table = (int)(255.0 * 255.0 * channels / m + 1.0);
  const float hhf = h * h * (float)channels;
  const double hh = (double)hhf, cut = 0.001 * t.mult;
  t.weight.clear();
  for (int d = 0; d < t.n_table; d++) {
    const double w = std::exp(-((double)d * m) / hh);
    const long v = std::lrint((double)t.mult * w);
    if ((double)v < cut) break;
    t.weight.push_back((int)v);
  }
  t.n_nonzero = (int)t.weight.size();
}

int nlm_reflect_host(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

// ---- CPU twin: one thread.  src / dst: channel c of pixel p at [p * stride + c]; dst may be src (the extended copy is made first) ----
void nlm_cpu(int rows, int cols, int C, const unsigned char* src, int src_stride, unsigned char* dst, int dst_stride, const NlmTable& t) {
  const int th = t.th, sh = t.sh, b = th + sh, tw = 2 * th + 1;
  const int ew = cols + 2 * b, eh = rows + 2 * b;   // the extended image
  const int pw = cols + 2 * th, ph = rows + 2 * th;  // the plane of squared differences: every pixel a patch touches
  std::vector<int> rx((size_t)ew), ry((size_t)eh);
  for (int x = 0; x < ew; x++) rx[(size_t)x] = nlm_reflect_host(x - b, cols);
  for (int y = 0; y < eh; y++) ry[(size_t)y] = nlm_reflect_host(y - b, rows);
  std::vector<unsigned char> ext((size_t)ew * eh * C);
  for (int y = 0; y < eh; y++)
    for (int x = 0; x < ew; x++)
      for (int c = 0; c < C; c++)
        ext[((size_t)y * ew + x) * C + c] = src[((size_t)ry[(size_t)y] * cols + rx[(size_t)x]) * src_stride + c];
  const size_t np = (size_t)rows * cols;
  std::vector<unsigned> est(np * C, 0u), ws(np, 0u);
  std::vector<int> d2((size_t)pw * ph), colsum((size_t)pw);
  const int n_nonzero = t.n_nonzero;
  const int* weight = t.weight.data();
  for (int dy = -sh; dy <= sh; dy++)
    for (int dx = -sh; dx <= sh; dx++) {
      for (int y = 0; y < ph; y++) {
        const unsigned char* pa = &ext[((size_t)(y + sh) * ew + sh) * C];
        const unsigned char* pb = &ext[((size_t)(y + sh + dy) * ew + sh + dx) * C];
        int* o = &d2[(size_t)y * pw];
        for (int x = 0; x < pw; x++) {
          int s = 0;
          for (int c = 0; c < C; c++) {
            const int d = (int)pa[x * C + c] - (int)pb[x * C + c];
            s += d * d;
          }
          o[x] = s;
        }
      }
      // column sums over the template's rows, moved down one row at a time; a sliding window along each row
      std::fill(colsum.begin(), colsum.end(), 0);
      for (int y = 0; y < tw - 1; y++)
        for (int x = 0; x < pw; x++) colsum[(size_t)x] += d2[(size_t)y * pw + x];
      for (int i = 0; i < rows; i++) {
        const int* add = &d2[(size_t)(i + tw - 1) * pw];
        for (int x = 0; x < pw; x++) colsum[(size_t)x] += add[x];
        int dist = 0;
        for (int x = 0; x < tw - 1; x++) dist += colsum[(size_t)x];
        const unsigned char* ctr = &ext[((size_t)(i + b + dy) * ew + b + dx) * C];
        for (int j = 0; j < cols; j++) {
          dist += colsum[(size_t)(j + tw - 1)];
          const int idx = dist >> t.shift;
          if (idx < n_nonzero) {
            const unsigned w = (unsigned)weight[idx];
            const size_t p = (size_t)i * cols + j;
            ws[p] += w;
            for (int c = 0; c < C; c++) est[p * C + c] += w * (unsigned)ctr[j * C + c];
          }
          dist -= colsum[(size_t)j];
        }
        const int* sub = &d2[(size_t)i * pw];
        for (int x = 0; x < pw; x++) colsum[(size_t)x] -= sub[x];
      }
    }
  for (size_t p = 0; p < np; p++)
    for (int c = 0; c < C; c++) {
      const unsigned v = (est[p * C + c] + ws[p] / 2u) / ws[p];
      dst[p * dst_stride + c] = (unsigned char)(v > 255u ? 255u : v);
    }
}

// ---- device route ----
// one plane group of the image in the scratch region: C channels starting at channel `first` of `stride`-channel pixels
struct NlmPass {
  int C, first;
  const NlmTable* table;
};

template <int C>
void nlm_launch(hipStream_t st, int th, dim3 grid, size_t lds, const NlmArgs& a) {
  switch (th) {
    case 0: hipLaunchKernelGGL((k_nlm<C, 0>), grid, dim3(NLM_THREADS), lds, st, a); break;
    case 1: hipLaunchKernelGGL((k_nlm<C, 1>), grid, dim3(NLM_THREADS), lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_nlm<C, 2>), grid, dim3(NLM_THREADS), lds, st, a); break;
    default: hipLaunchKernelGGL((k_nlm<C, 3>), grid, dim3(NLM_THREADS), lds, st, a); break;
  }
}

// One upload, the passes' launches, one download, one synchronisation; on upload_stream under upload_mutex.
int nlm_device(cvo_ctx* ctx, int rows, int cols, int stride, const unsigned char* src, unsigned char* dst, const NlmPass* pass, int n_pass,
               NlmStatsAcc& stats) {
  hipStream_t st = ctx->upload_stream;
  const size_t bytes = (size_t)rows * cols * stride;
  unsigned char *d_src = nullptr, *d_dst = nullptr;
  int* d_w[2] = {nullptr, nullptr};
  const int rc = ctx->nlm_scratch.lay_out(ctx, "denoising scratch", [&](ScratchLayout& l) {
    l.take(d_src, bytes);
    l.take(d_dst, bytes);
    for (int i = 0; i < n_pass; i++) l.take(d_w[i], (size_t)pass[i].table->n_nonzero);
  });
  if (rc != CVO_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_src, src, bytes, hipMemcpyHostToDevice, st));
  for (int i = 0; i < n_pass; i++) {
    const NlmTable& t = *pass[i].table;
    HIP_TRY(ctx, hipMemcpyAsync(d_w[i], t.weight.data(), sizeof(int) * (size_t)t.n_nonzero, hipMemcpyHostToDevice, st));
    NlmArgs a;
    a.src = d_src + pass[i].first;
    a.dst = d_dst + pass[i].first;
    a.src_stride = a.dst_stride = stride;
    a.rows = rows;
    a.cols = cols;
    a.sh = t.sh;
    a.weight = d_w[i];
    a.n_nonzero = t.n_nonzero;
    a.n_lds = std::min(t.n_nonzero, NLM_TABLE_LDS);
    a.shift = t.shift;
    const int W = nlm_tile_w(t.th);
    a.tiles_x = (cols + W - 1) / W;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)((rows + NLM_TILE_H - 1) / NLM_TILE_H));  // (at most 2^24 pixels: under 2^24 tiles)
    const size_t lds = sizeof(int) * (size_t)a.n_lds;
    if (pass[i].C == 1)
      nlm_launch<1>(st, t.th, grid, lds, a);
    else if (pass[i].C == 2)
      nlm_launch<2>(st, t.th, grid, lds, a);
    else
      nlm_launch<3>(st, t.th, grid, lds, a);
    HIP_TRY(ctx, hipGetLastError());
    stats.tile_w = W;
    stats.tile_h = NLM_TILE_H;
    stats.table_in_lds = stats.table_in_lds && a.n_lds == t.n_nonzero;
  }
  std::vector<unsigned char> out(bytes);  // (dst may be src, and nothing is written unless the call succeeds)
  HIP_TRY(ctx, hipMemcpyAsync(out.data(), d_dst, bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memcpy(dst, out.data(), bytes);
  return CVO_OK;
}

// the body of the four entry points: ctx == nullptr is the twin without a context
int nlm_run(cvo_ctx* ctx, int rows, int cols, int stride, const unsigned char* src, unsigned char* dst, const NlmPass* pass, int n_pass) {
  NlmStatsAcc stats;
  const NlmTable& last = *pass[n_pass - 1].table;
  stats.mult = last.mult;
  stats.shift = last.shift;
  stats.n_nonzero = last.n_nonzero;
  if (!ctx || nlm_on_host(ctx, (long long)rows * cols)) {
    std::vector<unsigned char> out((size_t)rows * cols * stride);
    for (int i = 0; i < n_pass; i++)
      nlm_cpu(rows, cols, pass[i].C, src + pass[i].first, stride, out.data() + pass[i].first, stride, *pass[i].table);
    std::memcpy(dst, out.data(), out.size());
  } else {
    stats.on_device = 1;
    stats.table_in_lds = 1;
    const int rc = nlm_device(ctx, rows, cols, stride, src, dst, pass, n_pass, stats);
    if (rc != CVO_OK) return rc;
  }
  if (ctx) ctx->nlm_last = stats;
  return CVO_OK;
}

int nlm_denoise(cvo_ctx* ctx, const char* who, int rows, int cols, int channels, const uint8_t* src, const cvo_nlm_config_t* cfg, uint8_t* dst) {
  std::string msg;
  std::string msg_cfg;
  int rc = nlm_validate_image(rows, cols, channels, src, dst, &msg);
  const int rc_cfg = nlm_validate_config(cfg, &msg_cfg);
  if (rc_cfg == CVO_E_INVALID || rc == CVO_OK) rc = rc_cfg, msg = msg_cfg;  // (an invalid argument outranks an unsupported one)
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] {
    NlmTable t;
    nlm_table(cfg->h, cfg->template_window, cfg->search_window, channels, t);
    const NlmPass pass{channels, 0, &t};
    return nlm_run(ctx, rows, cols, channels, src, dst, &pass, 1);
  });
}

int nlm_denoise_lab(cvo_ctx* ctx, const char* who, int rows, int cols, const uint8_t* lab, const cvo_nlm_config_t* cfg, float h_color, uint8_t* dst) {
  std::string msg;
  std::string msg_cfg;
  int rc = nlm_validate_image(rows, cols, 3, lab, dst, &msg);
  int rc_cfg = nlm_validate_config(cfg, &msg_cfg);
  if (rc_cfg != CVO_E_INVALID && (!std::isfinite(h_color) || !(h_color > 0.f))) {
    rc_cfg = CVO_E_INVALID;
    msg_cfg = "h_color must be finite and > 0";
  }
  if (rc_cfg == CVO_E_INVALID || rc == CVO_OK) rc = rc_cfg, msg = msg_cfg;
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] {
    NlmTable tl, tab;
    nlm_table(cfg->h, cfg->template_window, cfg->search_window, 1, tl);
    nlm_table(h_color, cfg->template_window, cfg->search_window, 2, tab);
    const NlmPass pass[2] = {{1, 0, &tl}, {2, 1, &tab}};
    return nlm_run(ctx, rows, cols, 3, lab, dst, pass, 2);
  });
}

}  // namespace

extern "C" {

void cvo_nlm_config_default(cvo_nlm_config_t* cfg) {
  if (!cfg) return;
  cfg->h = 10.f;
  cfg->template_window = 7;
  cfg->search_window = 21;
}

int cvo_nlm_weights(const cvo_nlm_config_t* cfg, int channels, int* weight, int capacity, int* n_table, int* n_nonzero, int* mult, int* shift) {
  std::string msg;
  const int rc = nlm_validate_config(cfg, &msg);
  if (rc != CVO_OK) return rc;
  if (channels < 1 || channels > 3 || (weight && capacity < 0)) return CVO_E_INVALID;
  return frontend_call(nullptr, "", [&] {
    NlmTable t;
    nlm_table(cfg->h, cfg->template_window, cfg->search_window, channels, t);
    if (weight)
      for (int i = 0; i < capacity && i < t.n_table; i++) weight[i] = i < t.n_nonzero ? t.weight[(size_t)i] : 0;
    if (n_table) *n_table = t.n_table;
    if (n_nonzero) *n_nonzero = t.n_nonzero;
    if (mult) *mult = t.mult;
    if (shift) *shift = t.shift;
    return CVO_OK;
  });
}

int cvo_nlm_denoise_host(int rows, int cols, int channels, const uint8_t* src, const cvo_nlm_config_t* cfg, uint8_t* dst) {
  return nlm_denoise(nullptr, "cvo_nlm_denoise_host", rows, cols, channels, src, cfg, dst);
}

int cvo_nlm_denoise(cvo_ctx* ctx, int rows, int cols, int channels, const uint8_t* src, const cvo_nlm_config_t* cfg, uint8_t* dst) {
  if (!ctx) return CVO_E_INVALID;
  return nlm_denoise(ctx, "cvo_nlm_denoise", rows, cols, channels, src, cfg, dst);
}

int cvo_nlm_denoise_lab_host(int rows, int cols, const uint8_t* lab, const cvo_nlm_config_t* cfg, float h_color, uint8_t* dst) {
  return nlm_denoise_lab(nullptr, "cvo_nlm_denoise_lab_host", rows, cols, lab, cfg, h_color, dst);
}

int cvo_nlm_denoise_lab(cvo_ctx* ctx, int rows, int cols, const uint8_t* lab, const cvo_nlm_config_t* cfg, float h_color, uint8_t* dst) {
  if (!ctx) return CVO_E_INVALID;
  return nlm_denoise_lab(ctx, "cvo_nlm_denoise_lab", rows, cols, lab, cfg, h_color, dst);
}

int cvo_debug_nlm_stats(cvo_ctx* ctx, int* on_device, int* mult, int* shift, int* n_nonzero, int* tile_w, int* tile_h, int* table_in_lds) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const NlmStatsAcc& s = ctx->nlm_last;
  if (on_device) *on_device = s.on_device;
  if (mult) *mult = s.mult;
  if (shift) *shift = s.shift;
  if (n_nonzero) *n_nonzero = s.n_nonzero;
  if (tile_w) *tile_w = s.tile_w;
  if (tile_h) *tile_h = s.tile_h;
  if (table_in_lds) *table_in_lds = s.table_in_lds;
  return CVO_OK;
}

}  // extern "C"
