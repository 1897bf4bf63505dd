// cvo_sgm.hip -- the stereo matcher (left + right gray planes to the float left disparity the stereo front end reads, invalid
// = -10): its refusals, its two routes, cvo_debug_sgm_stats and cvo_debug_sgm_readback; its entry points, cvo_stereo_disparity
// (_host), are in cvo_stereo_pair.hip with the chains that run it.  Semi-global matching over a 9 x 7 census cost - the
// project's OWN matcher, not upstream's libelas (StaticStereo::disparity) and not any other SGM implementation; tests/np_sgm.py
// states what is computed.  The CPU twin (sgm_cpu) walks the same lines (sgm_line) with the same arithmetic (cvo_sgm_math.h)
// as the kernels of cvo_k_sgm.h, one after the other.  A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
namespace {

// pixels; below, the CPU twin is the default route (profiles/sgm/crossover.txt)
constexpr int SGM_HOST_BELOW = 128;
constexpr long long SGM_MAX_PIXELS = 1ll << 24, SGM_MAX_WORKSPACE = 1ll << 31;

bool sgm_on_host(const cvo_ctx* ctx, long long np) { return route_on_host(ctx->opt.sgm_host, np, SGM_HOST_BELOW); }

// The matcher's refusals in two parts (a chain that makes the map itself has no pointer to it): the planes and the map ...
int sgm_validate_pointers(std::initializer_list<const void*> required, std::string* msg) {
  for (const void* p : required)
    if (!p) return *msg = "a required pointer is missing", CVO_E_INVALID;
  return CVO_OK;
}

// ... and the configuration with the sizes it admits
int sgm_validate_config(int rows, int cols, const cvo_sgm_config_t* cfg, std::string* msg) {
  if (!cfg) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (rows < 1 || cols < 1) return *msg = "rows and cols start at 1", CVO_E_INVALID;
  if (cfg->max_disparity != 64 && cfg->max_disparity != 128 && cfg->max_disparity != 256)
    return *msg = "max_disparity must be 64, 128 or 256, got " + std::to_string(cfg->max_disparity), CVO_E_INVALID;
  if (cfg->p1 < 0 || cfg->p1 > cfg->p2 || cfg->p2 > SGM_MAX_P2)
    return *msg = "0 <= p1 <= p2 <= 193 is required, got " + std::to_string(cfg->p1) + ", " + std::to_string(cfg->p2), CVO_E_INVALID;
  if (cfg->uniqueness < 0 || cfg->uniqueness > 99) return *msg = "uniqueness must be 0 .. 99, got " + std::to_string(cfg->uniqueness), CVO_E_INVALID;
  if (cfg->paths != 4 && cfg->paths != 8) return *msg = "paths must be 4 or 8, got " + std::to_string(cfg->paths), CVO_E_INVALID;
  if ((long long)rows * cols > SGM_MAX_PIXELS) return *msg = "more than 2^24 pixels", CVO_E_UNSUPPORTED;
  if ((long long)rows * cols * cfg->max_disparity * 2 > SGM_MAX_WORKSPACE)
    return *msg = "the sums of rows x cols x max_disparity hypotheses take more than 2 GiB", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

SgmConst sgm_const(int rows, int cols, const cvo_sgm_config_t& c) {
  return SgmConst{rows, cols, c.max_disparity, c.p1, c.p2, c.uniqueness, c.lr_max_diff, c.paths};
}

// ---- CPU twin: one thread ----
void sgm_census_cpu(int rows, int cols, const unsigned char* img, unsigned long long* out) {
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const int centre = img[(size_t)y * cols + x];
      unsigned long long word = 0;
      for (int dy = -SGM_HALO_Y; dy <= SGM_HALO_Y; dy++) {
        const unsigned char* row = img + (size_t)std::min(std::max(y + dy, 0), rows - 1) * cols;
        for (int dx = -SGM_HALO_X; dx <= SGM_HALO_X; dx++)
          if (dy != 0 || dx != 0) word = (word << 1) | (unsigned long long)((int)row[std::min(std::max(x + dx, 0), cols - 1)] < centre ? 1 : 0);
      }
      out[(size_t)y * cols + x] = word;
    }
}

void sgm_paths_cpu(const SgmConst& k, const unsigned long long* cl, const unsigned long long* cr, unsigned short* S) {
  const int D = k.D;
  std::vector<int> c((size_t)D), L((size_t)D), next((size_t)D);
  for (int dir = 0; dir < k.paths; dir++) {
    const int dv = sgm_dv(dir), du = sgm_du(dir), n_lines = sgm_line_count(dir, k.rows, k.cols);
    for (int line = 0; line < n_lines; line++) {
      int v, u, len, m = 0;
      sgm_line(dir, line, k.rows, k.cols, &v, &u, &len);
      for (int s = 0; s < len; s++, v += dv, u += du) {
        const size_t p = (size_t)v * k.cols + u;
        const unsigned long long word = cl[p];
        const int reach = std::min(D, u + 1);
        for (int d = 0; d < reach; d++) c[(size_t)d] = sgm_cost(word, cr[p - (size_t)d], true);
        for (int d = reach; d < D; d++) c[(size_t)d] = sgm_cost(word, 0, false);
        if (s == 0) {
          L = c;
        } else {
          for (int d = 0; d < D; d++)
            next[(size_t)d] = sgm_step(c[(size_t)d], L[(size_t)d], d > 0 ? L[(size_t)d - 1] : 0, d > 0, d < D - 1 ? L[(size_t)d + 1] : 0, d < D - 1, m, k.p1, k.p2);
          L.swap(next);
        }
        m = L[0];
        for (int d = 1; d < D; d++) m = std::min(m, L[(size_t)d]);
        unsigned short* sp = S + p * (size_t)D;
        for (int d = 0; d < D; d++) sp[d] = (unsigned short)((dir ? (int)sp[d] : 0) + L[(size_t)d]);
      }
    }
  }
}

void sgm_select_cpu(const SgmConst& k, const unsigned short* S, float* out) {
  const int D = k.D, cols = k.cols;
  std::vector<int> right;  // dR of a row
  for (int v = 0; v < k.rows; v++) {
    const unsigned short* row = S + (size_t)v * cols * D;
    if (k.lr_max_diff >= 0) {
      right.assign((size_t)cols, 0);
      for (int x = 0; x < cols; x++) {
        unsigned best = SGM_NO_COST;
        for (int d = 0; d < D && x + d < cols; d++) {
          const unsigned s = row[(size_t)(x + d) * D + d];
          if (s < best) best = s, right[(size_t)x] = d;
        }
      }
    }
    for (int u = 0; u < cols; u++) {
      const unsigned short* sp = row + (size_t)u * D;
      int d = 0;
      for (int i = 1; i < D; i++)
        if (sp[i] < sp[d]) d = i;
      const int s1 = sp[d];
      int s2 = (int)SGM_NO_COST;
      for (int i = 0; i < D; i++)
        if ((i < d - 1 || i > d + 1) && (int)sp[i] < s2) s2 = sp[i];
      bool valid = !sgm_ambiguous(s1, s2, k.uniqueness);
      const float disp = sgm_subpixel(d, D, d > 0 ? (int)sp[d - 1] : 0, s1, d < D - 1 ? (int)sp[d + 1] : 0);
      if (k.lr_max_diff >= 0 && (u - d < 0 || sgm_lr_differs(d, right[(size_t)(u - d)], k.lr_max_diff))) valid = false;
      out[(size_t)v * cols + u] = valid ? disp : SGM_INVALID;
    }
  }
}

void sgm_cpu(const SgmConst& k, const unsigned char* left, const unsigned char* right, float* out) {
  const size_t np = (size_t)k.rows * k.cols;
  std::vector<unsigned long long> cl(np), cr(np);
  std::vector<unsigned short> S(np * (size_t)k.D);
  sgm_census_cpu(k.rows, k.cols, left, cl.data());
  sgm_census_cpu(k.rows, k.cols, right, cr.data());
  sgm_paths_cpu(k, cl.data(), cr.data(), S.data());
  sgm_select_cpu(k, S.data(), out);
}

// ---- device route ----
template <int D, int DIR>
void sgm_launch_dir(hipStream_t st, const SgmPathArgs& a) {
  hipLaunchKernelGGL((k_sgm_path<D, DIR>), dim3((unsigned)a.n_lines), dim3(64), 0, st, a);
}

template <int D>
void sgm_launch_paths(hipStream_t st, SgmPathArgs a, int paths, int* lines) {
  for (int dir = 0; dir < paths; dir++) {
    a.n_lines = lines[dir] = sgm_line_count(dir, a.rows, a.cols);
    a.accumulate = dir > 0;
    switch (dir) {
      case 0: sgm_launch_dir<D, 0>(st, a); break;
      case 1: sgm_launch_dir<D, 1>(st, a); break;
      case 2: sgm_launch_dir<D, 2>(st, a); break;
      case 3: sgm_launch_dir<D, 3>(st, a); break;
      case 4: sgm_launch_dir<D, 4>(st, a); break;
      case 5: sgm_launch_dir<D, 5>(st, a); break;
      case 6: sgm_launch_dir<D, 6>(st, a); break;
      default: sgm_launch_dir<D, 7>(st, a); break;
    }
  }
}

template <int D>
void sgm_launch_select(hipStream_t st, const SgmSelectArgs& a) {
  const unsigned np = (unsigned)a.rows * (unsigned)a.cols;
  hipLaunchKernelGGL((k_sgm_select<D>), dim3((np + SGM_SELECT_WAVES - 1) / SGM_SELECT_WAVES), dim3(64 * SGM_SELECT_WAVES), 0, st, a);
}

// One upload, census, the directions' launches, the selection, one download, one synchronisation; on upload_stream under
// upload_mutex.  The census planes and S stay in the region for cvo_debug_sgm_readback until the next call.  out == nullptr:
// enqueued only, neither downloaded nor waited for - the map is at stats.o_disparity for the filter of cvo_dfilter.hip.
int sgm_device(cvo_ctx* ctx, const SgmConst& k, const unsigned char* left, const unsigned char* right, float* out, SgmStatsAcc& stats) {
  hipStream_t st = ctx->upload_stream;
  const size_t np = (size_t)k.rows * k.cols;
  SgmCensusArgs c;
  SgmPathArgs a;
  float* d_disp = nullptr;
  const int rc = ctx->sgm_scratch.lay_out(ctx, "stereo matcher scratch", [&](ScratchLayout& l) {  // (stats.o_*: where the read-back finds them)
    l.take(c.left, np);
    l.take(c.right, np);
    stats.o_census_left = l.off;
    l.take(c.census_left, np);
    stats.o_census_right = l.off;
    l.take(c.census_right, np);
    stats.o_S = l.off;
    l.take(a.S, np * (size_t)k.D);
    stats.o_disparity = l.off;
    l.take(d_disp, np);
  });
  if (rc != CVO_OK) return rc;
  HIP_TRY(ctx, hipMemcpyAsync((void*)c.left, left, np, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync((void*)c.right, right, np, hipMemcpyHostToDevice, st));
  c.rows = k.rows;
  c.cols = k.cols;
  c.tiles_x = (k.cols + SGM_TILE_W - 1) / SGM_TILE_W;
  const unsigned tiles = (unsigned)c.tiles_x * (unsigned)((k.rows + SGM_TILE_H - 1) / SGM_TILE_H);  // (at most 2^24 pixels: under 2^24 tiles)
  hipLaunchKernelGGL(k_sgm_census, dim3(tiles, 2), dim3(SGM_CENSUS_THREADS), 0, st, c);
  a.census_left = c.census_left;
  a.census_right = c.census_right;
  a.rows = k.rows;
  a.cols = k.cols;
  a.p1 = k.p1;
  a.p2 = k.p2;
  a.n_lines = 0;
  a.accumulate = 0;
  const SgmSelectArgs s{a.S, d_disp, k.rows, k.cols, k.uniqueness, k.lr_max_diff};
  if (k.D == 64) {
    sgm_launch_paths<64>(st, a, k.paths, stats.lines);
    sgm_launch_select<64>(st, s);
  } else if (k.D == 128) {
    sgm_launch_paths<128>(st, a, k.paths, stats.lines);
    sgm_launch_select<128>(st, s);
  } else {
    sgm_launch_paths<256>(st, a, k.paths, stats.lines);
    sgm_launch_select<256>(st, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (out) {
    std::vector<float> host(np);  // (nothing is written unless the call succeeds)
    HIP_TRY(ctx, hipMemcpyAsync(host.data(), d_disp, 4 * np, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(out, host.data(), 4 * np);
  }
  stats.tile_w = SGM_TILE_W;
  stats.tile_h = SGM_TILE_H;
  return CVO_OK;
}

}  // namespace

extern "C" {

void cvo_sgm_config_default(cvo_sgm_config_t* cfg) {
  if (!cfg) return;
  cfg->max_disparity = 128;
  cfg->p1 = 10;
  cfg->p2 = 120;
  cfg->uniqueness = 5;
  cfg->lr_max_diff = 1;
  cfg->paths = 8;
}

int cvo_debug_sgm_stats(cvo_ctx* ctx, int* on_device, int* max_disparity, int* paths, int* lines, int* rows, int* cols, int* tile_w, int* tile_h) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const SgmStatsAcc& s = ctx->sgm_last;
  if (on_device) *on_device = s.on_device;
  if (max_disparity) *max_disparity = s.D;
  if (paths) *paths = s.paths;
  if (lines) std::memcpy(lines, s.lines, sizeof s.lines);
  if (rows) *rows = s.rows;
  if (cols) *cols = s.cols;
  if (tile_w) *tile_w = s.tile_w;
  if (tile_h) *tile_h = s.tile_h;
  return CVO_OK;
}

int cvo_debug_sgm_readback(cvo_ctx* ctx, unsigned long long* census_left, unsigned long long* census_right, unsigned short* S) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  const SgmStatsAcc& s = ctx->sgm_last;
  if (!s.on_device || !ctx->sgm_scratch.p) return fail(ctx, CVO_E_INVALID, "cvo_debug_sgm_readback: the context's last cvo_stereo_disparity did not run on the device");
  const size_t np = (size_t)s.rows * s.cols;
  const char* base = ctx->sgm_scratch.p;
  if (census_left) HIP_TRY(ctx, hipMemcpyAsync(census_left, base + s.o_census_left, 8 * np, hipMemcpyDeviceToHost, ctx->upload_stream));
  if (census_right) HIP_TRY(ctx, hipMemcpyAsync(census_right, base + s.o_census_right, 8 * np, hipMemcpyDeviceToHost, ctx->upload_stream));
  if (S) HIP_TRY(ctx, hipMemcpyAsync(S, base + s.o_S, 2 * np * (size_t)s.D, hipMemcpyDeviceToHost, ctx->upload_stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  return CVO_OK;
}

}  // extern "C"
