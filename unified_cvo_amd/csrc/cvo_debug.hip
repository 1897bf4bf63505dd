// cvo_debug.hip -- test / profiling hooks of include/cvo_hip_debug.h: the device scalar maths on caller inputs, kernel replays and clocks, counters of the last call.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
extern "C" {

int cvo_debug_scalar_math(cvo_ctx* ctx, int op, int n, const double* in, double* out) {
  if (!ctx || !in || !out || n <= 0 || op < 0 || op > 13) return fail(ctx, CVO_E_INVALID, "cvo_debug_scalar_math: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n_in = op == 7 ? (size_t)n + 2 : 16 * (size_t)n, n_out = op == 7 ? (size_t)n : 16 * (size_t)n;
  DeviceRegion r_in, r_out, r_st;
  const char* who = "cvo_debug_scalar_math";
  int rc;
  if ((rc = r_in.reserve(ctx, sizeof(double) * n_in, who, nullptr)) != CVO_OK || (rc = r_out.reserve(ctx, sizeof(double) * n_out, who, nullptr)) != CVO_OK ||
      (rc = r_st.reserve(ctx, sizeof(PairState), who, nullptr)) != CVO_OK)
    return rc;
  double *d_in = r_in.as<double>(), *d_out = r_out.as<double>();
  PairState* d_st = r_st.as<PairState>();
  hipError_t e = hipMemcpyAsync(d_in, in, sizeof(double) * n_in, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, sizeof(double) * n_out, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_st, 0, sizeof(PairState), ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_scalar_math, dim3(op == 7 ? 1 : n), dim3(64), 0, ctx->stream, op, n, d_in, d_out, d_st);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(double) * n_out, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(ctx, CVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return CVO_OK;
}

// Every size the kernels index with is checked here: nothing the caller passes can make them leave the three arrays.
int cvo_debug_prim(cvo_ctx* ctx, int op, int n, int m, unsigned long long* k64, size_t n64, unsigned* a, size_t na, unsigned* b, size_t nb) {
  const char* who = "cvo_debug_prim";
  if (!ctx || n < 0 || m < 0 || n > (1 << 20) || m > (1 << 20) || (n64 && !k64) || (na && !a) || (nb && !b))
    return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  const size_t N = (size_t)n, M = (size_t)m;
  bool ok = false;
  int threads = 256, lanes = n;
  switch (op) {
    case PRIM_SCAN: ok = n <= COMPACT_MAX_ELEMENTS / COMPACT_THREADS && na >= N && nb >= 1; break;
    case PRIM_SORT: ok = n64 >= 2 * N && na >= 2 * N && nb >= 256 * ((N + SORT_THREADS - 1) / SORT_THREADS); break;
    case PRIM_WAVE_ALLOC: ok = na >= N && nb >= 1; break;
    case PRIM_INSERT: ok = m >= 2 && (m & (m - 1)) == 0 && 2 * N <= M && n64 >= N + M && na >= N && nb >= N + 1; break;
    case PRIM_UNION:
      ok = na >= 2 * M && nb >= N && n64 >= N;
      for (size_t e = 0; ok && e < 2 * M; e++) ok = a[e] < (unsigned)n;
      for (size_t c = 0; ok && c < N; c++) b[c] = (unsigned)c;  // every cell its own root
      lanes = m;
      break;
    case PRIM_RANK:
      ok = na >= N && nb >= (N + COMPACT_THREADS - 1) / COMPACT_THREADS && n64 >= N;
      threads = COMPACT_THREADS;
      break;
    default: break;
  }
  if (!ok) return fail(ctx, CVO_E_INVALID, std::string(who) + ": op " + std::to_string(op) + " with arrays too small for n, m, or a bad n, m");
  if (op == PRIM_INSERT) std::fill(k64 + N, k64 + N + M, TABLE_EMPTY);
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->upload_stream;
  unsigned long long* d64 = nullptr;
  unsigned *da = nullptr, *db = nullptr;
  DeviceRegion d;  // (of this call)
  const int rc = d.lay_out(ctx, who, [&](ScratchLayout& l) {
    l.take(d64, n64);
    l.take(da, na);
    l.take(db, nb);
  }, nullptr);
  if (rc != CVO_OK) return rc;
  void *host[3] = {k64, a, b}, *dev[3] = {d64, da, db};
  const size_t bytes[3] = {8 * n64, 4 * na, 4 * nb};
  hipError_t e = hipSuccess;
  for (int q = 0; q < 3 && e == hipSuccess; q++)
    if (bytes[q]) e = hipMemcpyAsync(dev[q], host[q], bytes[q], hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)std::max(1, (lanes + threads - 1) / threads));
    if (op == PRIM_SCAN) {
      hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(COMPACT_THREADS), 0, st, n, da, db);
    } else if (op == PRIM_SORT) {
      unsigned long long* const key[2] = {d64, d64 + N};
      unsigned* const val[2] = {da, da + N};
      sort_pairs_u64(ctx, (unsigned)n, key, val, db);
    } else {
      hipLaunchKernelGGL(k_prim, grid, dim3(threads), 0, st, op, n, m, d64, da, db);
      if (op == PRIM_UNION) hipLaunchKernelGGL(k_prim, dim3((unsigned)std::max(1, (n + 255) / 256)), dim3(256), 0, st, (int)PRIM_FIND, n, m, d64, da, db);
    }
    e = hipGetLastError();
  }
  for (int q = 0; q < 3 && e == hipSuccess; q++)
    if (bytes[q]) e = hipMemcpyAsync(host[q], dev[q], bytes[q], hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(ctx, CVO_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return CVO_OK;
}

int cvo_debug_cloud_order(const cvo_cloud* c, int* out) {
  if (!c || !out) return CVO_E_INVALID;
  for (int r = 0; r < c->n; r++) out[r] = c->h_order[r];
  return CVO_OK;
}

int cvo_debug_cloud_order_route(const cvo_cloud* c) { return c ? c->order_route : CVO_E_INVALID; }

int cvo_debug_order_route_rule(int n, int finite, const char* order_value, int no_sort) {
  CtxOptions o;
  const OptionSpec* spec = std::find_if(std::begin(kOptions), std::end(kOptions), [](const OptionSpec& s) { return s.kind == OptKind::Order; });
  parse_option(o, *spec, order_value);
  return order_route(n, finite != 0, o.order, no_sort != 0);
}

int cvo_debug_wide_plan(int n, int* W, int* rows, int capacity, int* n_rows) {
  const int leaf = CtxOptions().wide_leaf;
  const int rc = cvo_debug_wide_plan_at(n, leaf, rows, capacity, n_rows);
  if (rc == CVO_OK && W) *W = leaf;
  return rc;
}

int cvo_debug_wide_plan_at(int n, int leaf, int* rows, int capacity, int* n_rows) {
  if (n < 0 || n > KD_WIDE_MAX_POINTS || !n_rows || capacity < 0 || (capacity > 0 && !rows)) return CVO_E_INVALID;
  if (leaf < KD_THREADS || leaf > KD_MAX_POINTS) return CVO_E_INVALID;
  WidePlan P;
  wide_plan(n, leaf, P);
  *n_rows = (int)P.segs.size();
  for (int k = 0; k < std::min(capacity, *n_rows); k++) {
    const int row[4] = {P.seg_level[k], P.segs[k].lo, P.segs[k].hi, P.segs[k].left};
    std::memcpy(rows + 4 * (size_t)k, row, sizeof row);
  }
  return CVO_OK;
}

int cvo_debug_cloud_wide_pivots(const cvo_cloud* c, int capacity, unsigned* pivot, unsigned* rem, int* n_segments) {
  if (!c || !n_segments || capacity < 0 || (capacity > 0 && (!pivot || !rem))) return CVO_E_INVALID;
  if (c->order_route != ORDER_ROUTE_WIDE || c->h_wide_piv.empty()) return CVO_E_INVALID;
  *n_segments = (int)(c->h_wide_piv.size() / 2);
  for (int k = 0; k < std::min(capacity, *n_segments); k++) {
    pivot[k] = c->h_wide_piv[2 * (size_t)k];
    rem[k] = c->h_wide_piv[2 * (size_t)k + 1];
  }
  return CVO_OK;
}

int cvo_debug_device_memory(cvo_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
  if (!ctx || !free_bytes || !total_bytes) return fail(ctx, CVO_E_INVALID, "cvo_debug_device_memory: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemGetInfo(free_bytes, total_bytes));
  return CVO_OK;
}

int cvo_debug_device_buffer(cvo_ctx* ctx, size_t bytes, const void* host_src, void** d) {
  if (!ctx || !d || bytes == 0) return fail(ctx, CVO_E_INVALID, "cvo_debug_device_buffer: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool fresh = *d == nullptr;
  if (fresh) {
    const hipError_t e = hipMalloc(d, bytes);
    if (e != hipSuccess) {
      *d = nullptr;
      return fail(ctx, CVO_E_NOMEM, std::string("cvo_debug_device_buffer hipMalloc: ") + hipGetErrorString(e));
    }
  }
  if (host_src) {
    const hipError_t e = hipMemcpy(*d, host_src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (fresh) {
        (void)hipFree(*d);
        *d = nullptr;
      }
      return fail(ctx, CVO_E_HIP, std::string("cvo_debug_device_buffer copy: ") + hipGetErrorString(e));
    }
  }
  return CVO_OK;
}

int cvo_debug_device_release(cvo_ctx* ctx, void* d) {
  if (!ctx) return CVO_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (d) HIP_TRY(ctx, hipFree(d));
  return CVO_OK;
}

int cvo_debug_last_score_batch(const cvo_ctx* ctx, int* overlap_evals, int* chain_evals, int* launches) {
  if (!ctx) return CVO_E_INVALID;
  if (overlap_evals) *overlap_evals = ctx->last_score_overlap;
  if (chain_evals) *chain_evals = ctx->last_score_chain;
  if (launches) *launches = ctx->last_score_launches;
  return CVO_OK;
}

int cvo_debug_cloud_tiles(cvo_ctx* ctx, const cvo_cloud* cloud, float* out, int* n_tiles) {
  const char* who = "cvo_debug_cloud_tiles";
  if (!ctx || !cloud || !out || !n_tiles) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (cloud->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the cloud belongs to another context");
  if (cloud->n <= 0) return fail(ctx, CVO_E_INVALID, std::string(who) + ": empty cloud");
  if (ctx->queue_open) return fail(ctx, CVO_E_INVALID, "a batch queue is open on this context (cvo_batch_close it first)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the records the scores read: made here, on their stream, when no score has read this cloud yet - and kept
  if (const int rc = ensure_tiles(ctx, cloud, ctx->stream); rc != CVO_OK) return rc;
  const int nt = (cloud->n + 63) / 64;
  HIP_TRY(ctx, hipMemcpyAsync(out, cloud->tile4, sizeof(float4) * 2 * (size_t)nt, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_tiles = nt;
  return CVO_OK;
}

int cvo_debug_verified_rows(cvo_ctx* ctx, unsigned long long* rows) {
  if (!ctx || !rows || ctx->last_pairs < 1) return fail(ctx, CVO_E_INVALID, "cvo_debug_verified_rows: bad argument");
  unsigned long long t = 0;
  for (int p = 0; p < ctx->last_pairs; p++) t += ctx->h_states[p].verify_rows;
  *rows = t;
  return CVO_OK;
}

int cvo_debug_last_candidates(cvo_ctx* ctx, unsigned long long* out) {
  if (!ctx || !out || ctx->last_pairs < 1) return fail(ctx, CVO_E_INVALID, "cvo_debug_last_candidates: bad argument");
  *out = ctx->h_states[0].ncand;
  return CVO_OK;
}

int cvo_debug_time_kernels(cvo_ctx* ctx, int reps, float* ms_assoc, float* ms_coeff) {
  if (!ctx || reps <= 0 || ctx->last_pairs < 1 || !ms_assoc || !ms_coeff)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_time_kernels: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the per-iteration launches of the optimiser loop (one per sub-batch), replayed on the state the last call
  // left behind: same lists, same rows, same arithmetic; k_coeff's last block runs the update without writing
  // anything back
  const int n_pairs = ctx->last_pairs, G = ctx->last.G;
  const DevParams& dp = ctx->last_params;
  const LaunchGeom& g0 = ctx->last.geom;
  const IterWords w = iteration_words({.idx32 = !g0.idx16, .rebuild_follows = true, .replay = true});
  float out[2] = {0.f, 0.f};
  for (int which = 0; which < 2; which++) {
    auto sweep = [&]() {
      for (int q = 0; q < G; q++) {
        const LaunchGeom g = group_geom(ctx, ctx->last, n_pairs, q);
        const PairDesc* descs = ctx->d_descs + g.p0;
        if (which == 0)
          launch_assoc(ctx->stream, g.idx16, g.feat, g.instr, g.nba, g.n_pairs, descs, ctx->d_params, ctx->d_states + g.p0, g.arena,
                       w.assoc);
        else
          launch_coeff(ctx->stream, g.instr, g.nba, g.csplit, g.n_pairs, descs, ctx->d_params, ctx->d_states + g.p0, g.arena, w.iter);
      }
    };
    sweep();  // warm-up
    HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
    for (int r = 0; r < reps; r++) sweep();
    HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(&out[which], ctx->ev_start, ctx->ev_stop));
    out[which] /= (float)(reps * G);
  }
  if (dp.phase_ticks) {  // where the blocks of the last sub-batch's launches spent their time (see g_phase_ticks)
    static unsigned long long h[2][8192][4];
    HIP_TRY(ctx, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase_ticks), sizeof(h)));
    const int np = n_pairs - (int)((long)n_pairs * (G - 1) / G);
    for (int which = 0; which < 2; which++) {
      const int nb = std::min(4096, 8 * ((np + 7) / 8) * g0.nba * (which ? g0.csplit : 1));
      double sum[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
      int cnt = 0;
      for (int b = 0; b < nb; b++) {
        if (!h[which][b][0] || !h[which][b][3]) continue;
        for (int q = 0; q < 3; q++) {
          const double d = (double)(long long)(h[which][b][q + 1] - h[which][b][q]);
          sum[q] += d;
          mx[q] = std::max(mx[q], d);
        }
        cnt++;
      }
      if (!cnt) continue;
      fprintf(stderr, "[cvo] %s: %d blocks; ticks (avg / max) %s %.0f / %.0f, row loop %.0f / %.0f, %s %.0f / %.0f\n",
              which ? "k_coeff" : "k_assoc", cnt, which ? "prologue + twist" : "prologue", sum[0] / cnt, mx[0], sum[1] / cnt,
              mx[1], which ? "reduction + counter" : "reduction + flow gate", sum[2] / cnt, mx[2]);
      if (which)
        for (int p = 0; p < std::min(np, 3); p++)
          fprintf(stderr, "[cvo]   pair %d, updating block: entry -> counter %.0f, update %.0f ticks\n", p,
                  (double)(long long)(h[1][4096 + p][1] - h[1][4096 + p][0]),
                  (double)(long long)(h[1][4096 + p][2] - h[1][4096 + p][1]));
      if (which) {
        unsigned long long u[8];
        HIP_TRY(ctx, hipMemcpyFromSymbol(u, HIP_SYMBOL(g_upd_ticks), sizeof(u)));
        fprintf(stderr, "[cvo]   inside the update (last pair to run it): reduce %lld, step %lld, pose + distance + indicator %lld, "
                        "update_tf + list bookkeeping %lld, rest %lld, write-back %lld ticks\n",
                (long long)(u[1] - u[0]), (long long)(u[2] - u[1]), (long long)(u[3] - u[2]), (long long)(u[4] - u[3]),
                (long long)(u[5] - u[4]), (long long)(u[6] - u[5]));
      }
    }
  }
  *ms_assoc = out[0];
  *ms_coeff = out[1];
  return CVO_OK;
}

int cvo_debug_kernel_clock(cvo_ctx* ctx, float* ms_assoc, float* ms_coeff, unsigned long long* launches) {
  if (!ctx || ctx->last_pairs < 1 || !ms_assoc || !ms_coeff)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_kernel_clock: bad argument");
  if (!ctx->last_params.kernel_clock) return fail(ctx, CVO_E_INVALID, "cvo_debug_kernel_clock: the last call ran without CVO_KERNEL_CLOCK");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->clock_ms_per_tick <= 0.0) {  // the counter's rate, against HIP events around a kernel that waits 1e6 ticks
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    for (int rep = 0; rep < 2; rep++) {
      HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
      hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, ctx->stream, 1000000ull);
      HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    }
    ctx->clock_ms_per_tick = (double)ms / 1e6;
  }
  double sum[2] = {0, 0}, n[2] = {0, 0};
  for (int p = 0; p < ctx->last_pairs; p++)
    for (int w = 0; w < 2; w++) {
      sum[w] += (double)ctx->h_states[p].clk_sum[w];
      n[w] += (double)ctx->h_states[p].clk_n[w];
    }
  *ms_assoc = n[0] > 0 ? (float)(sum[0] / n[0] * ctx->clock_ms_per_tick) : 0.f;
  *ms_coeff = n[1] > 0 ? (float)(sum[1] / n[1] * ctx->clock_ms_per_tick) : 0.f;
  if (launches) *launches = (unsigned long long)n[1];
  return CVO_OK;
}

int cvo_debug_list_builds(cvo_ctx* ctx, unsigned long long* builds, unsigned long long* iterations,
                          unsigned long long* candidate_evaluations) {
  if (!ctx || !builds || ctx->last_pairs < 1) return fail(ctx, CVO_E_INVALID, "cvo_debug_list_builds: bad argument");
  unsigned long long b = 0, it = 0, ce = 0;
  for (int p = 0; p < ctx->last_pairs; p++) {
    b += (unsigned long long)ctx->h_states[p].n_builds;
    it += (unsigned long long)ctx->h_states[p].iterations;
    ce += ctx->h_states[p].ncand_total;
  }
  *builds = b;
  if (iterations) *iterations = it;
  if (candidate_evaluations) *candidate_evaluations = ce;
  return CVO_OK;
}

int cvo_debug_row_classes(cvo_ctx* ctx, int pair, int* overflow_rows, int* scanned_rows, int* dense_regime) {
  if (!ctx || pair < 0 || pair >= ctx->last_pairs) return fail(ctx, CVO_E_INVALID, "cvo_debug_row_classes: bad argument");
  const PairState& st = ctx->h_states[pair];
  if (overflow_rows) *overflow_rows = st.n_ovf;
  if (scanned_rows) *scanned_rows = st.n_scan;
  if (dense_regime) *dense_regime = st.all_dense;
  return CVO_OK;
}

int cvo_debug_speculation(cvo_ctx* ctx, int pair, int* adopted, int* iterations) {
  if (!ctx || pair < 0 || pair >= ctx->last_pairs) return fail(ctx, CVO_E_INVALID, "cvo_debug_speculation: bad argument");
  const PairState& st = ctx->h_states[pair];
  if (adopted) *adopted = st.n_adopted;
  if (iterations) *iterations = st.status ? st.iterations : st.k;  // (as cvo_align_info_t reports them)
  return CVO_OK;
}

int cvo_debug_scan_stats(cvo_ctx* ctx, unsigned long long* tiles, int* rows_per_tile, int* targets_per_tile) {
  if (!ctx || !tiles || ctx->last_pairs < 1) return fail(ctx, CVO_E_INVALID, "cvo_debug_scan_stats: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  unsigned long long total = 0;
  for (int p = 0; p < ctx->last_pairs; p++) {
    unsigned long long v = 0;
    HIP_TRY(ctx, hipMemcpy(&v, ctx->h_descs[p].tile_count, sizeof(v), hipMemcpyDeviceToHost));
    total += v;
  }
  *tiles = total;
  if (rows_per_tile) *rows_per_tile = ROWS_PER_GROUP;
  if (targets_per_tile) *targets_per_tile = 64 * ctx->last.geom.T;
  return CVO_OK;
}

int cvo_debug_last_geometry(cvo_ctx* ctx, int* n_groups, int* pairs_per_group) {
  if (!ctx || ctx->last_pairs < 1) return fail(ctx, CVO_E_INVALID, "cvo_debug_last_geometry: bad argument");
  if (n_groups) *n_groups = ctx->last.G;
  if (pairs_per_group) *pairs_per_group = (ctx->last_pairs + ctx->last.G - 1) / ctx->last.G;
  return CVO_OK;
}

int cvo_debug_time_scan(cvo_ctx* ctx, int reps, float* ms) {
  if (!ctx || !ms || reps <= 0 || ctx->last_pairs < 1)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_time_scan: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the same launches the optimiser loop issues: one k_scan per sub-batch, here back to back on one stream
  const int n_pairs = ctx->last_pairs, G = ctx->last.G;
  auto sweep = [&]() {  // (forced: the pairs' lists are current)
    for (int q = 0; q < G; q++) {
      const LaunchGeom g = group_geom(ctx, ctx->last, n_pairs, q);
      launch_scan(ctx->stream, g.T, dim3(g.gx, g.gy, g.n_pairs), ctx->d_descs + g.p0, ctx->d_params, ctx->d_states + g.p0, true);
    }
  };
  sweep();  // warm-up
  HIP_TRY(ctx, hipEventRecord(ctx->ev_start, ctx->stream));
  for (int r = 0; r < reps; r++) sweep();
  HIP_TRY(ctx, hipEventRecord(ctx->ev_stop, ctx->stream));
  HIP_TRY(ctx, hipGetLastError());
  // the extra scans leave slice bits behind; clean them so the workspace stays consistent
  for (int p = 0; p < n_pairs; p++) {
    const PairDesc& D = ctx->h_descs[p];
    HIP_TRY(ctx, hipMemsetAsync(D.rowbits, 0, sizeof(unsigned) * (size_t)(ctx->last.N + 4) * D.rbw, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  float t = 0;
  HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->ev_start, ctx->ev_stop));
  *ms = t / (reps * G);
  return CVO_OK;
}

}  // extern "C"
