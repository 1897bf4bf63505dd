// cvo_eval.hip -- scores: inner_product_gpu / function_angle, one job (cvo_inner_product / cvo_function_angle) or many
// (cvo_*_batch), all through score_batch: k_overlap (k_overlap_entry for up to three evaluations, k_overlap_table for more)
// or the list chain; run_single_eval for the association exports.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

int run_single_eval(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source, const cvo_cloud* target,
                    const float Tm[16], float ell, BatchSetup* S, const float* kernel_inv_and_cull = nullptr) {
  DevParams dp;
  const cvo_cloud* src[1] = {source};
  const cvo_cloud* tgt[1] = {target};
  const CallMode mode = kernel_inv_and_cull ? CALL_NONISO : CALL_SINGLE;
  int rc = setup_batch(ctx, {params, 1, src, tgt, Tm, nullptr, mode, ell, kernel_inv_and_cull, nullptr}, S, &dp);
  if (rc != CVO_OK) return rc;
  launch_init(ctx, S->geom);
  launch_rebuild(ctx, S->geom);
  launch_core(ctx, S->geom, {.idx32 = !S->geom.idx16, .rebuild_follows = true});  // (k_coeff is a no-op in a single evaluation ...
  hipLaunchKernelGGL(k_update<false>, dim3(1), dim3(64), 0, ctx->stream, ctx->d_descs, ctx->d_params, ctx->d_status,
                     iteration_words({.rebuild_follows = true}).iter);  // ... k_update collects the sums)
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_states.data(), ctx->d_states, sizeof(PairState), hipMemcpyDeviceToHost,
                              ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CVO_OK;
}

// Up to three evaluations in one launch of k_overlap (cvo_k_overlap.h) with the jobs as kernel ARGUMENTS: no table upload
// precedes the launch.
struct OverlapArgs {
  OverlapJob job[3];
  DevParams P;
};
static_assert(sizeof(OverlapArgs) <= 4096, "k_overlap takes its jobs as kernel arguments");
template <int FEAT>
__global__ __launch_bounds__(64 * OV_WAVES) void k_overlap_entry(const OverlapArgs A) {
  k_overlap<FEAT>(A.job[blockIdx.y], A.P, (int)blockIdx.x);
}

// The batched form (cvo_inner_product_batch / cvo_function_angle_batch): the jobs are a DEVICE table, the grid is flat -
// one block per row tile of every job, sum of the jobs' tiles, no idle blocks - and a block finds its (job, tile) by a
// binary search of the tiles' exclusive prefix sum tile_start[0 .. n_jobs] (wave-uniform: scalar loads, log2 n_jobs steps).
template <int FEAT>
__global__ __launch_bounds__(64 * OV_WAVES) void k_overlap_table(const OverlapJob* __restrict__ jobs, const int* __restrict__ tile_start,
                                                                 const int n_jobs, const DevParams P) {
  const int b = (int)blockIdx.x;
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tile_start[mid] <= b) lo = mid;
    else hi = mid - 1;
  }
  k_overlap<FEAT>(jobs[lo], P, b - tile_start[lo]);
}

// An OverlapJob's description of one evaluation <f_X, f_Y> under Tm (everything but its partials, gate words and result
// slots).
void fill_overlap_job(const cvo_cloud* X, const cvo_cloud* Y, const float* Tm, float ell, int K, OverlapJob& J) {
  J.D.N = X->n;
  J.D.M = Y->n;
  J.D.xs4 = X->xs4;
  J.D.ys4 = Y->xs4;
  J.D.xfeat = X->feat;
  J.D.yfeat = Y->feat;
  J.D.xlabel = X->label;
  J.D.ylabel = Y->label;
  J.D.xgeo = X->geo;
  J.D.ygeo = Y->geo;
  J.D.xlid = X->lid;
  J.D.ylid = Y->lid;
  J.xtile = X->tile4;
  J.ytile = Y->tile4;
  J.n_xtiles = (X->n + 63) / 64;
  J.n_ytiles = (Y->n + 63) / 64;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) J.R[3 * i + j] = Tm[4 * j + i];  // CvoGPU.cu:1363-1364 (as fill_pair)
    J.T[i] = Tm[12 + i];
  }
  {
    // |R^T v| <= stretch |v|: 1 (+ rounding) for a rotation, the Frobenius norm for anything else a caller may pass
    double dev = 0, fro = 0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        double g = 0;
        for (int k = 0; k < 3; k++) g += (double)J.R[3 * k + i] * (double)J.R[3 * k + j];
        dev = std::max(dev, std::fabs(g - (i == j ? 1.0 : 0.0)));
        fro += (double)J.R[3 * i + j] * (double)J.R[3 * i + j];
      }
    J.stretch = (dev <= 1e-4) ? 1.001f : (float)(std::sqrt(fro) * 1.001);
    if (!std::isfinite(J.stretch)) J.stretch = __builtin_inff();  // (every tile is visited)
  }
  J.ell = ell;
  J.K = K;
}

int ensure_tiles(cvo_ctx* ctx, const cvo_cloud* c, hipStream_t s) {
  if (c->tile4) return CVO_OK;
  const int nt = (c->n + 63) / 64;
  DeviceRegion t;
  if (const int rc = t.reserve(ctx, sizeof(float4) * 2 * (size_t)nt, "tile spheres", nullptr); rc != CVO_OK) return rc;
  hipLaunchKernelGGL(k_tile_spheres, dim3((nt + 3) / 4), dim3(256), 0, s, c->n, c->xs4, t.as<float4>());
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ctx, CVO_E_HIP, std::string("k_tile_spheres: ") + hipGetErrorString(e));
  c->tiles = std::move(t);
  c->tile4 = c->tiles.as<float4>();
  return CVO_OK;
}

// The list chain for n (< 8: one sub-batch) inner products of one lengthscale: INIT, the rebuild trio, [k_assoc_dense],
// k_assoc whose last block posts A_sum to pinned host memory - one upload, one graph launch, one synchronisation.  Every
// value is what the one-pair chain returns (a pair's sums do not depend on its company).
int run_ip_chain(cvo_ctx* ctx, const cvo_params_t* params, int n, const cvo_cloud* const* src, const cvo_cloud* const* tgt,
                 const float* Tms, float ell, double* out) {
  BatchSetup S;
  DevParams dp;
  int rc = setup_batch(ctx, {params, n, src, tgt, Tms, nullptr, CALL_SINGLE, ell, nullptr, nullptr}, &S, &dp);
  if (rc != CVO_OK) return rc;
  if (S.G != 1) return fail(ctx, CVO_E_INVALID, "run_ip_chain: too many pairs for one chain");
  const LaunchGeom& g = S.geom;
  GraphKey key = graph_key(g, ChunkPlan{});
  key.csplit = key.horizon_cap = 0;  // (no k_coeff, k_verify or lean iteration in the chain: see GraphKey)
  key.verify = false;
  rc = capture_graph(ctx, ctx->chain_graph, key, g.stream, nullptr, 0, "inner product graph", [&] {
    launch_init(ctx, g);
    launch_rebuild(ctx, g);
    launch_dense(g.stream, g.feat, g.wide, g.n_pairs, g.dense_blocks, ctx->d_descs, ctx->d_params, ctx->d_states);
    launch_assoc(g.stream, g.idx16, g.feat, g.instr, g.nba, g.n_pairs, ctx->d_descs, ctx->d_params, ctx->d_states, g.arena,
                 iteration_words({.asum_only = true}).assoc);
  });
  if (rc != CVO_OK) return rc;
  HIP_TRY(ctx, hipGraphLaunch(ctx->chain_graph.exec, g.stream));
  HIP_TRY(ctx, hipStreamSynchronize(g.stream));
  const volatile double* res = ctx->h_status[1].as<double>();
  for (int p = 0; p < n; p++) {
    out[p] = res[p];
    ctx->h_states[p].asum = res[p];
  }
  return CVO_OK;
}

// ---- scores: cvo_inner_product / cvo_function_angle (one job), cvo_inner_product_batch / cvo_function_angle_batch ------
// A job's value does not depend on its company - k_overlap sums a job's row tiles in tile order whatever shares the launch,
// the list chain's values do not depend on theirs - so every job of a batch gets, bit for bit, what the one-job call gets.
// One launch of k_overlap and one synchronisation per chunk of the evaluation list.
constexpr int SB_CHUNK_JOBS = 1024;    // jobs per launch (pinned results, device table and its staging are sized by it)
constexpr int SB_CHUNK_TILES = 65536;  // row tiles per launch (4M source rows), unless one job alone has more

struct ScoreResult {  // what k_overlap posts for one evaluation: the sum and its void flag in one 16-byte slot
  double sum;
  int over;
};

// The score workspace [gate words | partials]: the partials are its open tail, as many row tiles as the region has room for
struct ScoreWs {
  int* gate = nullptr;
  double* part = nullptr;
  auto list() {
    return [this](ScratchLayout& l) {
      l.take(gate, 2 * SB_CHUNK_JOBS);
      l.at(part, l.off);
    };
  }
};
// The job table [tile starts | jobs] of k_overlap_table, over the device table and over its pinned staging
struct ScoreTable {
  int* start = nullptr;
  OverlapJob* jobs = nullptr;
  auto list() {
    return [this](ScratchLayout& l) {
      l.take(start, SB_CHUNK_JOBS + 1);
      l.take(jobs, SB_CHUNK_JOBS);
    };
  }
};

// Room for `tiles` row tiles in the device workspace, and the pinned results (a small call's slots share one cache line).
// Gate words are zeroed once per region; the kernel leaves them at zero.  *tiles_cap: the tiles the region holds.
int score_ws_reserve(cvo_ctx* ctx, int tiles, ScoreWs* ws, int* tiles_cap) {
  const size_t gate_bytes = ScratchLayout().walk(ws->list());
  bool moved = false;
  int rc = ctx->d_sb.reserve(ctx, gate_bytes + sizeof(double) * (size_t)tiles, "score workspace", ctx->stream, &moved);
  if (rc != CVO_OK) return rc;
  ScratchLayout(ctx->d_sb.p).walk(ws->list());
  *tiles_cap = (int)((ctx->d_sb.bytes - gate_bytes) / sizeof(double));
  if (moved) HIP_TRY(ctx, hipMemsetAsync(ws->gate, 0, gate_bytes, ctx->stream));
  return ctx->h_sb_res.reserve(ctx, sizeof(ScoreResult) * SB_CHUNK_JOBS, "score results", nullptr);
}

struct ScoreEval {
  const cvo_cloud* X;
  const cvo_cloud* Y;
  const float* T;
  float ell;
  double ov = 0;       // k_overlap's sum ...
  bool over = false;   // ... void: some row found more than nearest_neighbors_max pairs
  bool chain = false;  // some job takes this evaluation from the list chain ...
  double ch = 0;       // ... its value there
};

struct ScoreJob {
  int ev[3] = {-1, -1, -1};  // its evaluations: <X, Y> (-1: an empty cloud, the job is 0) [, <X, X>, <Y, Y>]
  bool chain = false;        // all of them from the list chain
};

// All evaluations through k_overlap, each with its own partials, gate words and pinned result slot in the score workspace.
// Up to three (a single call's): ONE launch of k_overlap_entry on a grid of (largest tile count, n), no table copy in front
// of it.  More: k_overlap_table, jobs largest first (a launch's tail is its largest job's last tiles), cut into chunks of at
// most SB_CHUNK_JOBS jobs / SB_CHUNK_TILES tiles; the prefix of the pinned staging [tile starts | job table] that a chunk
// occupies goes up in one copy.  That table and its staging are made by the first call that needs them.
int score_overlap(cvo_ctx* ctx, const cvo_params_t* params, std::pmr::vector<ScoreEval>& ev) {
  hipStream_t stream = ctx->stream;
  const DevParams P = make_dev_params(ctx, *params, CALL_SINGLE);
  bool all_hot = !ctx->opt.no_onehot;  // (FEAT_HOT and FEAT_ALL give the same bits: test_gpu_parity.py)
  int rc, tiles_max = 0;
  size_t tiles_sum = 0;
  for (const ScoreEval& e : ev) {
    if ((rc = ensure_tiles(ctx, e.X, stream)) != CVO_OK || (rc = ensure_tiles(ctx, e.Y, stream)) != CVO_OK) return rc;
    all_hot = all_hot && e.X->lid != nullptr && e.Y->lid != nullptr;
    tiles_max = std::max(tiles_max, (e.X->n + 63) / 64);
    tiles_sum += (size_t)(e.X->n + 63) / 64;
  }
  const int feat = call_feat(P, all_hot);
  const bool by_args = ev.size() <= 3;
  std::pmr::vector<int> order(ev.size(), ev.get_allocator());
  for (size_t i = 0; i < ev.size(); i++) order[i] = (int)i;
  if (!by_args) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ev[a].X->n > ev[b].X->n; });
  ScoreWs ws;
  int tiles_cap = 0;
  if ((rc = score_ws_reserve(ctx, by_args ? (int)tiles_sum : std::max(SB_CHUNK_TILES, tiles_max), &ws, &tiles_cap)) != CVO_OK) return rc;
  OverlapArgs A;
  std::memset(&A, 0, sizeof(A));
  A.P = P;
  OverlapJob* jobs = A.job;
  ScoreTable dt, ht;
  if (!by_args) {
    if ((rc = ctx->d_sb_table.lay_out(ctx, "score table", dt.list(), nullptr)) != CVO_OK) return rc;
    if ((rc = ctx->h_sb.lay_out(ctx, "score table staging", ht.list(), nullptr)) != CVO_OK) return rc;
    jobs = ht.jobs;
  }
  int* const h_start = ht.start;
  const int* d_start = dt.start;
  const OverlapJob* d_jobs = dt.jobs;
  int* d_gate = ws.gate;
  double* d_part = ws.part;
  ScoreResult* h_res = ctx->h_sb_res.as<ScoreResult>();
  for (size_t pos = 0; pos < order.size();) {
    int n = 0, tiles = 0;
    while (pos + n < order.size() && n < SB_CHUNK_JOBS) {
      const ScoreEval& e = ev[order[pos + n]];
      const int t = (e.X->n + 63) / 64;
      if (n > 0 && tiles + t > tiles_cap) break;
      OverlapJob& J = jobs[n];
      std::memset(&J, 0, sizeof(J));
      fill_overlap_job(e.X, e.Y, e.T, e.ell, params->nearest_neighbors_max, J);
      J.part = d_part + tiles;
      J.gate = d_gate + 2 * n;
      J.sum_host = &h_res[n].sum;
      J.over_host = &h_res[n].over;
      if (!by_args) h_start[n] = tiles;
      tiles += t;
      n++;
    }
    const dim3 block(64 * OV_WAVES);
    if (by_args) {
      const dim3 grid(tiles_max, n);
      switch (feat) {
        case FEAT_GEO: hipLaunchKernelGGL((k_overlap_entry<FEAT_GEO>), grid, block, 0, stream, A); break;
        case FEAT_COL: hipLaunchKernelGGL((k_overlap_entry<FEAT_COL>), grid, block, 0, stream, A); break;
        case FEAT_HOT: hipLaunchKernelGGL((k_overlap_entry<FEAT_HOT>), grid, block, 0, stream, A); break;
        default: hipLaunchKernelGGL((k_overlap_entry<FEAT_ALL>), grid, block, 0, stream, A); break;
      }
    } else {
      h_start[n] = tiles;
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sb_table.p, ctx->h_sb.p, (size_t)((const char*)(jobs + n) - ctx->h_sb.p), hipMemcpyHostToDevice, stream));
      const dim3 grid(tiles);
      switch (feat) {
        case FEAT_GEO: hipLaunchKernelGGL((k_overlap_table<FEAT_GEO>), grid, block, 0, stream, d_jobs, d_start, n, P); break;
        case FEAT_COL: hipLaunchKernelGGL((k_overlap_table<FEAT_COL>), grid, block, 0, stream, d_jobs, d_start, n, P); break;
        case FEAT_HOT: hipLaunchKernelGGL((k_overlap_table<FEAT_HOT>), grid, block, 0, stream, d_jobs, d_start, n, P); break;
        default: hipLaunchKernelGGL((k_overlap_table<FEAT_ALL>), grid, block, 0, stream, d_jobs, d_start, n, P); break;
      }
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      (void)hipMemset(d_gate, 0, sizeof(int) * 2 * SB_CHUNK_JOBS);  // (a launch that died may have left gate words behind)
      return fail(ctx, CVO_E_HIP, std::string(by_args ? "k_overlap: " : "k_overlap_table: ") + hipGetErrorString(e));
    }
    for (int i = 0; i < n; i++) {
      ScoreEval& r = ev[order[pos + i]];
      const volatile ScoreResult& v = h_res[i];
      r.ov = v.sum;
      r.over = v.over != 0;
    }
    ctx->last_score_overlap += n;
    ctx->last_score_launches++;
    pos += n;
  }
  ctx->last_pairs = 0;  // (no workspace of the list chain belongs to this call: the debug getters have nothing to read)
  return CVO_OK;
}

// Calls the list chain evaluates whole: no geometric cut-off for k_overlap to cull by, or a context that asks for the chain
// (CVO_IP_CHAIN; the instrumented / verifying runs are the chain's).
bool chain_only(const cvo_ctx* ctx, const cvo_params_t* params) {
  const CtxOptions& o = ctx->opt;
  return !params->is_using_geometry || o.ip_chain || o.verify_lists || o.kernel_clock || o.phase_ticks;
}

// kind: 0 inner product, 1 approximate function_angle, 2 exact function_angle.  Validates the whole call before any device
// work; writes `out` only when every job has its value.
int score_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_jobs, const cvo_cloud* const* sources,
                const cvo_cloud* const* targets, const float* T, const float* ell, int kind, float* out, const char* name) {
  if (!ctx) return CVO_E_INVALID;
  if (!params || n_jobs < 0 || (n_jobs > 0 && (!sources || !targets || !T || !ell || !out)))
    return fail(ctx, CVO_E_INVALID, std::string(name) + ": bad argument");
  if (ctx->queue_open) return fail(ctx, CVO_E_INVALID, "a batch queue is open on this context (cvo_batch_close it first)");
  if (params->is_using_kdtree)
    return fail(ctx, CVO_E_UNSUPPORTED, "is_using_kdtree=1 is out of scope (SURVEY.md section 2, row 11)");
  // the call's bookkeeping lives in `scratch` while it fits (a single call allocates nothing), on the heap beyond
  alignas(std::max_align_t) char scratch[4096];
  std::pmr::monotonic_buffer_resource mem(scratch, sizeof(scratch));
  std::pmr::vector<int> live(&mem);  // jobs with two non-empty clouds (the others are 0, as the single call returns)
  std::pmr::vector<const cvo_cloud*> ls(&mem), lt(&mem);
  for (int k = 0; k < n_jobs; k++) {
    if (!sources[k] || !targets[k]) return fail(ctx, CVO_E_INVALID, "null cloud");
    if (sources[k]->n == 0 || targets[k]->n == 0) continue;
    live.push_back(k);
    ls.push_back(sources[k]);
    lt.push_back(targets[k]);
  }
  ctx->last_score_overlap = ctx->last_score_chain = ctx->last_score_launches = 0;
  const bool chain_all = chain_only(ctx, params);
  if (live.empty()) {
    if (params->nearest_neighbors_max <= 0) return fail(ctx, CVO_E_INVALID, "nearest_neighbors_max must be > 0");
  } else if (live.size() > 1 || !chain_all) {
    // (one chain-only job: its one run_ip_chain makes this check_call on the same clouds before any device work)
    int N = 0, M = 0;
    const int rc = check_call(ctx, params, (int)live.size(), ls.data(), lt.data(), nullptr, CALL_SINGLE, ell[live[0]], nullptr,
                                &N, &M);
    if (rc != CVO_OK) return rc;
    for (int k : live)  // (check_call's lengthscale rule, for every job's own ell)
      if (!(std::isfinite(ell[k]) && ell[k] >= 1e-30f && ell[k] <= 1e15f))
        return fail(ctx, CVO_E_INVALID, "lengthscale outside [1e-30, 1e15] (ell_init / ell_min / the ell of the call)");
  }
  static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // the evaluations: <X, Y> per job; the exact function_angle's <X, X> / <Y, Y> once per (cloud, ell)
  std::pmr::vector<ScoreEval> ev(&mem);
  ev.reserve(live.size() * (kind == 2 ? 3 : 1));
  std::pmr::vector<ScoreJob> jobs(n_jobs, &mem);
  std::pmr::map<std::pair<const cvo_cloud*, uint32_t>, int> self_ev(&mem);
  auto self_eval = [&](const cvo_cloud* c, float l) {
    uint32_t bits;
    std::memcpy(&bits, &l, 4);
    auto it = self_ev.find({c, bits});
    if (it != self_ev.end()) return it->second;
    ev.push_back(ScoreEval{c, c, identity, l});
    self_ev[{c, bits}] = (int)ev.size() - 1;
    return (int)ev.size() - 1;
  };
  for (int k : live) {
    jobs[k].ev[0] = (int)ev.size();
    ev.push_back(ScoreEval{sources[k], targets[k], T + 16 * (size_t)k, ell[k]});
    if (kind == 2) {
      jobs[k].ev[1] = self_eval(sources[k], ell[k]);
      jobs[k].ev[2] = self_eval(targets[k], ell[k]);
    }
  }
  int rc;
  if (!chain_all && !ev.empty() && (rc = score_overlap(ctx, params, ev)) != CVO_OK) return rc;
  // A job is void when one of ITS evaluations is (the exact function_angle: all three then come from the chain).
  for (int k : live) {
    ScoreJob& J = jobs[k];
    J.chain = chain_all;
    for (int i = 0; i < 3; i++) J.chain = J.chain || (J.ev[i] >= 0 && ev[J.ev[i]].over);
    if (J.chain)
      for (int i = 0; i < 3; i++)
        if (J.ev[i] >= 0) ev[J.ev[i]].chain = true;
  }
  // the chain's evaluations, in groups of up to seven of one lengthscale (one sub-batch, one synchronisation each)
  {
    std::pmr::map<uint32_t, std::pmr::vector<int>> by_ell(&mem);
    for (int i = 0; i < (int)ev.size(); i++)
      if (ev[i].chain) {
        uint32_t bits;
        std::memcpy(&bits, &ev[i].ell, 4);
        by_ell[bits].push_back(i);
      }
    for (auto& g : by_ell)
      for (size_t p0 = 0; p0 < g.second.size(); p0 += 7) {
        const int n = (int)std::min<size_t>(7, g.second.size() - p0);
        const cvo_cloud* src[7];
        const cvo_cloud* tgt[7];
        float Ts[16 * 7];
        double v[7];
        for (int i = 0; i < n; i++) {
          const ScoreEval& e = ev[g.second[p0 + i]];
          src[i] = e.X;
          tgt[i] = e.Y;
          std::memcpy(Ts + 16 * i, e.T, sizeof(float) * 16);
        }
        if ((rc = run_ip_chain(ctx, params, n, src, tgt, Ts, ev[g.second[p0]].ell, v)) != CVO_OK) return rc;
        for (int i = 0; i < n; i++) ev[g.second[p0 + i]].ch = v[i];
        ctx->last_score_chain += n;
        ctx->last_score_launches++;
      }
  }
  // the host arithmetic of inner_product_gpu / function_angle (CvoGPU.cu:1814-1846); nothing fails from here on, so `out`
  // is written only when every job has its value
  for (int k = 0; k < n_jobs; k++) {
    const ScoreJob& J = jobs[k];
    auto val = [&](int i) {
      const ScoreEval& e = ev[J.ev[i]];
      return J.chain ? e.ch : e.ov;
    };
    if (J.ev[0] < 0) {  // an empty cloud
      out[k] = 0.f;
      continue;
    }
    if (kind == 0) {
      out[k] = (float)val(0);
      continue;
    }
    float fxfz = (float)val(0), fx_norm, fz_norm;
    if (kind == 1) {
      fx_norm = (float)std::sqrt((double)sources[k]->n);
      fz_norm = (float)std::sqrt((double)targets[k]->n);
    } else {
      fx_norm = std::sqrt((float)val(1));
      fz_norm = std::sqrt((float)val(2));
    }
    out[k] = fxfz / (fx_norm * fz_norm);
  }
  return CVO_OK;
}

}  // namespace

extern "C" {

#ifdef CVO_OV_STAMPS
int cvo_debug_overlap_ticks(unsigned long long* out) {  // experiment builds only
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ov_ticks), sizeof(unsigned long long) * 4096 * 8) == hipSuccess ? 0 : -1;
}
#endif

int cvo_inner_product(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source, const cvo_cloud* target,
                      const float T[16], float ell, float* out) {
  if (!ctx || !out || !T) return fail(ctx, CVO_E_INVALID, "cvo_inner_product: bad argument");
  if (!source || !target) return fail(ctx, CVO_E_INVALID, "null cloud");
  if (source->n == 0 || target->n == 0) {
    *out = 0.f;
    return CVO_OK;
  }
  return score_batch(ctx, params, 1, &source, &target, T, &ell, 0, out, "cvo_inner_product");
}

int cvo_function_angle(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source, const cvo_cloud* target,
                       const float T[16], float ell, int is_approximate, float* out) {
  if (!ctx || !out || !T) return fail(ctx, CVO_E_INVALID, "cvo_function_angle: bad argument");
  if (!source || !target) return fail(ctx, CVO_E_INVALID, "null cloud");
  if (source->n == 0 || target->n == 0) {
    *out = 0.f;
    return CVO_OK;
  }
  return score_batch(ctx, params, 1, &source, &target, T, &ell, is_approximate ? 1 : 2, out, "cvo_function_angle");
}

int cvo_inner_product_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_jobs, const cvo_cloud* const* sources,
                            const cvo_cloud* const* targets, const float* T, const float* ell, float* out) {
  return score_batch(ctx, params, n_jobs, sources, targets, T, ell, 0, out, "cvo_inner_product_batch");
}

int cvo_function_angle_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_jobs, const cvo_cloud* const* sources,
                             const cvo_cloud* const* targets, const float* T, const float* ell, int is_approximate, float* out) {
  return score_batch(ctx, params, n_jobs, sources, targets, T, ell, is_approximate ? 1 : 2, out, "cvo_function_angle_batch");
}

}  // extern "C"
