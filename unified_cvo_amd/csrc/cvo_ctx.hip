// cvo_ctx.hip -- contexts: the hardware-queue contract, the stream pool, options, the workspace of a call (arena, control block, layout of one pair), defaults of cvo_params_t.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
// ---- the hardware-queue contract ---------------------------------------------------------------------------------
// A batch runs on four sub-batch streams that must sit on four DIFFERENT hardware queues (two streams on one queue take
// turns kernel by kernel: 0.37 s instead of 0.25 s per step measured under torchrun, where RCCL brings streams of its
// own; see also the note in cvo_ctx_create).  HIP deals streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and
// reads that variable once, when the runtime initialises - i.e. at the process's first HIP call.  So:
//   * the library never writes the process environment: how many hardware queues HIP opens is the host's (or the
//     machine's) choice; cvo_process_hint_hw_queues() only reports the value in force (4 when nothing is set);
//   * cvo_ctx_create checks what the variable says NOW and, below 8, leaves an advisory text in cvo_ctx_advice() and
//     prints it once per process (stderr).
extern "C" int cvo_process_hint_hw_queues(void) {
  const char* q = std::getenv("GPU_MAX_HW_QUEUES");
  return q ? atoi(q) : 4;
}

namespace {

Dims make_dims(int N, int M) {
  Dims d{};
  d.Mpad = (int)align_up((size_t)M, 512);
  d.nchunks = d.Mpad / 64;
  d.rbw_max = (int)align_up((size_t)(d.nchunks + 31) / 32, 4);  // slice bits per row, enough for T = 1
  d.nblk_assoc = (N + ASSOC_THREADS - 1) / ASSOC_THREADS;
  d.NG = (N + ROWS_PER_GROUP - 1) / ROWS_PER_GROUP;
  d.NGpad = (int)align_up((size_t)d.NG, 64) + 64;
  d.Npad = (int)align_up((size_t)N, ROW_PAD);
  return d;
}

// THE list of the regions of one pair's workspace: points the descriptor's pointers at the slot that begins at `base` and
// returns the slot's size.  Sizing a slot is the same walk from base 0 into a descriptor nobody uses (plan_batch).  N:
// the call's largest source cloud, d: make_dims of the call's largest clouds; every region ends on a multiple of 256 bytes.
size_t place_regions(PairDesc& D, uintptr_t base, int N, const Dims& d, int Kmax, int trace_capacity, bool long_lists) {
  ScratchLayout l((const void*)base);
  const size_t n = (size_t)N, words = (n + 63) / 64, nba = (size_t)d.nblk_assoc;
  // the row arrays of the per-iteration kernels first, at the fixed offsets of cvo_device.h (row_off_*)
  l.at(D.cand_cnt, row_off_cand_cnt(d.Npad));
  l.at(D.ip, row_off_ip(d.Npad));
  l.at(D.nnz_row, row_off_nnz(d.Npad));
  l.at(D.xp4, row_off_xp4(d.Npad));
  l.at(D.cand_j, row_off_cand_j(d.Npad));  // ASSOC_CAP16 x u16 == ASSOC_CAP32 x i32 == 128 bytes per row
  l.off = row_off_ell(d.Npad);
  l.take(D.ell, (size_t)d.Npad * Kmax);
  l.take(D.ell_j, (size_t)d.Npad * Kmax);
  l.take(D.ycull, (size_t)d.Mpad);
  l.take(D.xcull, n + XCULL_PAD);
  l.take(D.gbox, 2 * (size_t)d.NGpad);
  l.take(D.cellbox, 2 * (size_t)(d.NGpad / 16));
  l.take(D.sbox, 2 * (size_t)d.nchunks);
  l.take(D.masks, (n + 8) * d.nchunks);
  l.take(D.rowbits, (size_t)(N + 4) * d.rbw_max);
  l.take(D.row_cnt, n);
  l.take(D.tile_count, 1);
  l.take(D.ovf_rows, n);
  l.take(D.ovf_bits, words + 4);
  l.take(D.gate, 1);
  l.take(D.gate_flow, 1);
  l.take(D.dense_off, n);
  l.take(D.dense_rel, n);
  l.take(D.ovf_wsum, words + 4);
  l.take(D.word_base, words + 5);
  l.take(D.done, 1);
  l.take(D.rowperm, n);
  l.take(D.iorig, n);
  l.take(D.long_stamp, n);
  if (long_lists) l.take(D.long_j, n * LONG_CAP);
  l.take(D.rowres, n);
  // (rows x the pair's own coefficient split, coeff_split(): one slice above 4096 points, at most 32768 / rows below)
  l.take(D.rowcoef, 4 * (size_t)std::max(N, 32768));
  l.take(D.flow_part, FLOW_GRANULES * nba);
  l.take(D.cnt_part, 4 * nba);
  l.take(D.coef_part, COEF_GRANULES * nba * COEFF_SPLIT_MAX);  // (the coefficient phase uses the association's row blocks)
  l.take(D.shadow, SHADOW_WORDS);
  if (trace_capacity > 0) l.take(D.trace, (size_t)trace_capacity);
  return l.off;
}

void drop_graphs(cvo_ctx* c) {
  auto drop = [](CachedGraph& cg) {
    if (cg.exec) (void)hipGraphExecDestroy(cg.exec);
    cg.exec = nullptr;
  };
  for (auto& group : c->graphs)
    for (CachedGraph& cg : group) drop(cg);
  drop(c->chain_graph);
}

int ensure_workspace(cvo_ctx* c, int n_pairs, size_t bytes_per_pair) {
  // (no stream to drain: no call is in flight on this context, every call ends synchronised)
  int rc = CVO_OK;
  bool moved = false;
  if (n_pairs > c->cap_pairs) {
    const size_t n = (size_t)n_pairs;
    c->cap_pairs = 0;
    rc = c->d_ctl.lay_out(c, "control block", control_block_list(c->d_params, c->d_status, c->d_descs, c->d_states, n), nullptr, &moved);
    if (rc == CVO_OK) rc = c->h_ctl.lay_out(c, "control block staging", control_block_list(c->s_params, c->s_status, c->s_descs, c->s_states, n), nullptr);
    for (int i = 0; i < 2 && rc == CVO_OK; i++) rc = c->h_status[i].reserve(c, sizeof(int) * 2 * n, "status mirror", nullptr);
    if (rc == CVO_OK) c->cap_pairs = n_pairs;
  }
  if (rc == CVO_OK) rc = c->arena.reserve(c, bytes_per_pair * (size_t)n_pairs, "workspace", nullptr, &moved);
  if (moved) drop_graphs(c);  // (they hold the pointers)
  return rc;
}

int coeff_split(int n) {
  int s = 1;
  while (s < 8 && (long)n * (2 * s) <= 8192) s *= 2;
  // tiny clouds (the dense regime walks hundreds of entries per row): a few more slices as long as the launch stays small
  while (s >= 8 && s < COEFF_SPLIT_MAX && (long)n * (2 * s) <= 32768) s *= 2;
  return s;
}
}  // namespace

extern "C" {

const char* cvo_version(void) { return CVO_VERSION_STRING; }

void cvo_params_default(cvo_params_t* p) {
  // CvoParams::CvoParams(), CvoParams.hpp:75-126
  std::memset(p, 0, sizeof(*p));
  p->ell_init_first_frame = 0.5f;
  p->ell_init = 0.5f;
  p->ell_min = 0.05f;
  p->min_ell_iter_limit = 1;
  p->ell_max = 1.2f;
  p->dl = 0;
  p->dl_step = 0.3;
  p->sigma = 0.1f;
  p->sp_thres = 0.0006f;
  p->c = 7.0f;
  p->d = 7.0f;
  p->c_ell = 0.15f;
  p->c_sigma = 0.6f;
  p->s_ell = 0.1f;
  p->s_sigma = 0.8f;
  p->MAX_ITER = 10000;
  p->min_step = 2e-5f;
  p->eps = 0.00005f;
  p->eps_2 = 0.000012f;
  p->max_step = 0.8f;  // uninitialised upstream; see DESIGN.md
  p->step = 0.f;       // uninitialised upstream, unused by the path
  p->ell_decay_rate = 0.9f;
  p->ell_decay_rate_first_frame = 0.99f;
  p->ell_decay_start = 30;
  p->ell_decay_start_first_frame = 300;
  p->indicator_window_size = 15;
  p->indicator_stable_threshold = 0.2f;
  p->is_pcl_visualization_on = 0;
  p->is_using_least_square = 0;
  p->is_ell_adaptive = 0;
  p->is_full_ip_matrix = 0;
  p->is_using_geometry = 1;
  p->is_using_intensity = 0;
  p->is_using_semantics = 0;
  p->is_using_range_ell = 0;
  p->is_using_kdtree = 0;
  p->is_using_geometric_type = 0;
  p->is_exporting_association = 0;
  p->multiframe_using_cpu = 1;
  p->multiframe_max_iters = 200;
  p->nearest_neighbors_max = 512;
  p->multiframe_ell_init = 0.15f;
  p->multiframe_ell_min = 0.05f;
  p->multiframe_iter_per_ell = 10;
  p->multiframe_ell_decay_rate = 0.7f;
  p->multiframe_iterations_per_ell = 50;
  p->multiframe_iterations_per_solve = 8;
  p->multiframe_downsample_voxel_size = 0.5f;
  p->multiframe_expected_points = 1000;
  p->multiframe_num_neighbors = 128;
  p->multiframe_min_nonzeros = 300;
  p->multiframe_least_squares_num_threads = 24;
}

// The streams of a context - group 0 (= the context's stream), seven more sub-batch streams, the upload stream - are
// handed back to a per-device pool when the context is destroyed and reused, in the same roles, by the next context of
// that device.  HIP deals streams onto hardware queues as they are first used; a context created after another one had
// been DESTROYED found its four sub-batch streams sharing queues (214 ms instead of 64 ms per headline step,
// scripts/upload_probe.py) however carefully it ordered their creation.  Streams that are never destroyed keep the
// queues the first context's careful order gave them.  Contexts alive at the same time still get streams of their own.
namespace {
struct StreamSet {
  hipStream_t g[cvo_ctx::MAX_GROUPS] = {};
  hipStream_t upload = nullptr;
};
std::mutex g_stream_pool_mutex;
std::map<int, std::vector<StreamSet>> g_stream_pool;
}  // namespace

int cvo_ctx_create(int device, cvo_ctx** out) {
  if (!out) return CVO_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return CVO_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return CVO_E_HIP;
  cvo_ctx* c = new cvo_ctx();
  c->device = device;
  for (const OptionSpec& o : kOptions)  // the ONLY place the library reads the environment
    if (const char* v = std::getenv((std::string("CVO_") + o.name).c_str())) parse_option(c->opt, o, v);
  bool pooled = false;
  {
    std::lock_guard<std::mutex> lk(g_stream_pool_mutex);
    auto& pool = g_stream_pool[device];
    if (!pool.empty()) {
      const StreamSet ss = pool.back();
      pool.pop_back();
      for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++) c->gstream[g] = ss.g[g];
      c->stream = ss.g[0];
      c->upload_stream = ss.upload;
      pooled = true;
    }
  }
  bool ok = (pooled || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess) &&
            // (nothing here may run on the NULL stream - a synchronous hipMemset, say: its hardware queue would then be the
            // first one this process creates - see the note on the sub-batch streams below)
            hipEventCreate(&c->ev_start) == hipSuccess &&
            hipEventCreate(&c->ev_stop) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
  {  // the hardware-queue contract (top of this file)
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    const int nq = q ? atoi(q) : 4;
    if (nq < 8) {
      char msg[400];
      snprintf(msg, sizeof msg,
               "GPU_MAX_HW_QUEUES is %s%s: batches run on four sub-batch streams next to the upload stream and whatever "
               "RCCL / the host application adds; with fewer than 8 hardware queues streams share a queue and take turns "
               "(measured: 0.37 s instead of 0.25 s per 64-pair step under torchrun); the count is fixed at the process's "
               "first HIP call",
               q ? q : "unset (HIP's default: 4)", "");
      c->advice = msg;
      static std::atomic<bool> said{false};
      if (!said.exchange(true) && !std::getenv("CVO_QUIET")) fprintf(stderr, "[cvo] advice: %s\n", msg);
    }
  }
  c->gstream[0] = c->stream;
  for (int g = 0; ok && g < cvo_ctx::MAX_GROUPS; g++) {
    if (g && !pooled) ok = ok && hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2; i++) ok = ok && hipEventCreateWithFlags(&c->ev_chk[i][g], hipEventDisableTiming) == hipSuccess;
  }
  // HIP binds a stream to a hardware queue when the stream is first USED, in the order of first use, and the four
  // sub-batch streams of a batch must sit on four different compute pipes (two of them on one pipe take turns kernel by
  // kernel: 205 ms instead of 69 ms per step for the headline batch, measured when a process's first context uploaded
  // its clouds - a pool of temporary streams - before its first solve).  So the sub-batch streams are touched here, in
  // order, before any other stream of this context exists.
  for (int g = 0; ok && g < 4; g++) {
    hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, c->gstream[g], 0ull);
    ok = ok && hipGetLastError() == hipSuccess;
  }
  for (int g = 0; ok && g < 4; g++) ok = ok && hipStreamSynchronize(c->gstream[g]) == hipSuccess;
  if (!pooled) ok = ok && hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking) == hipSuccess;
  // k_kd_order keeps the keys of a whole cloud in LDS: up to 128 KB of dynamic shared memory
  ok = ok && hipFuncSetAttribute((const void*)k_kd_order, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(sizeof(unsigned long long) * KD_MAX_POINTS)) == hipSuccess;
  // ... and k_kd_wide_leaves those of a leaf: as much with WIDE_LEAF at its maximum
  ok = ok && hipFuncSetAttribute((const void*)k_kd_wide_leaves, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(sizeof(unsigned long long) * KD_MAX_POINTS)) == hipSuccess;
  if (!ok) {
    cvo_ctx_destroy(c);
    return CVO_E_HIP;
  }
  *out = c;
  return CVO_OK;
}

static void queue_release(cvo_batch_queue* q);

void cvo_ctx_destroy(cvo_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // an open batch queue goes first: its streams are drained, its pinned block freed and the handle orphaned - the host
  // object stays until its owner calls cvo_batch_close, every other call on it returns CVO_E_INVALID
  if (c->queue) queue_release(c->queue);
  // every stream of the set must be idle before the workspace goes (work queued by a call that returned early on an
  // error would otherwise run against freed memory) - and a set whose streams cannot be drained is not pooled
  bool drained = true;
  for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++)
    if (c->gstream[g]) drained = (hipStreamSynchronize(c->gstream[g]) == hipSuccess) && drained;
  if (c->upload_stream) drained = (hipStreamSynchronize(c->upload_stream) == hipSuccess) && drained;
  drop_graphs(c);
  for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++) {
    for (int i = 0; i < 2; i++)
      if (c->ev_chk[i][g]) (void)hipEventDestroy(c->ev_chk[i][g]);
    if (c->ev_join[g]) (void)hipEventDestroy(c->ev_join[g]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_start) (void)hipEventDestroy(c->ev_start);
  if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
  {  // a complete, drained set goes back to the device's pool (see StreamSet); anything else is destroyed
    bool complete = drained && c->upload_stream != nullptr;
    for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++) complete = complete && c->gstream[g] != nullptr;
    if (complete) {
      StreamSet ss;
      for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++) ss.g[g] = c->gstream[g];
      ss.upload = c->upload_stream;
      std::lock_guard<std::mutex> lk(g_stream_pool_mutex);
      g_stream_pool[c->device].push_back(ss);
    } else {
      for (int g = 1; g < cvo_ctx::MAX_GROUPS; g++)
        if (c->gstream[g]) (void)hipStreamDestroy(c->gstream[g]);
      if (c->stream) (void)hipStreamDestroy(c->stream);
      if (c->upload_stream) (void)hipStreamDestroy(c->upload_stream);
    }
  }
  delete c;  // (every region the context owns goes with it)
}

void cvo_shutdown(void) {
  // the pooled stream sets of destroyed contexts (contexts still alive keep theirs)
  std::lock_guard<std::mutex> lk(g_stream_pool_mutex);
  for (auto& kv : g_stream_pool) {
    (void)hipSetDevice(kv.first);
    for (StreamSet& ss : kv.second) {
      for (int g = 0; g < cvo_ctx::MAX_GROUPS; g++)
        if (ss.g[g]) (void)hipStreamDestroy(ss.g[g]);
      if (ss.upload) (void)hipStreamDestroy(ss.upload);
    }
    kv.second.clear();
  }
}

int cvo_ctx_set_option(cvo_ctx* ctx, const char* name, const char* value) {
  if (!ctx || !name) return CVO_E_INVALID;
  if (std::strncmp(name, "CVO_", 4) == 0) name += 4;
  const OptionSpec* spec = std::find_if(std::begin(kOptions), std::end(kOptions), [&](const OptionSpec& o) { return std::strcmp(o.name, name) == 0; });
  if (spec == std::end(kOptions)) return fail(ctx, CVO_E_INVALID, std::string("cvo_ctx_set_option: unknown option ") + name);
  // (an open queue has chunks in flight on graphs that bake the switches in, and re-captures from its own copy of them)
  if (ctx->queue_open) return fail(ctx, CVO_E_INVALID, "cvo_ctx_set_option: a batch queue is open on this context (cvo_batch_close it first)");
  parse_option(ctx->opt, *spec, value);
  drop_graphs(ctx);  // cached graphs bake some of the switches in
  return CVO_OK;
}

const char* cvo_last_error(const cvo_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
const char* cvo_ctx_advice(const cvo_ctx* ctx) { return ctx ? ctx->advice.c_str() : ""; }
void* cvo_ctx_stream(cvo_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int cvo_ctx_synchronize(cvo_ctx* ctx) {
  if (!ctx) return CVO_E_INVALID;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CVO_OK;
}

// Spatial permutation of a cloud (sorted position -> original index): a balanced k-d ordering whose
// splits fall on multiples of 512 / 64 / 4 points, so that every aligned run of 512, 64 (a k_scan

}  // extern "C"
