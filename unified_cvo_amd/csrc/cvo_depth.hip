// cvo_depth.hip -- the keyframe depth filter (main_depth_filtering.cpp:208-298) on the device: cvo_depth_filter_open (the
// keyframe's rows in original order into a region the filter owns, by k_cloud_unpack; a resident copy of the keyframe made
// of those rows, so that the caller's handle is never needed again), cvo_depth_filter_add (one frame: the non-isotropic
// association by run_single_eval, then k_depth_accumulate on the matrix where the evaluation left it), cvo_depth_filter_state,
// cvo_depth_filter_finish (k_depth_finish, the ordered compaction of the keep flags, the ingest of cvo_ingest.hip through the
// kept indices where they are), cvo_depth_filter (all of it in one call) and the CPU twin's two functions, which need no
// context.  No association, frame or row comes down to the host; what does: the compaction's total and the non-finite count
// (8 bytes), what the ordering route of the result brings down (cvo_cloud_from_device's rule), and the arrays a caller asks for.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.  Shared declarations: cvo_internal.h.

// The filter.  It holds everything it reads: its own region and `kf`, a resident cloud built from the keyframe's rows (the
// cloud cvo_cloud_from_device makes of them: the keyframe's spatial order, one-hot detection and bits).  The keyframe handle
// given to open may be freed right after open returns.  The context must outlive the filter.
struct cvo_depth_filter_s {
  cvo_ctx* ctx = nullptr;
  int n = 0;          // keyframe rows
  int present = 0;    // CVO_CLOUD_HAS_* of the keyframe
  int frames = 0;     // adds that ran an evaluation
  cvo_cloud* kf = nullptr;
  DeviceRegion region;
  UnpackJob* d_job = nullptr;
  // the keyframe's rows, original order (k_cloud_unpack's padded rows), and the copy of the coordinates finish moves
  float *xyz = nullptr, *xyz_out = nullptr;
  float4 *feat = nullptr, *label = nullptr;
  float2* geo = nullptr;
  // the state, original order
  float *depth_sum = nullptr, *weight_sum = nullptr;
  int* count = nullptr;
  // finish: refined depth and flag per row, the kept rows and their depths, the compaction's block counts, [total, n_nonfinite]
  float *depth = nullptr, *depth_kept = nullptr;
  unsigned char* flag = nullptr;
  int* kept = nullptr;
  unsigned *blocks = nullptr, *ctl = nullptr;
  unsigned* bad = nullptr;  // set by k_depth_accumulate when the matrix it reads is corrupt; read after every add
  bool broken = false;      // ... and then the state is no longer the statement's: every later call but close is refused
  // the evaluation of the last add (PairDesc::call_serial, 0: none) and its neighbour budget: what cvo_debug_depth_filter_rows goes by
  unsigned long long last_serial = 0;
  int last_K = 0;
};

namespace {

// THE list of the filter's region
auto depth_region_list(cvo_depth_filter_t& f) {
  return [&f](ScratchLayout& l) {
    const size_t nn = (size_t)std::max(f.n, 1);
    l.take(f.d_job, 1);
    unpacked_rows_list(l, f.present, nn, f.xyz, f.feat, f.label, f.geo);
    l.take(f.xyz_out, 3 * nn);
    l.take(f.depth_sum, nn);
    l.take(f.weight_sum, nn);
    l.take(f.count, nn);
    l.take(f.depth, nn);
    l.take(f.depth_kept, nn);
    l.take(f.flag, nn);
    l.take(f.kept, nn);
    l.take(f.blocks, (nn + COMPACT_THREADS - 1) / COMPACT_THREADS);
    l.take(f.ctl, 2);
    l.take(f.bad, 1);
  };
}

// the filter's rows as ingest rows: `xyz` is either copy of the coordinates
cvo_device_rows_t depth_rows(const cvo_depth_filter_t& f, const float* xyz, int n, const int* rows) {
  return device_rows(n, f.n, xyz, f.feat, FD_PAD, f.label, NC_PAD, f.geo, rows);
}

// the body of cvo_depth_filter_open under upload_mutex; staged: the filter's resident keyframe (none of an empty one), or what to release
int depth_open_locked(cvo_ctx* ctx, const cvo_cloud* keyframe, cvo_depth_filter_t& f, std::vector<StagedCloud>& staged) {
  const char* who = "cvo_depth_filter_open";
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  f.ctx = ctx;
  f.n = keyframe->n;
  f.present = cloud_present(keyframe);
  if (f.n == 0) return CVO_OK;  // (nothing to hold: add is a no-op, finish ingests no row)
  int rc = f.region.lay_out(ctx, "depth filter", depth_region_list(f), nullptr);
  if (rc != CVO_OK) return rc;
  const hipStream_t st = ctx->upload_stream;
  std::vector<UnpackJob> jobs;  // (alive until the synchronisation below)
  if ((rc = unpack_launch(ctx, 1, &keyframe, nullptr, jobs, f.d_job, UnpackOut{1, f.n, f.xyz, f.feat, f.label, f.geo})) != CVO_OK) return rc;
  const size_t nn = (size_t)f.n;
  HIP_TRY(ctx, hipMemsetAsync(f.depth_sum, 0, sizeof(float) * nn, st));
  HIP_TRY(ctx, hipMemsetAsync(f.weight_sum, 0, sizeof(float) * nn, st));
  HIP_TRY(ctx, hipMemsetAsync(f.count, 0, sizeof(int) * nn, st));
  HIP_TRY(ctx, hipMemsetAsync(f.bad, 0, sizeof(unsigned), st));
  // the filter's own resident keyframe, from the rows where they are
  const cvo_device_rows_t d = depth_rows(f, f.xyz, f.n, nullptr);
  rc = ingest_device_clouds(ctx, 1, &d, staged, who);  // (synchronises upload_stream; on error the cloud is released)
  if (rc != CVO_OK) (void)hipStreamSynchronize(st);
  return rc;
}

// everything cvo_depth_filter_add can refuse, before anything is written
int depth_add_check(cvo_depth_filter_t* df, const cvo_params_t* params, const cvo_cloud* frame, const float* T, const float* T_depth,
                    const float* kernel, const char* who) {
  cvo_ctx* ctx = df ? df->ctx : nullptr;
  if (!df || !params || !T || !T_depth || !kernel) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (!frame) return fail(ctx, CVO_E_INVALID, std::string(who) + ": null cloud");
  if (frame->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the frame belongs to another context");
  if (ctx->queue_open) return fail(ctx, CVO_E_INVALID, "a batch queue is open on this context (cvo_batch_close it first)");
  if (df->broken) return fail(ctx, CVO_E_INVALID, std::string(who) + ": an earlier add found a corrupt matrix; close the filter");
  for (int q = 0; q < 16; q++)
    if (!std::isfinite(T_depth[q])) return fail(ctx, CVO_E_INVALID, std::string(who) + ": non-finite T_depth");
  return CVO_OK;
}

// one frame into the accumulators; the arguments have been checked
int depth_add(cvo_depth_filter_t* df, const cvo_params_t* params, const cvo_cloud* frame, const float T[16], const float T_depth[16],
              const float kernel_colmajor[9]) {
  cvo_ctx* ctx = df->ctx;
  if (df->n == 0 || frame->n == 0) return CVO_OK;  // (as cvo_association_non_isotropic: no pair)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  float extra[10];
  noniso_extra(params, kernel_colmajor, extra);
  BatchSetup S;
  int rc = run_single_eval(ctx, params, df->kf, frame, T, 1.0f, &S, extra);
  if (rc != CVO_OK) return rc;
  const int N = df->n, K = ctx->last_params.K_max;
  hipLaunchKernelGGL(k_depth_accumulate, dim3((unsigned)((N + DEPTH_THREADS - 1) / DEPTH_THREADS)), dim3(DEPTH_THREADS), 0, ctx->stream,
                     (const PairDesc*)ctx->d_descs, K, (size_t)N * (size_t)K, (const float4*)frame->x4, frame->n, depth_row(T_depth), N,
                     df->depth_sum, df->weight_sum, df->count, df->bad);
  HIP_TRY(ctx, hipGetLastError());
  unsigned bad = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&bad, df->bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (finish reads the state on the upload stream; the frame may be freed on return)
  if (bad) {  // (as fetch_ell_values / fetch_ell refuse such a matrix; rows before the bad one have been folded)
    df->broken = true;
    return fail(ctx, CVO_E_HIP, "cvo_depth_filter_add: corrupt kernel matrix (a row, slot or column out of range); the filter's state is lost");
  }
  df->frames++;
  df->last_K = K;
  df->last_serial = ctx->h_descs[0].call_serial;
  return CVO_OK;
}

// the body of cvo_depth_filter_finish under upload_mutex; staged: the result, or what to release
int depth_finish_locked(cvo_depth_filter_t* df, int min_count, std::vector<StagedCloud>& staged, int* kept, float* depth, int* n_kept,
                        int* n_nonfinite) {
  const char* who = "cvo_depth_filter_finish";
  cvo_ctx* ctx = df->ctx;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n = df->n;
  unsigned h_ctl[2] = {0u, 0u};
  if (n > 0) {
    const hipStream_t st = ctx->upload_stream;
    HIP_TRY(ctx, hipMemsetAsync(df->ctl, 0, sizeof(unsigned) * 2, st));
    hipLaunchKernelGGL(k_depth_finish, dim3((unsigned)((n + DEPTH_THREADS - 1) / DEPTH_THREADS)), dim3(DEPTH_THREADS), 0, st, n, min_count,
                       (const float*)df->xyz, (const float*)df->depth_sum, (const float*)df->weight_sum, (const int*)df->count, df->xyz_out,
                       df->depth, df->flag, df->ctl + 1);
    HIP_TRY(ctx, hipGetLastError());
    const DepthKept pred{df->flag, df->depth, df->kept, df->depth_kept};
    int rc = compact(ctx, n, pred, df->blocks, scan_into(ctx, df->ctl));
    if (rc != CVO_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_ctl, df->ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if ((rc = compact_check(ctx, h_ctl[0], n, who, "rows")) != CVO_OK) return rc;
  }
  const int nk = (int)h_ctl[0];
  const cvo_device_rows_t d = depth_rows(*df, df->xyz_out, nk, df->kept);
  int rc = ingest_device_clouds(ctx, 1, &d, staged, who);  // (synchronises upload_stream)
  if (rc != CVO_OK) return rc;
  if (nk > 0 && kept) HIP_TRY(ctx, hipMemcpy(kept, df->kept, sizeof(int) * (size_t)nk, hipMemcpyDeviceToHost));
  if (nk > 0 && depth) HIP_TRY(ctx, hipMemcpy(depth, df->depth_kept, sizeof(float) * (size_t)nk, hipMemcpyDeviceToHost));
  if (n_kept) *n_kept = nk;
  if (n_nonfinite) *n_nonfinite = (int)h_ctl[1];
  return CVO_OK;
}

int depth_finish(cvo_depth_filter_t* df, int min_count, cvo_cloud** out, int* kept, float* depth, int* n_kept, int* n_nonfinite) {
  const char* who = "cvo_depth_filter_finish";
  cvo_ctx* ctx = df->ctx;
  const int rc = handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) {
    return depth_finish_locked(df, min_count, staged, kept, depth, n_kept, n_nonfinite);
  });
  if (rc != CVO_OK) {
    if (n_kept) *n_kept = 0;
    if (n_nonfinite) *n_nonfinite = 0;
  }
  return rc;
}

int depth_open(cvo_ctx* ctx, const cvo_cloud* keyframe, cvo_depth_filter_t** out, const char* who) {
  if (keyframe->n > COMPACT_MAX_ELEMENTS) return fail(ctx, CVO_E_UNSUPPORTED, std::string(who) + ": more than 2^24 rows");
  cvo_depth_filter_t* f = nullptr;
  cvo_cloud* kf = nullptr;  // (the hand-over frame's `out` is the filter's keyframe here)
  const int rc = handover_call(ctx, who, &kf, [&](std::vector<StagedCloud>& staged) {
    f = new cvo_depth_filter_t();
    return depth_open_locked(ctx, keyframe, *f, staged);
  });
  if (rc != CVO_OK) {
    delete f;
    return rc;
  }
  f->kf = kf;
  *out = f;
  return CVO_OK;
}

void depth_close(cvo_depth_filter_t* df) {
  if (!df) return;
  if (df->kf) cvo_cloud_free(df->kf);
  delete df;  // (every call that used the region synchronised before it returned)
}

}  // namespace

extern "C" {

int cvo_depth_filter_open(cvo_ctx* ctx, const cvo_cloud* keyframe, cvo_depth_filter_t** out) {
  const char* who = "cvo_depth_filter_open";
  if (out) *out = nullptr;
  if (!ctx || !out) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (!keyframe) return fail(ctx, CVO_E_INVALID, std::string(who) + ": null cloud");
  if (keyframe->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the keyframe belongs to another context");
  return depth_open(ctx, keyframe, out, who);
}

int cvo_depth_filter_add(cvo_depth_filter_t* df, const cvo_params_t* params, const cvo_cloud* frame, const float T[16],
                         const float T_depth[16], const float kernel_colmajor[9]) {
  const int rc = depth_add_check(df, params, frame, T, T_depth, kernel_colmajor, "cvo_depth_filter_add");
  if (rc != CVO_OK) return rc;
  return depth_add(df, params, frame, T, T_depth, kernel_colmajor);
}

int cvo_depth_filter_size(const cvo_depth_filter_t* df) { return df ? df->n : 0; }

int cvo_depth_filter_state(cvo_depth_filter_t* df, float* depth_sum, float* weight_sum, int* count) {
  if (!df) return fail(nullptr, CVO_E_INVALID, "cvo_depth_filter_state: bad argument");
  cvo_ctx* ctx = df->ctx;
  if (df->broken) return fail(ctx, CVO_E_INVALID, "cvo_depth_filter_state: an earlier add found a corrupt matrix; close the filter");
  if (df->n == 0) return CVO_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)df->n;
  if (depth_sum) HIP_TRY(ctx, hipMemcpy(depth_sum, df->depth_sum, sizeof(float) * nn, hipMemcpyDeviceToHost));
  if (weight_sum) HIP_TRY(ctx, hipMemcpy(weight_sum, df->weight_sum, sizeof(float) * nn, hipMemcpyDeviceToHost));
  if (count) HIP_TRY(ctx, hipMemcpy(count, df->count, sizeof(int) * nn, hipMemcpyDeviceToHost));
  return CVO_OK;
}

int cvo_depth_filter_finish(cvo_depth_filter_t* df, int min_count, cvo_cloud** out, int* kept, float* depth, int* n_kept,
                            int* n_nonfinite) {
  if (out) *out = nullptr;
  if (n_kept) *n_kept = 0;
  if (n_nonfinite) *n_nonfinite = 0;
  if (!df) return fail(nullptr, CVO_E_INVALID, "cvo_depth_filter_finish: bad argument");
  if (!out) return fail(df->ctx, CVO_E_INVALID, "cvo_depth_filter_finish: bad argument");
  if (df->broken) return fail(df->ctx, CVO_E_INVALID, "cvo_depth_filter_finish: an earlier add found a corrupt matrix; close the filter");
  if (min_count < 0) return fail(df->ctx, CVO_E_INVALID, "cvo_depth_filter_finish: min_count < 0");
  return depth_finish(df, min_count, out, kept, depth, n_kept, n_nonfinite);
}

void cvo_depth_filter_close(cvo_depth_filter_t* df) { depth_close(df); }

int cvo_depth_filter(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* keyframe, int n_frames,
                     const cvo_cloud* const* frames, const float* T, const float* T_depth, const float kernel_colmajor[9],
                     int min_count, cvo_cloud** out, int* kept, float* depth, int* n_kept, int* n_nonfinite) {
  const char* who = "cvo_depth_filter";
  if (out) *out = nullptr;
  if (n_kept) *n_kept = 0;
  if (n_nonfinite) *n_nonfinite = 0;
  if (!ctx || !params || !out || n_frames < 0 || !kernel_colmajor || (n_frames > 0 && (!frames || !T || !T_depth)))
    return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (!keyframe) return fail(ctx, CVO_E_INVALID, std::string(who) + ": null cloud");
  if (keyframe->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the keyframe belongs to another context");
  if (min_count < 0) return fail(ctx, CVO_E_INVALID, std::string(who) + ": min_count < 0");
  cvo_depth_filter_t probe;  // (the checks of add need a filter's context only)
  probe.ctx = ctx;
  for (int q = 0; q < n_frames; q++) {
    const int rc = depth_add_check(&probe, params, frames[q], T + 16 * (size_t)q, T_depth + 16 * (size_t)q, kernel_colmajor, who);
    if (rc != CVO_OK) return rc;
  }
  cvo_depth_filter_t* df = nullptr;
  int rc = depth_open(ctx, keyframe, &df, who);
  for (int q = 0; rc == CVO_OK && q < n_frames; q++)
    rc = depth_add(df, params, frames[q], T + 16 * (size_t)q, T_depth + 16 * (size_t)q, kernel_colmajor);
  if (rc == CVO_OK) rc = depth_finish(df, min_count, out, kept, depth, n_kept, n_nonfinite);
  depth_close(df);
  return rc;
}

// How the rows of the last add's matrix were stored (by position): rows with no entry, rows in the slot-major matrix the
// thread-per-row kernels wrote, rows the wave-per-row kernels wrote slot-major (NNZ_DENSE_FLAG, dense_off < 0) and as
// row-major runs (dense_off >= 0), rows that hold exactly the neighbour budget K (cut there, or just full), the longest row,
// and the rows k_assoc_dense gave a whole block (its wide_row predicate, restated over what the launch was given: the wide
// instantiation, at most a block's worth of overflow rows, the row's candidate count k_list left in xp4.w - or, beyond a long
// list, all M targets - in (256, 4 x 304]).  Only while the context's last evaluation IS this filter's last add (its
// call serial); any pointer may be NULL.
int cvo_debug_depth_filter_rows(cvo_depth_filter_t* df, int* n_empty, int* n_list, int* n_dense_slot, int* n_run, int* n_full,
                                int* max_nnz, int* K, int* n_wide) {
  if (!df) return fail(nullptr, CVO_E_INVALID, "cvo_debug_depth_filter_rows: bad argument");
  cvo_ctx* ctx = df->ctx;
  if (df->last_serial == 0 || df->n == 0 || ctx->last_pairs < 1 || ctx->h_descs[0].call_serial != df->last_serial)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_depth_filter_rows: the context's last evaluation is not an add of this filter");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const PairDesc& D = ctx->h_descs[0];
  const PairState& st = ctx->h_states[0];
  const size_t nn = (size_t)df->n;
  std::vector<unsigned> nnz(nn, 0u);
  std::vector<int> off(nn, -1);
  std::vector<float4> xp(nn);
  HIP_TRY(ctx, hipMemcpy(nnz.data(), D.nnz_row, sizeof(unsigned) * nn, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(off.data(), D.dense_off, sizeof(int) * nn, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(xp.data(), D.xp4, sizeof(float4) * nn, hipMemcpyDeviceToHost));
  const bool wide_mode = ctx->last.geom.wide && st.n_ovf <= ctx->last.geom.dense_blocks;
  const bool long_lists = !st.all_dense && ctx->last_params.long_lists != 0 && D.long_j != nullptr;
  int e = 0, l = 0, ds = 0, r = 0, fu = 0, mx = 0, w = 0;
  for (size_t q = 0; q < nn; q++) {
    const unsigned v = nnz[q];
    const int c = std::min((int)nnz_count(v), df->last_K);
    mx = std::max(mx, c);
    if (c == df->last_K) fu++;
    if (v & NNZ_DENSE_FLAG) {
      int cnt;
      std::memcpy(&cnt, &xp[q].w, sizeof cnt);
      const int n_cand = long_lists && cnt <= LONG_CAP ? cnt : D.M;
      if (wide_mode && n_cand > 256 && n_cand <= 4 * 304) w++;  // (WIDE_MIN, DENSE_WAVES x WIDE_CAP of k_assoc_dense)
    }
    if (c == 0) e++;
    else if (!(v & NNZ_DENSE_FLAG)) l++;
    else if (off[q] >= 0) r++;
    else ds++;
  }
  if (n_empty) *n_empty = e;
  if (n_list) *n_list = l;
  if (n_dense_slot) *n_dense_slot = ds;
  if (n_run) *n_run = r;
  if (n_full) *n_full = fu;
  if (max_nnz) *max_nnz = mx;
  if (K) *K = df->last_K;
  if (n_wide) *n_wide = w;
  return CVO_OK;
}

// ---- the CPU twin: pure arithmetic over an association the caller already has ----

int cvo_depth_filter_accumulate_host(int n_rows, const int* row_ptr, const int* col, const float* val, int n_target,
                                     const float* target_xyz, const float T_depth[16], float* depth_sum, float* weight_sum, int* count) {
  if (n_rows < 0 || n_target < 0 || !row_ptr || !T_depth || (n_rows > 0 && (!depth_sum || !weight_sum || !count))) return CVO_E_INVALID;
  if (row_ptr[0] != 0) return CVO_E_INVALID;
  for (int i = 0; i < n_rows; i++)
    if (row_ptr[i + 1] < row_ptr[i]) return CVO_E_INVALID;
  const int nnz = row_ptr[n_rows];
  if (nnz > 0 && (!col || !val || !target_xyz)) return CVO_E_INVALID;
  for (int e = 0; e < nnz; e++)
    if (col[e] < 0 || col[e] >= n_target) return CVO_E_INVALID;
  const DepthRow t = depth_row(T_depth);
  for (int i = 0; i < n_rows; i++)
    for (int e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
      const float* y = target_xyz + 3 * (size_t)col[e];
      depth_fold(depth_sum[i], weight_sum[i], count[i], depth_zj(t, y[0], y[1], y[2]), val[e]);
    }
  return CVO_OK;
}

int cvo_depth_filter_finish_host(int n_rows, const float* xyz, const float* depth_sum, const float* weight_sum, const int* count,
                                 int min_count, float* xyz_out, int* kept, float* depth, int* n_kept, int* n_nonfinite) {
  if (n_kept) *n_kept = 0;
  if (n_nonfinite) *n_nonfinite = 0;
  if (n_rows < 0 || min_count < 0 || (n_rows > 0 && (!xyz || !depth_sum || !weight_sum || !count))) return CVO_E_INVALID;
  int nk = 0, nf = 0;
  for (int i = 0; i < n_rows; i++) {
    float out[3], d = 0.f;
    const int what = depth_finish_row(depth_sum[i], weight_sum[i], count[i], min_count, xyz + 3 * (size_t)i, out, &d);
    if (what == DEPTH_NONFINITE) nf++;
    if (what != DEPTH_KEEP) continue;
    if (xyz_out) std::memcpy(xyz_out + 3 * (size_t)nk, out, sizeof out);
    if (kept) kept[nk] = i;
    if (depth) depth[nk] = d;
    nk++;
  }
  if (n_kept) *n_kept = nk;
  if (n_nonfinite) *n_nonfinite = nf;
  return CVO_OK;
}

}  // extern "C"
