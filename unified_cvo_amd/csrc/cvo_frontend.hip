// cvo_frontend.hip -- what the front ends (cvo_voxel.hip, cvo_rgbd.hip, cvo_fast.hip, cvo_stereo.hip, cvo_lidar.hip, cvo_nlm.hip,
// cvo_sgm.hip, cvo_dfilter.hip, cvo_stereo_pair.hip) share on the host: the growable scratch regions (a front end writes ONE list of its buffers, DeviceScratch::lay_out
// sizes and binds it, draining upload_stream before the region moves: cvo_internal.h), the launches of an ordered compaction (cvo_k_compact.h) and of the radix sort (cvo_k_sort.h), the read-back of
// a compaction's total, the route rule, the frame of an entry point and the copy-out of the kept indices.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.  Shared declarations: cvo_internal.h.
//
// The entry frame, once for every front end.  A pair cvo_X_host / cvo_X is two one-line extern "C" functions over ONE
// X_entry(ctx /* nullptr: the twin */, who, ...), and an upload entry point has the same three steps:
//   validate  X_entry checks the arguments, before any lock, and refuses through fail(ctx, code, who + ": " + text): with a
//             context the text is what cvo_last_error returns, the twin returns the bare code;
//   lock      frontend_call(ctx, who, body) takes the context's upload_mutex ONCE around the body.  Whatever the body calls
//             (the routes, dfilter_run, upload_one_locked, stereo_upload_locked ...) has the contract "the caller holds
//             upload_mutex" and never enters an extern "C" function: the mutex is not recursive;
//   commit    the body chooses the route (!ctx || route_on_host(...) is the CPU twin) and, as its last statement and only with
//             a context, stores ctx->X_last = stats: a call that fails or is refused leaves the previous call's stats.

namespace {

// the scan of a compaction that leaves nothing but its total
auto scan_into(cvo_ctx* ctx, unsigned* total) {
  return [=](int nb, unsigned* blocks) {
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(COMPACT_THREADS), 0, ctx->upload_stream, nb, blocks, total);
  };
}

// An ordered compaction of n elements whose per-block counts are already in `blocks` (k_rgbd_select makes them itself):
// scan(nb, blocks) enqueues the one-block scan that turns them into offsets and leaves the total for compact_total,
// k_compact_write<P> writes the survivors.  On upload_stream, no synchronisation.
template <class P, class Scan>
int compact_counted(cvo_ctx* ctx, int n, const P& pred, unsigned* blocks, Scan scan) {
  const int nb = (n + COMPACT_THREADS - 1) / COMPACT_THREADS;
  scan(nb, blocks);
  hipLaunchKernelGGL(k_compact_write<P>, dim3(nb), dim3(COMPACT_THREADS), 0, ctx->upload_stream, n, pred, (const unsigned*)blocks);
  HIP_TRY(ctx, hipGetLastError());
  return CVO_OK;
}

// count -> scan -> write
template <class P, class Scan>
int compact(cvo_ctx* ctx, int n, const P& pred, unsigned* blocks, Scan scan) {
  hipLaunchKernelGGL(k_compact_count<P>, dim3((n + COMPACT_THREADS - 1) / COMPACT_THREADS), dim3(COMPACT_THREADS), 0, ctx->upload_stream, n, pred, blocks);
  return compact_counted(ctx, n, pred, blocks, scan);
}

// a total above n is refused as `who`: the device kept more `what` than it was given
int compact_check(cvo_ctx* ctx, unsigned kept, int n, const char* who, const char* what) {
  if (kept > (unsigned)n) return fail(ctx, CVO_E_HIP, std::string(who) + ": the device kept more " + what + " than it was given");
  return CVO_OK;
}

// the total a compaction left: one copy, one synchronisation
int compact_total(cvo_ctx* ctx, const unsigned* total, int n, const char* who, const char* what, unsigned* h) {
  HIP_TRY(ctx, hipMemcpyAsync(h, total, sizeof *h, hipMemcpyDeviceToHost, ctx->upload_stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
  return compact_check(ctx, *h, n, who, what);
}

// the radix sort of cvo_k_sort.h, enqueued: n pairs in key[0] / val[0], sorted there again; key[1] / val[1]: as much room,
// hist: 256 counters per block of SORT_THREADS pairs
void sort_pairs_u64(cvo_ctx* ctx, unsigned n, unsigned long long* const key[2], unsigned* const val[2], unsigned* hist) {
  const unsigned nb = (n + SORT_THREADS - 1) / SORT_THREADS;
  for (int pass = 0; pass < 8 && n > 1; pass++) {
    const int from = pass & 1, to = from ^ 1;  // (eight passes: the result is back in key[0] / val[0])
    hipLaunchKernelGGL(k_sort_hist, dim3(nb), dim3(SORT_THREADS), 0, ctx->upload_stream, n, (const unsigned long long*)key[from], 8 * pass, hist);
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(256), 0, ctx->upload_stream, nb, hist);
    hipLaunchKernelGGL(k_sort_scatter, dim3(nb), dim3(SORT_THREADS), 0, ctx->upload_stream, n, (const unsigned long long*)key[from],
                       (const unsigned*)val[from], 8 * pass, (const unsigned*)hist, key[to], val[to]);
  }
}

// The route rule of every front end.  The context's X_HOST switch forces the CPU twin (> 0) or the kernels (0); left alone
// (< 0), a call smaller than the front end's measured crossover (its X_HOST_BELOW, in its own section) takes the twin.
bool route_on_host(int host_switch, long long size, long long below) { return host_switch > 0 || (host_switch < 0 && size < below); }

// The frame of a front end's entry point once its arguments are checked: body() under the context's upload_mutex; an
// exception (the allocation of a host buffer) becomes CVO_E_NOMEM with its text.  The _host entry points have no context:
// nothing to lock, the bare code.
template <class Body>
int frontend_call(cvo_ctx* ctx, const char* who, Body body) {
  try {
    std::unique_lock<std::mutex> lk;
    if (ctx) lk = std::unique_lock<std::mutex>(ctx->upload_mutex);
    return body();
  } catch (const std::exception& e) {
    return fail(ctx, CVO_E_NOMEM, std::string(who) + ": " + e.what());
  }
}

// THE hand-over frame of every entry point that makes resident clouds of rows on the device (cvo_cloud_from_device*, cvo_cloud_merge,
// cvo_depth_filter_finish, cvo_cloud_from_rgbd_device*, cvo_map_cloud_resident): body(staged) under frontend_call.  CVO_OK:
// out[q] = staged[q].c for every staged cloud.  Anything else: no out[q] is written (the entry point has nulled them) and
// whatever `staged` still holds is freed: an exception, or a failure after the ingest, left it behind; a failed ingest or upload
// released it itself.
template <class Body>
int handover_call(cvo_ctx* ctx, const char* who, cvo_cloud** out, Body body) {
  std::vector<StagedCloud> staged;
  const int rc = frontend_call(ctx, who, [&] { return body(staged); });
  for (size_t q = 0; q < staged.size(); q++) {
    if (rc == CVO_OK) out[q] = staged[q].c;
    else if (staged[q].c) cvo_cloud_free(staged[q].c);
  }
  return rc;
}

// the kept indices, their number and - n_edge >= 0 - the flag of the first n_edge of them, to the caller's arrays that are given
void copy_kept(const std::vector<int>& kept, int* out, int* n, unsigned char* is_edge = nullptr, int n_edge = -1) {
  if (out && !kept.empty()) std::memcpy(out, kept.data(), sizeof(int) * kept.size());
  if (is_edge)
    for (size_t i = 0; i < kept.size(); i++) is_edge[i] = (int)i < n_edge ? 1 : 0;
  if (n) *n = (int)kept.size();
}

}  // namespace
