// cvo_voxel.hip -- voxel-grid downsampling (cvo::VoxelMap): cvo_voxel_select (kernels of cvo_k_voxel.h on the upload stream),
// cvo_voxel_select_host (the same contract on one CPU thread), cvo_cloud_upload_voxel (selection, then the ordinary upload
// path over the survivors' rows), cvo_debug_voxel_stats.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

// The refusals of the contract, with the text cvo_last_error returns: voxel size, non-finite coordinates, |k| >= 2^20.
int voxel_validate(int n, const float* xyz, float s, std::string* msg) {
  if (!std::isfinite(s) || !(s > 0.f)) {
    if (msg) *msg = "voxel size must be finite and > 0, got " + std::to_string(s);
    return CVO_E_INVALID;
  }
  for (int i = 0; i < n; i++) {
    unsigned long long key;
    const unsigned bad = vox_key(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], s, &key);
    if (!bad) continue;
    if (msg) {
      char buf[256];
      if (bad & VOX_BAD_FINITE) {
        snprintf(buf, sizeof buf, "point %d has a non-finite coordinate", i);
      } else {
        const int axis = bad & VOX_BAD_X ? 0 : (bad & VOX_BAD_Y ? 1 : 2);
        snprintf(buf, sizeof buf, "point %d: %c = %g is voxel %.0f of side %g; the grid extends to |k| < %d per axis (+-%g)", i, "xyz"[axis],
                 (double)xyz[3 * (size_t)i + axis], (double)rintf(xyz[3 * (size_t)i + axis] / s), (double)s, VOX_KMAX,
                 (double)s * VOX_KMAX);
      }
      *msg = buf;
    }
    return CVO_E_INVALID;
  }
  return CVO_OK;
}

// One thread, one pass: points arrive in ascending index, so the point that takes a slot is its voxel's lowest.
void voxel_select_cpu(int n, const float* xyz, float s, std::vector<int>& kept) {
  kept.clear();
  size_t cap = 64;
  while (cap < 2 * (size_t)n) cap *= 2;
  std::vector<unsigned long long> keys(cap, TABLE_EMPTY);
  for (int i = 0; i < n; i++) {
    unsigned long long key = 0;
    (void)vox_key(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], s, &key);
    size_t g = (size_t)key_mix(key) & (cap - 1);
    while (keys[g] != TABLE_EMPTY && keys[g] != key) g = (g + 1) & (cap - 1);
    if (keys[g] == TABLE_EMPTY) {
      keys[g] = key;
      kept.push_back(i);
    }
  }
}

// The kernels, on upload_stream (the caller holds upload_mutex); n >= 1, s validated.  The coordinates are n x 3 host
// floats `xyz`, staged into the scratch region here, or - d_xyz != nullptr - already on the device, written by earlier
// work on upload_stream (the RGB-D front end; xyz may then be nullptr).  kept (optional): the kept indices; d_kept_out
// (optional): where they are on the device, valid until the next selection.  ctx->vox_last.n_kept: their number.
int voxel_run_device(cvo_ctx* ctx, int n, const float* xyz, const float* d_xyz_given, float s, std::vector<int>* kept, const int** d_kept_out) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t cap = 1024;
  while (cap < 2 * (size_t)n) cap *= 2;
  const int nb = (n + VOX_THREADS - 1) / VOX_THREADS;
  VoxelCtl* ctl = nullptr;
  VoxelBlockStats* stats = nullptr;
  unsigned long long* keys = nullptr;
  unsigned *first = nullptr, *slot = nullptr, *blocks = nullptr;
  const char* table_end = nullptr;  // keys and first[] are adjacent: one fill
  int* d_kept = nullptr;
  const float* d_xyz = d_xyz_given;
  int rc = ctx->vox_scratch.lay_out(ctx, "voxel scratch", [&](ScratchLayout& l) {
    l.take(ctl, 1);
    l.take(stats, VOX_INSERT_BLOCKS);
    l.take(keys, cap);
    l.take(first, cap);
    l.at(table_end, l.off);
    if (!d_xyz_given) l.take(d_xyz, 3 * (size_t)n);
    l.take(slot, (size_t)n);
    l.take(blocks, (size_t)nb);
    l.take(d_kept, (size_t)n);
  });
  if (rc != CVO_OK) return rc;
  hipStream_t st = ctx->upload_stream;
  const unsigned mask = (unsigned)(cap - 1);
  HIP_TRY(ctx, hipMemsetAsync(ctl, 0, sizeof(VoxelCtl), st));
  HIP_TRY(ctx, hipMemsetAsync(keys, 0xFF, (size_t)(table_end - (const char*)keys), st));
  if (!d_xyz_given) HIP_TRY(ctx, hipMemcpyAsync((void*)d_xyz, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
  const int grid = std::min(nb, VOX_INSERT_BLOCKS);
  if (ctx->opt.voxel_prepass)
    hipLaunchKernelGGL(k_voxel_insert<true>, dim3(grid), dim3(VOX_THREADS), 0, st, n, d_xyz, s, mask, keys, first, slot, ctl, stats);
  else
    hipLaunchKernelGGL(k_voxel_insert<false>, dim3(grid), dim3(VOX_THREADS), 0, st, n, d_xyz, s, mask, keys, first, slot, ctl, stats);
  auto scan = [&](int nbs, unsigned* count) {  // (the selection's own: the block statistics are summed in the same launch)
    hipLaunchKernelGGL(k_voxel_scan, dim3(1), dim3(VOX_THREADS), 0, st, nbs, count, ctl, grid, (const VoxelBlockStats*)stats);
  };
  if ((rc = compact(ctx, n, VoxelFirst{mask, first, slot, d_kept}, blocks, scan)) != CVO_OK) return rc;
  VoxelCtl h{};
  // (at most n points are ever kept: the "kept more than it was given" refusal and the one of h.status cannot meet)
  HIP_TRY(ctx, hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));  // (the whole control word: one copy, one synchronisation)
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if ((rc = compact_check(ctx, h.n_kept, n, "voxel selection", "points")) != CVO_OK) return rc;
  if (h.status) {
    std::string msg;
    std::vector<float> back;
    if (!xyz) {  // (the refusal names the point: fetch what the device was given)
      back.resize(3 * (size_t)n);
      HIP_TRY(ctx, hipMemcpy(back.data(), d_xyz, sizeof(float) * back.size(), hipMemcpyDeviceToHost));
      xyz = back.data();
    }
    (void)voxel_validate(n, xyz, s, &msg);
    return fail(ctx, CVO_E_INVALID, "voxel selection: " + msg);
  }
  if (kept) {
    kept->resize(h.n_kept);
    if (h.n_kept) {
      HIP_TRY(ctx, hipMemcpyAsync(kept->data(), d_kept, sizeof(int) * (size_t)h.n_kept, hipMemcpyDeviceToHost, st));
      HIP_TRY(ctx, hipStreamSynchronize(st));
    }
  }
  if (d_kept_out) *d_kept_out = d_kept;
  ctx->vox_capacity = cap;
  ctx->vox_last = h;
  return CVO_OK;
}

// Below this many points the CPU twin is the faster route (scripts/voxel_probe.py --sizes 2000 10000 50000: 0.02 ms against
// the kernels' flat 0.09 ms of launches, copies and two synchronisations at 2000 points, 0.12 against 0.09 at 10 000): the
// default route of small frames.  VOXEL_HOST=0 / 1 forces one route for every size.
constexpr int VOX_HOST_BELOW = 4096;

// Size checks + the route the context's switches choose (ctx == nullptr: the twin).  The caller holds upload_mutex.
int voxel_select(cvo_ctx* ctx, const char* who, int n, const float* xyz, float s, std::vector<int>& kept) {
  if (n > COMPACT_MAX_ELEMENTS) return fail(ctx, CVO_E_UNSUPPORTED, std::string(who) + ": more than 2^24 points");
  std::string msg;
  if (voxel_validate(0, nullptr, s, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + msg);
  kept.clear();
  if (!ctx || n == 0 || route_on_host(ctx->opt.voxel_host, n, VOX_HOST_BELOW)) {
    if (voxel_validate(n, xyz, s, &msg) != CVO_OK) return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + msg);
    voxel_select_cpu(n, xyz, s, kept);
    if (ctx) {
      ctx->vox_capacity = 0;  // (no table: cvo_debug_voxel_stats reads zeros)
      ctx->vox_last = VoxelCtl{};
    }
    return CVO_OK;
  }
  return voxel_run_device(ctx, n, xyz, nullptr, s, &kept, nullptr);
}

// the body of cvo_voxel_select_host and cvo_voxel_select: n and the pointers, then voxel_select's refusals
int voxel_entry(cvo_ctx* ctx, const char* who, int n, const float* xyz, float voxel_size, int* kept, int* n_kept) {
  if (n < 0 || (n > 0 && (!xyz || !kept)) || !n_kept) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  return frontend_call(ctx, who, [&] {
    std::vector<int> k;
    const int rc = voxel_select(ctx, who, n, xyz, voxel_size, k);
    if (rc != CVO_OK) return rc;
    copy_kept(k, kept, n_kept);
    return CVO_OK;
  });
}

}  // namespace

extern "C" {

int cvo_voxel_select_host(int n, const float* xyz, float voxel_size, int* kept, int* n_kept) {
  return voxel_entry(nullptr, "cvo_voxel_select_host", n, xyz, voxel_size, kept, n_kept);
}

int cvo_voxel_select(cvo_ctx* ctx, int n, const float* xyz, float voxel_size, int* kept, int* n_kept) {
  if (!ctx) return CVO_E_INVALID;
  return voxel_entry(ctx, "cvo_voxel_select", n, xyz, voxel_size, kept, n_kept);
}

// Coordinates go to the device alone (12 bytes per point); the survivors' rows are gathered on the host straight into the
// staging buffer of the ordinary upload (HostCloud::rows), so the cloud is the one cvo_cloud_upload makes of those rows.
int cvo_cloud_upload_voxel(cvo_ctx* ctx, int n, const float* xyz, const float* feat, const float* label, const float* geotype,
                           float voxel_size, cvo_cloud** out, int* kept, int* n_kept) {
  if (!ctx || !out || n < 0 || (n > 0 && !xyz)) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_voxel: bad argument");
  return frontend_call(ctx, "cvo_cloud_upload_voxel", [&] {
    std::vector<int> k;
    int rc = voxel_select(ctx, "cvo_cloud_upload_voxel", n, xyz, voxel_size, k);
    if (rc != CVO_OK) return rc;
    HostCloud h{(int)k.size(), (const char*)xyz, 12, (const char*)feat, sizeof(float) * FD, (const char*)label, sizeof(float) * NC,
                (const char*)geotype, 8};
    h.rows = k.data();
    if ((rc = upload_one_locked(ctx, h, out)) != CVO_OK) return rc;
    copy_kept(k, kept, n_kept);
    return CVO_OK;
  });
}

int cvo_debug_voxel_stats(cvo_ctx* ctx, unsigned long long* capacity, unsigned long long* occupied, unsigned long long* probes_total,
                          unsigned long long* probe_longest, unsigned long long* entered) {
  if (!ctx) return CVO_E_INVALID;
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  if (capacity) *capacity = ctx->vox_capacity;
  if (occupied) *occupied = ctx->vox_last.occupied;
  if (probes_total) *probes_total = ctx->vox_last.probes;
  if (probe_longest) *probe_longest = ctx->vox_last.longest;
  if (entered) *entered = ctx->vox_last.entered;
  return CVO_OK;
}

}  // extern "C"
