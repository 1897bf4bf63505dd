// cvo_merge.hip -- resident clouds merged on the device and read back: cvo_cloud_merge (k_cloud_unpack over all inputs, the
// voxel selection of cvo_voxel.hip on the moved rows where they are, the ingest of cvo_ingest.hip through the kept indices
// where they are) and cvo_cloud_download (k_cloud_unpack of one cloud, one copy per array the caller asked for).
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

// an attribute array the cloud really holds: in its own slab (an align call may have pointed it into the zero slab since)
template <class T>
const T* held(const cvo_cloud* c, const T* p) {
  const char* q = (const char*)p;
  return q && q >= c->slab.p && q < c->slab.p + c->slab.bytes ? p : nullptr;
}

enum : int { HAS_FEAT = CVO_CLOUD_HAS_FEAT, HAS_LABEL = CVO_CLOUD_HAS_LABEL, HAS_GEOTYPE = CVO_CLOUD_HAS_GEOTYPE };

int cloud_present(const cvo_cloud* c) {
  if (c->n == 0) return 0;
  return (held(c, c->feat) ? HAS_FEAT : 0) | (held(c, c->label) ? HAS_LABEL : 0) | (held(c, c->geo) ? HAS_GEOTYPE : 0);
}

// THE list of unpacked rows (k_cloud_unpack's padded rows, original order): nn rows of the coordinates and of the attributes
// `present` names, for a region's typed walk.  The arrays it does not name stay null.
void unpacked_rows_list(ScratchLayout& l, int present, size_t nn, float*& xyz, float4*& feat, float4*& label, float2*& geo) {
  l.take(xyz, 3 * nn);
  if (present & HAS_FEAT) l.take(feat, FD_PAD / 4 * nn);
  if (present & HAS_LABEL) l.take(label, NC_PAD / 4 * nn);
  if (present & HAS_GEOTYPE) l.take(geo, nn);
}

// THE unpack: the rows of the non-empty clouds of `clouds` in original order, cloud after cloud, each under its pose (poses: 12
// doubles per cloud, cast to float as multiframe_refresh casts them, or nullptr: not moved), into o's arrays (a null attribute
// array: not wanted): the job table copied to d_jobs (room for a job per non-empty cloud), one k_cloud_unpack launch on
// upload_stream, not synchronised.  `jobs` is the table on the host: alive until the stream has been synchronised.  The caller
// holds upload_mutex; the clouds are the context's and hold o.total in 1 .. 2^24 rows together.
int unpack_launch(cvo_ctx* ctx, int n_clouds, const cvo_cloud* const* clouds, const double* poses, std::vector<UnpackJob>& jobs, UnpackJob* d_jobs,
                  UnpackOut o) {
  jobs.clear();
  int base = 0;
  for (int q = 0; q < n_clouds; q++) {
    const cvo_cloud* c = clouds[q];
    if (c->n == 0) continue;  // (no job: the first rows of the table stay strictly ascending)
    UnpackJob j{};
    j.n = c->n;
    j.base = base;
    j.has_pose = poses ? 1 : 0;
    for (int k = 0; poses && k < 12; k++) j.pose[k] = (float)poses[12 * (size_t)q + k];
    j.x4 = c->x4;
    j.inv = c->inv;
    j.feat = held(c, c->feat);
    j.label = held(c, c->label);
    j.geo = held(c, c->geo);
    jobs.push_back(j);
    base += c->n;
  }
  o.n_jobs = (int)jobs.size();
  HIP_TRY(ctx, hipMemcpyAsync(d_jobs, jobs.data(), sizeof(UnpackJob) * jobs.size(), hipMemcpyHostToDevice, ctx->upload_stream));
  const int grid = std::min((o.total + UNPACK_THREADS - 1) / UNPACK_THREADS, UNPACK_MAX_BLOCKS);
  hipLaunchKernelGGL(k_cloud_unpack, dim3((unsigned)grid), dim3(UNPACK_THREADS), 0, ctx->upload_stream, (const UnpackJob*)d_jobs, o);
  HIP_TRY(ctx, hipGetLastError());
  return CVO_OK;
}

// The rows of `clouds` (`total` of them together) unpacked into the context's merge region.  *d describes them as ingest rows:
// xyz packed, the attributes of `want` that some cloud holds at strides 32 / 80 / 8, the others null.  jobs: see unpack_launch.
int unpack_clouds(cvo_ctx* ctx, int n_clouds, const cvo_cloud* const* clouds, const double* poses, int want, int total,
                  std::vector<UnpackJob>& jobs, cvo_device_rows_t* d) {
  *d = cvo_device_rows_t{};
  jobs.clear();
  if (total == 0) return CVO_OK;
  int any = 0, n_jobs = 0;
  for (int q = 0; q < n_clouds; q++) {
    any |= cloud_present(clouds[q]);
    n_jobs += clouds[q]->n > 0 ? 1 : 0;
  }
  UnpackJob* d_jobs = nullptr;
  UnpackOut o{};
  o.total = total;
  int rc = ctx->merge_scratch.lay_out(ctx, "merge scratch", [&](ScratchLayout& l) {
    l.take(d_jobs, (size_t)n_jobs);
    unpacked_rows_list(l, any & want, (size_t)total, o.xyz, o.feat, o.label, o.geo);
  });
  if (rc != CVO_OK) return rc;
  if ((rc = unpack_launch(ctx, n_clouds, clouds, poses, jobs, d_jobs, o)) != CVO_OK) return rc;
  *d = device_rows(total, total, o.xyz, o.feat, FD_PAD, o.label, NC_PAD, o.geo);
  return CVO_OK;
}

// the body of cvo_cloud_merge under upload_mutex; the arguments have been checked.  staged: the result, or what to release
int merge_locked(cvo_ctx* ctx, int n_clouds, const cvo_cloud* const* clouds, const double* poses, float voxel_size, int total,
                 std::vector<StagedCloud>& staged, int* kept, int* n_kept) {
  const char* who = "cvo_cloud_merge";
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<UnpackJob> jobs;
  cvo_device_rows_t d{};
  int rc = unpack_clouds(ctx, n_clouds, clouds, poses, HAS_FEAT | HAS_LABEL | HAS_GEOTYPE, total, jobs, &d);
  if (rc != CVO_OK) return rc;
  std::vector<int> k;
  const bool select = voxel_size > 0.f && total > 0;
  if (select) {  // the selection reads the moved coordinates where they are and leaves the kept indices where the ingest reads them
    const int* d_kept = nullptr;
    if ((rc = voxel_run_device(ctx, total, nullptr, (const float*)d.xyz, voxel_size, kept ? &k : nullptr, &d_kept)) != CVO_OK) return rc;
    d.n = (int)ctx->vox_last.n_kept;
    d.rows = d_kept;
  }
  if ((rc = ingest_device_clouds(ctx, 1, &d, staged, who)) != CVO_OK) return rc;  // (synchronises upload_stream)
  if (kept && !select)
    for (int i = 0; i < total; i++) kept[i] = i;
  if (kept && select) copy_kept(k, kept, nullptr);
  if (n_kept) *n_kept = d.n;
  return CVO_OK;
}

// the body of cvo_cloud_download under upload_mutex
int download_locked(cvo_ctx* ctx, const cvo_cloud* c, float* xyz, float* feat, float* label, float* geotype) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n = c->n, has = cloud_present(c);
  const size_t nn = (size_t)n;
  // an attribute the cloud lacks: zeros, written here
  if (feat && !(has & HAS_FEAT)) std::memset(feat, 0, sizeof(float) * FD * nn);
  if (label && !(has & HAS_LABEL)) std::memset(label, 0, sizeof(float) * NC * nn);
  if (geotype && !(has & HAS_GEOTYPE)) std::memset(geotype, 0, sizeof(float) * 2 * nn);
  if (n == 0) return CVO_OK;
  const int want = (feat ? HAS_FEAT : 0) | (label ? HAS_LABEL : 0) | (geotype ? HAS_GEOTYPE : 0);
  if (!xyz && !(want & has)) return CVO_OK;
  std::vector<UnpackJob> jobs;
  cvo_device_rows_t d{};
  const int rc = unpack_clouds(ctx, 1, &c, nullptr, want, n, jobs, &d);
  if (rc != CVO_OK) return rc;
  // one copy per array; the padded rows (8 of 5, 20 of 19 floats) lose their padding on the host
  std::vector<float> f8, l20;
  const hipStream_t st = ctx->upload_stream;
  if (xyz) HIP_TRY(ctx, hipMemcpyAsync(xyz, d.xyz, sizeof(float) * 3 * nn, hipMemcpyDeviceToHost, st));
  if (d.feat) {
    f8.resize(FD_PAD * nn);
    HIP_TRY(ctx, hipMemcpyAsync(f8.data(), d.feat, sizeof(float) * f8.size(), hipMemcpyDeviceToHost, st));
  }
  if (d.label) {
    l20.resize(NC_PAD * nn);
    HIP_TRY(ctx, hipMemcpyAsync(l20.data(), d.label, sizeof(float) * l20.size(), hipMemcpyDeviceToHost, st));
  }
  if (d.geotype) HIP_TRY(ctx, hipMemcpyAsync(geotype, d.geotype, sizeof(float) * 2 * nn, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < nn && d.feat; i++) std::memcpy(feat + FD * i, &f8[FD_PAD * i], sizeof(float) * FD);
  for (size_t i = 0; i < nn && d.label; i++) std::memcpy(label + NC * i, &l20[NC_PAD * i], sizeof(float) * NC);
  return CVO_OK;
}

}  // namespace

extern "C" {

int cvo_cloud_merge(cvo_ctx* ctx, int n_clouds, const cvo_cloud* const* clouds, const double* poses, float voxel_size, cvo_cloud** out,
                    int* kept, int* n_kept) {
  const char* who = "cvo_cloud_merge";
  if (out) *out = nullptr;
  if (n_kept) *n_kept = 0;
  if (!ctx || !out || n_clouds < 1 || !clouds) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (n_clouds > UNPACK_MAX_JOBS) return fail(ctx, CVO_E_UNSUPPORTED, std::string(who) + ": more than " + std::to_string(UNPACK_MAX_JOBS) + " clouds");
  if (!std::isfinite(voxel_size) || voxel_size < 0.f)
    return fail(ctx, CVO_E_INVALID, std::string(who) + ": voxel size must be finite and >= 0, got " + std::to_string(voxel_size));
  long long total = 0;
  for (int q = 0; q < n_clouds; q++) {
    if (!clouds[q]) return fail(ctx, CVO_E_INVALID, std::string(who) + ": cloud " + std::to_string(q) + " is NULL");
    if (clouds[q]->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": cloud " + std::to_string(q) + " belongs to another context");
    total += clouds[q]->n;
  }
  if (total > COMPACT_MAX_ELEMENTS) return fail(ctx, CVO_E_UNSUPPORTED, std::string(who) + ": more than 2^24 rows in total");
  const int rc = handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) {
    return merge_locked(ctx, n_clouds, clouds, poses, voxel_size, (int)total, staged, kept, n_kept);
  });
  if (rc != CVO_OK && n_kept) *n_kept = 0;
  return rc;
}

int cvo_cloud_download(cvo_ctx* ctx, const cvo_cloud* cloud, float* xyz, float* feat, float* label, float* geotype, int* present) {
  const char* who = "cvo_cloud_download";
  if (!ctx || !cloud) return fail(ctx, CVO_E_INVALID, std::string(who) + ": bad argument");
  if (cloud->ctx != ctx) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the cloud belongs to another context");
  return frontend_call(ctx, who, [&] {
    const int rc = download_locked(ctx, cloud, xyz, feat, label, geotype);
    if (rc == CVO_OK && present) *present = cloud_present(cloud);
    return rc;
  });
}

}  // extern "C"
