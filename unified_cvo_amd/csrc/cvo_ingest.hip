// cvo_ingest.hip -- resident clouds from rows that are already in device memory: cvo_cloud_from_device / _many / _aos192.
// The argument checks (every pointer is classified before anything reads through it), one k_cloud_ingest launch over all
// clouds of a call, one read-back of the control blocks, then upload_host_cloud's route rule: k_kd_order or the wide
// ordering through finish_uploads, or the host's spatial_order on the coordinates alone + k_cloud_gather.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.  Shared declarations: cvo_internal.h; the
// helpers shared with the host route (spatial_order, cloud_slab_list, finish_uploads): cvo_upload.hip.
namespace {

// One array a caller hands over in device memory (an array of a cvo_device_rows_t, a plane of a cvo_rgbd_device_frame_t): `need`
// bytes of `units` (rows, bytes) from p, aligned to `align` bytes, must lie in ONE allocation of the context's device.  The
// pointer is classified here, before anything reads through it.  *why: the refusal's text.
bool device_extent_ok(cvo_ctx* ctx, const char* what, const void* p, size_t align, size_t need, const std::string& units, std::string* why) {
  const std::string w(what);
  if (((uintptr_t)p & (align - 1)) != 0) return *why = w + " is not " + std::to_string(align) + "-byte aligned", false;
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // (an unregistered host pointer: the error is this call's answer, not the process's state)
    return *why = w + " is not device memory", false;
  }
  if (attr.type != hipMemoryTypeDevice) return *why = w + " is not device memory (host, pinned and managed memory are refused)", false;
  if (attr.device != ctx->device)
    return *why = w + " is memory of device " + std::to_string(attr.device) + ", the context's is " + std::to_string(ctx->device), false;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();
    return *why = w + ": no allocation found behind the pointer", false;
  }
  const size_t room = (size_t)((const char*)base + size - (const char*)p);
  if (need > room) return *why = w + ": " + units + " need " + std::to_string(need) + " bytes, the allocation ends after " + std::to_string(room), false;
  return true;
}

// One array of a cvo_device_rows_t: n_rows rows of row_bytes, `stride` bytes apart
bool device_rows_ok(cvo_ctx* ctx, const char* what, const void* p, size_t stride, size_t row_bytes, size_t n_rows, std::string* why) {
  const std::string w(what);
  if (((uintptr_t)p & 3u) != 0) return *why = w + " is not 4-byte aligned", false;
  if (stride < row_bytes || (stride & 3u) != 0 || stride > 0xffffffffull)
    return *why = w + ": a stride of " + std::to_string(stride) + " bytes (rows of " + std::to_string(row_bytes) + " bytes, multiples of 4)", false;
  return device_extent_ok(ctx, what, p, 4, (n_rows - 1) * stride + row_bytes, std::to_string(n_rows) + " rows", why);
}

// THE row table of rows at the fixed strides (xyz 12 bytes, geotype 8): n rows of n_records, feature rows of feat_floats and
// label rows of label_floats floats, through `rows` where it is given.  A null attribute pointer: absent (its stride is not read).
cvo_device_rows_t device_rows(int n, int n_records, const float* xyz, const void* feat, size_t feat_floats, const void* label, size_t label_floats,
                              const void* geotype, const int* rows = nullptr) {
  return cvo_device_rows_t{n, n_records, xyz, 12, feat, sizeof(float) * feat_floats, label, sizeof(float) * label_floats, geotype, 8, rows};
}

// everything the host can decide about one cvo_device_rows_t, before any launch
int check_device_rows(cvo_ctx* ctx, const cvo_device_rows_t& d, const char* who) {
  auto bad = [&](const std::string& why) { return fail(ctx, CVO_E_INVALID, std::string(who) + ": " + why); };
  if (d.n < 0) return bad("n < 0");
  if (d.n == 0) return CVO_OK;  // (an empty cloud reads nothing)
  if (!d.xyz) return bad("xyz is NULL");
  if (d.n_records < 1) return bad("n_records < 1");
  if (!d.rows && d.n_records < d.n) return bad("n_records (" + std::to_string(d.n_records) + ") < n (" + std::to_string(d.n) + ") without rows");
  std::string why;
  const size_t nr = (size_t)d.n_records;
  if (!device_rows_ok(ctx, "xyz", d.xyz, d.xyz_stride, 12, nr, &why)) return bad(why);
  if (d.feat && !device_rows_ok(ctx, "feat", d.feat, d.feat_stride, sizeof(float) * FD, nr, &why)) return bad(why);
  if (d.label && !device_rows_ok(ctx, "label", d.label, d.label_stride, sizeof(float) * NC, nr, &why)) return bad(why);
  if (d.geotype && !device_rows_ok(ctx, "geotype", d.geotype, d.geotype_stride, 8, nr, &why)) return bad(why);
  if (d.rows && !device_rows_ok(ctx, "rows", d.rows, 4, 4, (size_t)d.n, &why)) return bad(why);
  return CVO_OK;
}

// The clouds of one call into staged[].c; the caller holds upload_mutex.  On error every cloud of the call has been released.
int ingest_device_clouds(cvo_ctx* ctx, int n_clouds, const cvo_device_rows_t* rows, std::vector<StagedCloud>& staged, const char* who) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int q = 0; q < n_clouds; q++) {
    const int rc = check_device_rows(ctx, rows[q], who);
    if (rc != CVO_OK) return rc;
  }
  if (n_clouds == 0) return CVO_OK;
  const hipStream_t stream = ctx->upload_stream;
  staged.resize((size_t)n_clouds);
  std::vector<SlabShape> shapes((size_t)n_clouds);
  auto release = [&]() {
    for (auto& sc : staged) {
      if (sc.c) cvo_cloud_free(sc.c);
      sc.c = nullptr;
    }
  };
  auto hip_fail = [&](const char* what, hipError_t e) {
    release();
    return fail(ctx, e == hipErrorOutOfMemory ? CVO_E_NOMEM : CVO_E_HIP, std::string(who) + ": " + what + ": " + hipGetErrorString(e));
  };
  // ---- slabs.  What the host route knows before it lays a slab out and this one learns only from the ingest: whether the
  // coordinates are finite (k_kd_order's scratch is reserved whenever size and switches allow the device ordering) and
  // whether the label rows are one-hot (raw_lid / lid are reserved whenever labels are given and NO_ONEHOT is not set; the
  // cloud's lid pointer stays null when a row fails the rule).  ONE walk, no second allocation; the raw arrays stay in
  // the slab on both routes (k_cloud_gather reads them where the host route would have staged the final form).
  int gx = 1, n_jobs = 0;
  for (int q = 0; q < n_clouds; q++) {
    const cvo_device_rows_t& d = rows[q];
    cvo_cloud* c = new cvo_cloud();
    staged[q].c = c;
    c->ctx = ctx;
    c->device = ctx->device;
    c->n = d.n;
    int NP = KD_THREADS;
    while (NP < d.n) NP *= 2;
    const bool has = d.n > 0;
    shapes[q] = SlabShape{(size_t)std::max(d.n, 1), NP, has && d.feat, has && d.label, has && d.geotype, has && d.label && !ctx->opt.no_onehot,
                          has, order_route(d.n, true, ctx->opt.order, ctx->opt.no_sort) == ORDER_ROUTE_BLOCK};
    size_t unused = 0;
    if (const int rc = c->slab.lay_out(ctx, "cloud", cloud_slab_list(*c, shapes[q], &unused), nullptr); rc != CVO_OK) {
      release();
      return rc;
    }
    if (has) {
      n_jobs++;
      gx = std::max(gx, std::min((d.n + INGEST_THREADS - 1) / INGEST_THREADS, INGEST_MAX_BLOCKS));
    }
  }
  if (n_jobs == 0) return CVO_OK;  // empty clouds only: nothing to read
  // ---- the context's ingest region, laid out anew by every call: the ingest jobs, the gather jobs, a control block (flags + gx partials) per job
  IngestJob* d_jobs = nullptr;
  KdJob* d_gather = nullptr;
  char* d_ctl = nullptr;
  const size_t ctl_stride = sizeof(IngestFlags) + sizeof(IngestPartial) * (size_t)gx;
  auto region = [&](ScratchLayout& l) {
    l.take(d_jobs, (size_t)n_jobs);
    l.take(d_gather, (size_t)n_jobs);
    l.take(d_ctl, ctl_stride * (size_t)n_jobs);
  };
  const int rc_region = ctx->ingest_scratch.lay_out(ctx, "ingest control block", region);
  if (rc_region != CVO_OK) {
    release();
    return rc_region;
  }
  std::vector<IngestJob> jobs;
  std::vector<int> cloud_of;  // job -> cloud of the call
  for (int q = 0; q < n_clouds; q++) {
    const cvo_device_rows_t& d = rows[q];
    if (d.n == 0) continue;
    cvo_cloud* c = staged[q].c;
    IngestJob j{};
    j.n = d.n;
    j.n_records = d.n_records;
    j.xyz = (const char*)d.xyz;
    j.xyz_stride = (unsigned)d.xyz_stride;
    j.feat = (const char*)d.feat;
    j.feat_stride = (unsigned)d.feat_stride;
    j.label = (const char*)d.label;
    j.label_stride = (unsigned)d.label_stride;
    j.geo = (const char*)d.geotype;
    j.geo_stride = (unsigned)d.geotype_stride;
    j.rows = d.rows;
    j.x4 = c->x4;
    j.raw_feat = c->raw_feat;
    j.raw_label = c->raw_label;
    j.raw_geo = c->raw_geo;
    j.raw_lid = c->raw_lid;
    char* ctl = d_ctl + ctl_stride * jobs.size();
    j.flags = reinterpret_cast<IngestFlags*>(ctl);
    j.partial = reinterpret_cast<IngestPartial*>(ctl + sizeof(IngestFlags));
    jobs.push_back(j);
    cloud_of.push_back(q);
  }
  std::vector<char> h_ctl(ctl_stride * (size_t)n_jobs);
  hipError_t e = hipMemcpyAsync(d_jobs, jobs.data(), sizeof(IngestJob) * jobs.size(), hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_ctl, 0xff, h_ctl.size(), stream);  // (the flag words: all set; every partial is written)
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_cloud_ingest, dim3((unsigned)gx, (unsigned)n_jobs), dim3(INGEST_THREADS), 0, stream, (const IngestJob*)d_jobs);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_ctl.data(), d_ctl, h_ctl.size(), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail("ingest", e);
  // ---- what the ingest found
  std::vector<KdJob> gather;
  std::vector<cvo_cloud*> host_ordered;
  for (size_t k = 0; k < jobs.size(); k++) {
    const int q = cloud_of[k];
    cvo_cloud* c = staged[q].c;
    const int n = c->n;
    IngestFlags f;
    std::memcpy(&f, h_ctl.data() + ctl_stride * k, sizeof f);
    if (f.bad_pos != ~0u) {
      release();
      return fail(ctx, CVO_E_INVALID, std::string(who) + ": rows[" + std::to_string(f.bad_pos) + "] of cloud " + std::to_string(q) +
                                          " is outside [0, n_records = " + std::to_string(rows[q].n_records) + ")");
    }
    double sx = 0, sy = 0, sz = 0, r2max = 0;
    for (int b = 0; b < gx; b++) {  // (block order: the documented sum order of k_cloud_ingest)
      IngestPartial p;
      std::memcpy(&p, h_ctl.data() + ctl_stride * k + sizeof(IngestFlags) + sizeof(IngestPartial) * (size_t)b, sizeof p);
      sx += p.sx;
      sy += p.sy;
      sz += p.sz;
      if (r2max == r2max && !(p.r2max <= r2max)) r2max = p.r2max;
    }
    c->rmax = (float)(std::sqrt(r2max) * 1.000001);
    c->cx = (float)(sx / n);
    c->cy = (float)(sy / n);
    c->cz = (float)(sz / n);
    if (!std::isfinite(c->cx) || !std::isfinite(c->cy) || !std::isfinite(c->cz)) c->cx = c->cy = c->cz = 0.f;
    const bool has_lid = shapes[q].lid && f.onehot != 0u;
    if (!has_lid) c->lid = c->raw_lid = nullptr;  // (reserved, unused: the kernels take the one-hot path from a non-null lid)
    c->order_route = order_route(n, f.finite != 0u, ctx->opt.order, ctx->opt.no_sort);  // the route rule of upload_host_cloud
    KdJob job{};
    size_t unused = 0;  // the job's pointers: the same list over the same slab, minus the class ids of a cloud that is not one-hot
    ScratchLayout(c->slab.p).walk(cloud_slab_list(job, shapes[q], &unused));
    if (!has_lid) job.raw_lid = job.lid = nullptr;
    job.n = n;
    job.NP = shapes[q].NP;
    c->h_order.assign((size_t)n, 0);
    staged[q].wide = c->order_route == ORDER_ROUTE_WIDE;
    if (c->order_route != ORDER_ROUTE_HOST) {
      staged[q].job = job;
    } else {
      staged[q].job = KdJob{};
      gather.push_back(job);
      host_ordered.push_back(c);
    }
  }
  // ---- host ordering: only x4 comes down (16 B per point), the order goes up, k_cloud_gather permutes on the device
  if (!gather.empty()) {
    std::vector<std::vector<float>> x4(gather.size());
    for (size_t k = 0; e == hipSuccess && k < gather.size(); k++) {
      x4[k].resize(4 * (size_t)gather[k].n);
      e = hipMemcpyAsync(x4[k].data(), gather[k].x4, sizeof(float) * x4[k].size(), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    int ggx = 1;
    for (size_t k = 0; e == hipSuccess && k < gather.size(); k++) {
      cvo_cloud* c = host_ordered[k];
      spatial_order(x4[k].data(), c->n, c->h_order, ctx->opt.no_sort, ctx->opt.order == CloudOrder::Virtual);
      e = hipMemcpyAsync(c->order, c->h_order.data(), sizeof(int) * (size_t)c->n, hipMemcpyHostToDevice, stream);
      ggx = std::max(ggx, (int)std::min<long long>((5ll * c->n + GATHER_THREADS - 1) / GATHER_THREADS, 4 * INGEST_MAX_BLOCKS));
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_gather, gather.data(), sizeof(KdJob) * gather.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_cloud_gather, dim3((unsigned)ggx, (unsigned)gather.size()), dim3(GATHER_THREADS), 0, stream, (const KdJob*)d_gather);
      e = hipGetLastError();
    }
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(stream);
      return hip_fail("gather", e);
    }
  }
  // ---- device ordering: one k_kd_order launch over the clouds that asked for it, the wide clouds' launches, the orders back, THE synchronisation
  return finish_uploads(ctx, staged);  // (on error every cloud released)
}

// the entry frame: the clouds of one call through THE hand-over frame (cvo_frontend.hip) - all of them, or none
int from_device_call(cvo_ctx* ctx, int n_clouds, const cvo_device_rows_t* rows, cvo_cloud** out, const char* who) {
  for (int q = 0; q < n_clouds; q++) out[q] = nullptr;
  return handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) { return ingest_device_clouds(ctx, n_clouds, rows, staged, who); });
}

}  // namespace

extern "C" {

int cvo_cloud_from_device(cvo_ctx* ctx, const cvo_device_rows_t* rows, cvo_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !rows || !out) return fail(ctx, CVO_E_INVALID, "cvo_cloud_from_device: bad argument");
  return from_device_call(ctx, 1, rows, out, "cvo_cloud_from_device");
}

int cvo_cloud_from_device_many(cvo_ctx* ctx, int n_clouds, const cvo_device_rows_t* rows, cvo_cloud** out) {
  if (!ctx || !out || n_clouds < 0 || (n_clouds > 0 && !rows)) return fail(ctx, CVO_E_INVALID, "cvo_cloud_from_device_many: bad argument");
  return from_device_call(ctx, n_clouds, rows, out, "cvo_cloud_from_device_many");
}

int cvo_cloud_from_device_aos192(cvo_ctx* ctx, int n, const void* d_pts, cvo_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !out || n < 0 || (n > 0 && !d_pts)) return fail(ctx, CVO_E_INVALID, "cvo_cloud_from_device_aos192: bad argument");
  // PointSegmentedDistribution<5,19> byte offsets, as cvo_cloud_upload_aos192 reads them: xyz@0, features@20,
  // label_distribution@44, geometric_type@120, sizeof = 192
  const char* b = (const char*)d_pts;
  const cvo_device_rows_t d{n, n, b, 192, n > 0 ? b + 20 : nullptr, 192, n > 0 ? b + 44 : nullptr, 192, n > 0 ? b + 120 : nullptr, 192, nullptr};
  return from_device_call(ctx, 1, &d, out, "cvo_cloud_from_device_aos192");
}

}  // extern "C"
