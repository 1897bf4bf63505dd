// cvo_upload.hip -- resident clouds: the route rule of the ordering, the host's plan and launches of the multi-block ordering (ORDER=wide), host-side spatial ordering (the twin of k_kd_order), staging, one allocation + one copy per cloud, cvo_cloud_upload / _aos192 / _many, cvo_cloud_transformed, zero slabs for attributes a cloud was uploaded without.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

// *created (optional) is set when this call allocated the slab: its zero fill is in flight on ctx->stream.
int ensure_attributes(cvo_ctx* ctx, const cvo_cloud* c, bool need_feat, bool need_label, bool need_geo, bool* created = nullptr) {
  if ((!need_feat || c->feat) && (!need_label || c->label) && (!need_geo || c->geo)) return CVO_OK;
  cvo_cloud* m = const_cast<cvo_cloud*>(c);
  const size_t nn = (size_t)std::max(c->n, 1);
  CloudArrays z;
  auto list = [&](ScratchLayout& l) {
    l.take(z.feat, 2 * nn);
    l.take(z.label, 5 * nn);
    l.take(z.geo, nn);
  };
  if (!m->zero_slab.p) {
    HIP_TRY(ctx, hipSetDevice(c->device));
    if (const int rc = m->zero_slab.lay_out(ctx, "cloud", list, nullptr); rc != CVO_OK) return rc;
    const hipError_t e = hipMemsetAsync(m->zero_slab.p, 0, m->zero_slab.bytes, ctx->stream);
    if (e != hipSuccess) {
      m->zero_slab.release();  // never hand the kernels an allocated-but-not-zeroed "zero" slab on a later call
      return fail(ctx, CVO_E_HIP, std::string("cloud hipMemsetAsync: ") + hipGetErrorString(e));
    }
    if (created) *created = true;
  }
  ScratchLayout(m->zero_slab.p).walk(list);
  if (!m->feat) m->feat = z.feat;
  if (!m->label) m->label = z.label;
  if (!m->geo) m->geo = z.geo;
  return CVO_OK;
}

// THE route rule of an upload, host rows or device rows: who orders a cloud of n points (cvo_debug_cloud_order_route's values).
// Fewer than 8 points, a non-finite coordinate and NO_SORT are the identity, which the host writes.
enum { ORDER_ROUTE_HOST = 0, ORDER_ROUTE_BLOCK = 1, ORDER_ROUTE_WIDE = 2 };
int order_route(int n, bool finite, CloudOrder order, bool no_sort) {
  if (n < 8 || !finite || no_sort) return ORDER_ROUTE_HOST;
  if (order != CloudOrder::Device && order != CloudOrder::Wide) return ORDER_ROUTE_HOST;
  if (n <= KD_MAX_POINTS) return ORDER_ROUTE_BLOCK;
  return order == CloudOrder::Wide && n <= KD_WIDE_MAX_POINTS ? ORDER_ROUTE_WIDE : ORDER_ROUTE_HOST;
}

// The plan of the multi-block ordering (cvo_k_kd_wide.h) of n points with leaves of at most `leaf`: kd_left cuts by count, so
// every segment of every level is known before anything runs.  Level by level, by position inside a level: the cuts of the
// segments of more than `leaf` points, tiles of up to KD_WIDE_TILE positions over them, and every segment of at most `leaf`
// points as a leaf of the level at which it appeared.
struct WidePlan {
  std::vector<KdWideSeg> segs;
  std::vector<int> seg_level;  // of segs[i]
  std::vector<KdWideTile> tiles;
  std::vector<int> tile0;      // the first tile of every level, and the total behind them
  std::vector<KdWideLeaf> leaves;
  int sop_total = 0, np_max = 0;
  int levels() const { return (int)tile0.size() - 1; }
};
void wide_plan(int n, int leaf, WidePlan& P) {
  P = WidePlan{};
  std::vector<std::pair<int, int>> cur{{0, n}}, nxt;
  for (int level = 0;; level++) {
    P.tile0.push_back((int)P.tiles.size());
    nxt.clear();
    for (const auto& [lo, hi] : cur) {
      if (hi - lo > leaf) {
        const int left = kd_left(hi - lo);
        P.segs.push_back(KdWideSeg{lo, hi, left, (int)P.tiles.size()});
        for (int at = lo; at < hi; at += KD_WIDE_TILE) P.tiles.push_back(KdWideTile{at, std::min(KD_WIDE_TILE, hi - at), (int)P.segs.size() - 1});
        P.seg_level.push_back(level);
        nxt.emplace_back(lo, lo + left);
        nxt.emplace_back(lo + left, hi);
      } else {
        int NP = KD_THREADS;
        while (NP < hi - lo) NP *= 2;
        P.leaves.push_back(KdWideLeaf{lo, hi - lo, NP, level, P.sop_total});
        P.sop_total += NP;
        P.np_max = std::max(P.np_max, NP);
      }
    }
    if (nxt.empty()) break;
    cur.swap(nxt);
  }
}

// THE list of the wide ordering's scratch region for the clouds of one call: the plans' tables (the prefix the host stages
// and uploads with one copy), every cloud's small tables, and the per-point buffers, which the clouds share - they run one
// after another on the upload stream.
struct WideShape {
  size_t n_max = 0, sop_max = 0, leaves_max = 0;
  int seg_stride = 0;
};
template <class A>
inline void wide_tables_list(ScratchLayout& l, A& a, const WidePlan& P) {
  l.take(a.segs, P.segs.size());
  l.take(a.tiles, P.tiles.size());
  l.take(a.leaves, P.leaves.size());
}
inline auto wide_region_list(std::vector<KdWide>& J, const std::vector<WidePlan>& P, const WideShape& s, size_t* up_bytes) {
  return [&J, &P, s, up_bytes](ScratchLayout& l) {
    for (size_t k = 0; k < J.size(); k++) wide_tables_list(l, J[k], P[k]);
    *up_bytes = l.off;
    for (size_t k = 0; k < J.size(); k++) {
      l.take(J[k].box, 6 * KD_WIDE_BOX_BLOCKS + 3);
      l.take(J[k].hist, 1024 * P[k].segs.size());
      l.take(J[k].tile_cnt, P[k].tiles.size());
      l.take(J[k].seg_piv, P[k].segs.size());
    }
    KdWide& a = J[0];
    l.take(a.buf[0], s.n_max);
    l.take(a.buf[1], s.n_max);
    l.take(a.keys, s.n_max);
    l.take(a.seg_of_pos, s.sop_max);
    l.take(a.seg_lo, 2 * (size_t)s.seg_stride * s.leaves_max);
    for (size_t k = 1; k < J.size(); k++) {
      J[k].buf[0] = a.buf[0], J[k].buf[1] = a.buf[1], J[k].keys = a.keys;
      J[k].seg_of_pos = a.seg_of_pos, J[k].seg_lo = a.seg_lo;
    }
  };
}

// The launches of one cloud's wide ordering, back to back on `stream`: nothing comes back, nothing waits.  J.order holds the
// order when they have run.
hipError_t enqueue_wide_order(const KdWide& J, const WidePlan& P, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(J.hist, 0, sizeof(unsigned) * 1024 * P.segs.size(), stream);
  if (e != hipSuccess) return e;
  const int gb = std::min((J.n + 4 * KD_WIDE_THREADS - 1) / (4 * KD_WIDE_THREADS), KD_WIDE_BOX_BLOCKS);
  hipLaunchKernelGGL(k_kd_wide_box, dim3((unsigned)gb), dim3(KD_WIDE_THREADS), 0, stream, J);
  hipLaunchKernelGGL(k_kd_wide_ext, dim3(1), dim3(64), 0, stream, J, gb);
  for (int g = 0; g < P.levels(); g++) {
    const int t0 = P.tile0[g];
    const dim3 grid((unsigned)(P.tile0[g + 1] - t0));
    for (int pass = 0; pass < 4; pass++) hipLaunchKernelGGL(k_kd_wide_hist, grid, dim3(KD_WIDE_THREADS), 0, stream, J, g, t0, pass);
    hipLaunchKernelGGL(k_kd_wide_count, grid, dim3(KD_WIDE_THREADS), 0, stream, J, t0);
    hipLaunchKernelGGL(k_kd_wide_scatter, grid, dim3(KD_WIDE_THREADS), 0, stream, J, g, t0);
  }
  hipLaunchKernelGGL(k_kd_wide_leaves, dim3((unsigned)P.leaves.size()), dim3(KD_THREADS), sizeof(unsigned long long) * (size_t)P.np_max, stream, J);
  return hipGetLastError();
}

}  // namespace

extern "C" {

// k_scan's tile culling depends on it, never a result (CVO_NO_SORT=1 keeps the identity order).
struct KdPoint {
  float c[3];
  int i;
};
// vext != nullptr: the split axis comes from the root box's extents, halved once per split along that axis - one axis
// per level, what k_kd_order does on the device (option ORDER=virtual: the host twin of the device ordering)
static void kd_split(KdPoint* pts, int lo, int hi, const float* vext = nullptr) {
  const int n = hi - lo;
  if (n <= 4) return;
  const int unit = n > 512 ? 512 : (n > 64 ? 64 : 4);
  int left = ((n / 2 + unit - 1) / unit) * unit;
  if (left >= n) left -= unit;
  if (left <= 0) return;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (!vext)
    for (int k = lo; k < hi; k++)
      for (int c = 0; c < 3; c++) {
        const float v = pts[k].c[c];
        mn[c] = std::min(mn[c], v);
        mx[c] = std::max(mx[c], v);
      }
  else
    for (int c = 0; c < 3; c++) {
      mn[c] = 0.f;
      mx[c] = vext[c];
    }
  int axis = 0;
  for (int c = 1; c < 3; c++)
    if (mx[c] - mn[c] > mx[axis] - mn[axis]) axis = c;
  float vnext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
  vnext[axis] *= 0.5f;
  // the records themselves are permuted (no index indirection in the comparator: ~4x faster at 10k points)
  std::nth_element(pts + lo, pts + lo + left, pts + hi, [axis](const KdPoint& a, const KdPoint& b) {
    return a.c[axis] < b.c[axis] || (a.c[axis] == b.c[axis] && a.i < b.i);
  });
  kd_split(pts, lo, lo + left, vext ? vnext : nullptr);
  kd_split(pts, lo + left, hi, vext ? vnext : nullptr);
}

static void spatial_order(const float* x4, int n, std::vector<int>& order, bool no_sort, bool level_axes) {
  order.resize(n);
  for (int i = 0; i < n; i++) order[i] = i;
  if (n < 8 || no_sort) return;

  std::vector<KdPoint> pts((size_t)n);
  for (int i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) {
      const float v = x4[4 * (size_t)i + c];
      if (!std::isfinite(v)) return;  // keep the identity order for odd inputs
      pts[i].c[c] = v;
    }
    pts[i].i = i;
  }
  if (level_axes) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; i++)
      for (int c = 0; c < 3; c++) {
        mn[c] = std::min(mn[c], pts[i].c[c]);
        mx[c] = std::max(mx[c], pts[i].c[c]);
      }
    const float ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    kd_split(pts.data(), 0, n, ext);
  } else {
    kd_split(pts.data(), 0, n);
  }
  for (int r = 0; r < n; r++) order[r] = pts[r].i;
}

// One cloud: spatial order on the calling thread, ONE device allocation and ONE host-to-device copy (a hipMalloc / a
// synchronous copy cost ~100 us each) of exactly the arrays the caller supplied.  xyz: n x 3 (stride3) or n x 4
// records of `stride` bytes; feat / label / geo may be NULL.  Self-contained and thread-safe: it touches the context
// only to read its device ordinal, and copies on the stream it is given.
struct HostCloud {
  int n;
  const char* xyz;   size_t xyz_stride;    // 3 floats at xyz + i * xyz_stride
  const char* feat;  size_t feat_stride;   // FD floats, or NULL
  const char* label; size_t label_stride;  // NC floats, or NULL
  const char* geo;   size_t geo_stride;    // 2 floats, or NULL
  const int* rows = nullptr;               // optional: point i of the cloud is row rows[i] of the arrays (cvo_cloud_upload_voxel)
  size_t row(int i) const { return rows ? (size_t)rows[i] : (size_t)i; }
};

// A cloud whose spatial ordering runs on the device (k_kd_order): staged and copied, not yet ordered.  The staging
// buffer lives until the caller has synchronised the stream the copy was enqueued on.
struct StagedCloud {
  cvo_cloud* c = nullptr;
  KdJob job{};          // job.n == 0: ordered on the host, nothing left to do
  bool wide = false;    // the job is the wide ordering's (cvo_k_kd_wide.h) and k_cloud_gather's, not k_kd_order's
  std::vector<char> stage;
};

static int upload_host_cloud(cvo_ctx* ctx, const HostCloud& h, hipStream_t stream, StagedCloud* sc) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n = h.n;
  cvo_cloud* c = new cvo_cloud();
  c->ctx = ctx;
  c->device = ctx->device;
  c->n = n;
  const size_t nn = (size_t)std::max(n, 1);
  // Where the ordering runs (order_route): on the device for clouds k_kd_order holds in LDS (the host then only stages,
  // allocates and copies: ~0.1 ms of CPU per 10k cloud instead of 1.2) and, under CVO_ORDER=wide, for larger ones; on this
  // thread otherwise (tiny, huge or non-finite clouds, CVO_NO_SORT, CVO_ORDER=host).
  bool finite = true;
  for (int i = 0; i < n && finite; i++) {
    const float* p = reinterpret_cast<const float*>(h.xyz + h.row(i) * h.xyz_stride);
    finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
  }
  const int route = order_route(n, finite, ctx->opt.order, ctx->opt.no_sort);
  const bool device_order = route != ORDER_ROUTE_HOST;
  c->order_route = route;
  // one-hot class rows?  (exactly: the fast path replaces arithmetic on the rows by two constants)
  std::vector<int> lid_host;
  if (h.label && n > 0 && !ctx->opt.no_onehot) {
    lid_host.resize((size_t)n);
    bool onehot = true;
    for (int i = 0; i < n && onehot; i++) {
      lid_host[i] = label_onehot_class(reinterpret_cast<const float*>(h.label + h.row(i) * h.label_stride));  // (cvo_k_ingest.h)
      onehot = lid_host[i] >= 0;
    }
    if (!onehot) lid_host.clear();
  }
  const bool has_lid = !lid_host.empty();
  int NP = KD_THREADS;
  while (NP < n) NP *= 2;
  // (device ordering: the caller's arrays go up in ORIGINAL order - x4 stays, the raw attribute arrays are scratch - and
  // the kernel writes the spatially ordered ones; host ordering: everything is staged in its final form)
  // THE list of the slab's arrays (cloud_slab_list), walked over two bases: the staging buffer (into s) and the slab (into
  // the cloud itself and, for k_kd_order, into the job)
  size_t up_bytes = 0;  // the prefix of the slab that is staged and uploaded
  const SlabShape shape{nn, NP, h.feat != nullptr, h.label != nullptr, h.geo != nullptr, has_lid, device_order, route == ORDER_ROUTE_BLOCK};
  auto list = [&](auto& a) { return cloud_slab_list(a, shape, &up_bytes); };
  CloudArrays s;
  ScratchLayout().walk(list(s));
  std::vector<char>& stage = sc->stage;
  stage.assign(up_bytes, 0);  // (pageable: kept alive by the caller until the stream has been synchronised)
  ScratchLayout(stage.data()).walk(list(s));
  float* x4 = reinterpret_cast<float*>(s.x4);
  double sx = 0, sy = 0, sz = 0, r2max = 0;
  for (int i = 0; i < n; i++) {
    const float* p = reinterpret_cast<const float*>(h.xyz + h.row(i) * h.xyz_stride);
    x4[4 * (size_t)i] = p[0];
    x4[4 * (size_t)i + 1] = p[1];
    x4[4 * (size_t)i + 2] = p[2];
    const double px = p[0], py = p[1], pz = p[2];
    sx += px;
    sy += py;
    sz += pz;
    const double r2 = px * px + py * py + pz * pz;
    if (r2max == r2max && !(r2 <= r2max)) r2max = r2;  // a NaN sticks (an unbounded cloud is refused by the solvers)
  }
  c->rmax = (float)(std::sqrt(r2max) * 1.000001);
  if (n > 0) {
    c->cx = (float)(sx / n);
    c->cy = (float)(sy / n);
    c->cz = (float)(sz / n);
  }
  if (!std::isfinite(c->cx) || !std::isfinite(c->cy) || !std::isfinite(c->cz)) c->cx = c->cy = c->cz = 0.f;
  if (device_order) {
    if (h.feat)
      for (int i = 0; i < n; i++) std::memcpy(&s.raw_feat[FD * (size_t)i], h.feat + h.row(i) * h.feat_stride, sizeof(float) * FD);
    if (h.label)
      for (int i = 0; i < n; i++) std::memcpy(&s.raw_label[NC * (size_t)i], h.label + h.row(i) * h.label_stride, sizeof(float) * NC);
    if (h.geo)
      for (int i = 0; i < n; i++) std::memcpy(&s.raw_geo[2 * (size_t)i], h.geo + h.row(i) * h.geo_stride, sizeof(float) * 2);
    if (has_lid) std::memcpy(s.raw_lid, lid_host.data(), sizeof(int) * (size_t)n);
  } else {
    std::vector<int> order;
    spatial_order(x4, n, order, ctx->opt.no_sort, ctx->opt.order == CloudOrder::Virtual);
    // colour, class distributions and geometric types are kept in SPATIAL order only (position r holds the attributes of
    // point order[r]): the kernels index them by sorted position, like the coordinates they gather per candidate
    if (h.feat)
      for (int r = 0; r < n; r++) std::memcpy(&s.feat[FD_PAD / 4 * (size_t)r], h.feat + h.row(order[r]) * h.feat_stride, sizeof(float) * FD);
    if (h.label)
      for (int r = 0; r < n; r++) std::memcpy(&s.label[NC_PAD / 4 * (size_t)r], h.label + h.row(order[r]) * h.label_stride, sizeof(float) * NC);
    if (h.geo)
      for (int r = 0; r < n; r++) std::memcpy(&s.geo[r], h.geo + h.row(order[r]) * h.geo_stride, sizeof(float) * 2);
    if (has_lid)
      for (int r = 0; r < n; r++) s.lid[r] = lid_host[(size_t)order[r]];
    for (int r = 0; r < n; r++) s.xs4[r] = s.x4[order[r]];
    if (n > 0) std::memcpy(s.order, order.data(), sizeof(int) * (size_t)n);
    for (int r = 0; r < n; r++) s.inv[order[r]] = r;
    c->h_order = std::move(order);
  }
  if (const int rc = c->slab.lay_out(ctx, "cloud", list(*c), nullptr); rc != CVO_OK) {
    cvo_cloud_free(c);
    return rc;
  }
  if (n > 0) {
    const hipError_t e = hipMemcpyAsync(c->slab.p, stage.data(), up_bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) {
      cvo_cloud_free(c);
      return fail(ctx, CVO_E_HIP, std::string("cloud upload: ") + hipGetErrorString(e));
    }
  }
  sc->c = c;
  sc->job = KdJob{};
  sc->wide = route == ORDER_ROUTE_WIDE;
  if (device_order) {
    ScratchLayout(c->slab.p).walk(list(sc->job));
    sc->job.n = n;
    sc->job.NP = NP;
    c->h_order.assign((size_t)n, 0);
  }
  return CVO_OK;
}

// Second half of an upload: the copies of `clouds` have been enqueued (and, for upload_many, completed) - order the
// clouds that asked for it with ONE launch of k_kd_order (a block per cloud) on the context's upload stream and, one after
// another, the clouds of the wide ordering (its launches, then k_cloud_gather over all of them), bring the permutations
// back (exports map rows through them), synchronise - once.  On error every cloud of the list is released.
static int finish_uploads(cvo_ctx* ctx, std::vector<StagedCloud>& clouds) {
  std::vector<KdJob> jobs, wide_jobs;
  int np_max = 0, ggx = 1;
  for (auto& sc : clouds)
    if (sc.c && sc.job.n > 0 && !sc.wide) {
      jobs.push_back(sc.job);
      np_max = std::max(np_max, sc.job.NP);
    }
  for (auto& sc : clouds)
    if (sc.c && sc.job.n > 0 && sc.wide) {
      wide_jobs.push_back(sc.job);
      ggx = std::max(ggx, (int)std::min<long long>((5ll * sc.job.n + GATHER_THREADS - 1) / GATHER_THREADS, 4 * INGEST_MAX_BLOCKS));
    }
  // the wide clouds' plans and the staging copy of their tables (read by the copy below: alive until the synchronisation)
  std::vector<WidePlan> plans(wide_jobs.size());
  std::vector<KdWide> wide(wide_jobs.size()), wide_host(wide_jobs.size());
  std::vector<char> wide_stage;
  WideShape ws;
  ws.seg_stride = ctx->opt.wide_leaf / 2 + 2;
  for (size_t k = 0; k < wide_jobs.size(); k++) {
    wide_plan(wide_jobs[k].n, ctx->opt.wide_leaf, plans[k]);
    ws.n_max = std::max(ws.n_max, (size_t)wide_jobs[k].n);
    ws.sop_max = std::max(ws.sop_max, (size_t)plans[k].sop_total);
    ws.leaves_max = std::max(ws.leaves_max, plans[k].leaves.size());
  }
  hipError_t e = hipSuccess;
  int rc = CVO_OK;
  std::lock_guard<std::mutex> lk(ctx->kd_mutex);
  if (!jobs.empty() || !wide_jobs.empty()) {
    // (nothing to drain: the launch that read the table last was synchronised below, under this mutex)
    const std::vector<KdJob>* tables[2] = {&jobs, &wide_jobs};
    KdJob* d_jobs[2] = {nullptr, nullptr};
    rc = ctx->d_kd_jobs.lay_out(ctx, "ordering job table", [&](ScratchLayout& l) {
      l.take(d_jobs[0], jobs.size());
      l.take(d_jobs[1], wide_jobs.size());
    }, nullptr);
    for (int q = 0; q < 2; q++)
      if (rc == CVO_OK && e == hipSuccess && !tables[q]->empty())
        e = hipMemcpyAsync(d_jobs[q], tables[q]->data(), sizeof(KdJob) * tables[q]->size(), hipMemcpyHostToDevice, ctx->upload_stream);
    if (rc == CVO_OK && e == hipSuccess && !jobs.empty()) {
      hipLaunchKernelGGL(k_kd_order, dim3((unsigned)jobs.size()), dim3(KD_THREADS), sizeof(unsigned long long) * (size_t)np_max,
                         ctx->upload_stream, (const KdJob*)d_jobs[0]);
      e = hipGetLastError();
    }
    if (rc == CVO_OK && e == hipSuccess && !wide_jobs.empty()) {
      size_t up_bytes = 0;
      rc = ctx->d_kd_wide.lay_out(ctx, "wide ordering scratch", wide_region_list(wide, plans, ws, &up_bytes), nullptr);
      if (rc == CVO_OK) {
        wide_stage.assign(up_bytes, 0);
        ScratchLayout host(wide_stage.data());
        for (size_t k = 0; k < wide.size(); k++) {
          wide_tables_list(host, wide_host[k], plans[k]);
          std::memcpy(const_cast<KdWideSeg*>(wide_host[k].segs), plans[k].segs.data(), sizeof(KdWideSeg) * plans[k].segs.size());
          std::memcpy(const_cast<KdWideTile*>(wide_host[k].tiles), plans[k].tiles.data(), sizeof(KdWideTile) * plans[k].tiles.size());
          std::memcpy(const_cast<KdWideLeaf*>(wide_host[k].leaves), plans[k].leaves.data(), sizeof(KdWideLeaf) * plans[k].leaves.size());
        }
        e = hipMemcpyAsync(ctx->d_kd_wide.p, wide_stage.data(), up_bytes, hipMemcpyHostToDevice, ctx->upload_stream);
      }
      for (size_t k = 0; rc == CVO_OK && e == hipSuccess && k < wide.size(); k++) {
        wide[k].n = wide_jobs[k].n;
        wide[k].seg_stride = ws.seg_stride;
        wide[k].x4 = wide_jobs[k].x4;
        wide[k].order = wide_jobs[k].order;
        e = enqueue_wide_order(wide[k], plans[k], ctx->upload_stream);
      }
      if (rc == CVO_OK && e == hipSuccess) {
        hipLaunchKernelGGL(k_cloud_gather, dim3((unsigned)ggx, (unsigned)wide_jobs.size()), dim3(GATHER_THREADS), 0, ctx->upload_stream,
                           (const KdJob*)d_jobs[1]);
        e = hipGetLastError();
      }
    }
    for (auto& sc : clouds)
      if (rc == CVO_OK && e == hipSuccess && sc.c && sc.job.n > 0)
        e = hipMemcpyAsync(sc.c->h_order.data(), sc.c->order, sizeof(int) * (size_t)sc.job.n, hipMemcpyDeviceToHost, ctx->upload_stream);
    // WIDE_RECORD=1 (tests): the select's pivots of every wide cloud come down next to its order
    if (ctx->opt.wide_record && !wide_jobs.empty()) {
      size_t k = 0;
      for (auto& sc : clouds) {
        if (!(sc.c && sc.job.n > 0 && sc.wide)) continue;
        if (rc == CVO_OK && e == hipSuccess) {
          static_assert(sizeof(uint2) == 2 * sizeof(unsigned), "seg_piv is two words a segment");
          sc.c->h_wide_piv.assign(2 * plans[k].segs.size(), 0u);
          e = hipMemcpyAsync(sc.c->h_wide_piv.data(), wide[k].seg_piv, sizeof(uint2) * plans[k].segs.size(), hipMemcpyDeviceToHost, ctx->upload_stream);
        }
        k++;
      }
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->upload_stream);
  if (rc != CVO_OK || e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->upload_stream);  // (launches that read this call's tables and clouds may be in flight)
    for (auto& sc : clouds) {
      if (sc.c) cvo_cloud_free(sc.c);
      sc.c = nullptr;
    }
    return rc != CVO_OK ? rc : fail(ctx, CVO_E_HIP, std::string("cloud upload (ordering): ") + hipGetErrorString(e));
  }
  return CVO_OK;
}

// One cloud on the context's upload stream; the caller holds upload_mutex (the front ends' uploads, upload_one).
static int upload_one_locked(cvo_ctx* ctx, const HostCloud& h, cvo_cloud** out) {
  std::vector<StagedCloud> one(1);
  int rc = upload_host_cloud(ctx, h, ctx->upload_stream, &one[0]);
  if (rc != CVO_OK) return rc;
  rc = finish_uploads(ctx, one);
  if (rc != CVO_OK) return rc;
  *out = one[0].c;
  return CVO_OK;
}

// ... taking the mutex (cvo_cloud_upload, cvo_cloud_upload_aos192)
static int upload_one(cvo_ctx* ctx, const HostCloud& h, cvo_cloud** out) {
  std::lock_guard<std::mutex> lk(ctx->upload_mutex);
  return upload_one_locked(ctx, h, out);
}

int cvo_cloud_upload(cvo_ctx* ctx, int n, const float* xyz, const float* feat, const float* label,
                     const float* geotype, cvo_cloud** out) {
  if (!ctx || !out || n < 0 || (n > 0 && !xyz)) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload: bad argument");
  const HostCloud h{n, (const char*)xyz, 12, (const char*)feat, sizeof(float) * FD, (const char*)label, sizeof(float) * NC,
                    (const char*)geotype, 8};
  return upload_one(ctx, h, out);
}

// n_clouds clouds from a pool of host threads (each cloud: spatial ordering on its thread, one allocation, one copy on
// that thread's own stream).  Arrays of per-cloud pointers; feat / label / geotype (the arrays or single entries) may be
// NULL.  On error every cloud of the call is released.
static int upload_many_impl(cvo_ctx* ctx, int n_clouds, const int* n, const float* const* xyz, const float* const* feat,
                            const float* const* label, const float* const* geotype, int threads, cvo_cloud** out) {
  if (!ctx || !out || n_clouds < 0 || (n_clouds > 0 && (!n || !xyz)))
    return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_many: bad argument");
  for (int q = 0; q < n_clouds; q++) {
    out[q] = nullptr;
    if (n[q] < 0 || (n[q] > 0 && !xyz[q])) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_many: bad cloud");
  }
  if (n_clouds == 0) return CVO_OK;
  // (with the ordering on the device a cloud costs its thread ~0.08 ms - staging, one hipMalloc, one copy - and the
  // allocator serialises: 128 clouds take 10.0 / 8.0 / 7.3 / 8.2 ms of wall time with 1 / 2 / 4 / 16 threads)
  const int T = std::max(1, std::min(std::min(threads > 0 ? threads : 4, n_clouds), 64));
  std::vector<int> rcs(T, CVO_OK);
  std::vector<std::string> errs(T);
  std::atomic<int> next(0);
  std::vector<StagedCloud> staged((size_t)n_clouds);
  auto work_body = [&](int t) {
    // Every thread copies on the context's ONE upload stream (enqueueing from several threads is legal; a pageable
    // source makes each copy synchronous for its thread anyway).  No temporary streams: HIP deals streams onto hardware
    // queues in creation order, and streams created between two contexts used to push a later context's sub-batch
    // streams onto shared queues (3x slower batches, scripts/upload_probe.py).
    hipStream_t s = ctx->upload_stream;
    if (hipSetDevice(ctx->device) != hipSuccess) {
      rcs[t] = CVO_E_HIP;
      errs[t] = "cvo_cloud_upload_many: hipSetDevice failed";
      return;
    }
    cvo_ctx local;  // error text of this thread (the shared context's string is not thread-safe)
    local.device = ctx->device;
    local.opt = ctx->opt;
    for (;;) {
      const int q = next.fetch_add(1);
      if (q >= n_clouds || rcs[t] != CVO_OK) break;
      const HostCloud h{n[q], (const char*)xyz[q], 12, (const char*)(feat ? feat[q] : nullptr), sizeof(float) * FD,
                        (const char*)(label ? label[q] : nullptr), sizeof(float) * NC,
                        (const char*)(geotype ? geotype[q] : nullptr), 8};
      const int rc = upload_host_cloud(&local, h, s, &staged[q]);
      if (rc != CVO_OK) {
        rcs[t] = rc;
        errs[t] = local.err;
        break;
      }
      staged[q].c->ctx = ctx;
      out[q] = staged[q].c;
    }
    // (the ordering kernel of the call is launched on the same stream: it runs after every copy)
  };
  auto work = [&](int t) {  // (bad_alloc of a staging buffer etc. must not leave a worker or cross the C ABI)
    try {
      work_body(t);
    } catch (const std::exception& e) {
      rcs[t] = CVO_E_NOMEM;
      errs[t] = std::string("cvo_cloud_upload_many: ") + e.what();
    } catch (...) {
      rcs[t] = CVO_E_NOMEM;
      errs[t] = "cvo_cloud_upload_many: unknown exception";
    }
  };
  std::vector<std::thread> pool;
  try {
    for (int t = 1; t < T; t++) pool.emplace_back(work, t);
  } catch (const std::exception&) {  // thread limit: the threads already started share the work with this one
  }
  work(0);
  for (auto& th : pool) th.join();
  for (int t = 0; t < T; t++)
    if (rcs[t] != CVO_OK) {
      for (int q = 0; q < n_clouds; q++) {
        if (out[q]) cvo_cloud_free(out[q]);
        out[q] = nullptr;
      }
      return fail(ctx, rcs[t], errs[t]);
    }
  const int rc = finish_uploads(ctx, staged);  // the spatial ordering of all clouds: one kernel launch
  if (rc != CVO_OK)
    for (int q = 0; q < n_clouds; q++) out[q] = nullptr;
  return rc;
}

int cvo_cloud_upload_many(cvo_ctx* ctx, int n_clouds, const int* n, const float* const* xyz, const float* const* feat,
                          const float* const* label, const float* const* geotype, int threads, cvo_cloud** out) {
  try {
    return upload_many_impl(ctx, n_clouds, n, xyz, feat, label, geotype, threads, out);
  } catch (const std::exception& e) {  // (allocation of the pool's bookkeeping itself)
    if (out)
      for (int q = 0; q < n_clouds; q++) {
        if (out[q]) cvo_cloud_free(out[q]);
        out[q] = nullptr;
      }
    return fail(ctx, CVO_E_NOMEM, std::string("cvo_cloud_upload_many: ") + e.what());
  }
}

int cvo_cloud_upload_aos192(cvo_ctx* ctx, int n, const void* pts, cvo_cloud** out) {
  if (!ctx || !out || n < 0 || (n > 0 && !pts)) return fail(ctx, CVO_E_INVALID, "cvo_cloud_upload_aos192: bad argument");
  // PointSegmentedDistribution<5,19> byte offsets: xyz@0, features@20,
  // label_distribution@44, geometric_type@120, sizeof = 192: read in place, record by record.
  const char* b = (const char*)pts;
  const HostCloud h{n, b, 192, b + 20, 192, b + 44, 192, b + 120, 192};
  return upload_one(ctx, h, out);
}

// ---- multi-frame edge kernel ---------------------------------------------------------
// cull centre and motion bound of a cloud moved by a pose (neither influences a result)
static void transformed_bounds(const cvo_cloud* in, const float T[12], cvo_cloud* c) {
  c->cx = T[0] * in->cx + T[1] * in->cy + T[2] * in->cz + T[3];
  c->cy = T[4] * in->cx + T[5] * in->cy + T[6] * in->cz + T[7];
  c->cz = T[8] * in->cx + T[9] * in->cy + T[10] * in->cz + T[11];
  if (!std::isfinite(c->cx) || !std::isfinite(c->cy) || !std::isfinite(c->cz)) c->cx = c->cy = c->cz = 0.f;
  double fro = 0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) fro += (double)T[4 * i + j] * T[4 * i + j];
  c->rmax = (float)((std::sqrt(fro) * in->rmax + std::sqrt((double)T[3] * T[3] + (double)T[7] * T[7] + (double)T[11] * T[11])) * 1.000001);
}

int cvo_cloud_transformed(cvo_ctx* ctx, const cvo_cloud* in, const float pose12[12], cvo_cloud** out) {
  if (!ctx || !in || !pose12 || !out) return fail(ctx, CVO_E_INVALID, "cvo_cloud_transformed: bad argument");
  if (in->ctx != ctx) return fail(ctx, CVO_E_INVALID, "cloud belongs to another context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  cvo_cloud* c = new cvo_cloud();
  c->ctx = ctx;
  c->device = ctx->device;
  c->n = in->n;
  c->h_order = in->h_order;
  c->order_route = in->order_route;
  if (const int rc = c->slab.reserve(ctx, in->slab.bytes, "cloud", nullptr); rc != CVO_OK) {
    delete c;
    return rc;
  }
  // same slab layout: features, labels, geometric types and the spatial order are copied, coordinates rewritten
  // (attributes the input was uploaded without - NULL or pointing into its zero slab - stay absent in the copy)
  const ScratchLayout l(c->slab.p);
  auto rebase = [&](auto*& to, const auto* from) {
    const char* q = (const char*)from;
    if (q && q >= in->slab.p && q < in->slab.p + in->slab.bytes) l.at(to, (size_t)(q - in->slab.p));
  };
  rebase(c->x4, in->x4);
  rebase(c->xs4, in->xs4);
  rebase(c->feat, in->feat);
  rebase(c->label, in->label);
  rebase(c->geo, in->geo);
  rebase(c->lid, in->lid);
  rebase(c->order, in->order);
  rebase(c->inv, in->inv);
  Pose12 P;
  for (int q = 0; q < 12; q++) P.T[q] = pose12[q];
  if (in->n > 0) {
    hipError_t e = hipMemcpyAsync(c->slab.p, in->slab.p, in->slab.bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_transform_pose, dim3((in->n + 255) / 256), dim3(256), 0, ctx->stream, in->n, P, in->x4, in->xs4,
                         c->x4, c->xs4);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      cvo_cloud_free(c);
      return fail(ctx, CVO_E_HIP, std::string("cvo_cloud_transformed: ") + hipGetErrorString(e));
    }
  }
  transformed_bounds(in, pose12, c);
  *out = c;
  return CVO_OK;
}

int cvo_cloud_size(const cvo_cloud* c) { return c ? c->n : 0; }

void cvo_cloud_free(cvo_cloud* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

}  // extern "C"
