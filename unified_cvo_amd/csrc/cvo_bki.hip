// cvo_bki.hip -- the semantic voxel map: cvo_map_open / _insert / _insert_posed / _size / _cloud / _close, their _host twins
// on a map without a context, cvo_map_insert_cloud / cvo_map_cloud_resident (a resident cloud in, a resident cloud out: the
// hits staged by k_bki_stage, the rows read out handed to cvo_ingest.hip where they are), the read side (cvo_map_query /
// _raycast / _render) and cvo_debug_map_stats.  What is computed: tests/np_bki.py, np_bki_sparse.py (cvo_map_set_kernel
// chooses), np_bki_query.py.  A map lives on ONE side: a map of a context takes its side at its first insert (switch
// BKI_HOST; unset: by that insert's training points) and keeps it, its table does not migrate.  HERE: the handle, the side
// rule and the device side (the table, the inserts' one tail, the read-out, the read calls with one output table each).
// The host side is cvo_bki_twin.h (BkiTwin: plain C++ that knows nothing of this file); both share cvo_bki_math.h.
// A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
#include "cvo_bki_twin.h"

using namespace cvo_bki;

namespace {

// training points of a map's FIRST insert below which the map lives on the host: the smallest frame whose ten inserts and
// read-out took the device less time than the twin (profiles/bki/bki_probe.txt)
constexpr long long BKI_HOST_BELOW = 2129;
// ... and the same for a map whose kernel is the sparse one at its first insert (profiles/bki_sparse/bki_sparse_probe.txt): the
// twin's sparse insert costs several times its counting insert, the device's less than twice
constexpr long long BKI_SPARSE_HOST_BELOW = 547;

// the device side of a map: one allocation behind the table; the hits of an insert and its work arrays
struct BkiDeviceMap {
  BkiTable t{};
  DeviceRegion slab;
  unsigned long long slots = 0, voxels = 0, initial_slots = 0;
  int growths = 0;
  DeviceScratch in_scratch, work_scratch;
};

}  // namespace

struct cvo_map {
  cvo_ctx* ctx = nullptr;  // nullptr: a host-only map.  From here to `last`: what both sides share
  cvo_map_config_t cfg{};
  BkiConst k{};
  int side = -1;  // -1: no insert yet; 0: the device; 1: the host
  int kernel = CVO_MAP_KERNEL_CSM;  // cvo_map_set_kernel: what the next insert runs
  bool broken = false;
  long long occupied = -1;  // -1: not counted since the last insert
  BkiStats last{};
  BkiTwin host;      // live on side 1 (and read, empty, while the side is undecided)
  BkiDeviceMap dev;  // live on side 0; initial_slots from cvo_map_open on
};

namespace {

int bki_validate_config(const cvo_map_config_t* c, std::string* msg) {
  if (!c) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (!std::isfinite(c->resolution) || !(c->resolution > 0.f)) return *msg = "resolution must be finite and > 0", CVO_E_INVALID;
  if (!std::isfinite(c->free_resolution) || !(c->free_resolution > 0.f)) return *msg = "free_resolution must be finite and > 0", CVO_E_INVALID;
  if (!(c->free_thresh >= 0.f && c->free_thresh <= 1.f) || !(c->occupied_thresh >= 0.f && c->occupied_thresh <= 1.f))
    return *msg = "free_thresh and occupied_thresh lie in [0, 1]", CVO_E_INVALID;
  if (!std::isfinite(c->prior) || c->prior < 0.f) return *msg = "prior must be finite and >= 0", CVO_E_INVALID;
  if (!std::isfinite(c->max_range)) return *msg = "max_range must be finite (<= 0: off)", CVO_E_INVALID;
  if (c->num_classes < 0 || c->num_classes > BKI_MAX_CLASSES) return *msg = "num_classes lies in 0 .. 19", CVO_E_INVALID;
  if (c->block_depth != 1) return *msg = "only block_depth 1 is built", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

BkiConst bki_const(const cvo_map_config_t& c) {
  BkiConst k;
  k.size = c.resolution;
  k.half = c.resolution / 2.0f;
  k.prior = c.prior;
  k.free_thresh = c.free_thresh;
  k.occupied_thresh = c.occupied_thresh;
  k.free_resolution = c.free_resolution;
  k.max_range = c.max_range;
  k.C = c.num_classes;
  k.nclass = std::max(c.num_classes, 1) + 1;
  return k;
}

// what every insert of host rows checks before either route: the pointers, the size, every coordinate finite
int bki_validate_insert(const cvo_map* m, int n, const float* xyz, const float* label, const float* origin, std::string* msg) {
  if (!m || !origin || n < 0 || (n > 0 && !xyz)) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (n > 0 && m->k.C > 0 && !label) return *msg = BKI_SAYS_NEEDS_LABELS, CVO_E_INVALID;
  if (m->broken) return *msg = BKI_SAYS_BROKEN, CVO_E_HIP;
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return *msg = "the origin is not finite", CVO_E_INVALID;
  for (size_t i = 0; i < 3 * (size_t)n; i++)
    if (!std::isfinite(xyz[i])) return *msg = "hit " + std::to_string(i / 3) + " has a coordinate that is not finite", CVO_E_INVALID;
  if ((long long)n >= BKI_MAX_TRAINING) return *msg = BKI_SAYS_MANY_ROWS, CVO_E_UNSUPPORTED;
  return CVO_OK;
}

// ---- device route ----
unsigned bki_blocks(unsigned long long n) { return (unsigned)((n + BKI_THREADS - 1) / BKI_THREADS); }
unsigned bki_stride_blocks(unsigned long long n) { return std::max(1u, std::min(bki_blocks(n), (unsigned)BKI_GRID_MAX)); }

// a fresh table of `slots` slots: keys empty, ms = prior, fs and the counters zero
int bki_table_alloc(cvo_map* m, unsigned long long slots, BkiTable* t, DeviceRegion* slab) {
  cvo_ctx* ctx = m->ctx;
  const BkiConst& k = m->k;
  const int ncnt = k.nclass + 1;
  *t = BkiTable{nullptr, nullptr, nullptr, nullptr, nullptr, (unsigned)(slots - 1), k.nclass, ncnt};
  auto list = [&](ScratchLayout& l) {
    l.take(t->keys, slots);
    l.take(t->ms, slots * (size_t)k.nclass);
    l.take(t->fs, slots * BKI_FEAT);
    l.take(t->cnt, slots * (size_t)ncnt);
    l.take(t->segoff, slots);
  };
  if (const int rc = slab->lay_out(ctx, "voxel map table", list, nullptr); rc != CVO_OK) return rc;
  hipStream_t st = ctx->upload_stream;
  hipError_t r = hipMemsetAsync(t->keys, 0xFF, 8 * slots, st);
  if (r == hipSuccess) r = hipMemsetAsync(t->fs, 0, 4 * slots * BKI_FEAT, st);
  if (r == hipSuccess) r = hipMemsetAsync(t->cnt, 0, 4 * slots * (size_t)ncnt, st);
  if (r == hipSuccess) {
    hipLaunchKernelGGL(k_bki_fill, dim3(bki_stride_blocks(slots * (size_t)k.nclass)), dim3(BKI_THREADS), 0, st, t->ms, (size_t)slots * k.nclass, k.prior);
    r = hipGetLastError();
  }
  if (r != hipSuccess) {
    (void)hipStreamSynchronize(st);  // (what was enqueued writes the table: it goes with the caller's owner only after this)
    slab->release();
    return fail(ctx, CVO_E_HIP, std::string("voxel map table: ") + hipGetErrorString(r));
  }
  return CVO_OK;
}

// The table doubles - a fresh one, k_bki_rehash of the old one into it - until `need` voxels fill at most half of it.  The
// old table goes only once its contents stand in the new one: an error leaves the map as it was.
int bki_table_grow(cvo_map* m, unsigned long long need) {
  BkiDeviceMap& d = m->dev;
  while (2 * need > d.slots) {
    const unsigned long long slots = d.slots ? 2 * d.slots : d.initial_slots;
    if (slots > BKI_MAX_SLOTS) return fail(m->ctx, CVO_E_UNSUPPORTED, "the voxel map would need more than 2^30 slots");
    BkiTable t{};
    DeviceRegion slab;
    int rc = bki_table_alloc(m, slots, &t, &slab);
    if (rc != CVO_OK) return rc;
    hipError_t e = hipSuccess;
    if (d.slab.p) {
      hipLaunchKernelGGL(k_bki_rehash, dim3(bki_stride_blocks(d.slots)), dim3(BKI_THREADS), 0, m->ctx->upload_stream, d.t, t);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(m->ctx->upload_stream);
    if (e != hipSuccess) return fail(m->ctx, CVO_E_HIP, std::string("voxel map rehash: ") + hipGetErrorString(e));
    if (d.slab.p) d.growths++;
    d.slab = std::move(slab);  // (the old table goes here)
    d.t = t;
    d.slots = slots;
  }
  return CVO_OK;
}

// The insert scratch of n hits, the layout k_bki_count ... k_bki_long read (and k_bki_stage writes): `a` bound to it, its
// control block enqueued in its start state.  has_feat: the hits carry feature rows.
int bki_insert_scratch(cvo_map* m, int n, bool has_feat, const float* origin, BkiInsertArgs* a) {
  cvo_ctx* ctx = m->ctx;
  const BkiConst& k = m->k;
  const size_t nn = (size_t)n;
  *a = BkiInsertArgs{};
  a->k = k;
  a->n = n;
  for (int q = 0; q < 3; q++) a->origin[q] = origin[q];
  const int rc = m->dev.in_scratch.lay_out(ctx, "voxel map insert scratch", [&](ScratchLayout& l) {
    l.take(a->ctl, 1);
    l.take(a->xyz, 3 * nn);
    if (has_feat) l.take(a->feat, BKI_FEAT * nn);
    if (k.C > 0) l.take(a->label, (size_t)k.C * nn);
    l.take(a->mc, nn + 1);
    l.take(a->hslot, BKI_HIT_SLOTS * nn);
  });
  if (rc != CVO_OK) return rc;
  BkiCtl h{};
  h.bad_index = h.nonfinite = ~0u;
  HIP_TRY(ctx, hipMemcpyAsync(a->ctl, &h, sizeof h, hipMemcpyHostToDevice, ctx->upload_stream));
  return CVO_OK;
}

// what k_bki_count found that refuses the insert, as `who`
int bki_count_refusal(cvo_ctx* ctx, const std::string& who, const BkiCtl& h, int n) {
  // (the caps come first, as in the statement: k_bki_count goes on counting behind a bad block index)
  if (h.status & BKI_BAD_TOO_MANY)  // (bad_index is the first bad hit of any kind: named only when this is the one kind)
    return fail(ctx, CVO_E_UNSUPPORTED, who + ": " + (h.status == BKI_BAD_TOO_MANY ? bki_bad_text(h.status, h.bad_index, n) : std::string("a hit needs 65536 beam samples or more")));
  if (h.training >= (unsigned long long)BKI_MAX_TRAINING) return fail(ctx, CVO_E_UNSUPPORTED, who + ": " + BKI_SAYS_MANY_TRAINING);
  if (h.status) return fail(ctx, h.status & BKI_BAD_RANGE ? CVO_E_INVALID : CVO_E_UNSUPPORTED, who + ": " + bki_bad_text(h.status, h.bad_index, n));
  return CVO_OK;
}

// THE tail of an insert whose hits are staged and counted (h: the control block k_bki_count left, nothing refused) and whose
// work scratch is laid out: the table grows until `more` new voxels fit and is bound to a.t, launch() enqueues the kernels of
// the map's kernel, the control block comes back with what they counted.
template <class Launch>
int bki_insert_run(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, unsigned long long more, BkiStats* stats, Launch&& launch) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  if (const int rc = bki_table_grow(m, m->dev.voxels + more); rc != CVO_OK) return rc;
  a.t = m->dev.t;
  m->broken = true;  // (until the table's counters are back at zero)
  launch();
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  m->broken = false;
  m->dev.voxels += h.fresh;
  stats->training = h.training;
  stats->members = h.members;
  stats->longest_run = h.longest_run;
  stats->longest_probe = h.longest_probe;
  return CVO_OK;
}

// The counting insert: its work arrays, room in the table for every membership to be a new voxel, k_bki_emit ... k_bki_long.
int bki_insert_counted(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, BkiStats* stats) {
  hipStream_t st = m->ctx->upload_stream;
  const size_t nn = (size_t)a.n;
  const dim3 per_hit(bki_blocks(nn + 1)), block(BKI_THREADS);
  const int rc = m->dev.work_scratch.lay_out(m->ctx, "voxel map work scratch", [&](ScratchLayout& l) {
    l.take(a.rec, h.members);
    l.take(a.seg, h.hit_members);
    l.take(a.seg2, h.hit_members);
    l.take(a.longlist, 2 * (h.hit_members / (BKI_SHORT_RUN + 1) + 1));  // ((slot, hits) per voxel)
  });
  if (rc != CVO_OK) return rc;
  return bki_insert_run(m, a, h, h.members, stats, [&] {
    hipLaunchKernelGGL(k_bki_emit, per_hit, block, 0, st, a);
    hipLaunchKernelGGL(k_bki_alloc, dim3(bki_stride_blocks(h.members)), block, 0, st, a);
    if (a.n) hipLaunchKernelGGL(k_bki_scatter, dim3(bki_blocks(nn * BKI_HIT_SLOTS)), block, 0, st, a);
    hipLaunchKernelGGL(k_bki_update, dim3(bki_stride_blocks(h.members)), block, 0, st, a);
    if (a.feat && h.hit_members > (unsigned long long)BKI_SHORT_RUN)
      hipLaunchKernelGGL(k_bki_long, dim3((unsigned)std::min<unsigned long long>(h.hit_members / (BKI_SHORT_RUN + 1), BKI_GRID_MAX)), dim3(BKI_WAVE), 0, st, a);
  });
}

// The insert under the sparse kernel: the table grows by seven voxels per membership - a block and its face neighbours -, the
// records are stored, sorted by block, summed per test voxel (cvo_k_bki_sparse.h).
int bki_insert_counted_sparse(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, BkiStats* stats, const std::string& who) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  if (h.members >= (unsigned long long)BKI_SPARSE_MAX_RECORDS) return fail(ctx, CVO_E_UNSUPPORTED, who + ": " + BKI_SAYS_MANY_RECORDS);
  const size_t nrec = (size_t)h.members, nn = (size_t)a.n;
  const unsigned nb = (unsigned)((nrec + SORT_THREADS - 1) / SORT_THREADS);
  BkiSparseArgs s{};
  unsigned* hist = nullptr;
  const int rc = m->dev.work_scratch.lay_out(ctx, "voxel map work scratch", [&](ScratchLayout& l) {
    l.take(s.key[0], nrec);
    l.take(s.key[1], nrec);
    l.take(s.val[0], nrec);
    l.take(s.val[1], nrec);
    l.take(s.pt, 3 * nrec);
    l.take(s.meta, nrec);
    l.take(s.base, nn + 2);
    l.take(hist, 256 * (size_t)nb);
    l.take(s.tests, BKI_SPARSE_SLOTS * nrec);
    l.take(s.longlist, BKI_SPARSE_SLOTS * nrec / (BKI_SHORT_RUN + 1) + 1);
  });
  if (rc != CVO_OK) return rc;
  s.sf2 = m->cfg.sf2;
  s.ell = m->cfg.ell;
  s.n_rec = (unsigned)nrec;
  return bki_insert_run(m, a, h, BKI_SPARSE_SLOTS * h.members, stats, [&] {
    s.a = a;  // (with the table bound)
    if (!nrec) return;  // (no membership: the origin alone, in a rounding gap between two boxes)
    const dim3 block(BKI_THREADS);
    hipLaunchKernelGGL(k_bkis_offsets, dim3(1), dim3(BKIS_SCAN_THREADS), 0, st, s);
    hipLaunchKernelGGL(k_bkis_emit, dim3(bki_blocks(nn + 1)), block, 0, st, s);
    sort_pairs_u64(ctx, s.n_rec, s.key, s.val, hist);
    const unsigned tests_grid = bki_stride_blocks(BKI_SPARSE_SLOTS * nrec);
    hipLaunchKernelGGL(k_bkis_heads, dim3(bki_blocks(nrec)), block, 0, st, s);
    hipLaunchKernelGGL(k_bkis_update, dim3(tests_grid), block, 0, st, s);
    hipLaunchKernelGGL(k_bkis_long, dim3((unsigned)std::min<size_t>(BKI_SPARSE_SLOTS * nrec / (BKI_SHORT_RUN + 1) + 1, BKI_GRID_MAX)), dim3(BKI_WAVE), 0, st, s);
    hipLaunchKernelGGL(k_bkis_reset, dim3(tests_grid), block, 0, st, s);
  });
}

// The hits of an insert are staged in `a`.  counted: the control block k_bki_count left, already read (the resident route
// decides its side by it); nullptr: k_bki_count runs here.  Then the refusal by what it found, or the insert of the map's kernel.
int bki_insert_staged(cvo_map* m, const std::string& who, BkiInsertArgs& a, const BkiCtl* counted, BkiStats* stats) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  BkiCtl h{};
  if (counted) {
    h = *counted;
  } else {
    hipLaunchKernelGGL(k_bki_count, dim3(bki_blocks((size_t)a.n + 1)), dim3(BKI_THREADS), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  if (const int rc = bki_count_refusal(ctx, who, h, a.n); rc != CVO_OK) return rc;
  return m->kernel == CVO_MAP_KERNEL_SPARSE ? bki_insert_counted_sparse(m, a, h, stats, who) : bki_insert_counted(m, a, h, stats);
}

// host rows onto the device: staged by three copies, then as above
int bki_insert_device(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  const BkiConst& k = m->k;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  BkiInsertArgs a{};
  const int rc = bki_insert_scratch(m, n, feat != nullptr, origin, &a);
  if (rc != CVO_OK) return rc;
  if (n) HIP_TRY(ctx, hipMemcpyAsync((void*)a.xyz, xyz, 12 * nn, hipMemcpyHostToDevice, st));
  if (n && feat) HIP_TRY(ctx, hipMemcpyAsync((void*)a.feat, feat, 4 * BKI_FEAT * nn, hipMemcpyHostToDevice, st));
  if (n && k.C > 0) HIP_TRY(ctx, hipMemcpyAsync((void*)a.label, label, 4 * (size_t)k.C * nn, hipMemcpyHostToDevice, st));
  return bki_insert_staged(m, "cvo_map_insert", a, nullptr, stats);
}

// The fork every insert ends in once its side is known.  Side 1: the twin on host rows, its text wrapped.  Side 0: the
// device, on the hits staged in *staged (counted: see bki_insert_staged) or, without any, on the host rows.  Then the map
// takes the side and the insert's statistics.
int bki_insert_on_side(cvo_map* m, const std::string& who, int side, int n, const float* xyz, const float* feat, const float* label,
                       const float* origin, BkiInsertArgs* staged, const BkiCtl* counted) {
  BkiStats stats;
  int r = CVO_OK;
  if (side == 1) {
    std::string text;
    r = m->kernel == CVO_MAP_KERNEL_SPARSE ? m->host.insert_sparse(m->k, m->cfg.sf2, m->cfg.ell, n, xyz, feat, label, origin, &stats, &text)
                                           : m->host.insert_csm(m->k, n, xyz, feat, label, origin, &stats, &text);
    if (r != CVO_OK) return fail(m->ctx, r, who + ": " + text);
  } else {
    stats.on_device = 1;
    r = staged ? bki_insert_staged(m, who, *staged, counted, &stats) : bki_insert_device(m, n, xyz, feat, label, origin, &stats);
    if (r != CVO_OK) return r;
  }
  m->side = side;
  m->last = stats;
  m->occupied = -1;
  return CVO_OK;
}

// Collects and sorts the occupied voxels of a device map; *okey / *oslot point at the sorted arrays in work_scratch, *rows at
// room for the rows behind them.  count_only: one pass over the table that writes nothing but the number.
int bki_collect_device(cvo_map* m, bool count_only, unsigned* n_occ, const unsigned long long** okey, const unsigned** oslot, float** rows) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t V = count_only ? 0 : (size_t)m->dev.voxels, nbmax = bki_blocks(V);
  BkiCtl* ctl = nullptr;
  unsigned long long* key[2] = {nullptr, nullptr};
  unsigned *slot[2] = {nullptr, nullptr}, *hist = nullptr;
  const int rc = m->dev.work_scratch.lay_out(ctx, "voxel map work scratch", [&](ScratchLayout& l) {
    l.take(ctl, 1);
    l.take(key[0], V);
    l.take(key[1], V);
    l.take(slot[0], V);
    l.take(slot[1], V);
    l.take(hist, 256 * nbmax);
    l.take(*rows, V * (size_t)(3 + BKI_FEAT + NC_PAD));  // (label rows: packed, or at the resident cloud's padded stride)
  });
  if (rc != CVO_OK) return rc;
  *okey = key[0];
  *oslot = slot[0];
  *n_occ = 0;
  if (!m->dev.voxels) return m->occupied = 0, CVO_OK;
  BkiCtl h{};
  HIP_TRY(ctx, hipMemsetAsync(ctl, 0, sizeof *ctl, st));
  hipLaunchKernelGGL(k_bki_occupied, dim3(bki_stride_blocks(m->dev.slots)), dim3(BKI_THREADS), 0, st, m->k, m->dev.t, count_only ? nullptr : key[0],
                     count_only ? nullptr : slot[0], ctl);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (h.n_occ > m->dev.voxels) return fail(ctx, CVO_E_HIP, "cvo_map_cloud: the device found more occupied voxels than the map holds");
  const unsigned n = h.n_occ;
  if (!count_only) sort_pairs_u64(ctx, n, key, slot, hist);
  HIP_TRY(ctx, hipGetLastError());
  *n_occ = n;
  m->occupied = n;
  return CVO_OK;
}

// THE read-out of a device map: the occupied voxels collected, their rows carved out of the work scratch and - want_rows - written
// by k_bki_rows in ascending key order, a label row every `label_stride` floats; *d names them as ingest rows.  Nothing is synchronised.
int bki_rows_device(cvo_map* m, bool want_rows, int label_stride, cvo_device_rows_t* d) {
  cvo_ctx* ctx = m->ctx;
  unsigned n = 0;
  const unsigned long long* okey;
  const unsigned* oslot;
  float* xyz;
  const int rc = bki_collect_device(m, !want_rows, &n, &okey, &oslot, &xyz);
  if (rc != CVO_OK) return rc;
  *d = cvo_device_rows_t{};
  d->n = d->n_records = (int)n;
  if (!want_rows) return CVO_OK;  // (counted only: no row is laid out, *d names none)
  float *feat = xyz + 3 * (size_t)n, *label = feat + BKI_FEAT * (size_t)n;
  *d = device_rows((int)n, (int)n, xyz, feat, BKI_FEAT, m->k.C > 0 ? label : nullptr, (size_t)label_stride, nullptr);  // (no geotype: absent)
  if (!n) return CVO_OK;
  hipLaunchKernelGGL(k_bki_rows, dim3(bki_blocks(n)), dim3(BKI_THREADS), 0, ctx->upload_stream, m->k, m->dev.t, n, okey, oslot, xyz, feat, label,
                     label_stride, label_stride);
  HIP_TRY(ctx, hipGetLastError());
  return CVO_OK;
}

// the cloud read out, on the host, of either side; without want_rows its size alone
int bki_rows(cvo_map* m, bool want_rows, BkiRows* out) {
  const BkiConst& k = m->k;
  if (m->side != 0) {
    m->host.rows(k, want_rows, out);
    m->occupied = out->n;
    return CVO_OK;
  }
  cvo_ctx* ctx = m->ctx;
  cvo_device_rows_t d{};
  const int rc = bki_rows_device(m, want_rows, k.C, &d);
  if (rc != CVO_OK) return rc;
  const size_t n = (size_t)d.n;
  out->n = d.n;
  if (!want_rows || !n) return CVO_OK;
  hipStream_t st = ctx->upload_stream;
  out->xyz.resize(3 * n);
  out->feat.resize(BKI_FEAT * n);
  out->label.resize((size_t)k.C * n);
  HIP_TRY(ctx, hipMemcpyAsync(out->xyz.data(), d.xyz, 12 * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(out->feat.data(), d.feat, 4 * BKI_FEAT * n, hipMemcpyDeviceToHost, st));
  if (k.C > 0) HIP_TRY(ctx, hipMemcpyAsync(out->label.data(), d.label, 4 * (size_t)k.C * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

// the crossover of an undecided map: by the kernel its first insert runs
long long bki_host_below(const cvo_map* m) { return m->kernel == CVO_MAP_KERNEL_SPARSE ? BKI_SPARSE_HOST_BELOW : BKI_HOST_BELOW; }

// the side of a context's map, taken at its first insert
int bki_choose_side(const cvo_map* m, int n, const float* xyz, const float* origin) {
  const int sw = m->ctx->opt.bki_host;
  if (sw >= 0) return sw > 0 ? 1 : 0;
  // (the count stops at the crossover: a large frame costs this no more than a small one)
  const long long below = bki_host_below(m);
  return route_on_host(-1, (long long)bki_training_count(m->k, n, xyz, origin, (unsigned long long)below), below) ? 1 : 0;
}

int bki_insert_entry(cvo_map* m, bool host_call, const char* who, int n, const float* xyz, const float* feat, const float* label, const float* origin) {
  if (!m || host_call != (m->ctx == nullptr)) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  std::string msg;
  const int rc = bki_validate_insert(m, n, xyz, label, origin, &msg);
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  return frontend_call(ctx, who, [&] {
    const int side = m->side >= 0 ? m->side : (ctx ? bki_choose_side(m, n, xyz, origin) : 1);
    return bki_insert_on_side(m, who, side, n, xyz, feat, label, origin, nullptr, nullptr);
  });
}

int bki_open(cvo_ctx* ctx, const char* who, const cvo_map_config_t* cfg, long long initial_voxels, cvo_map** out) {
  std::string msg;
  if (!out) return fail(ctx, CVO_E_INVALID, std::string(who) + ": a required pointer is missing");
  const int rc = bki_validate_config(cfg, &msg);
  if (rc != CVO_OK) return fail(ctx, rc, std::string(who) + ": " + msg);
  if (initial_voxels < 0 || (unsigned long long)initial_voxels > BKI_MAX_SLOTS / 2) return fail(ctx, CVO_E_INVALID, std::string(who) + ": initial_voxels lies in 0 .. 2^29");
  cvo_map* m = new cvo_map();
  m->ctx = ctx;
  m->cfg = *cfg;
  m->k = bki_const(*cfg);
  unsigned long long slots = 32;  // (twice the voxels, a power of two)
  while (slots < 2 * (unsigned long long)initial_voxels) slots *= 2;
  m->dev.initial_slots = slots;
  if (!ctx) m->side = 1;
  *out = m;
  return CVO_OK;
}

// what cvo_cloud_upload makes of the rows read out; a label row of fewer than NC classes is followed by zeros
int bki_upload_rows(cvo_ctx* ctx, int C, const BkiRows& rows, cvo_cloud** resident) {
  std::vector<float> wide;
  if (C > 0 && C < NC) {
    wide.assign((size_t)NC * rows.n, 0.f);
    for (long long i = 0; i < rows.n; i++) std::memcpy(&wide[(size_t)NC * i], &rows.label[(size_t)C * i], 4 * (size_t)C);
  }
  const float* lab = C == 0 ? nullptr : (C < NC ? wide.data() : rows.label.data());
  const HostCloud h{(int)rows.n, (const char*)rows.xyz.data(), 12, (const char*)rows.feat.data(), sizeof(float) * FD, (const char*)lab,
                    sizeof(float) * NC, nullptr, 8};
  return upload_one_locked(ctx, h, resident);
}

int bki_cloud_entry(cvo_map* m, bool host_call, const char* who, long long capacity, float* xyz, float* feat, float* label, long long* n, cvo_cloud** resident) {
  if (!m || host_call != (m->ctx == nullptr)) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  if (!n || capacity < 0) return fail(ctx, CVO_E_INVALID, std::string(who) + ": a required pointer is missing");
  if (m->broken) return fail(ctx, CVO_E_HIP, std::string(who) + ": " + BKI_SAYS_BROKEN);
  if (resident) *resident = nullptr;
  return frontend_call(ctx, who, [&] {
    BkiRows rows;
    const bool want = xyz || feat || label || resident;
    int rc = bki_rows(m, want, &rows);
    if (rc != CVO_OK) return rc;
    *n = rows.n;
    if (!want) return (int)CVO_OK;
    if ((xyz || feat || label) && capacity < rows.n) return fail(ctx, CVO_E_INVALID, std::string(who) + ": the cloud has more rows than `capacity`");
    if (xyz && rows.n) std::memcpy(xyz, rows.xyz.data(), 4 * rows.xyz.size());
    if (feat && rows.n) std::memcpy(feat, rows.feat.data(), 4 * rows.feat.size());
    if (label && rows.n && m->k.C > 0) std::memcpy(label, rows.label.data(), 4 * rows.label.size());
    if (resident && (rc = bki_upload_rows(ctx, m->k.C, rows, resident)) != CVO_OK) return rc;
    return (int)CVO_OK;
  });
}

// ---- a resident cloud in, a resident cloud out: no row passes through the host on a map of the device side ----

// The hits of cvo_map_insert_cloud staged on the device, then the side rule and either side's insert.  The caller holds
// upload_mutex; pose (or nullptr) and origin are finite.
int bki_insert_cloud_locked(cvo_map* m, const cvo_cloud* c, const float* pose12, const float* origin) {
  const std::string who = "cvo_map_insert_cloud";
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  const BkiConst& k = m->k;
  const int n = c->n;
  const size_t nn = (size_t)n;
  // what the cloud really holds (an attribute pointed into the zero slab counts as missing: cvo_merge.hip)
  const float4* c_feat = n ? held(c, c->feat) : nullptr;
  const float4* c_label = n ? held(c, c->label) : nullptr;
  if (n > 0 && k.C > 0 && !c_label) return fail(ctx, CVO_E_INVALID, who + ": " + BKI_SAYS_NEEDS_LABELS);
  if (m->broken) return fail(ctx, CVO_E_HIP, who + ": " + BKI_SAYS_BROKEN);
  if ((long long)n >= BKI_MAX_TRAINING) return fail(ctx, CVO_E_UNSUPPORTED, who + ": " + BKI_SAYS_MANY_ROWS);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  BkiInsertArgs a{};
  const int rc = bki_insert_scratch(m, n, c_feat != nullptr, origin, &a);
  if (rc != CVO_OK) return rc;
  if (n) {
    BkiStageArgs s{};
    s.n = n;
    s.C = k.C;
    s.has_pose = pose12 ? 1 : 0;
    for (int q = 0; pose12 && q < 12; q++) s.pose[q] = pose12[q];
    s.x4 = c->x4;
    s.inv = c->inv;
    s.feat = reinterpret_cast<const float*>(c_feat);
    s.label = reinterpret_cast<const float*>(c_label);
    s.xyz = const_cast<float*>(a.xyz);
    s.ofeat = const_cast<float*>(a.feat);
    s.olabel = const_cast<float*>(a.label);
    s.ctl = a.ctl;
    const int grid = std::min((n + BKI_STAGE_THREADS - 1) / BKI_STAGE_THREADS, BKI_STAGE_MAX_BLOCKS);
    hipLaunchKernelGGL(k_bki_stage, dim3((unsigned)grid), dim3(BKI_STAGE_THREADS), 0, st, s);
    HIP_TRY(ctx, hipGetLastError());
  }
  // The side: the map's; on a map without one the switch's; with the switch unset the training points k_bki_count finds
  // in the staged hits decide (the count bki_choose_side makes on the host for rows that are there).
  int side = m->side >= 0 ? m->side : (ctx->opt.bki_host >= 0 ? (ctx->opt.bki_host > 0 ? 1 : 0) : -1);
  if (side != 1) {
    hipLaunchKernelGGL(k_bki_count, dim3(bki_blocks(nn + 1)), dim3(BKI_THREADS), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
  }
  BkiCtl h{};
  HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  // (bki_validate_insert's check, made where the moved rows are)
  if (h.nonfinite != ~0u) return fail(ctx, CVO_E_INVALID, who + ": hit " + std::to_string(h.nonfinite) + " has a coordinate that is not finite");
  if (side < 0) side = route_on_host(-1, (long long)h.training, bki_host_below(m)) ? 1 : 0;
  std::vector<float> hx, hf, hl;
  if (side == 1) {  // the staged arrays are the three the twin's insert takes
    hx.resize(3 * nn), hf.resize(c_feat ? BKI_FEAT * nn : 0), hl.resize((size_t)k.C * nn);
    if (n) HIP_TRY(ctx, hipMemcpyAsync(hx.data(), a.xyz, 12 * nn, hipMemcpyDeviceToHost, st));
    if (n && c_feat) HIP_TRY(ctx, hipMemcpyAsync(hf.data(), a.feat, 4 * BKI_FEAT * nn, hipMemcpyDeviceToHost, st));
    if (n && k.C > 0) HIP_TRY(ctx, hipMemcpyAsync(hl.data(), a.label, 4 * (size_t)k.C * nn, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return bki_insert_on_side(m, who, side, n, hx.data(), c_feat ? hf.data() : nullptr, k.C > 0 ? hl.data() : nullptr, origin, &a, &h);
}

// The occupied voxels of a device map as ingest rows where k_bki_rows leaves them - label rows at the padded stride
// k_cloud_ingest reads, zeros behind the map's classes - and cvo_cloud_from_device's body on them: its route rule orders the
// cloud.  The caller holds upload_mutex.
int bki_cloud_resident_device(cvo_map* m, const char* who, std::vector<StagedCloud>& staged, long long* n_out) {
  cvo_device_rows_t d{};
  const int rc = bki_rows_device(m, true, NC_PAD, &d);
  if (rc != CVO_OK) return rc;
  *n_out = d.n;
  return ingest_device_clouds(m->ctx, 1, &d, staged, who);  // (synchronises upload_stream; on error the cloud is released)
}

// ---- the read side: point queries, ray casts, a rendered view (tests/np_bki_query.py; the kernels: cvo_k_bki_query.h) ----

// One output of a read call, named ONCE: the caller's host array (null: not wanted), where the kernel argument that points
// at its device copy stands, the size of an element on both sides, the elements.
struct BkiOut {
  void* host;
  void* arg;
  size_t size, count;
  template <class H, class D>
  BkiOut(H* h, D** d, size_t n) : host(h), arg(d), size(sizeof(D)), count(n) { static_assert(sizeof(H) == sizeof(D), "element sizes differ"); }
};

// room in the work scratch behind every kernel argument whose output is wanted; the others become null
template <size_t N>
void bki_outs_take(ScratchLayout& l, const BkiOut (&outs)[N]) {
  for (const BkiOut& o : outs) {
    void* d = nullptr;
    if (o.host) l.take_as<unsigned char>(d, o.size * o.count);
    std::memcpy(o.arg, &d, sizeof d);
  }
}

// behind a read call's launch: its error, the wanted outputs to their callers' arrays, the stream synchronised
template <size_t N>
int bki_outs_down(cvo_ctx* ctx, const BkiOut (&outs)[N], hipStream_t st) {
  HIP_TRY(ctx, hipGetLastError());
  for (const BkiOut& o : outs) {
    void* d = nullptr;
    std::memcpy(&d, o.arg, sizeof d);
    if (o.host && o.count) HIP_TRY(ctx, hipMemcpyAsync(o.host, d, o.size * o.count, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

// points from host rows (xyz) or from a resident cloud under a pose (cloud; pose12 or nullptr)
int bki_query_device(cvo_map* m, int n, const float* xyz, const cvo_cloud* cloud, const float* pose12, const cvo_map_query_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n, nc = (size_t)m->k.nclass;
  BkiQueryArgs a{};
  const BkiOut outs[] = {{o.found, &a.found, nn},          {o.state, &a.state, nn},          {o.semantics, &a.semantics, nn}, {o.probs, &a.probs, nc * nn},
                         {o.vars, &a.vars, nc * nn},       {o.feat, &a.feat, BKI_FEAT * nn}, {o.centre, &a.centre, 3 * nn}};
  float* d_xyz = nullptr;
  const int rc = m->dev.work_scratch.lay_out(ctx, "voxel map query scratch", [&](ScratchLayout& l) {
    if (xyz) l.take(d_xyz, 3 * nn);
    bki_outs_take(l, outs);
  });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->dev.t;
  a.n = n;
  if (xyz) {
    HIP_TRY(ctx, hipMemcpyAsync(d_xyz, xyz, 12 * nn, hipMemcpyHostToDevice, st));
    a.xyz = d_xyz;
  } else {
    a.x4 = cloud->x4;
    a.has_pose = pose12 ? 1 : 0;
    for (int q = 0; pose12 && q < 12; q++) a.pose[q] = pose12[q];
  }
  const unsigned tiles = (unsigned)((nn + BKI_QUERY_THREADS - 1) / BKI_QUERY_THREADS);
  hipLaunchKernelGGL(k_bki_query, dim3(std::min(tiles, (unsigned)BKI_GRID_MAX)), dim3(BKI_QUERY_THREADS), 0, st, a);
  return bki_outs_down(ctx, outs, st);
}

int bki_raycast_device(cvo_map* m, int n, const float* origin, const float* end, unsigned stop_mask, int max_steps, const cvo_map_ray_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  BkiRaycastArgs a{};
  const BkiOut outs[] = {{o.status, &a.out.status, nn}, {o.key, &a.out.key, nn},     {o.centre, &a.out.centre, 3 * nn},   {o.t, &a.out.t, nn},
                         {o.steps, &a.out.steps, nn},   {o.state, &a.out.state, nn}, {o.semantics, &a.out.semantics, nn}};
  float *d_o = nullptr, *d_e = nullptr;
  const int rc = m->dev.work_scratch.lay_out(ctx, "voxel map ray scratch", [&](ScratchLayout& l) {
    l.take(d_o, 3 * nn);
    l.take(d_e, 3 * nn);
    bki_outs_take(l, outs);
  });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->dev.t;
  a.n = n;
  a.stop_mask = stop_mask;
  a.max_steps = max_steps;
  a.origin = d_o;
  a.end = d_e;
  HIP_TRY(ctx, hipMemcpyAsync(d_o, origin, 12 * nn, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_e, end, 12 * nn, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_bki_raycast, dim3(bki_blocks(nn)), dim3(BKI_THREADS), 0, st, a);
  return bki_outs_down(ctx, outs, st);
}

int bki_render_device(cvo_map* m, const BkiCamera& cam, unsigned stop_mask, const cvo_map_render_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)cam.rows * cam.cols, C = (size_t)m->k.C;
  BkiRenderArgs a{};
  const BkiOut outs[] = {{o.depth, &a.depth, px}, {o.semantics, &a.semantics, px}, {o.feat, &a.feat, BKI_FEAT * px}, {C ? o.label : nullptr, &a.label, C * px}};
  const int rc = m->dev.work_scratch.lay_out(ctx, "voxel map render scratch", [&](ScratchLayout& l) { bki_outs_take(l, outs); });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->dev.t;
  a.rows = cam.rows;
  a.cols = cam.cols;
  a.stop_mask = stop_mask;
  for (int q = 0; q < 12; q++) a.pose[q] = cam.pose[q];
  a.fx = cam.fx, a.fy = cam.fy, a.cx = cam.cx, a.cy = cam.cy, a.z_far = cam.z_far;
  const unsigned long long tiles = (unsigned long long)((cam.cols + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE) * ((cam.rows + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE);
  hipLaunchKernelGGL(k_bki_render, dim3((unsigned)((tiles + BKI_THREADS / BKI_WAVE - 1) / (BKI_THREADS / BKI_WAVE))), dim3(BKI_THREADS), 0, st, a);
  return bki_outs_down(ctx, outs, st);
}

// what every read checks first: the handle, the kind of map the entry point is for, a map an insert left half way
int bki_read_check(cvo_map* m, bool host_call, const std::string& who) {
  if (!m) return CVO_E_INVALID;
  if (host_call != (m->ctx == nullptr))
    return fail(m->ctx, CVO_E_INVALID, who + (host_call ? ": the map belongs to a context" : ": the map is one of cvo_map_open_host"));
  if (m->broken) return fail(m->ctx, CVO_E_HIP, who + ": " + BKI_SAYS_BROKEN);
  return CVO_OK;
}

int bki_query_entry(cvo_map* m, bool host_call, const char* who, int n, const float* xyz, const cvo_map_query_out_t* out) {
  int rc = bki_read_check(m, host_call, who);
  if (rc != CVO_OK) return rc;
  cvo_ctx* ctx = m->ctx;
  if (n < 0) return fail(ctx, CVO_E_INVALID, std::string(who) + ": n is negative");
  if (n > 0 && !xyz) return fail(ctx, CVO_E_INVALID, std::string(who) + ": a required pointer is missing");
  const cvo_map_query_out_t o = out ? *out : cvo_map_query_out_t{};
  return frontend_call(ctx, who, [&] {
    if (n == 0) return (int)CVO_OK;
    if (m->side == 0) return bki_query_device(m, n, xyz, nullptr, nullptr, o);
    m->host.query(m->k, n, xyz, o);  // (a map of the host side; an undecided map holds nothing and stays undecided)
    return (int)CVO_OK;
  });
}

int bki_ray_check(cvo_ctx* ctx, const std::string& who, unsigned stop_mask) {
  if (stop_mask > 15u) return fail(ctx, CVO_E_INVALID, who + ": stop_mask has bits beyond FREE 1, OCCUPIED 2, UNKNOWN 4, not stored 8");
  return CVO_OK;
}

int bki_raycast_entry(cvo_map* m, bool host_call, const char* who, int n, const float* origin, const float* end, unsigned stop_mask, int max_steps,
                      const cvo_map_ray_out_t* out) {
  int rc = bki_read_check(m, host_call, who);
  if (rc != CVO_OK) return rc;
  cvo_ctx* ctx = m->ctx;
  if (n < 0) return fail(ctx, CVO_E_INVALID, std::string(who) + ": n_rays is negative");
  if (n > 0 && (!origin || !end)) return fail(ctx, CVO_E_INVALID, std::string(who) + ": a required pointer is missing");
  if (max_steps < 1 || max_steps > BKI_RAY_MAX_STEPS) return fail(ctx, CVO_E_INVALID, std::string(who) + ": max_steps lies in 1 .. 2^20");
  if ((rc = bki_ray_check(ctx, who, stop_mask)) != CVO_OK) return rc;
  const cvo_map_ray_out_t o = out ? *out : cvo_map_ray_out_t{};
  return frontend_call(ctx, who, [&] {
    if (n == 0) return (int)CVO_OK;
    if (m->side == 0) return bki_raycast_device(m, n, origin, end, stop_mask, max_steps, o);
    m->host.raycast(m->k, n, origin, end, stop_mask, max_steps, o);
    return (int)CVO_OK;
  });
}

int bki_render_entry(cvo_map* m, bool host_call, const char* who, const float* pose12, float fx, float fy, float cx, float cy, int rows, int cols,
                     float z_far, unsigned stop_mask, const cvo_map_render_out_t* out) {
  int rc = bki_read_check(m, host_call, who);
  if (rc != CVO_OK) return rc;
  cvo_ctx* ctx = m->ctx;
  const std::string w = who;
  if (!pose12) return fail(ctx, CVO_E_INVALID, w + ": a required pointer is missing");
  if (rows < 1 || cols < 1) return fail(ctx, CVO_E_INVALID, w + ": rows and cols are at least 1");
  for (const float f : {fx, fy, z_far})
    if (!std::isfinite(f) || !(f > 0.f)) return fail(ctx, CVO_E_INVALID, w + ": fx, fy and z_far are finite and > 0");
  if (!std::isfinite(cx) || !std::isfinite(cy)) return fail(ctx, CVO_E_INVALID, w + ": cx and cy are finite");
  for (int q = 0; q < 12; q++)
    if (!std::isfinite(pose12[q])) return fail(ctx, CVO_E_INVALID, w + ": the pose is not finite");
  if ((rc = bki_ray_check(ctx, w, stop_mask)) != CVO_OK) return rc;
  if ((long long)rows * cols > BKI_RENDER_MAX_PIXELS) return fail(ctx, CVO_E_UNSUPPORTED, w + ": more than 2^24 pixels");
  BkiCamera cam{};
  for (int q = 0; q < 12; q++) cam.pose[q] = pose12[q];
  cam.fx = fx, cam.fy = fy, cam.cx = cx, cam.cy = cy, cam.z_far = z_far, cam.rows = rows, cam.cols = cols;
  const cvo_map_render_out_t o = out ? *out : cvo_map_render_out_t{};
  return frontend_call(ctx, who, [&] {
    if (m->side == 0) return bki_render_device(m, cam, stop_mask, o);
    m->host.render(m->k, cam, stop_mask, o);
    return (int)CVO_OK;
  });
}

}  // namespace

extern "C" {

void cvo_map_config_default(cvo_map_config_t* cfg) {
  if (!cfg) return;
  cfg->resolution = 0.05f;
  cfg->block_depth = 1;
  cfg->num_classes = 0;
  cfg->sf2 = 1.f;
  cfg->ell = 1.f;
  cfg->prior = 0.f;
  cfg->var_thresh = 1.f;
  cfg->free_thresh = 0.65f;
  cfg->occupied_thresh = 0.9f;
  cfg->ds_resolution = -1.f;
  cfg->free_resolution = 1.f;
  cfg->max_range = -1.f;
}

int cvo_map_open(cvo_ctx* ctx, const cvo_map_config_t* cfg, long long initial_voxels, cvo_map** out) {
  if (!ctx) return CVO_E_INVALID;
  return bki_open(ctx, "cvo_map_open", cfg, initial_voxels, out);
}

int cvo_map_open_host(const cvo_map_config_t* cfg, cvo_map** out) { return bki_open(nullptr, "cvo_map_open_host", cfg, 0, out); }

void cvo_map_close(cvo_map* m) {
  if (!m) return;
  std::unique_lock<std::mutex> lk;
  if (m->ctx) {
    lk = std::unique_lock<std::mutex>(m->ctx->upload_mutex);
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->upload_stream);
  }
  delete m;  // (the table and both scratch regions go with it)
}

void cvo_map_close_host(cvo_map* m) {
  if (m && !m->ctx) delete m;
}

int cvo_map_insert(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float origin[3]) {
  return bki_insert_entry(m, false, "cvo_map_insert", n, xyz, feat, label, origin);
}

int cvo_map_insert_host(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float origin[3]) {
  return bki_insert_entry(m, true, "cvo_map_insert_host", n, xyz, feat, label, origin);
}

int cvo_map_insert_posed(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float pose12[12]) {
  if (!m || !m->ctx) return CVO_E_INVALID;
  if (!pose12 || n < 0 || (n > 0 && !xyz)) return fail(m->ctx, CVO_E_INVALID, "cvo_map_insert_posed: a required pointer is missing");
  // the rows under the pose as cvo_cloud_transformed moves them (pose_point), the translation as origin
  std::vector<float> moved;
  try {
    moved.resize(3 * (size_t)n);
  } catch (const std::exception& e) {
    return fail(m->ctx, CVO_E_NOMEM, std::string("cvo_map_insert_posed: ") + e.what());
  }
  for (size_t i = 0; i < (size_t)n; i++) pose_point(pose12, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &moved[3 * i]);
  const float origin[3] = {pose12[3], pose12[7], pose12[11]};
  return bki_insert_entry(m, false, "cvo_map_insert_posed", n, moved.data(), feat, label, origin);
}

int cvo_map_set_kernel(cvo_map* m, int kernel) {
  if (!m) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  if (kernel != CVO_MAP_KERNEL_CSM && kernel != CVO_MAP_KERNEL_SPARSE) return fail(ctx, CVO_E_INVALID, "cvo_map_set_kernel: an unknown kernel");
  if (kernel == CVO_MAP_KERNEL_SPARSE && !(std::isfinite(m->cfg.sf2) && m->cfg.sf2 > 0.f && std::isfinite(m->cfg.ell) && m->cfg.ell > 0.f))
    return fail(ctx, CVO_E_INVALID, "cvo_map_set_kernel: the sparse kernel needs sf2 and ell finite and > 0");
  return frontend_call(ctx, "cvo_map_set_kernel", [&] {
    m->kernel = kernel;
    return (int)CVO_OK;
  });
}

int cvo_map_size(cvo_map* m, long long* voxels, long long* occupied) {
  if (!m) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  if (m->broken) return fail(ctx, CVO_E_HIP, std::string("cvo_map_size: ") + BKI_SAYS_BROKEN);
  return frontend_call(ctx, "cvo_map_size", [&] {
    if (occupied && m->occupied < 0) {
      BkiRows rows;
      const int rc = bki_rows(m, false, &rows);
      if (rc != CVO_OK) return rc;
    }
    if (voxels) *voxels = m->side == 0 ? (long long)m->dev.voxels : (long long)m->host.keys.size();
    if (occupied) *occupied = m->occupied;
    return (int)CVO_OK;
  });
}

int cvo_map_cloud(cvo_map* m, long long capacity, float* xyz, float* feat, float* label, long long* n, cvo_cloud** resident) {
  return bki_cloud_entry(m, false, "cvo_map_cloud", capacity, xyz, feat, label, n, resident);
}

int cvo_map_cloud_host(cvo_map* m, long long capacity, float* xyz, float* feat, float* label, long long* n) {
  return bki_cloud_entry(m, true, "cvo_map_cloud_host", capacity, xyz, feat, label, n, nullptr);
}

int cvo_map_insert_cloud(cvo_map* m, const cvo_cloud* cloud, const float pose12[12], const float origin[3]) {
  const std::string who = "cvo_map_insert_cloud";
  if (!m || !m->ctx) return CVO_E_INVALID;  // (a host map has no context to hold a text, and no device to stage on)
  cvo_ctx* ctx = m->ctx;
  if (!cloud) return fail(ctx, CVO_E_INVALID, who + ": a required pointer is missing");
  if (cloud->ctx != ctx) return fail(ctx, CVO_E_INVALID, who + ": the cloud belongs to another context");
  if (!pose12 && !origin) return fail(ctx, CVO_E_INVALID, who + ": neither a pose nor an origin is given");
  for (int q = 0; pose12 && q < 12; q++)
    if (!std::isfinite(pose12[q])) return fail(ctx, CVO_E_INVALID, who + ": the pose is not finite");
  const float o[3] = {origin ? origin[0] : pose12[3], origin ? origin[1] : pose12[7], origin ? origin[2] : pose12[11]};
  for (int q = 0; q < 3; q++)
    if (!std::isfinite(o[q])) return fail(ctx, CVO_E_INVALID, who + ": the origin is not finite");
  return frontend_call(ctx, who.c_str(), [&] { return bki_insert_cloud_locked(m, cloud, pose12, o); });
}

int cvo_map_cloud_resident(cvo_map* m, cvo_cloud** out, long long* n) {
  const char* who = "cvo_map_cloud_resident";
  if (out) *out = nullptr;
  if (n) *n = 0;
  if (!m || !m->ctx) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  if (!out) return fail(ctx, CVO_E_INVALID, std::string(who) + ": a required pointer is missing");
  if (m->broken) return fail(ctx, CVO_E_HIP, std::string(who) + ": " + BKI_SAYS_BROKEN);
  long long rows_n = 0;
  const int rc = handover_call(ctx, who, out, [&](std::vector<StagedCloud>& staged) {
    if (m->side == 0) return bki_cloud_resident_device(m, who, staged, &rows_n);
    // a map of the host side (or without an insert): the twin's rows, uploaded (the upload writes its cloud only when it succeeds)
    BkiRows rows;
    const int r = bki_rows(m, true, &rows);
    if (r != CVO_OK) return r;
    rows_n = rows.n;
    staged.resize(1);
    return bki_upload_rows(ctx, m->k.C, rows, &staged[0].c);
  });
  if (rc == CVO_OK && n) *n = rows_n;
  return rc;
}

int cvo_map_query(cvo_map* m, int n, const float* xyz, const cvo_map_query_out_t* out) {
  return bki_query_entry(m, false, "cvo_map_query", n, xyz, out);
}

int cvo_map_query_host(cvo_map* m, int n, const float* xyz, const cvo_map_query_out_t* out) {
  return bki_query_entry(m, true, "cvo_map_query_host", n, xyz, out);
}

int cvo_map_query_cloud(cvo_map* m, const cvo_cloud* cloud, const float pose12[12], const cvo_map_query_out_t* out) {
  const std::string who = "cvo_map_query_cloud";
  const int rc = bki_read_check(m, false, who);
  if (rc != CVO_OK) return rc;
  cvo_ctx* ctx = m->ctx;
  if (!cloud) return fail(ctx, CVO_E_INVALID, who + ": a required pointer is missing");
  if (cloud->ctx != ctx) return fail(ctx, CVO_E_INVALID, who + ": the cloud belongs to another context");
  for (int q = 0; pose12 && q < 12; q++)
    if (!std::isfinite(pose12[q])) return fail(ctx, CVO_E_INVALID, who + ": the pose is not finite");
  const cvo_map_query_out_t o = out ? *out : cvo_map_query_out_t{};
  return frontend_call(ctx, who.c_str(), [&] {
    const int n = cloud->n;
    if (n == 0) return (int)CVO_OK;
    if (m->side == 0) return bki_query_device(m, n, nullptr, cloud, pose12, o);
    // a map of the host side, or one without an insert: the coordinates come down and are moved as the kernel moves them
    std::vector<float4> x4((size_t)n);
    std::vector<float> xyz(3 * (size_t)n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(x4.data(), cloud->x4, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, ctx->upload_stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->upload_stream));
    for (size_t i = 0; i < (size_t)n; i++) {
      xyz[3 * i] = x4[i].x, xyz[3 * i + 1] = x4[i].y, xyz[3 * i + 2] = x4[i].z;
      if (pose12) pose_point(pose12, x4[i].x, x4[i].y, x4[i].z, &xyz[3 * i]);
    }
    m->host.query(m->k, n, xyz.data(), o);
    return (int)CVO_OK;
  });
}

int cvo_map_raycast(cvo_map* m, int n_rays, const float* origin, const float* end, unsigned stop_mask, int max_steps, const cvo_map_ray_out_t* out) {
  return bki_raycast_entry(m, false, "cvo_map_raycast", n_rays, origin, end, stop_mask, max_steps, out);
}

int cvo_map_raycast_host(cvo_map* m, int n_rays, const float* origin, const float* end, unsigned stop_mask, int max_steps,
                         const cvo_map_ray_out_t* out) {
  return bki_raycast_entry(m, true, "cvo_map_raycast_host", n_rays, origin, end, stop_mask, max_steps, out);
}

int cvo_map_render(cvo_map* m, const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far, unsigned stop_mask,
                   const cvo_map_render_out_t* out) {
  return bki_render_entry(m, false, "cvo_map_render", pose12, fx, fy, cx, cy, rows, cols, z_far, stop_mask, out);
}

int cvo_map_render_host(cvo_map* m, const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far,
                        unsigned stop_mask, const cvo_map_render_out_t* out) {
  return bki_render_entry(m, true, "cvo_map_render_host", pose12, fx, fy, cx, cy, rows, cols, z_far, stop_mask, out);
}

int cvo_debug_map_stats(cvo_map* m, int* on_device, unsigned long long* counts, unsigned long long* keys, float* ms, float* fs) {
  if (!m) return CVO_E_INVALID;
  cvo_ctx* ctx = m->ctx;
  return frontend_call(ctx, "cvo_debug_map_stats", [&] {
    const bool dev = m->side == 0;
    const unsigned long long capacity = dev ? m->dev.slots : m->host.keys.size();
    if (on_device) *on_device = m->last.on_device;
    if (counts) {
      counts[0] = m->last.training;
      counts[1] = m->last.members;
      counts[2] = m->last.longest_run;
      counts[3] = capacity;
      counts[4] = (unsigned long long)m->dev.growths;
      counts[5] = m->last.longest_probe;
      counts[6] = dev ? m->dev.voxels : m->host.keys.size();
      counts[7] = (unsigned long long)m->k.nclass;
    }
    if (!keys && !ms && !fs) return (int)CVO_OK;
    if (!dev) {
      if (keys && capacity) std::memcpy(keys, m->host.keys.data(), 8 * capacity);
      if (ms && capacity) std::memcpy(ms, m->host.ms.data(), 4 * m->host.ms.size());
      if (fs && capacity) std::memcpy(fs, m->host.fs.data(), 4 * m->host.fs.size());
      return (int)CVO_OK;
    }
    hipStream_t st = ctx->upload_stream;
    if (keys) HIP_TRY(ctx, hipMemcpyAsync(keys, m->dev.t.keys, 8 * capacity, hipMemcpyDeviceToHost, st));
    if (ms) HIP_TRY(ctx, hipMemcpyAsync(ms, m->dev.t.ms, 4 * capacity * (size_t)m->k.nclass, hipMemcpyDeviceToHost, st));
    if (fs) HIP_TRY(ctx, hipMemcpyAsync(fs, m->dev.t.fs, 4 * capacity * BKI_FEAT, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return (int)CVO_OK;
  });
}

}  // extern "C"
