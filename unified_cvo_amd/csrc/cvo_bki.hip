// cvo_bki.hip -- the semantic voxel map: cvo_map_open / _insert / _insert_posed / _size / _cloud / _close, their _host twins
// on a map without a context, cvo_map_insert_cloud / cvo_map_cloud_resident (a resident cloud in, a resident cloud out: the
// hits staged by k_bki_stage, the rows read out handed to cvo_ingest.hip where they are) and cvo_debug_map_stats.  It is semantic_bki::SemanticBKIOctoMap::insert_pointcloud_csm at
// block_depth 1 with the read-out of CvoPointCloud(const SemanticBKIOctoMap*, num_classes); tests/np_bki.py states what is
// computed, the CPU twin (BkiHostMap) and the kernels of cvo_k_bki.h share cvo_bki_math.h.  A map lives on ONE side: a map
// of a context takes its side at its first insert (switch BKI_HOST; unset: by that insert's training points) and keeps it,
// its table does not migrate.  cvo_map_set_kernel chooses what an insert computes: the counting sensor model above or the sparse
// kernel (predict / covSparse over a block and its face neighbours; tests/np_bki_sparse.py, the twin bki_insert_sparse_cpu, the
// kernels of cvo_k_bki_sparse.h).  A SECTION of the one translation unit cvo_hip.hip; not compiled on its own.
#include <unordered_map>

namespace {

// training points of a map's FIRST insert below which the map lives on the host: the smallest frame whose ten inserts and
// read-out took the device less time than the twin (profiles/bki/bki_probe.txt)
constexpr long long BKI_HOST_BELOW = 2129;
// ... and the same for a map whose kernel is the sparse one at its first insert (profiles/bki_sparse/bki_sparse_probe.txt): the
// twin's sparse insert costs several times its counting insert, the device's less than twice
constexpr long long BKI_SPARSE_HOST_BELOW = 547;

struct BkiStats {
  int on_device = 0;
  unsigned long long training = 0, members = 0, longest_run = 0, longest_probe = 0;
};

// ---- CPU twin: one thread ----
struct BkiHostMap {
  std::unordered_map<unsigned long long, unsigned> index;
  std::vector<unsigned long long> keys;
  std::vector<float> ms, fs;
};

struct BkiMember {
  unsigned long long key;
  int cls;  // 0: a beam sample or the origin
  int hit;
};

}  // namespace

struct cvo_map {
  cvo_ctx* ctx = nullptr;  // nullptr: a host-only map
  cvo_map_config_t cfg{};
  BkiConst k{};
  int side = -1;  // -1: no insert yet; 0: the device; 1: the host
  int kernel = CVO_MAP_KERNEL_CSM;  // cvo_map_set_kernel: what the next insert runs
  bool broken = false;
  BkiHostMap host;
  // the device side: one allocation behind the table; the hits of an insert and its work arrays
  BkiTable t{};
  DeviceRegion slab;
  unsigned long long slots = 0, voxels = 0, initial_slots = 0;
  long long occupied = -1;  // -1: not counted since the last insert
  int growths = 0;
  DeviceScratch in_scratch, work_scratch;
  BkiStats last{};
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

// what every insert checks before either route: the pointers, the size, every coordinate finite
int bki_validate_insert(const cvo_map* m, int n, const float* xyz, const float* label, const float* origin, std::string* msg) {
  if (!m || !origin || n < 0 || (n > 0 && !xyz)) return *msg = "a required pointer is missing", CVO_E_INVALID;
  if (n > 0 && m->k.C > 0 && !label) return *msg = "a map with classes needs label rows", CVO_E_INVALID;
  if (m->broken) return *msg = "an earlier insert failed on the device half way: the map cannot be used", CVO_E_HIP;
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(origin[a])) return *msg = "the origin is not finite", CVO_E_INVALID;
  for (size_t i = 0; i < 3 * (size_t)n; i++)
    if (!std::isfinite(xyz[i])) return *msg = "hit " + std::to_string(i / 3) + " has a coordinate that is not finite", CVO_E_INVALID;
  if ((long long)n >= BKI_MAX_TRAINING) return *msg = "more than 2^24 training points in one insert", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

std::string bki_bad_text(unsigned status, unsigned index, int n) {
  const std::string who = (int)index >= n ? std::string("the origin") : "hit " + std::to_string(index);
  if (status & BKI_BAD_RANGE) return who + " or one of its beam samples leaves the map's 2^20 blocks per axis";
  if (status & BKI_BAD_TOO_MANY) return who + " needs 65536 beam samples or more";
  return who + " belongs to more than 8 blocks";
}

// The training points of one insert - hits max_range keeps, their beam samples, the origin -, counted without any block
// arithmetic; stops as soon as `limit` is reached (a ray of BKI_MAX_RAY samples or more counts as `limit`).
unsigned long long bki_training_count(const BkiConst& k, int n, const float* xyz, const float* origin, unsigned long long limit) {
  unsigned long long training = 1;
  for (int i = 0; i < n && training < limit; i++) {
    const float* p = xyz + 3 * (size_t)i;
    if (!bki_in_range(k, p, origin)) continue;
    unsigned too_many = 0;
    bki_hit_points(k, p, origin, &too_many, [&](float, float, float, bool) { return ++training < limit; });
    if (too_many) return limit;
  }
  return training;
}

// The memberships of one insert in upstream's order, or the refusal.  `training` counts the points.
int bki_members_cpu(const BkiConst& k, int n, const float* xyz, const float* label, const float* origin, std::vector<BkiMember>* out,
                    unsigned long long* training, std::string* msg) {
  unsigned bad = 0;
  *training = 0;
  auto point = [&](int i, int cls) {
    return [&, i, cls](float x, float y, float z, bool hit) {
      const int c = hit ? cls : 0;
      const int m = bki_members(k, x, y, z, [&](unsigned long long key) { if (out) out->push_back(BkiMember{key, c, hit ? i : -1}); });
      if (m < 0) return bad |= BKI_BAD_RANGE, false;
      (*training)++;
      return true;
    };
  };
  for (int i = 0; i < n && !bad; i++) {
    const float* p = xyz + 3 * (size_t)i;
    if (!bki_in_range(k, p, origin)) continue;
    unsigned too_many = 0;
    bki_hit_points(k, p, origin, &too_many, point(i, k.C > 0 ? bki_class(label + (size_t)i * k.C, k.C) : 1));
    if (too_many) bad |= BKI_BAD_TOO_MANY;
    if (bad) return *msg = bki_bad_text(bad, (unsigned)i, n), bad & BKI_BAD_RANGE ? CVO_E_INVALID : CVO_E_UNSUPPORTED;
  }
  point(n, 0)(origin[0], origin[1], origin[2], false);
  if (bad) return *msg = bki_bad_text(bad, (unsigned)n, n), CVO_E_INVALID;
  if (*training >= (unsigned long long)BKI_MAX_TRAINING) return *msg = "more than 2^24 training points in one insert", CVO_E_UNSUPPORTED;
  return CVO_OK;
}

int bki_insert_cpu(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats, std::string* msg) {
  const BkiConst& k = m->k;
  std::vector<BkiMember> mem;
  unsigned long long training = 0;
  // (the caps come first, as in the statement, and before any membership is stored)
  if (bki_training_count(k, n, xyz, origin, (unsigned long long)BKI_MAX_TRAINING) >= (unsigned long long)BKI_MAX_TRAINING)
    return *msg = "2^24 training points or more in one insert, or a hit with 65536 beam samples or more", CVO_E_UNSUPPORTED;
  const int rc = bki_members_cpu(k, n, xyz, label, origin, &mem, &training, msg);
  if (rc != CVO_OK) return rc;
  // per block touched: integer class counts, the float sum of its hits' feature rows in ascending hit index, from 0
  std::unordered_map<unsigned long long, unsigned> touched;
  std::vector<unsigned long long> tkeys;
  std::vector<unsigned> counts;
  std::vector<float> fbar;
  for (const BkiMember& e : mem) {
    auto it = touched.find(e.key);
    if (it == touched.end()) {
      it = touched.emplace(e.key, (unsigned)tkeys.size()).first;
      tkeys.push_back(e.key);
      counts.resize(counts.size() + (size_t)k.nclass, 0u);
      fbar.resize(fbar.size() + BKI_FEAT, 0.f);
    }
    const size_t b = it->second;
    counts[b * (size_t)k.nclass + (size_t)e.cls]++;
    if (e.hit >= 0 && feat)
      for (int f = 0; f < BKI_FEAT; f++) fbar[b * BKI_FEAT + f] += feat[(size_t)e.hit * BKI_FEAT + f];
  }
  BkiHostMap& h = m->host;
  unsigned long long longest = 0;
  for (size_t b = 0; b < tkeys.size(); b++) {
    auto it = h.index.find(tkeys[b]);
    if (it == h.index.end()) {
      it = h.index.emplace(tkeys[b], (unsigned)h.keys.size()).first;
      h.keys.push_back(tkeys[b]);
      h.ms.resize(h.ms.size() + (size_t)k.nclass, k.prior);
      h.fs.resize(h.fs.size() + BKI_FEAT, 0.f);
    }
    const size_t v = it->second;
    unsigned long long hits = 0;
    for (int c = 0; c < k.nclass; c++) {
      h.ms[v * (size_t)k.nclass + c] += (float)counts[b * (size_t)k.nclass + c];
      if (c) hits += counts[b * (size_t)k.nclass + c];
    }
    for (int f = 0; f < BKI_FEAT; f++) h.fs[v * BKI_FEAT + f] += fbar[b * BKI_FEAT + f];
    longest = std::max(longest, hits);
  }
  stats->training = training;
  stats->members = mem.size();
  stats->longest_run = longest;
  return CVO_OK;
}

// ---- the sparse kernel on one thread (tests/np_bki_sparse.py) ----
struct BkiSparseRecord {
  unsigned long long key;
  float p[3];
  int cls, hit;
};

int bki_insert_sparse_cpu(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats,
                          std::string* msg) {
  const BkiConst& k = m->k;
  const float sf2 = m->cfg.sf2, ell = m->cfg.ell;
  if (bki_training_count(k, n, xyz, origin, (unsigned long long)BKI_MAX_TRAINING) >= (unsigned long long)BKI_MAX_TRAINING)
    return *msg = "2^24 training points or more in one insert, or a hit with 65536 beam samples or more", CVO_E_UNSUPPORTED;
  // a first walk counts and checks (bki_members_cpu without a list), the second stores the records in training order
  unsigned long long training = 0;
  const int rc = bki_members_cpu(k, n, xyz, label, origin, nullptr, &training, msg);
  if (rc != CVO_OK) return rc;
  std::vector<BkiSparseRecord> rec;
  auto point = [&](int i, int cls) {
    return [&, i, cls](float x, float y, float z, bool hit) {
      bki_members(k, x, y, z, [&](unsigned long long key) { rec.push_back(BkiSparseRecord{key, {x, y, z}, hit ? cls : 0, hit ? i : -1}); });
      return rec.size() < (size_t)BKI_SPARSE_MAX_RECORDS;
    };
  };
  for (int i = 0; i < n && rec.size() < (size_t)BKI_SPARSE_MAX_RECORDS; i++) {
    const float* p = xyz + 3 * (size_t)i;
    if (!bki_in_range(k, p, origin)) continue;
    unsigned too_many = 0;
    bki_hit_points(k, p, origin, &too_many, point(i, k.C > 0 ? bki_class(label + (size_t)i * k.C, k.C) : 1));
  }
  if (rec.size() < (size_t)BKI_SPARSE_MAX_RECORDS) point(n, 0)(origin[0], origin[1], origin[2], false);
  if (rec.size() >= (size_t)BKI_SPARSE_MAX_RECORDS) return *msg = "2^24 block memberships or more in one insert under the sparse kernel", CVO_E_UNSUPPORTED;
  // a block's training list: its records in training order, contiguous after a stable sort by key
  std::stable_sort(rec.begin(), rec.end(), [](const BkiSparseRecord& a, const BkiSparseRecord& b) { return a.key < b.key; });
  std::unordered_map<unsigned long long, std::pair<size_t, size_t>> seg;
  unsigned long long longest = 0;
  for (size_t b = 0; b < rec.size();) {
    size_t e = b + 1;
    while (e < rec.size() && rec[e].key == rec[b].key) e++;
    seg.emplace(rec[b].key, std::make_pair(b, e));
    longest = std::max<unsigned long long>(longest, e - b);
    b = e;
  }
  // the test voxels: every touched block and its face neighbours, each once, new ones stored with ms = prior
  BkiHostMap& h = m->host;
  std::vector<unsigned> tests;
  std::unordered_map<unsigned long long, char> seen;
  for (size_t b = 0; b < rec.size(); b = seg[rec[b].key].second)
    for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
      unsigned long long key;
      if (!bki_sparse_slot(rec[b].key, j, &key) || !seen.emplace(key, 1).second) continue;
      auto it = h.index.find(key);
      if (it == h.index.end()) {
        it = h.index.emplace(key, (unsigned)h.keys.size()).first;
        h.keys.push_back(key);
        h.ms.resize(h.ms.size() + (size_t)k.nclass, k.prior);
        h.fs.resize(h.fs.size() + BKI_FEAT, 0.f);
      }
      tests.push_back(it->second);
    }
  for (const unsigned v : tests) {
    const unsigned long long vkey = h.keys[v];
    const float centre[3] = {bki_centre((long long)(vkey >> 40), k.size), bki_centre((long long)((vkey >> 20) & 0xFFFFFull), k.size),
                             bki_centre((long long)(vkey & 0xFFFFFull), k.size)};
    for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
      unsigned long long key;
      if (!bki_sparse_slot(vkey, j, &key)) continue;
      const auto it = seg.find(key);
      if (it == seg.end()) continue;
      float ybar[BKI_MAX_CLASSES + 1] = {}, fbar[BKI_FEAT] = {};
      for (size_t r = it->second.first; r < it->second.second; r++) {
        const float w = bki_sparse_k(centre, rec[r].p, sf2, ell);
        ybar[rec[r].cls] += w;
        if (rec[r].hit >= 0 && feat)
          for (int f = 0; f < BKI_FEAT; f++) fbar[f] += w * feat[(size_t)rec[r].hit * BKI_FEAT + f];
      }
      for (int c = 0; c < k.nclass; c++) h.ms[v * (size_t)k.nclass + c] += ybar[c];
      for (int f = 0; f < BKI_FEAT; f++) h.fs[v * BKI_FEAT + f] += fbar[f];
    }
  }
  stats->training = training;
  stats->members = rec.size();
  stats->longest_run = longest;
  return CVO_OK;
}

int bki_insert_cpu_kernel(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats,
                          std::string* msg) {
  return m->kernel == CVO_MAP_KERNEL_SPARSE ? bki_insert_sparse_cpu(m, n, xyz, feat, label, origin, stats, msg)
                                            : bki_insert_cpu(m, n, xyz, feat, label, origin, stats, msg);
}

// the occupied voxels of the host map in ascending key order
std::vector<std::pair<unsigned long long, unsigned>> bki_occupied_cpu(const cvo_map* m) {
  std::vector<std::pair<unsigned long long, unsigned>> occ;
  for (size_t v = 0; v < m->host.keys.size(); v++)
    if (bki_state(m->k, &m->host.ms[v * (size_t)m->k.nclass]) == BKI_OCCUPIED) occ.emplace_back(m->host.keys[v], (unsigned)v);
  std::sort(occ.begin(), occ.end());
  return occ;
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
  cvo_ctx* ctx = m->ctx;
  while (2 * need > m->slots) {
    const unsigned long long slots = m->slots ? 2 * m->slots : m->initial_slots;
    if (slots > BKI_MAX_SLOTS) return fail(ctx, CVO_E_UNSUPPORTED, "the voxel map would need more than 2^30 slots");
    BkiTable t{};
    DeviceRegion slab;
    int rc = bki_table_alloc(m, slots, &t, &slab);
    if (rc != CVO_OK) return rc;
    hipError_t e = hipSuccess;
    if (m->slab.p) {
      hipLaunchKernelGGL(k_bki_rehash, dim3(bki_stride_blocks(m->slots)), dim3(BKI_THREADS), 0, ctx->upload_stream, m->t, t);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->upload_stream);
    if (e != hipSuccess) return fail(ctx, CVO_E_HIP, std::string("voxel map rehash: ") + hipGetErrorString(e));
    if (m->slab.p) m->growths++;
    m->slab = std::move(slab);  // (the old table goes here)
    m->t = t;
    m->slots = slots;
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
  const int rc = m->in_scratch.lay_out(ctx, "voxel map insert scratch", [&](ScratchLayout& l) {
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
  if (h.training >= (unsigned long long)BKI_MAX_TRAINING) return fail(ctx, CVO_E_UNSUPPORTED, who + ": 2^24 training points or more in one insert");
  if (h.status) return fail(ctx, h.status & BKI_BAD_RANGE ? CVO_E_INVALID : CVO_E_UNSUPPORTED, who + ": " + bki_bad_text(h.status, h.bad_index, n));
  return CVO_OK;
}

// The rest of an insert whose hits are staged and counted (h: the control block k_bki_count left, nothing refused): the
// table grows, k_bki_emit ... k_bki_long run.
int bki_insert_counted(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, BkiStats* stats) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  const int n = a.n;
  const size_t nn = (size_t)n;
  const float* feat = a.feat;
  const dim3 per_hit(bki_blocks(nn + 1)), block(BKI_THREADS);
  // the work arrays, and room in the table for every membership to be a new voxel
  int rc = m->work_scratch.lay_out(ctx, "voxel map work scratch", [&](ScratchLayout& l) {
    l.take(a.rec, h.members);
    l.take(a.seg, h.hit_members);
    l.take(a.seg2, h.hit_members);
    l.take(a.longlist, 2 * (h.hit_members / (BKI_SHORT_RUN + 1) + 1));  // ((slot, hits) per voxel)
  });
  if (rc != CVO_OK) return rc;
  if ((rc = bki_table_grow(m, m->voxels + h.members)) != CVO_OK) return rc;
  a.t = m->t;
  m->broken = true;  // (until the table's counters are back at zero)
  m->occupied = -1;
  hipLaunchKernelGGL(k_bki_emit, per_hit, block, 0, st, a);
  hipLaunchKernelGGL(k_bki_alloc, dim3(bki_stride_blocks(h.members)), block, 0, st, a);
  if (n) hipLaunchKernelGGL(k_bki_scatter, dim3(bki_blocks(nn * BKI_HIT_SLOTS)), block, 0, st, a);
  hipLaunchKernelGGL(k_bki_update, dim3(bki_stride_blocks(h.members)), block, 0, st, a);
  if (feat && h.hit_members > (unsigned long long)BKI_SHORT_RUN)
    hipLaunchKernelGGL(k_bki_long, dim3((unsigned)std::min<unsigned long long>(h.hit_members / (BKI_SHORT_RUN + 1), BKI_GRID_MAX)), dim3(BKI_WAVE), 0, st, a);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  m->broken = false;
  m->voxels += h.fresh;
  stats->training = h.training;
  stats->members = h.members;
  stats->longest_run = h.longest_run;
  stats->longest_probe = h.longest_probe;
  return CVO_OK;
}

// The rest of an insert under the sparse kernel, as bki_insert_counted: the table grows by seven voxels per membership - a
// block and its face neighbours -, the records are stored, sorted by block, summed per test voxel (cvo_k_bki_sparse.h).
int bki_insert_counted_sparse(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, BkiStats* stats, const char* who) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  if (h.members >= (unsigned long long)BKI_SPARSE_MAX_RECORDS)
    return fail(ctx, CVO_E_UNSUPPORTED, std::string(who) + ": 2^24 block memberships or more in one insert under the sparse kernel");
  const size_t nrec = (size_t)h.members, nn = (size_t)a.n;
  const unsigned nb = (unsigned)((nrec + SORT_THREADS - 1) / SORT_THREADS);
  BkiSparseArgs s{};
  unsigned* hist = nullptr;
  int rc = m->work_scratch.lay_out(ctx, "voxel map work scratch", [&](ScratchLayout& l) {
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
  if ((rc = bki_table_grow(m, m->voxels + BKI_SPARSE_SLOTS * h.members)) != CVO_OK) return rc;
  a.t = m->t;
  s.a = a;
  s.sf2 = m->cfg.sf2;
  s.ell = m->cfg.ell;
  s.n_rec = (unsigned)nrec;
  m->broken = true;  // (until the table's counters are back at zero)
  m->occupied = -1;
  const dim3 block(BKI_THREADS);
  if (nrec) {  // (no membership: the origin alone, in a rounding gap between two boxes)
    hipLaunchKernelGGL(k_bkis_offsets, dim3(1), dim3(BKIS_SCAN_THREADS), 0, st, s);
    hipLaunchKernelGGL(k_bkis_emit, dim3(bki_blocks(nn + 1)), block, 0, st, s);
    sort_pairs_u64(ctx, s.n_rec, s.key, s.val, hist);
    const unsigned tests_grid = bki_stride_blocks(BKI_SPARSE_SLOTS * nrec);
    hipLaunchKernelGGL(k_bkis_heads, dim3(bki_blocks(nrec)), block, 0, st, s);
    hipLaunchKernelGGL(k_bkis_update, dim3(tests_grid), block, 0, st, s);
    hipLaunchKernelGGL(k_bkis_long, dim3((unsigned)std::min<size_t>(BKI_SPARSE_SLOTS * nrec / (BKI_SHORT_RUN + 1) + 1, BKI_GRID_MAX)), dim3(BKI_WAVE), 0, st, s);
    hipLaunchKernelGGL(k_bkis_reset, dim3(tests_grid), block, 0, st, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  m->broken = false;
  m->voxels += h.fresh;
  stats->training = h.training;
  stats->members = h.members;
  stats->longest_run = h.longest_run;
  stats->longest_probe = h.longest_probe;
  return CVO_OK;
}

int bki_insert_counted_kernel(cvo_map* m, BkiInsertArgs& a, BkiCtl& h, BkiStats* stats, const char* who) {
  return m->kernel == CVO_MAP_KERNEL_SPARSE ? bki_insert_counted_sparse(m, a, h, stats, who) : bki_insert_counted(m, a, h, stats);
}

int bki_insert_device(cvo_map* m, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  const BkiConst& k = m->k;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  BkiInsertArgs a{};
  int rc = bki_insert_scratch(m, n, feat != nullptr, origin, &a);
  if (rc != CVO_OK) return rc;
  BkiCtl h{};
  if (n) HIP_TRY(ctx, hipMemcpyAsync((void*)a.xyz, xyz, 12 * nn, hipMemcpyHostToDevice, st));
  if (n && feat) HIP_TRY(ctx, hipMemcpyAsync((void*)a.feat, feat, 4 * BKI_FEAT * nn, hipMemcpyHostToDevice, st));
  if (n && k.C > 0) HIP_TRY(ctx, hipMemcpyAsync((void*)a.label, label, 4 * (size_t)k.C * nn, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_bki_count, dim3(bki_blocks(nn + 1)), dim3(BKI_THREADS), 0, st, a);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, a.ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if ((rc = bki_count_refusal(ctx, "cvo_map_insert", h, n)) != CVO_OK) return rc;
  return bki_insert_counted_kernel(m, a, h, stats, "cvo_map_insert");
}

// Collects and sorts the occupied voxels of a device map; *okey / *oslot point at the sorted arrays in work_scratch, *rows at
// room for the rows behind them.  count_only: one pass over the table that writes nothing but the number.
int bki_collect_device(cvo_map* m, bool count_only, unsigned* n_occ, const unsigned long long** okey, const unsigned** oslot, float** rows) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t V = count_only ? 0 : (size_t)m->voxels, nbmax = bki_blocks(V);
  BkiCtl* ctl = nullptr;
  unsigned long long* key[2] = {nullptr, nullptr};
  unsigned *slot[2] = {nullptr, nullptr}, *hist = nullptr;
  const int rc = m->work_scratch.lay_out(ctx, "voxel map work scratch", [&](ScratchLayout& l) {
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
  if (!m->voxels) return m->occupied = 0, CVO_OK;
  BkiCtl h{};
  HIP_TRY(ctx, hipMemsetAsync(ctl, 0, sizeof *ctl, st));
  hipLaunchKernelGGL(k_bki_occupied, dim3(bki_stride_blocks(m->slots)), dim3(BKI_THREADS), 0, st, m->k, m->t, count_only ? nullptr : key[0],
                     count_only ? nullptr : slot[0], ctl);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (h.n_occ > m->voxels) return fail(ctx, CVO_E_HIP, "cvo_map_cloud: the device found more occupied voxels than the map holds");
  const unsigned n = h.n_occ;
  if (!count_only) sort_pairs_u64(ctx, n, key, slot, hist);
  HIP_TRY(ctx, hipGetLastError());
  *n_occ = n;
  m->occupied = n;
  return CVO_OK;
}

// the rows of the cloud read out, on the host: xyz n x 3, feat n x 5, label n x C
struct BkiRows {
  long long n = 0;
  std::vector<float> xyz, feat, label;
};

int bki_rows(cvo_map* m, bool want_rows, BkiRows* out) {
  const BkiConst& k = m->k;
  if (m->side != 0) {
    const auto occ = bki_occupied_cpu(m);
    out->n = (long long)occ.size();
    m->occupied = out->n;
    if (!want_rows) return CVO_OK;
    out->xyz.resize(3 * occ.size());
    out->feat.resize(BKI_FEAT * occ.size());
    out->label.resize((size_t)k.C * occ.size());
    for (size_t i = 0; i < occ.size(); i++) {
      const size_t v = occ[i].second;
      bki_row(k, occ[i].first, &m->host.ms[v * (size_t)k.nclass], &m->host.fs[v * BKI_FEAT], &out->xyz[3 * i], &out->feat[BKI_FEAT * i],
              k.C > 0 ? &out->label[(size_t)k.C * i] : nullptr);
    }
    return CVO_OK;
  }
  cvo_ctx* ctx = m->ctx;
  unsigned n = 0;
  const unsigned long long* okey;
  const unsigned* oslot;
  float* d_xyz;
  const int rc = bki_collect_device(m, !want_rows, &n, &okey, &oslot, &d_xyz);
  if (rc != CVO_OK) return rc;
  out->n = n;
  if (!want_rows || !n) return CVO_OK;
  float* d_feat = d_xyz + 3 * (size_t)n;
  float* d_label = d_feat + BKI_FEAT * (size_t)n;
  hipStream_t st = ctx->upload_stream;
  hipLaunchKernelGGL(k_bki_rows, dim3(bki_blocks(n)), dim3(BKI_THREADS), 0, st, k, m->t, n, okey, oslot, d_xyz, d_feat, d_label, k.C, k.C);
  HIP_TRY(ctx, hipGetLastError());
  out->xyz.resize(3 * (size_t)n);
  out->feat.resize(BKI_FEAT * (size_t)n);
  out->label.resize((size_t)k.C * n);
  HIP_TRY(ctx, hipMemcpyAsync(out->xyz.data(), d_xyz, 12 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(out->feat.data(), d_feat, 4 * BKI_FEAT * (size_t)n, hipMemcpyDeviceToHost, st));
  if (k.C > 0) HIP_TRY(ctx, hipMemcpyAsync(out->label.data(), d_label, 4 * (size_t)k.C * n, hipMemcpyDeviceToHost, st));
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
    BkiStats stats;
    int r;
    const int side = m->side >= 0 ? m->side : (ctx ? bki_choose_side(m, n, xyz, origin) : 1);
    if (side == 1) {
      std::string text;
      r = bki_insert_cpu_kernel(m, n, xyz, feat, label, origin, &stats, &text);
      if (r != CVO_OK) return fail(ctx, r, std::string(who) + ": " + text);
      m->occupied = -1;
    } else {
      stats.on_device = 1;
      if ((r = bki_insert_device(m, n, xyz, feat, label, origin, &stats)) != CVO_OK) return r;
    }
    m->side = side;
    m->last = stats;
    return (int)CVO_OK;
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
  m->initial_slots = slots;
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
  if (m->broken) return fail(ctx, CVO_E_HIP, std::string(who) + ": an earlier insert failed on the device half way: the map cannot be used");
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
  if (n > 0 && k.C > 0 && !c_label) return fail(ctx, CVO_E_INVALID, who + ": a map with classes needs label rows");
  if (m->broken) return fail(ctx, CVO_E_HIP, who + ": an earlier insert failed on the device half way: the map cannot be used");
  if ((long long)n >= BKI_MAX_TRAINING) return fail(ctx, CVO_E_UNSUPPORTED, who + ": more than 2^24 training points in one insert");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  BkiInsertArgs a{};
  int rc = bki_insert_scratch(m, n, c_feat != nullptr, origin, &a);
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
  BkiStats stats;
  if (side == 1) {  // the staged arrays are the three bki_insert_cpu takes
    std::vector<float> hx(3 * nn), hf(c_feat ? BKI_FEAT * nn : 0), hl((size_t)k.C * nn);
    if (n) HIP_TRY(ctx, hipMemcpyAsync(hx.data(), a.xyz, 12 * nn, hipMemcpyDeviceToHost, st));
    if (n && c_feat) HIP_TRY(ctx, hipMemcpyAsync(hf.data(), a.feat, 4 * BKI_FEAT * nn, hipMemcpyDeviceToHost, st));
    if (n && k.C > 0) HIP_TRY(ctx, hipMemcpyAsync(hl.data(), a.label, 4 * (size_t)k.C * nn, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::string text;
    rc = bki_insert_cpu_kernel(m, n, hx.data(), c_feat ? hf.data() : nullptr, k.C > 0 ? hl.data() : nullptr, origin, &stats, &text);
    if (rc != CVO_OK) return fail(ctx, rc, who + ": " + text);
    m->occupied = -1;
  } else {
    stats.on_device = 1;
    if ((rc = bki_count_refusal(ctx, who, h, n)) != CVO_OK) return rc;
    if ((rc = bki_insert_counted_kernel(m, a, h, &stats, who.c_str())) != CVO_OK) return rc;
  }
  m->side = side;
  m->last = stats;
  return CVO_OK;
}

// The occupied voxels of a device map as ingest rows where k_bki_rows leaves them - label rows at the padded stride
// k_cloud_ingest reads, zeros behind the map's classes - and cvo_cloud_from_device's body on them: its route rule orders the
// cloud.  The caller holds upload_mutex.
int bki_cloud_resident_device(cvo_map* m, const char* who, std::vector<StagedCloud>& staged, long long* n_out) {
  cvo_ctx* ctx = m->ctx;
  const BkiConst& k = m->k;
  unsigned n = 0;
  const unsigned long long* okey;
  const unsigned* oslot;
  float* d_xyz;
  const int rc = bki_collect_device(m, false, &n, &okey, &oslot, &d_xyz);
  if (rc != CVO_OK) return rc;
  float* d_feat = d_xyz + 3 * (size_t)n;
  float* d_label = d_feat + BKI_FEAT * (size_t)n;
  if (n) {
    hipLaunchKernelGGL(k_bki_rows, dim3(bki_blocks(n)), dim3(BKI_THREADS), 0, ctx->upload_stream, k, m->t, n, okey, oslot, d_xyz, d_feat, d_label,
                       NC_PAD, NC_PAD);
    HIP_TRY(ctx, hipGetLastError());
  }
  cvo_device_rows_t d{};
  d.n = d.n_records = (int)n;
  d.xyz = d_xyz;
  d.xyz_stride = 12;
  d.feat = d_feat;
  d.feat_stride = sizeof(float) * BKI_FEAT;
  d.label = k.C > 0 ? d_label : nullptr;
  d.label_stride = sizeof(float) * NC_PAD;
  *n_out = n;
  return ingest_device_clouds(ctx, 1, &d, staged, who);  // (synchronises upload_stream; on error the cloud is released)
}

// ---- the read side: point queries, ray casts, a rendered view (tests/np_bki_query.py; the kernels: cvo_k_bki_query.h) ----

// a voxel of the host map, or the default node (ms = prior, fs = 0) in `def`
struct BkiHostNode {
  bool stored = false;
  const float *ms = nullptr, *fs = nullptr;
  float def_ms[BKI_MAX_CLASSES + 1], def_fs[BKI_FEAT];
};

void bki_node_cpu(const cvo_map* m, bool inside, unsigned long long key, BkiHostNode* node) {
  const BkiConst& k = m->k;
  node->stored = false;
  if (inside) {
    const auto it = m->host.index.find(key);
    if (it != m->host.index.end()) {
      node->stored = true;
      node->ms = &m->host.ms[(size_t)it->second * (size_t)k.nclass];
      node->fs = &m->host.fs[(size_t)it->second * BKI_FEAT];
      return;
    }
  }
  for (int c = 0; c < k.nclass; c++) node->def_ms[c] = k.prior;
  for (int c = 0; c < BKI_FEAT; c++) node->def_fs[c] = 0.f;
  node->ms = node->def_ms;
  node->fs = node->def_fs;
}

void bki_node_class_cpu(const cvo_map* m, const BkiHostNode& node, int* state, int* semantics) {
  *state = BKI_UNKNOWN;
  *semantics = -1;
  if (!node.stored) return;
  const float* ms = node.ms;
  *state = bki_state(m->k, ms);
  *semantics = bki_semantics([&](int c) { return ms[c]; }, bki_sum(ms, 0, m->k.nclass), m->k.nclass);
}

unsigned bki_look_cpu(const cvo_map* m, unsigned long long key) {
  const auto it = m->host.index.find(key);
  return it == m->host.index.end() ? (unsigned)BKI_BIT_ABSENT : bki_state_bit(m->k, &m->host.ms[(size_t)it->second * (size_t)m->k.nclass]);
}

void bki_centre3(float size, bool valid, unsigned long long key, float* out) {
  out[0] = valid ? bki_centre((long long)(key >> 40), size) : bki_nan();
  out[1] = valid ? bki_centre((long long)((key >> 20) & 0xFFFFFull), size) : bki_nan();
  out[2] = valid ? bki_centre((long long)(key & 0xFFFFFull), size) : bki_nan();
}

void bki_query_cpu(const cvo_map* m, int n, const float* xyz, const cvo_map_query_out_t& o) {
  const BkiConst& k = m->k;
  BkiHostNode node;
  for (size_t i = 0; i < (size_t)n; i++) {
    unsigned long long key = 0;
    const bool inside = bki_point_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], k.size, &key);
    bki_node_cpu(m, inside, key, &node);
    int state, sem;
    bki_node_class_cpu(m, node, &state, &sem);
    const float sum = bki_sum(node.ms, 0, k.nclass), occ = bki_sum(node.ms, 1, k.nclass);
    if (o.found) o.found[i] = (uint8_t)(!inside ? BKI_Q_OUTSIDE : (node.stored ? BKI_Q_FOUND : BKI_Q_ABSENT));
    if (o.state) o.state[i] = (uint8_t)state;
    if (o.semantics) o.semantics[i] = sem;
    for (int c = 0; o.probs && c < k.nclass; c++) o.probs[i * (size_t)k.nclass + c] = bki_prob(node.ms[c], sum);
    for (int c = 0; o.vars && c < k.nclass; c++) o.vars[i * (size_t)k.nclass + c] = bki_var(node.ms[c], sum);
    for (int c = 0; o.feat && c < BKI_FEAT; c++) o.feat[i * BKI_FEAT + c] = node.fs[c] / occ;
    if (o.centre) bki_centre3(k.size, inside, key, o.centre + 3 * i);
  }
}

void bki_raycast_cpu(const cvo_map* m, int n, const float* origin, const float* end, unsigned stop_mask, int max_steps, const cvo_map_ray_out_t& o) {
  const BkiConst& k = m->k;
  BkiHostNode node;
  for (size_t i = 0; i < (size_t)n; i++) {
    const BkiRay r = bki_ray_walk(k.size, origin + 3 * i, end + 3 * i, stop_mask, max_steps, [&](unsigned long long key) { return bki_look_cpu(m, key); });
    const bool walked = r.key != BKI_NO_KEY;
    bki_node_cpu(m, walked, r.key, &node);
    int state, sem;
    bki_node_class_cpu(m, node, &state, &sem);
    if (o.status) o.status[i] = (uint8_t)r.status;
    if (o.key) o.key[i] = r.key;
    if (o.centre) bki_centre3(k.size, walked, r.key, o.centre + 3 * i);
    if (o.t) o.t[i] = r.t;
    if (o.steps) o.steps[i] = r.steps;
    if (o.state) o.state[i] = (uint8_t)state;
    if (o.semantics) o.semantics[i] = sem;
  }
}

struct BkiCamera {
  float pose[12], fx, fy, cx, cy, z_far;
  int rows, cols;
};

void bki_render_cpu(const cvo_map* m, const BkiCamera& cam, unsigned stop_mask, const cvo_map_render_out_t& out) {
  const BkiConst& k = m->k;
  const float* T = cam.pose;
  const float o[3] = {T[3], T[7], T[11]};
  BkiHostNode node;
  for (int v = 0; v < cam.rows; v++)
    for (int u = 0; u < cam.cols; u++) {
      const size_t px = (size_t)v * cam.cols + u;
      float c[3], e[3];
      bki_pixel_end(u, v, cam.fx, cam.fy, cam.cx, cam.cy, cam.z_far, c);
      for (int r = 0; r < 3; r++) e[r] = std::fmaf(T[4 * r], c[0], T[4 * r + 1] * c[1]) + std::fmaf(T[4 * r + 2], c[2], T[4 * r + 3]);
      const BkiRay ray = bki_ray_walk(k.size, o, e, stop_mask, BKI_RAY_MAX_STEPS, [&](unsigned long long key) { return bki_look_cpu(m, key); });
      const bool stop = ray.status == BKI_RAY_STOPPED;
      bki_node_cpu(m, stop, ray.key, &node);
      int state, sem;
      bki_node_class_cpu(m, node, &state, &sem);
      if (out.depth) out.depth[px] = stop ? (float)(ray.td * (double)cam.z_far) : 0.f;
      if (out.semantics) out.semantics[px] = sem;
      const float sum = bki_sum(node.ms, 0, k.nclass), occ = bki_sum(node.ms, 1, k.nclass);
      for (int q = 0; out.feat && q < BKI_FEAT; q++) out.feat[BKI_FEAT * px + q] = stop ? node.fs[q] / occ : 0.f;
      for (int q = 1; out.label && q <= k.C; q++) out.label[(size_t)k.C * px + q - 1] = stop ? node.ms[q] / sum : 0.f;
    }
}

// room for `count` elements behind *d when the caller wants that output
template <class T>
void bki_take_if(ScratchLayout& l, const void* wanted, T*& d, size_t count) {
  d = nullptr;
  if (wanted) l.take(d, count);
}

template <class T>
hipError_t bki_copy_down(T* host, const T* dev, size_t count, hipStream_t st) {
  return host && count ? hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, st) : hipSuccess;
}

// points from host rows (xyz) or from a resident cloud under a pose (cloud; pose12 or nullptr)
int bki_query_device(cvo_map* m, int n, const float* xyz, const cvo_cloud* cloud, const float* pose12, const cvo_map_query_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n, nc = (size_t)m->k.nclass;
  BkiQueryArgs a{};
  float* d_xyz = nullptr;
  const int rc = m->work_scratch.lay_out(ctx, "voxel map query scratch", [&](ScratchLayout& l) {
    if (xyz) l.take(d_xyz, 3 * nn);
    bki_take_if(l, o.found, a.found, nn);
    bki_take_if(l, o.state, a.state, nn);
    bki_take_if(l, o.semantics, a.semantics, nn);
    bki_take_if(l, o.probs, a.probs, nc * nn);
    bki_take_if(l, o.vars, a.vars, nc * nn);
    bki_take_if(l, o.feat, a.feat, BKI_FEAT * nn);
    bki_take_if(l, o.centre, a.centre, 3 * nn);
  });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->t;
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
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, bki_copy_down((unsigned char*)o.found, (const unsigned char*)a.found, nn, st));
  HIP_TRY(ctx, bki_copy_down((unsigned char*)o.state, (const unsigned char*)a.state, nn, st));
  HIP_TRY(ctx, bki_copy_down((int*)o.semantics, (const int*)a.semantics, nn, st));
  HIP_TRY(ctx, bki_copy_down(o.probs, (const float*)a.probs, nc * nn, st));
  HIP_TRY(ctx, bki_copy_down(o.vars, (const float*)a.vars, nc * nn, st));
  HIP_TRY(ctx, bki_copy_down(o.feat, (const float*)a.feat, BKI_FEAT * nn, st));
  HIP_TRY(ctx, bki_copy_down(o.centre, (const float*)a.centre, 3 * nn, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

int bki_raycast_device(cvo_map* m, int n, const float* origin, const float* end, unsigned stop_mask, int max_steps, const cvo_map_ray_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  BkiRaycastArgs a{};
  float *d_o = nullptr, *d_e = nullptr;
  const int rc = m->work_scratch.lay_out(ctx, "voxel map ray scratch", [&](ScratchLayout& l) {
    l.take(d_o, 3 * nn);
    l.take(d_e, 3 * nn);
    bki_take_if(l, o.status, a.out.status, nn);
    bki_take_if(l, o.key, a.out.key, nn);
    bki_take_if(l, o.centre, a.out.centre, 3 * nn);
    bki_take_if(l, o.t, a.out.t, nn);
    bki_take_if(l, o.steps, a.out.steps, nn);
    bki_take_if(l, o.state, a.out.state, nn);
    bki_take_if(l, o.semantics, a.out.semantics, nn);
  });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->t;
  a.n = n;
  a.stop_mask = stop_mask;
  a.max_steps = max_steps;
  a.origin = d_o;
  a.end = d_e;
  HIP_TRY(ctx, hipMemcpyAsync(d_o, origin, 12 * nn, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d_e, end, 12 * nn, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_bki_raycast, dim3(bki_blocks(nn)), dim3(BKI_THREADS), 0, st, a);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, bki_copy_down((unsigned char*)o.status, (const unsigned char*)a.out.status, nn, st));
  HIP_TRY(ctx, bki_copy_down((unsigned long long*)o.key, (const unsigned long long*)a.out.key, nn, st));
  HIP_TRY(ctx, bki_copy_down(o.centre, (const float*)a.out.centre, 3 * nn, st));
  HIP_TRY(ctx, bki_copy_down(o.t, (const float*)a.out.t, nn, st));
  HIP_TRY(ctx, bki_copy_down((int*)o.steps, (const int*)a.out.steps, nn, st));
  HIP_TRY(ctx, bki_copy_down((unsigned char*)o.state, (const unsigned char*)a.out.state, nn, st));
  HIP_TRY(ctx, bki_copy_down((int*)o.semantics, (const int*)a.out.semantics, nn, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

int bki_render_device(cvo_map* m, const BkiCamera& cam, unsigned stop_mask, const cvo_map_render_out_t& o) {
  cvo_ctx* ctx = m->ctx;
  hipStream_t st = ctx->upload_stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)cam.rows * cam.cols, C = (size_t)m->k.C;
  BkiRenderArgs a{};
  const int rc = m->work_scratch.lay_out(ctx, "voxel map render scratch", [&](ScratchLayout& l) {
    bki_take_if(l, o.depth, a.depth, px);
    bki_take_if(l, o.semantics, a.semantics, px);
    bki_take_if(l, o.feat, a.feat, BKI_FEAT * px);
    bki_take_if(l, C ? o.label : nullptr, a.label, C * px);
  });
  if (rc != CVO_OK) return rc;
  a.k = m->k;
  a.t = m->t;
  a.rows = cam.rows;
  a.cols = cam.cols;
  a.stop_mask = stop_mask;
  for (int q = 0; q < 12; q++) a.pose[q] = cam.pose[q];
  a.fx = cam.fx, a.fy = cam.fy, a.cx = cam.cx, a.cy = cam.cy, a.z_far = cam.z_far;
  const unsigned long long tiles = (unsigned long long)((cam.cols + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE) * ((cam.rows + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE);
  hipLaunchKernelGGL(k_bki_render, dim3((unsigned)((tiles + BKI_THREADS / BKI_WAVE - 1) / (BKI_THREADS / BKI_WAVE))), dim3(BKI_THREADS), 0, st, a);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, bki_copy_down(o.depth, (const float*)a.depth, px, st));
  HIP_TRY(ctx, bki_copy_down((int*)o.semantics, (const int*)a.semantics, px, st));
  HIP_TRY(ctx, bki_copy_down(o.feat, (const float*)a.feat, BKI_FEAT * px, st));
  if (C) HIP_TRY(ctx, bki_copy_down(o.label, (const float*)a.label, C * px, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return CVO_OK;
}

// what every read checks first: the handle, the kind of map the entry point is for, a map an insert left half way
int bki_read_check(cvo_map* m, bool host_call, const std::string& who) {
  if (!m) return CVO_E_INVALID;
  if (host_call != (m->ctx == nullptr))
    return fail(m->ctx, CVO_E_INVALID, who + (host_call ? ": the map belongs to a context" : ": the map is one of cvo_map_open_host"));
  if (m->broken) return fail(m->ctx, CVO_E_HIP, who + ": an earlier insert failed on the device half way: the map cannot be used");
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
    bki_query_cpu(m, n, xyz, o);  // (a map of the host side; an undecided map holds nothing and stays undecided)
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
    bki_raycast_cpu(m, n, origin, end, stop_mask, max_steps, o);
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
    bki_render_cpu(m, cam, stop_mask, o);
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
  // the rows under the pose as cvo_cloud_transformed moves them (transform_point_pose_vec), the translation as origin
  std::vector<float> moved;
  try {
    moved.resize(3 * (size_t)n);
  } catch (const std::exception& e) {
    return fail(m->ctx, CVO_E_NOMEM, std::string("cvo_map_insert_posed: ") + e.what());
  }
  const float* T = pose12;
  for (int i = 0; i < n; i++) {
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    for (int r = 0; r < 3; r++) moved[3 * (size_t)i + r] = std::fmaf(T[4 * r], x, T[4 * r + 1] * y) + std::fmaf(T[4 * r + 2], z, T[4 * r + 3]);
  }
  const float origin[3] = {T[3], T[7], T[11]};
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
  if (m->broken) return fail(ctx, CVO_E_HIP, "cvo_map_size: an earlier insert failed on the device half way: the map cannot be used");
  return frontend_call(ctx, "cvo_map_size", [&] {
    if (occupied && m->occupied < 0) {
      BkiRows rows;
      const int rc = bki_rows(m, false, &rows);
      if (rc != CVO_OK) return rc;
    }
    if (voxels) *voxels = m->side == 0 ? (long long)m->voxels : (long long)m->host.keys.size();
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
  if (m->broken) return fail(ctx, CVO_E_HIP, std::string(who) + ": an earlier insert failed on the device half way: the map cannot be used");
  std::vector<StagedCloud> staged;
  long long rows_n = 0;
  const int rc = frontend_call(ctx, who, [&] {
    if (m->side == 0) return bki_cloud_resident_device(m, who, staged, &rows_n);
    // a map of the host side (or without an insert): the twin's rows, uploaded
    BkiRows rows;
    int r = bki_rows(m, true, &rows);
    if (r != CVO_OK) return r;
    staged.resize(1);
    if ((r = bki_upload_rows(ctx, m->k.C, rows, &staged[0].c)) != CVO_OK) return staged[0].c = nullptr, r;
    rows_n = rows.n;
    return (int)CVO_OK;
  });
  for (auto& sc : staged) {
    if (rc == CVO_OK) *out = sc.c;
    else if (sc.c) cvo_cloud_free(sc.c);  // (an exception left it behind; an error return released it itself)
  }
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
    const float* T = pose12;
    for (size_t i = 0; i < (size_t)n; i++) {
      const float x = x4[i].x, y = x4[i].y, z = x4[i].z;
      xyz[3 * i] = x, xyz[3 * i + 1] = y, xyz[3 * i + 2] = z;
      for (int r = 0; T && r < 3; r++) xyz[3 * i + r] = std::fmaf(T[4 * r], x, T[4 * r + 1] * y) + std::fmaf(T[4 * r + 2], z, T[4 * r + 3]);
    }
    bki_query_cpu(m, n, xyz.data(), o);
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
    const unsigned long long capacity = dev ? m->slots : m->host.keys.size();
    if (on_device) *on_device = m->last.on_device;
    if (counts) {
      counts[0] = m->last.training;
      counts[1] = m->last.members;
      counts[2] = m->last.longest_run;
      counts[3] = capacity;
      counts[4] = (unsigned long long)m->growths;
      counts[5] = m->last.longest_probe;
      counts[6] = dev ? m->voxels : m->host.keys.size();
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
    if (keys) HIP_TRY(ctx, hipMemcpyAsync(keys, m->t.keys, 8 * capacity, hipMemcpyDeviceToHost, st));
    if (ms) HIP_TRY(ctx, hipMemcpyAsync(ms, m->t.ms, 4 * capacity * (size_t)m->k.nclass, hipMemcpyDeviceToHost, st));
    if (fs) HIP_TRY(ctx, hipMemcpyAsync(fs, m->t.fs, 4 * capacity * BKI_FEAT, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return (int)CVO_OK;
  });
}

}  // extern "C"
