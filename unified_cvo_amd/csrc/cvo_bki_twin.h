// cvo_bki_twin.h -- the semantic voxel map on ONE CPU thread, without a device: the twin every kernel of cvo_k_bki.h,
// cvo_k_bki_sparse.h and cvo_k_bki_query.h equals bit for bit, and the whole map behind the _host entry points.  BkiTwin owns
// the voxels (index / keys / ms / fs) and takes the map's BkiConst with every call; it knows no cvo_map, no context and no
// stream, so a host compiler builds it alone (with sanitizers, if wanted).  The arithmetic is cvo_bki_math.h, shared with the
// kernels; tests/np_bki.py, np_bki_sparse.py and np_bki_query.py state what is computed.  Also here, because both sides say
// them: the refusal sentences and bki_bad_text.  Plain C++17: cvo_bki_math.h, cvo_pose_math.h, the public cvo_hip.h, standard headers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/cvo_hip.h"
#include "cvo_bki_math.h"
#include "cvo_pose_math.h"

namespace cvo_bki {
using namespace cvo_dev;

// ---- the sentences more than one route refuses with ----
constexpr const char* BKI_SAYS_BROKEN = "an earlier insert failed on the device half way: the map cannot be used";
constexpr const char* BKI_SAYS_NEEDS_LABELS = "a map with classes needs label rows";
constexpr const char* BKI_SAYS_MANY_ROWS = "more than 2^24 training points in one insert";          // by the rows or the points walked
constexpr const char* BKI_SAYS_MANY_TRAINING = "2^24 training points or more in one insert";        // by the caps count
constexpr const char* BKI_SAYS_MANY_RECORDS = "2^24 block memberships or more in one insert under the sparse kernel";
inline std::string bki_says_caps() { return std::string(BKI_SAYS_MANY_TRAINING) + ", or a hit with 65536 beam samples or more"; }

inline std::string bki_bad_text(unsigned status, unsigned index, int n) {
  const std::string who = (int)index >= n ? std::string("the origin") : "hit " + std::to_string(index);
  if (status & BKI_BAD_RANGE) return who + " or one of its beam samples leaves the map's 2^20 blocks per axis";
  if (status & BKI_BAD_TOO_MANY) return who + " needs 65536 beam samples or more";
  return who + " belongs to more than 8 blocks";
}

struct BkiStats {
  int on_device = 0;
  unsigned long long training = 0, members = 0, longest_run = 0, longest_probe = 0;
};

// the rows of the cloud read out, on the host: xyz n x 3, feat n x 5, label n x C
struct BkiRows {
  long long n = 0;
  std::vector<float> xyz, feat, label;
};

struct BkiCamera {
  float pose[12], fx, fy, cx, cy, z_far;
  int rows, cols;
};

// THE beam walk of one insert: its training points in upstream's order - per hit max_range keeps the hit and its beam samples
// (bki_hit_points), hits ascending, the origin last - as visit(i, x, y, z, is_hit), i == n for the origin; false stops it.
// *at: the hit the walk ended at.  BKI_WALK_TOO_MANY: that hit needs BKI_MAX_RAY samples or more.
enum : int { BKI_WALK_DONE = 0, BKI_WALK_STOPPED = 1, BKI_WALK_TOO_MANY = 2 };
template <class Visit>
int bki_beam_walk(const BkiConst& k, int n, const float* xyz, const float* origin, int* at, Visit&& visit) {
  for (*at = 0; *at < n; (*at)++) {
    const int i = *at;
    const float* p = xyz + 3 * (size_t)i;
    if (!bki_in_range(k, p, origin)) continue;
    unsigned too_many = 0;
    if (!bki_hit_points(k, p, origin, &too_many, [&](float x, float y, float z, bool hit) { return visit(i, x, y, z, hit); }))
      return too_many ? BKI_WALK_TOO_MANY : BKI_WALK_STOPPED;
  }
  return visit(n, origin[0], origin[1], origin[2], false) ? BKI_WALK_DONE : BKI_WALK_STOPPED;
}

// Visitor 1, the caps: the training points counted without any block arithmetic; the walk stops as soon as `limit` is
// reached (a ray of BKI_MAX_RAY samples or more counts as `limit`), so a large frame costs no more than a small one.
inline unsigned long long bki_training_count(const BkiConst& k, int n, const float* xyz, const float* origin, unsigned long long limit) {
  unsigned long long training = 0;
  int at = 0;
  const int r = bki_beam_walk(k, n, xyz, origin, &at, [&](int, float, float, float, bool) { return ++training < limit; });
  return r == BKI_WALK_DONE ? training : limit;
}

// Visitors 2 and 3, the memberships in upstream's order, or the refusal: sink(key, x, y, z, cls, hit) per block that holds a
// training point - cls 0 and hit -1: a beam sample or the origin - returns false once its list is full, which ends the walk
// without a refusal.  `training` counts the points.
template <class Sink>
int bki_twin_members(const BkiConst& k, int n, const float* xyz, const float* label, const float* origin, unsigned long long* training,
                     std::string* msg, Sink&& sink) {
  *training = 0;
  bool full = false;
  int at = 0;
  const int r = bki_beam_walk(k, n, xyz, origin, &at, [&](int i, float x, float y, float z, bool hit) {
    const int cls = !hit ? 0 : (k.C > 0 ? bki_class(label + (size_t)i * k.C, k.C) : 1);
    const int m = bki_members(k, x, y, z, [&](unsigned long long key) { if (!sink(key, x, y, z, cls, hit ? i : -1)) full = true; });
    if (m < 0 || full) return false;
    (*training)++;
    return true;
  });
  if (full) return CVO_OK;
  if (r == BKI_WALK_TOO_MANY) return *msg = bki_bad_text(BKI_BAD_TOO_MANY, (unsigned)at, n), CVO_E_UNSUPPORTED;
  if (r == BKI_WALK_STOPPED) return *msg = bki_bad_text(BKI_BAD_RANGE, (unsigned)at, n), CVO_E_INVALID;
  if (*training >= (unsigned long long)BKI_MAX_TRAINING) return *msg = BKI_SAYS_MANY_ROWS, CVO_E_UNSUPPORTED;
  return CVO_OK;
}

// (the caps come first, as in the statement, and before any membership is stored)
inline int bki_twin_caps(const BkiConst& k, int n, const float* xyz, const float* origin, std::string* msg) {
  const unsigned long long cap = (unsigned long long)BKI_MAX_TRAINING;
  return bki_training_count(k, n, xyz, origin, cap) >= cap ? (*msg = bki_says_caps(), CVO_E_UNSUPPORTED) : CVO_OK;
}

struct BkiMember {
  unsigned long long key;
  int cls;  // 0: a beam sample or the origin
  int hit;
};

struct BkiSparseRecord {
  unsigned long long key;
  float p[3];
  int cls, hit;
};

// a voxel, or the default node (ms = prior, fs = 0) in `def`; state and semantics as the node getters answer (not stored: UNKNOWN, -1)
struct BkiTwinNode {
  bool stored = false;
  const float *ms = nullptr, *fs = nullptr;
  float def_ms[BKI_MAX_CLASSES + 1], def_fs[BKI_FEAT];
  int state = BKI_UNKNOWN, semantics = -1;
};

struct BkiTwin {
  static constexpr unsigned NONE = ~0u;
  std::unordered_map<unsigned long long, unsigned> index;
  std::vector<unsigned long long> keys;
  std::vector<float> ms, fs;

  // the voxel of `key`, or NONE
  unsigned find(unsigned long long key) const {
    const auto it = index.find(key);
    return it == index.end() ? NONE : it->second;
  }

  // the voxel of `key`; a new one is stored with ms = prior, fs = 0
  unsigned voxel(const BkiConst& k, unsigned long long key) {
    auto it = index.find(key);
    if (it == index.end()) {
      it = index.emplace(key, (unsigned)keys.size()).first;
      keys.push_back(key);
      ms.resize(ms.size() + (size_t)k.nclass, k.prior);
      fs.resize(fs.size() + BKI_FEAT, 0.f);
    }
    return it->second;
  }

  // ---- the counting sensor model (tests/np_bki.py) ----
  int insert_csm(const BkiConst& k, int n, const float* xyz, const float* feat, const float* label, const float* origin, BkiStats* stats,
                 std::string* msg) {
    std::vector<BkiMember> mem;
    unsigned long long training = 0;
    int rc = bki_twin_caps(k, n, xyz, origin, msg);
    if (rc != CVO_OK) return rc;
    rc = bki_twin_members(k, n, xyz, label, origin, &training, msg, [&](unsigned long long key, float, float, float, int cls, int hit) {
      mem.push_back(BkiMember{key, cls, hit});
      return true;
    });
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
    unsigned long long longest = 0;
    for (size_t b = 0; b < tkeys.size(); b++) {
      const size_t v = voxel(k, tkeys[b]);
      unsigned long long hits = 0;
      for (int c = 0; c < k.nclass; c++) {
        ms[v * (size_t)k.nclass + c] += (float)counts[b * (size_t)k.nclass + c];
        if (c) hits += counts[b * (size_t)k.nclass + c];
      }
      for (int f = 0; f < BKI_FEAT; f++) fs[v * BKI_FEAT + f] += fbar[b * BKI_FEAT + f];
      longest = std::max(longest, hits);
    }
    stats->training = training;
    stats->members = mem.size();
    stats->longest_run = longest;
    return CVO_OK;
  }

  // ---- the sparse kernel (tests/np_bki_sparse.py) ----
  int insert_sparse(const BkiConst& k, float sf2, float ell, int n, const float* xyz, const float* feat, const float* label, const float* origin,
                    BkiStats* stats, std::string* msg) {
    int rc = bki_twin_caps(k, n, xyz, origin, msg);
    if (rc != CVO_OK) return rc;
    // a first walk counts and checks - every refusal of it wins over a full record list -, the second stores the records in
    // training order
    unsigned long long training = 0, again = 0;
    rc = bki_twin_members(k, n, xyz, label, origin, &training, msg, [](unsigned long long, float, float, float, int, int) { return true; });
    if (rc != CVO_OK) return rc;
    std::vector<BkiSparseRecord> rec;
    (void)bki_twin_members(k, n, xyz, label, origin, &again, msg, [&](unsigned long long key, float x, float y, float z, int cls, int hit) {
      rec.push_back(BkiSparseRecord{key, {x, y, z}, cls, hit});
      return rec.size() < (size_t)BKI_SPARSE_MAX_RECORDS;
    });
    if (rec.size() >= (size_t)BKI_SPARSE_MAX_RECORDS) return *msg = BKI_SAYS_MANY_RECORDS, CVO_E_UNSUPPORTED;
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
    std::vector<unsigned> tests;
    std::unordered_map<unsigned long long, char> seen;
    for (size_t b = 0; b < rec.size(); b = seg[rec[b].key].second)
      for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
        unsigned long long key;
        if (bki_sparse_slot(rec[b].key, j, &key) && seen.emplace(key, 1).second) tests.push_back(voxel(k, key));
      }
    for (const unsigned v : tests) {
      const unsigned long long vkey = keys[v];
      float centre[3];
      bki_key_centre(vkey, k.size, centre);
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
        for (int c = 0; c < k.nclass; c++) ms[v * (size_t)k.nclass + c] += ybar[c];
        for (int f = 0; f < BKI_FEAT; f++) fs[v * BKI_FEAT + f] += fbar[f];
      }
    }
    stats->training = training;
    stats->members = rec.size();
    stats->longest_run = longest;
    return CVO_OK;
  }

  // ---- the read-out ----
  // the occupied voxels in ascending key order
  std::vector<std::pair<unsigned long long, unsigned>> occupied(const BkiConst& k) const {
    std::vector<std::pair<unsigned long long, unsigned>> occ;
    for (size_t v = 0; v < keys.size(); v++)
      if (bki_state(k, &ms[v * (size_t)k.nclass]) == BKI_OCCUPIED) occ.emplace_back(keys[v], (unsigned)v);
    std::sort(occ.begin(), occ.end());
    return occ;
  }

  // their number, and with want_rows their rows
  void rows(const BkiConst& k, bool want_rows, BkiRows* out) const {
    const auto occ = occupied(k);
    out->n = (long long)occ.size();
    if (!want_rows) return;
    out->xyz.resize(3 * occ.size());
    out->feat.resize(BKI_FEAT * occ.size());
    out->label.resize((size_t)k.C * occ.size());
    for (size_t i = 0; i < occ.size(); i++) {
      const size_t v = occ[i].second;
      bki_row(k, occ[i].first, &ms[v * (size_t)k.nclass], &fs[v * BKI_FEAT], &out->xyz[3 * i], &out->feat[BKI_FEAT * i],
              k.C > 0 ? &out->label[(size_t)k.C * i] : nullptr);
    }
  }

  // ---- the read side: point queries, ray casts, a rendered view (tests/np_bki_query.py) ----
  void node(const BkiConst& k, bool inside, unsigned long long key, BkiTwinNode* nd) const {
    const unsigned v = inside ? find(key) : NONE;
    nd->stored = v != NONE;
    nd->state = BKI_UNKNOWN;
    nd->semantics = -1;
    if (nd->stored) {
      const float* m = nd->ms = &ms[(size_t)v * (size_t)k.nclass];
      nd->fs = &fs[(size_t)v * BKI_FEAT];
      nd->state = bki_state(k, m);
      nd->semantics = bki_semantics([&](int c) { return m[c]; }, bki_sum(m, 0, k.nclass), k.nclass);
      return;
    }
    for (int c = 0; c < k.nclass; c++) nd->def_ms[c] = k.prior;
    for (int c = 0; c < BKI_FEAT; c++) nd->def_fs[c] = 0.f;
    nd->ms = nd->def_ms;
    nd->fs = nd->def_fs;
  }

  unsigned look(const BkiConst& k, unsigned long long key) const {
    const unsigned v = find(key);
    return v == NONE ? (unsigned)BKI_BIT_ABSENT : bki_state_bit(k, &ms[(size_t)v * (size_t)k.nclass]);
  }

  void query(const BkiConst& k, int n, const float* xyz, const cvo_map_query_out_t& o) const {
    BkiTwinNode nd;
    const size_t nc = (size_t)k.nclass;  // (a local: the compiler counts the two division loops below and vectorizes them)
    for (size_t i = 0; i < (size_t)n; i++) {
      unsigned long long key = 0;
      const bool inside = bki_point_key(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], k.size, &key);
      node(k, inside, key, &nd);
      const float sum = bki_sum(nd.ms, 0, k.nclass), occ = bki_sum(nd.ms, 1, k.nclass);
      if (o.found) o.found[i] = (uint8_t)(!inside ? BKI_Q_OUTSIDE : (nd.stored ? BKI_Q_FOUND : BKI_Q_ABSENT));
      if (o.state) o.state[i] = (uint8_t)nd.state;
      if (o.semantics) o.semantics[i] = nd.semantics;
      for (size_t c = 0; o.probs && c < nc; c++) o.probs[i * nc + c] = bki_prob(nd.ms[c], sum);
      for (size_t c = 0; o.vars && c < nc; c++) o.vars[i * nc + c] = bki_var(nd.ms[c], sum);
      for (int c = 0; o.feat && c < BKI_FEAT; c++) o.feat[i * BKI_FEAT + c] = nd.fs[c] / occ;
      if (o.centre) bki_key_centre_or_nan(inside, key, k.size, o.centre + 3 * i);
    }
  }

  void raycast(const BkiConst& k, int n, const float* origin, const float* end, unsigned stop_mask, int max_steps, const cvo_map_ray_out_t& o) const {
    BkiTwinNode nd;
    for (size_t i = 0; i < (size_t)n; i++) {
      const BkiRay r = bki_ray_walk(k.size, origin + 3 * i, end + 3 * i, stop_mask, max_steps, [&](unsigned long long key) { return look(k, key); });
      const bool walked = r.key != BKI_NO_KEY;
      node(k, walked, r.key, &nd);
      if (o.status) o.status[i] = (uint8_t)r.status;
      if (o.key) o.key[i] = r.key;
      if (o.centre) bki_key_centre_or_nan(walked, r.key, k.size, o.centre + 3 * i);
      if (o.t) o.t[i] = r.t;
      if (o.steps) o.steps[i] = r.steps;
      if (o.state) o.state[i] = (uint8_t)nd.state;
      if (o.semantics) o.semantics[i] = nd.semantics;
    }
  }

  void render(const BkiConst& k, const BkiCamera& cam, unsigned stop_mask, const cvo_map_render_out_t& out) const {
    const float o[3] = {cam.pose[3], cam.pose[7], cam.pose[11]};
    const size_t C = (size_t)k.C;  // (a local, as in query)
    BkiTwinNode nd;
    for (int v = 0; v < cam.rows; v++)
      for (int u = 0; u < cam.cols; u++) {
        const size_t px = (size_t)v * cam.cols + u;
        float c[3], e[3];
        bki_pixel_end(u, v, cam.fx, cam.fy, cam.cx, cam.cy, cam.z_far, c);
        pose_point(cam.pose, c[0], c[1], c[2], e);
        const BkiRay ray = bki_ray_walk(k.size, o, e, stop_mask, BKI_RAY_MAX_STEPS, [&](unsigned long long key) { return look(k, key); });
        const bool stop = ray.status == BKI_RAY_STOPPED;
        node(k, stop, ray.key, &nd);
        if (out.depth) out.depth[px] = stop ? (float)(ray.td * (double)cam.z_far) : 0.f;
        if (out.semantics) out.semantics[px] = nd.semantics;
        const float sum = bki_sum(nd.ms, 0, k.nclass), occ = bki_sum(nd.ms, 1, k.nclass);
        for (int q = 0; out.feat && q < BKI_FEAT; q++) out.feat[BKI_FEAT * px + q] = stop ? nd.fs[q] / occ : 0.f;
        for (size_t q = 1; out.label && q <= C; q++) out.label[C * px + q - 1] = stop ? nd.ms[q] / sum : 0.f;
      }
  }
};

}  // namespace cvo_bki
