// cvo_k_bki.h -- the semantic voxel map on the device (semantic_bki::SemanticBKIOctoMap::insert_pointcloud_csm at
// block_depth 1, and the read-out of CvoPointCloud(const SemanticBKIOctoMap*, num_classes)); the arithmetic is cvo_bki_math.h,
// the statement tests/np_bki.py.  The map is a persistent open-addressing table in HBM: per slot a 64-bit key, ms (one float
// per class), fs (5 floats), and the counters of the running insert, which are all zero between inserts.
//
// One insert:
//   k_bki_count    a lane per hit (and one for the origin) walks the hit's beam and counts its training points and block
//                  memberships, checks every block index; nothing is written to the table.  The host reads the totals,
//                  refuses or grows the table (k_bki_fill, k_bki_rehash), then enqueues the rest:
//   k_bki_emit     the same walk; every membership enters the table (table_insert, cvo_k_prims.h) and
//                  bumps the slot's INTEGER counters: all memberships, and per class of a hit.  The lane whose bump found
//                  the total at zero marks its record FIRST: it stands for the voxel in the passes below.  Hits also note
//                  their (at most 8) slots.
//   k_bki_alloc    a lane per record: a FIRST record whose voxel has hits takes a segment of the hit-index buffer.
//   k_bki_scatter  a lane per (hit, slot): the hit's index goes into its voxel's segment, in arrival order.
//   k_bki_update   a lane per record, FIRST only: ms += float(counts), once per class; a segment of up to BKI_SHORT_RUN
//                  hits is summed in ASCENDING HIT INDEX by picking the next larger index each step; a longer one is left
//                  to k_bki_long.  The counters return to zero.
//   k_bki_long     a wave per long voxel: every index finds its rank among the segment's, the ranked copy is summed 64 rows
//                  at a time through LDS, sequentially, one lane per feature column.  The ranking is h^2 / 64 loads per lane for
//                  h hits: microseconds at 3000, about a second at 10^5 (DESIGN.md section 3 names the cliff).
// Which slot a voxel lands in, which record is FIRST and the order inside a segment depend on arrival; no output does.
//
// An insert of a resident cloud (cvo_map_insert_cloud) has k_bki_stage (cvo_k_bki_stage.h) write the hits where the host
// would have copied them; the six kernels above follow unchanged.
//
// The read-out: k_bki_occupied collects (key, slot) of the OCCUPIED voxels (wave_alloc), the radix sort of cvo_k_sort.h puts
// them in ascending key order, k_bki_rows writes the rows.  Part of the kernel set of cvo_kernels.h; compiled only as part of
// cvo_hip.hip.
#pragma once
#include "cvo_bki_math.h"
#include "cvo_k_prims.h"

namespace cvo_dev {

constexpr int BKI_THREADS = 256;          // lanes per block of every kernel here but k_bki_long
constexpr int BKI_WAVE = 64;
constexpr int BKI_SHORT_RUN = 16;         // hits of one voxel that k_bki_update sums itself
constexpr int BKI_HIT_SLOTS = 8;          // blocks a hit can belong to: two per axis
constexpr int BKI_GRID_MAX = 2048;        // blocks of the striding kernels
constexpr unsigned BKI_FIRST = 1u << 31;  // flag of a record; a table has at most 2^30 slots
constexpr unsigned long long BKI_MAX_SLOTS = 1ull << 30;

struct BkiTable {
  unsigned long long* keys;  // TABLE_EMPTY: free
  float* ms;                 // nclass per slot; `prior` in every free slot
  float* fs;                 // BKI_FEAT per slot
  unsigned* cnt;             // ncnt per slot: [memberships, segment fill, hits of class 1 .. nclass - 1] of the running insert
  unsigned* segoff;          // where the slot's hit segment starts (valid during an insert, for voxels with hits)
  unsigned mask;             // slots - 1
  int nclass, ncnt;
};

struct BkiCtl {
  unsigned status, bad_index;  // OR of BKI_BAD_*; the lowest hit index with a bad point (n: the origin)
  unsigned long long training, members, hit_members;
  unsigned rec_used, seg_used, n_long, fresh, longest_probe, longest_run, n_occ;
  unsigned nonfinite;  // k_bki_stage (cvo_k_bki_stage.h): the lowest row whose moved coordinate is not finite, ~0u: none
};

struct BkiInsertArgs {
  BkiConst k;
  BkiTable t;
  int n;
  const float *xyz, *feat, *label;  // feat / label may be null (label: only with C = 0)
  float origin[3];
  unsigned* mc;        // n + 1: memberships of hit i with its samples; [n]: the origin's
  unsigned* rec;       // a slot per membership, BKI_FIRST on one record of every voxel touched
  unsigned* hslot;     // n x BKI_HIT_SLOTS: the slots of hit i, SLOT_NONE behind them
  unsigned *seg, *seg2;  // hit indices per voxel; seg2: the ranked copy of the long ones
  unsigned* longlist;  // (slot, hits) of the voxels left to k_bki_long
  BkiCtl* ctl;
};

// the training points of lane i: hit i < n with its beam, or the origin (i == n).  f(x, y, z, is_hit) as bki_hit_points.
template <class F>
__device__ __forceinline__ void bki_lane_points(const BkiInsertArgs& a, int i, unsigned* bad, F&& f) {
  if (i == a.n) {
    f(a.origin[0], a.origin[1], a.origin[2], false);
    return;
  }
  const float p[3] = {a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2]};
  if (!bki_in_range(a.k, p, a.origin)) return;
  unsigned too_many = 0;
  bki_hit_points(a.k, p, a.origin, &too_many, f);
  if (too_many) *bad |= BKI_BAD_TOO_MANY;
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_count(BkiInsertArgs a) {
  const int i = blockIdx.x * BKI_THREADS + (int)threadIdx.x;
  unsigned training = 0, members = 0, hit_members = 0, bad = 0;
  if (i <= a.n) {
    bki_lane_points(a, i, &bad, [&](float x, float y, float z, bool hit) {
      const int m = bki_members(a.k, x, y, z, [](unsigned long long) {});
      training++;
      if (m < 0) return bad |= BKI_BAD_RANGE, true;  // (the walk goes on: the host refuses by the training count first)
      if (hit && m > BKI_HIT_SLOTS) return bad |= BKI_BAD_INTERNAL, false;
      members += (unsigned)m;
      if (hit) hit_members = (unsigned)m;
      return true;
    });
    a.mc[i] = bad ? 0u : members;
    if (bad) {
      atomicOr(&a.ctl->status, bad);
      atomicMin(&a.ctl->bad_index, (unsigned)i);
    }
  }
  // (a lane's counts stay below 2^28: exact in a double)
  const double t = wave_sum((double)training), m = wave_sum((double)members), h = wave_sum((double)hit_members);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&a.ctl->training, (unsigned long long)t);
    atomicAdd(&a.ctl->members, (unsigned long long)m);
    atomicAdd(&a.ctl->hit_members, (unsigned long long)h);
  }
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_emit(BkiInsertArgs a) {
  const int i = blockIdx.x * BKI_THREADS + (int)threadIdx.x;
  const unsigned want = i <= a.n ? a.mc[i] : 0u;
  unsigned at = wave_alloc(want, &a.ctl->rec_used);
  unsigned fresh = 0, longest = 0, len;
  if (i < a.n)
    for (int m = 0; m < BKI_HIT_SLOTS; m++) a.hslot[(size_t)i * BKI_HIT_SLOTS + m] = SLOT_NONE;
  if (want) {
    const int cls = (i < a.n && a.k.C > 0) ? bki_class(a.label + (size_t)i * a.k.C, a.k.C) : 1;
    unsigned bad = 0;
    int hm = 0;
    bki_lane_points(a, i, &bad, [&](float x, float y, float z, bool hit) {
      bki_members(a.k, x, y, z, [&](unsigned long long key) {
        const unsigned g = table_insert(a.t.keys, a.t.mask, (unsigned)key_mix(key), key, &fresh, &len);
        longest = max(longest, len);
        unsigned* c = a.t.cnt + (size_t)g * a.t.ncnt;
        const unsigned first = atomicAdd(&c[0], 1u) == 0u ? BKI_FIRST : 0u;
        if (hit) {
          atomicAdd(&c[1 + cls], 1u);
          a.hslot[(size_t)i * BKI_HIT_SLOTS + hm++] = g;
        }
        a.rec[at++] = g | first;
      });
      return true;
    });
  }
  fresh = wave_sum_u32(fresh);
  longest = wave_max_u32(longest);
  if ((threadIdx.x & 63) == 0) {
    if (fresh) atomicAdd(&a.ctl->fresh, fresh);
    atomicMax(&a.ctl->longest_probe, longest);
  }
}

__device__ __forceinline__ unsigned bki_slot_hits(const BkiTable& t, unsigned g) {
  unsigned h = 0;
  for (int c = 2; c < t.ncnt; c++) h += t.cnt[(size_t)g * t.ncnt + c];
  return h;
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_alloc(BkiInsertArgs a) {
  const unsigned nrec = a.ctl->rec_used;
  for (unsigned base = blockIdx.x * BKI_THREADS; base < nrec; base += gridDim.x * BKI_THREADS) {  // (uniform per block)
    const unsigned r = base + threadIdx.x;
    unsigned g = 0, h = 0;
    if (r < nrec && (a.rec[r] & BKI_FIRST)) {
      g = a.rec[r] & ~BKI_FIRST;
      h = bki_slot_hits(a.t, g);
    }
    const unsigned off = wave_alloc(h, &a.ctl->seg_used);
    if (h) a.t.segoff[g] = off;
  }
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_scatter(BkiInsertArgs a) {
  const size_t e = (size_t)blockIdx.x * BKI_THREADS + threadIdx.x;
  if (e >= (size_t)a.n * BKI_HIT_SLOTS) return;
  const unsigned g = a.hslot[e];
  if (g == SLOT_NONE) return;
  const unsigned at = atomicAdd(&a.t.cnt[(size_t)g * a.t.ncnt + 1], 1u);
  a.seg[a.t.segoff[g] + at] = (unsigned)(e / BKI_HIT_SLOTS);
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_update(BkiInsertArgs a) {
  const unsigned nrec = a.ctl->rec_used;
  unsigned longest = 0;
  for (unsigned base = blockIdx.x * BKI_THREADS; base < nrec; base += gridDim.x * BKI_THREADS) {
    const unsigned r = base + threadIdx.x;
    if (r >= nrec || !(a.rec[r] & BKI_FIRST)) continue;
    const unsigned g = a.rec[r] & ~BKI_FIRST;
    unsigned* c = a.t.cnt + (size_t)g * a.t.ncnt;
    float* ms = a.t.ms + (size_t)g * a.t.nclass;
    unsigned h = 0;
    for (int q = 1; q < a.t.nclass; q++) {
      const unsigned v = c[1 + q];
      h += v;
      ms[q] += (float)v;  // (ybar: an exact float, one add per class and insert)
      c[1 + q] = 0;
    }
    ms[0] += (float)(c[0] - h);
    c[0] = 0;
    c[1] = 0;
    longest = max(longest, h);
    if (!h || !a.feat) continue;  // (fbar = 0: fs + 0 is fs, fs is never -0)
    if (h > (unsigned)BKI_SHORT_RUN) {
      const unsigned q = atomicAdd(&a.ctl->n_long, 1u);
      a.longlist[2 * (size_t)q] = g;
      a.longlist[2 * (size_t)q + 1] = h;
      continue;
    }
    const unsigned* seg = a.seg + a.t.segoff[g];
    float fbar[BKI_FEAT] = {0.f, 0.f, 0.f, 0.f, 0.f};
    long long last = -1;
    for (unsigned s = 0; s < h; s++) {  // the next larger hit index (they are distinct)
      long long next = LLONG_MAX;
      for (unsigned q = 0; q < h; q++) {
        const long long v = (long long)seg[q];
        if (v > last && v < next) next = v;
      }
      if (next == LLONG_MAX) break;  // (cannot happen: the indices of a segment are distinct)
      for (int f = 0; f < BKI_FEAT; f++) fbar[f] += a.feat[(size_t)next * BKI_FEAT + f];
      last = next;
    }
    for (int f = 0; f < BKI_FEAT; f++) a.t.fs[(size_t)g * BKI_FEAT + f] += fbar[f];
  }
  longest = wave_max_u32(longest);
  if ((threadIdx.x & 63) == 0) atomicMax(&a.ctl->longest_run, longest);
}

__global__ __launch_bounds__(BKI_WAVE) void k_bki_long(BkiInsertArgs a) {
  __shared__ float rows[BKI_WAVE][BKI_FEAT];
  const unsigned n_long = a.ctl->n_long, lane = threadIdx.x;
  for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
    const unsigned g = a.longlist[2 * (size_t)q], h = a.longlist[2 * (size_t)q + 1];
    const unsigned* seg = a.seg + a.t.segoff[g];
    unsigned* ranked = a.seg2 + a.t.segoff[g];
    for (unsigned e = lane; e < h; e += BKI_WAVE) {
      const unsigned v = seg[e];
      unsigned rank = 0;
      for (unsigned s = 0; s < h; s++) rank += seg[s] < v ? 1u : 0u;
      ranked[rank] = v;
    }
    __syncthreads();
    float acc = 0.f;
    for (unsigned c0 = 0; c0 < h; c0 += BKI_WAVE) {
      if (c0 + lane < h) {
        const unsigned v = min(ranked[c0 + lane], (unsigned)a.n - 1u);  // (a hit index, always below n)
        for (int c = 0; c < BKI_FEAT; c++) rows[lane][c] = a.feat[(size_t)v * BKI_FEAT + c];
      }
      __syncthreads();
      if (lane < (unsigned)BKI_FEAT) {
        const unsigned m = min((unsigned)BKI_WAVE, h - c0);
        for (unsigned s = 0; s < m; s++) acc += rows[s][lane];
      }
      __syncthreads();
    }
    if (lane < (unsigned)BKI_FEAT) a.t.fs[(size_t)g * BKI_FEAT + lane] += acc;
  }
}

// ---- the table: a fresh one, and an old one moved into it ----
__global__ __launch_bounds__(BKI_THREADS) void k_bki_fill(float* ms, size_t n, float prior) {
  for (size_t i = (size_t)blockIdx.x * BKI_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * BKI_THREADS) ms[i] = prior;
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_rehash(BkiTable from, BkiTable to) {
  for (size_t s = (size_t)blockIdx.x * BKI_THREADS + threadIdx.x; s <= from.mask; s += (size_t)gridDim.x * BKI_THREADS) {
    const unsigned long long key = from.keys[s];
    if (key == TABLE_EMPTY) continue;
    const unsigned g = table_insert(to.keys, to.mask, (unsigned)key_mix(key), key);
    for (int c = 0; c < from.nclass; c++) to.ms[(size_t)g * to.nclass + c] = from.ms[s * from.nclass + c];
    for (int c = 0; c < BKI_FEAT; c++) to.fs[(size_t)g * BKI_FEAT + c] = from.fs[s * BKI_FEAT + c];
  }
}

// ---- the read-out ----
__global__ __launch_bounds__(BKI_THREADS) void k_bki_occupied(BkiConst k, BkiTable t, unsigned long long* okey, unsigned* oslot, BkiCtl* ctl) {
  const unsigned slots = t.mask + 1u;
  for (unsigned base = blockIdx.x * BKI_THREADS; base < slots; base += gridDim.x * BKI_THREADS) {  // (uniform per block)
    const unsigned g = base + threadIdx.x;
    unsigned long long key = TABLE_EMPTY;
    if (g < slots) key = t.keys[g];
    const bool occ = key != TABLE_EMPTY && bki_state(k, t.ms + (size_t)g * t.nclass) == BKI_OCCUPIED;
    const unsigned at = wave_alloc(occ ? 1u : 0u, &ctl->n_occ);
    if (occ && okey) {  // (okey == nullptr: counted only)
      okey[at] = key;
      oslot[at] = g;
    }
  }
}

// label rows: label_stride floats apart, the C values followed by zeros up to label_width (the packed rows of cvo_map_cloud:
// both C; the rows k_cloud_ingest reads at a stride of 80 bytes, cvo_map_cloud_resident: both NC_PAD)
__global__ __launch_bounds__(BKI_THREADS) void k_bki_rows(BkiConst k, BkiTable t, unsigned n, const unsigned long long* key, const unsigned* slot,
                                                          float* xyz, float* feat, float* label, int label_stride, int label_width) {
  const unsigned i = blockIdx.x * BKI_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned g = slot[i];
  float* lab = k.C > 0 ? label + (size_t)label_stride * i : nullptr;
  bki_row(k, key[i], t.ms + (size_t)g * t.nclass, t.fs + (size_t)g * BKI_FEAT, xyz + 3 * (size_t)i, feat + (size_t)BKI_FEAT * i, lab);
  for (int c = k.C; lab && c < label_width; c++) lab[c] = 0.f;
}

}  // namespace cvo_dev
