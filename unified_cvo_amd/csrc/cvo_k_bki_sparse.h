// cvo_k_bki_sparse.h -- one insert into the semantic voxel map under the SPARSE kernel (SemanticBKInference::predict with
// covSparse over get_extended_block's seven blocks; tests/np_bki_sparse.py states it, the arithmetic is cvo_bki_math.h).  Every
// training point votes into the voxels around it with a float weight, and a voxel's sums are taken in a fixed order - slot by
// slot, inside a slot in ascending training order - so nothing here adds floats with atomics: the memberships are STORED as
// records, sorted, and every test voxel then sums its own segments.
//
// k_bki_count (cvo_k_bki.h) has counted the memberships of every hit's beam (mc[]); the host has read the totals, refused or
// grown the table by seven voxels per membership.  Then:
//   k_bkis_offsets  one block: the exclusive prefix sums of mc[] - where the records of hit i start.  A record's place is
//                   therefore its rank in training order (hits ascending, each with its samples, the origin last).
//   k_bkis_emit     k_bki_emit's walk: a record per membership - block key, the point, class and hit index.
//   (sort)          the stable radix sort of cvo_k_sort.h by key, the record's place as value: a block's records become one
//                   contiguous segment in ascending training order.
//   k_bkis_heads    a lane per sorted record: the first of a segment enters its block and the block's face neighbours into
//                   the table and notes where the segment starts, the last where it ends; whoever claims a voxel first
//                   appends it to the list of test voxels.
//   k_bkis_update   a lane per test voxel finds its up to seven segments; up to BKI_SHORT_RUN records in all it sums itself,
//                   a voxel with more goes to
//   k_bkis_long     a wave per voxel: 64 records at a time, the lanes evaluate the weight in parallel, then one lane per
//                   output column (a class of ms, a component of fs) adds the 64 values in order.  Linear in the records:
//                   the voxels next to the sensor origin collect the first beam sample of every ray.
//   k_bkis_reset    the counters of every test voxel return to zero.
// Which slot a voxel lands in and the order of the test voxel list depend on arrival; no output does.
// Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.
#pragma once
#include "cvo_k_bki.h"

namespace cvo_dev {

constexpr int BKIS_SCAN_THREADS = 256;   // lanes of k_bkis_offsets' one block
constexpr unsigned BKIS_HIT_MASK = (1u << 24) - 1u;  // a record's meta word: class << 24 | hit index (class 0: not a hit)

struct BkiSparseArgs {
  BkiInsertArgs a;     // the staged hits, the table, mc[] and the control block, as the counting insert has them
  float sf2, ell;
  unsigned n_rec;      // memberships of the insert (the host's copy of ctl->members)
  unsigned* base;      // n + 2: exclusive prefix sums of mc[]
  unsigned long long* key[2];  // records' keys; [1]: the sort's other buffer
  unsigned* val[2];    // records' places
  float* pt;           // 3 per record, by place
  unsigned* meta;      // by place
  unsigned* tests;     // slots of the test voxels (ctl->seg_used of them)
  unsigned* longlist;  // slots of the test voxels left to k_bkis_long (ctl->n_long)
};
// the per-slot counters of the running insert (BkiTable::cnt): [0] where the block's segment ends (0: no training points),
// [1] claimed as a test voxel; BkiTable::segoff: where the segment starts

__global__ __launch_bounds__(BKIS_SCAN_THREADS) void k_bkis_offsets(BkiSparseArgs s) {
  __shared__ unsigned part[BKIS_SCAN_THREADS];
  const unsigned total = (unsigned)s.a.n + 1u, chunk = (total + BKIS_SCAN_THREADS - 1) / BKIS_SCAN_THREADS;
  const unsigned lo = min(threadIdx.x * chunk, total), hi = min(lo + chunk, total);
  unsigned sum = 0;
  for (unsigned i = lo; i < hi; i++) sum += s.a.mc[i];
  unsigned run = block_scan_incl<BKIS_SCAN_THREADS>(part, sum) - sum;
  for (unsigned i = lo; i < hi; i++) {
    s.base[i] = run;
    run += s.a.mc[i];
  }
  if (hi == total && lo < total) s.base[total] = run;
}

__global__ __launch_bounds__(BKI_THREADS) void k_bkis_emit(BkiSparseArgs s) {
  const BkiInsertArgs& a = s.a;
  const int i = blockIdx.x * BKI_THREADS + (int)threadIdx.x;
  if (i > a.n || !a.mc[i]) return;
  unsigned at = s.base[i];
  const unsigned end = min(s.base[i + 1], s.n_rec);  // (the walk is k_bki_count's: it stores what that one counted)
  const unsigned cls = (i < a.n && a.k.C > 0) ? (unsigned)bki_class(a.label + (size_t)i * a.k.C, a.k.C) : 1u;
  unsigned bad = 0;
  bki_lane_points(a, i, &bad, [&](float x, float y, float z, bool hit) {
    bki_members(a.k, x, y, z, [&](unsigned long long key) {
      if (at >= end) return;
      s.key[0][at] = key;
      s.val[0][at] = at;
      s.pt[3 * (size_t)at] = x;
      s.pt[3 * (size_t)at + 1] = y;
      s.pt[3 * (size_t)at + 2] = z;
      s.meta[at] = hit ? (cls << 24) | (unsigned)i : 0u;
      at++;
    });
    return true;
  });
}

__global__ __launch_bounds__(BKI_THREADS) void k_bkis_heads(BkiSparseArgs s) {
  const BkiTable& t = s.a.t;
  const unsigned p = blockIdx.x * BKI_THREADS + threadIdx.x;
  unsigned fresh = 0, longest = 0, len = 0, g = SLOT_NONE;
  unsigned long long key = 0;
  bool head = false;
  if (p < s.n_rec) {
    key = s.key[0][p];
    head = p == 0 || s.key[0][p - 1] != key;
    const bool tail = p + 1 == s.n_rec || s.key[0][p + 1] != key;
    if (head || tail) {
      g = table_insert(t.keys, t.mask, (unsigned)key_mix(key), key, &fresh, &len);
      longest = len;
      if (head) t.segoff[g] = p;
      if (tail) t.cnt[(size_t)g * t.ncnt] = p + 1u;  // (one lane per block; read in a later launch)
    }
  }
  for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {  // (every lane of the wave: wave_alloc)
    unsigned long long nkey;
    unsigned gn = SLOT_NONE;
    bool won = false;
    if (head && bki_sparse_slot(key, j, &nkey)) {
      gn = j ? table_insert(t.keys, t.mask, (unsigned)key_mix(nkey), nkey, &fresh, &len) : g;
      longest = max(longest, len);
      won = atomicExch(&t.cnt[(size_t)gn * t.ncnt + 1], 1u) == 0u;
    }
    const unsigned at = wave_alloc(won ? 1u : 0u, &s.a.ctl->seg_used);
    if (won) s.tests[at] = gn;
  }
  fresh = wave_sum_u32(fresh);
  longest = wave_max_u32(longest);
  if ((threadIdx.x & 63) == 0) {
    if (fresh) atomicAdd(&s.a.ctl->fresh, fresh);
    atomicMax(&s.a.ctl->longest_probe, longest);
  }
}

// what a test voxel reads of neighbour slot j: the segment [*from, *to) of the sorted records, empty without training points
__device__ __forceinline__ bool bkis_segment(const BkiTable& t, unsigned long long vkey, unsigned g, int j, unsigned* from, unsigned* to) {
  unsigned long long key;
  if (!bki_sparse_slot(vkey, j, &key)) return false;
  const unsigned gn = j ? table_find(t.keys, t.mask, (unsigned)key_mix(key), key) : g;  // (no kernel is writing keys now)
  if (gn == SLOT_NONE) return false;
  *to = t.cnt[(size_t)gn * t.ncnt];
  if (!*to) return false;
  *from = t.segoff[gn];
  return *from < *to;
}

constexpr int BKIS_ACC = BKI_MAX_CLASSES + 1 + BKI_FEAT;  // a voxel's columns: ybar of every class, fbar
constexpr int BKIS_ACC_STRIDE = BKIS_ACC + 2;             // (27 words: odd, the lanes of a wave fall into different banks)

__global__ __launch_bounds__(BKI_THREADS) void k_bkis_update(BkiSparseArgs s) {
  __shared__ float acc_all[BKI_THREADS * BKIS_ACC_STRIDE];
  const BkiTable& t = s.a.t;
  const BkiConst& k = s.a.k;
  const unsigned n_tests = s.a.ctl->seg_used;
  float* acc = acc_all + threadIdx.x * BKIS_ACC_STRIDE;
  unsigned longest = 0;
  for (unsigned q = blockIdx.x * BKI_THREADS + threadIdx.x; q < n_tests; q += gridDim.x * BKI_THREADS) {
    const unsigned g = s.tests[q];
    const unsigned long long vkey = t.keys[g];
    unsigned from[BKI_SPARSE_SLOTS], to[BKI_SPARSE_SLOTS], total = 0;
    for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
      if (bkis_segment(t, vkey, g, j, &from[j], &to[j])) total += to[j] - from[j];
      else from[j] = to[j] = 0;
    }
    longest = max(longest, to[0] - from[0]);
    if (total > (unsigned)BKI_SHORT_RUN) {
      s.longlist[atomicAdd(&s.a.ctl->n_long, 1u)] = g;
      continue;
    }
    float centre[3];
    bki_key_centre(vkey, k.size, centre);
    float* ms = t.ms + (size_t)g * t.nclass;
    float* fs = t.fs + (size_t)g * BKI_FEAT;
    for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
      if (from[j] == to[j]) continue;
      for (int c = 0; c < BKIS_ACC; c++) acc[c] = 0.f;
      for (unsigned e = from[j]; e < to[j]; e++) {
        const unsigned r = min(s.val[0][e], s.n_rec - 1u), meta = s.meta[r];  // (a record's place, always below n_rec)
        const float p[3] = {s.pt[3 * (size_t)r], s.pt[3 * (size_t)r + 1], s.pt[3 * (size_t)r + 2]};
        const float w = bki_sparse_k(centre, p, s.sf2, s.ell);
        acc[meta >> 24] += w;
        if (meta && s.a.feat) {
          const float* row = s.a.feat + (size_t)min(meta & BKIS_HIT_MASK, (unsigned)s.a.n - 1u) * BKI_FEAT;
          for (int f = 0; f < BKI_FEAT; f++) acc[BKI_MAX_CLASSES + 1 + f] += w * row[f];
        }
      }
      for (int c = 0; c < t.nclass; c++) ms[c] += acc[c];
      for (int f = 0; f < BKI_FEAT; f++) fs[f] += acc[BKI_MAX_CLASSES + 1 + f];
    }
  }
  longest = wave_max_u32(longest);
  if ((threadIdx.x & 63) == 0) atomicMax(&s.a.ctl->longest_run, longest);
}

__global__ __launch_bounds__(BKI_WAVE) void k_bkis_long(BkiSparseArgs s) {
  __shared__ float w_of[BKI_WAVE], wf[BKI_WAVE][BKI_FEAT];
  __shared__ unsigned cls_of[BKI_WAVE];
  const BkiTable& t = s.a.t;
  const unsigned n_long = s.a.ctl->n_long, lane = threadIdx.x;
  const unsigned nclass = (unsigned)t.nclass;
  for (unsigned q = blockIdx.x; q < n_long; q += gridDim.x) {
    const unsigned g = s.longlist[q];
    const unsigned long long vkey = t.keys[g];
    float centre[3];
    bki_key_centre(vkey, s.a.k.size, centre);
    // lane c < nclass holds ms[c], lane nclass + f holds fs[f]
    const bool is_ms = lane < nclass, is_fs = lane >= nclass && lane < nclass + (unsigned)BKI_FEAT;
    float* out = is_ms ? t.ms + (size_t)g * nclass + lane : (is_fs ? t.fs + (size_t)g * BKI_FEAT + (lane - nclass) : nullptr);
    float value = out ? *out : 0.f;
    for (int j = 0; j < BKI_SPARSE_SLOTS; j++) {
      unsigned from = 0, to = 0;
      if (!bkis_segment(t, vkey, g, j, &from, &to)) continue;  // (uniform: every lane reads the same words)
      float acc = 0.f;
      for (unsigned c0 = from; c0 < to; c0 += BKI_WAVE) {
        const unsigned m = min((unsigned)BKI_WAVE, to - c0);
        if (lane < m) {
          const unsigned r = min(s.val[0][c0 + lane], s.n_rec - 1u), meta = s.meta[r];
          const float p[3] = {s.pt[3 * (size_t)r], s.pt[3 * (size_t)r + 1], s.pt[3 * (size_t)r + 2]};
          const float w = bki_sparse_k(centre, p, s.sf2, s.ell);
          w_of[lane] = w;
          cls_of[lane] = meta >> 24;
          const bool rows = meta && s.a.feat;
          const float* row = rows ? s.a.feat + (size_t)min(meta & BKIS_HIT_MASK, (unsigned)s.a.n - 1u) * BKI_FEAT : nullptr;
          for (int f = 0; f < BKI_FEAT; f++) wf[lane][f] = rows ? w * row[f] : 0.f;
        }
        __syncthreads();
        if (is_ms) {
          for (unsigned e = 0; e < m; e++)
            if (cls_of[e] == lane) acc += w_of[e];
        } else if (is_fs && s.a.feat) {
          for (unsigned e = 0; e < m; e++)
            if (cls_of[e]) acc += wf[e][lane - nclass];
        }
        __syncthreads();
      }
      value += acc;
    }
    if (out) *out = value;
  }
}

__global__ __launch_bounds__(BKI_THREADS) void k_bkis_reset(BkiSparseArgs s) {
  const BkiTable& t = s.a.t;
  const unsigned n_tests = s.a.ctl->seg_used;
  for (unsigned q = blockIdx.x * BKI_THREADS + threadIdx.x; q < n_tests; q += gridDim.x * BKI_THREADS) {
    const unsigned g = s.tests[q];
    t.cnt[(size_t)g * t.ncnt] = 0;
    t.cnt[(size_t)g * t.ncnt + 1] = 0;
  }
}

}  // namespace cvo_dev
