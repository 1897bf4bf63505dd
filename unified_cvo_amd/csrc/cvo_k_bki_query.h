// cvo_k_bki_query.h -- the read side of the semantic voxel map on the device: what is at this point (k_bki_query, upstream's
// SemanticBKIOctoMap::search with the node's getters), what does this segment meet first (k_bki_raycast), what does the map
// look like from this pose (k_bki_render).  The arithmetic is cvo_bki_math.h, shared with the CPU twin (cvo_bki_twin.h); the
// statement is tests/np_bki_query.py.  The three kernels only READ the table (table_find, cvo_k_prims.h): the host enqueues
// them on the upload stream behind every insert, no counter, key, ms or fs is written.
//
//   k_bki_query    a lane per point, a tile of 256 points per block trip.  Phase 1: the lane forms its key (bki_point_key - the
//                  k0 per axis, NOT the up to 8 closed-box memberships of the insert), finds its slot, computes the sums of
//                  its ms, the state and the semantics, and leaves slot and sums in LDS.  Phase 2: the tile's probs / vars /
//                  feat / centre rows are each ONE flat run of dwords - 256 nclass, 256 nclass, 1280, 768 - and thread t
//                  takes elements t, t + 256 ...: consecutive lanes store consecutive dwords, every store instruction
//                  writes whole cache lines, as k_bki_stage does; the ms / fs loads of a row's lanes fall into one run.
//                  The points come packed (n x 3 floats, host rows copied up) or as a resident cloud's x4[i] in ORIGINAL
//                  order under an optional pose (transform_point_pose_vec), the way k_bki_stage addresses them.
//   k_bki_raycast  a lane per segment: bki_ray_walk with a table_find per voxel.
//   k_bki_render   a lane per pixel; a wave covers a compact block of 8 x 8 pixels (lane & 7 across, lane >> 3 down), so
//                  neighbouring rays probe neighbouring keys and diverge late.  The ray is made here from the pixel index
//                  (bki_pixel_end, the pose): no ray array exists anywhere.
//
// Both loops of a walk are bounded by construction: the step loop by 1 + N[x] + N[y] + N[z] <= max_steps <= 2^20, fixed
// before the first step; the probe loop by the first empty slot (the table is never past half full) and by the slot count.
//
// What bounds them.  The claim, from reading the code: each voxel of a walk costs one dependent random probe into the table (a
// 64-bit key load whose address comes out of the previous step's arithmetic, then nclass floats of ms for a stored voxel), a
// few dozen double operations in between; a lane waits out a memory latency per voxel, hidden only by the other waves of the
// CU - not VALU and not bandwidth.  What is measured (profiles/map_query/: whole calls by scripts/map_query_probe.py, kernel times
// by one rocprofv3 --kernel-trace --stats pass; no counter run was made): the same 16 686 rays of 5 - 60 m take k_bki_raycast
// 3.0 ms on a table of 2^19 slots, 3.7 ms on 2^20, 6.1 ms on 2^24 and 10.0 ms on 2^26 - the arithmetic is the same, the time
// follows where the table sits - and at most 16.2 M probes in 6.1 ms are under 0.2 TB/s of cache lines.  That is what a latency
// bound looks like and what neither a VALU nor a bandwidth bound would give; the longest ray (about 2000 voxels) is the critical
// path, and 66 blocks of 256 lanes leave most CUs idle.  k_bki_query has one probe per point: 30 - 45 us of a 0.3 ms call, which
// is the launch and the copies around it at the sizes a frame has.  Part of the kernel set of cvo_kernels.h; compiled only as part of
// cvo_hip.hip.  Host side: cvo_bki.hip (the twin: cvo_bki_twin.h).
#pragma once
#include "cvo_k_bki.h"

namespace cvo_dev {

constexpr int BKI_QUERY_THREADS = 256;  // threads of a block = points of a tile
constexpr int BKI_RENDER_TILE = 8;      // a wave's pixel block: 8 x 8

struct BkiQueryArgs {
  BkiConst k;
  BkiTable t;
  int n;
  int has_pose;
  float pose[12];       // 3x4 row-major (has_pose != 0; x4 only)
  const float* xyz;     // n x 3, or null: the points are x4's
  const float4* x4;     // a resident cloud's coordinates, original order
  unsigned char *found, *state;  // every output may be null
  int* semantics;
  float *probs, *vars, *feat, *centre;
};

struct BkiRayOut {
  unsigned char* status;
  unsigned long long* key;
  float *centre, *t;
  int* steps;
  unsigned char* state;
  int* semantics;
};

struct BkiRaycastArgs {
  BkiConst k;
  BkiTable t;
  int n;
  unsigned stop_mask;
  int max_steps;
  const float *origin, *end;  // n x 3 each
  BkiRayOut out;
};

struct BkiRenderArgs {
  BkiConst k;
  BkiTable t;
  int rows, cols;
  unsigned stop_mask;
  float pose[12];
  float fx, fy, cx, cy, z_far;
  float* depth;
  int* semantics;
  float *feat, *label;
};

// the bit of the voxel `key` in a stop mask; *slot: where it is stored, SLOT_NONE: nowhere
__device__ __forceinline__ unsigned bki_look(const BkiConst& k, const BkiTable& t, unsigned long long key, unsigned* slot) {
  const unsigned g = table_find(t.keys, t.mask, (unsigned)key_mix(key), key);
  *slot = g;
  return g == SLOT_NONE ? (unsigned)BKI_BIT_ABSENT : bki_state_bit(k, t.ms + (size_t)g * t.nclass);
}

// state and semantics of the voxel in `slot` (SLOT_NONE: the default node - UNKNOWN, -1)
__device__ __forceinline__ void bki_node_class(const BkiConst& k, const BkiTable& t, unsigned slot, int* state, int* semantics) {
  if (slot == SLOT_NONE) {
    *state = BKI_UNKNOWN;
    *semantics = -1;
    return;
  }
  const float* ms = t.ms + (size_t)slot * t.nclass;
  *state = bki_state(k, ms);
  *semantics = bki_semantics([&](int c) { return ms[c]; }, bki_sum(ms, 0, k.nclass), k.nclass);
}

__global__ __launch_bounds__(BKI_QUERY_THREADS) void k_bki_query(BkiQueryArgs a) {
  __shared__ unsigned s_slot[BKI_QUERY_THREADS];
  __shared__ float s_sum[BKI_QUERY_THREADS], s_occ[BKI_QUERY_THREADS], s_centre[3 * BKI_QUERY_THREADS];
  const int tid = threadIdx.x, nclass = a.k.nclass;
  const int tiles = (a.n + BKI_QUERY_THREADS - 1) / BKI_QUERY_THREADS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform per block)
    const int row0 = tile * BKI_QUERY_THREADS, cnt = min(BKI_QUERY_THREADS, a.n - row0), row = row0 + tid;
    // ---- phase 1: a lane per point
    if (tid < cnt) {
      float x, y, z;
      if (a.xyz) {
        x = a.xyz[3 * (size_t)row], y = a.xyz[3 * (size_t)row + 1], z = a.xyz[3 * (size_t)row + 2];
      } else {
        const float4 p = a.x4[row];
        x = p.x, y = p.y, z = p.z;
        if (a.has_pose) {
          const V3 m = transform_point_pose_vec(a.pose, p.x, p.y, p.z);
          x = m.x, y = m.y, z = m.z;
        }
      }
      unsigned long long key = 0;
      const bool inside = bki_point_key(x, y, z, a.k.size, &key);
      unsigned slot = SLOT_NONE;
      if (inside) slot = table_find(a.t.keys, a.t.mask, (unsigned)key_mix(key), key);
      int state, sem;
      bki_node_class(a.k, a.t, slot, &state, &sem);
      float sum = 0.f, occ = 0.f;
      if (slot != SLOT_NONE) {
        sum = bki_sum(a.t.ms + (size_t)slot * nclass, 0, nclass);
        occ = bki_sum(a.t.ms + (size_t)slot * nclass, 1, nclass);
      } else {  // the default node: ms = prior in every class, summed as a stored voxel's
        for (int c = 0; c < nclass; c++) sum += a.k.prior;
        for (int c = 1; c < nclass; c++) occ += a.k.prior;
      }
      s_slot[tid] = slot;
      s_sum[tid] = sum;
      s_occ[tid] = occ;
      bki_key_centre_or_nan(inside, key, a.k.size, s_centre + 3 * tid);
      if (a.found) a.found[row] = (unsigned char)(!inside ? BKI_Q_OUTSIDE : (slot != SLOT_NONE ? BKI_Q_FOUND : BKI_Q_ABSENT));
      if (a.state) a.state[row] = (unsigned char)state;
      if (a.semantics) a.semantics[row] = sem;
    }
    __syncthreads();
    // ---- phase 2: every float array of the tile as one flat run of dwords
    if (a.probs || a.vars) {
      float* probs = a.probs ? a.probs + (size_t)nclass * row0 : nullptr;
      float* vars = a.vars ? a.vars + (size_t)nclass * row0 : nullptr;
      for (int e = tid; e < cnt * nclass; e += BKI_QUERY_THREADS) {
        const int r = e / nclass, c = e - nclass * r;
        const unsigned slot = s_slot[r];
        const float m = slot != SLOT_NONE ? a.t.ms[(size_t)slot * nclass + c] : a.k.prior;
        if (probs) probs[e] = bki_prob(m, s_sum[r]);
        if (vars) vars[e] = bki_var(m, s_sum[r]);
      }
    }
    if (a.feat) {
      float* feat = a.feat + (size_t)BKI_FEAT * row0;
      for (int e = tid; e < cnt * BKI_FEAT; e += BKI_QUERY_THREADS) {
        const int r = e / BKI_FEAT, c = e - BKI_FEAT * r;
        const unsigned slot = s_slot[r];
        const float f = slot != SLOT_NONE ? a.t.fs[(size_t)slot * BKI_FEAT + c] : 0.f;
        feat[e] = f / s_occ[r];
      }
    }
    if (a.centre) {
      float* centre = a.centre + 3 * (size_t)row0;
      for (int e = tid; e < cnt * 3; e += BKI_QUERY_THREADS) centre[e] = s_centre[e];
    }
    __syncthreads();  // (the next tile overwrites the LDS rows)
  }
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_raycast(BkiRaycastArgs a) {
  const int i = blockIdx.x * BKI_THREADS + (int)threadIdx.x;
  if (i >= a.n) return;
  const float o[3] = {a.origin[3 * (size_t)i], a.origin[3 * (size_t)i + 1], a.origin[3 * (size_t)i + 2]};
  const float e[3] = {a.end[3 * (size_t)i], a.end[3 * (size_t)i + 1], a.end[3 * (size_t)i + 2]};
  unsigned slot = SLOT_NONE;
  const BkiRay r = bki_ray_walk(a.k.size, o, e, a.stop_mask, a.max_steps, [&](unsigned long long key) { return bki_look(a.k, a.t, key, &slot); });
  const bool walked = r.key != BKI_NO_KEY;
  int state, sem;
  bki_node_class(a.k, a.t, walked ? slot : SLOT_NONE, &state, &sem);
  const BkiRayOut& out = a.out;
  if (out.status) out.status[i] = (unsigned char)r.status;
  if (out.key) out.key[i] = r.key;
  if (out.centre) {  // (bki_key_centre_or_nan, written out: through the one pointer the compiler schedules the kernel differently)
    out.centre[3 * (size_t)i] = walked ? bki_key_centre1(r.key, 0, a.k.size) : bki_nan();
    out.centre[3 * (size_t)i + 1] = walked ? bki_key_centre1(r.key, 1, a.k.size) : bki_nan();
    out.centre[3 * (size_t)i + 2] = walked ? bki_key_centre1(r.key, 2, a.k.size) : bki_nan();
  }
  if (out.t) out.t[i] = r.t;
  if (out.steps) out.steps[i] = r.steps;
  if (out.state) out.state[i] = (unsigned char)state;
  if (out.semantics) out.semantics[i] = sem;
}

__global__ __launch_bounds__(BKI_THREADS) void k_bki_render(BkiRenderArgs a) {
  // wave w of the launch takes pixel block (w % tiles_x, w / tiles_x); the block shape is uniform per wave
  const int tiles_x = (a.cols + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE, tiles_y = (a.rows + BKI_RENDER_TILE - 1) / BKI_RENDER_TILE;
  const long long w = (long long)blockIdx.x * (BKI_THREADS / BKI_WAVE) + (threadIdx.x >> 6);
  if (w >= (long long)tiles_x * tiles_y) return;
  const int lane = threadIdx.x & 63;
  const int u = (int)(w % tiles_x) * BKI_RENDER_TILE + (lane & 7), v = (int)(w / tiles_x) * BKI_RENDER_TILE + (lane >> 3);
  if (u >= a.cols || v >= a.rows) return;
  const size_t px = (size_t)v * a.cols + u;
  float cam[3];
  bki_pixel_end(u, v, a.fx, a.fy, a.cx, a.cy, a.z_far, cam);
  const V3 m = transform_point_pose_vec(a.pose, cam[0], cam[1], cam[2]);
  const float o[3] = {a.pose[3], a.pose[7], a.pose[11]}, e[3] = {m.x, m.y, m.z};
  unsigned slot = SLOT_NONE;
  const BkiRay r = bki_ray_walk(a.k.size, o, e, a.stop_mask, BKI_RAY_MAX_STEPS, [&](unsigned long long key) { return bki_look(a.k, a.t, key, &slot); });
  const bool stop = r.status == BKI_RAY_STOPPED;
  if (!stop) slot = SLOT_NONE;
  if (a.depth) a.depth[px] = stop ? (float)(r.td * (double)a.z_far) : 0.f;
  if (a.semantics) {
    int state, sem = -1;
    if (stop) bki_node_class(a.k, a.t, slot, &state, &sem);
    a.semantics[px] = sem;
  }
  // get_features / get_occupied_probs of the stopping voxel (bki_row); a stop at a voxel that is not stored: the default node's
  if (a.feat || (a.label && a.k.C > 0)) {
    float* feat = a.feat ? a.feat + BKI_FEAT * px : nullptr;
    float* label = a.label && a.k.C > 0 ? a.label + (size_t)a.k.C * px : nullptr;
    if (stop && slot != SLOT_NONE) {
      bki_row(a.k, r.key, a.t.ms + (size_t)slot * a.t.nclass, a.t.fs + (size_t)slot * BKI_FEAT, nullptr, feat, label);
    } else {
      float sum = 0.f, occ = 0.f;
      for (int c = 0; c < a.k.nclass; c++) sum += a.k.prior;
      for (int c = 1; c < a.k.nclass; c++) occ += a.k.prior;
      for (int c = 0; feat && c < BKI_FEAT; c++) feat[c] = stop ? 0.f / occ : 0.f;
      for (int c = 0; label && c < a.k.C; c++) label[c] = stop ? a.k.prior / sum : 0.f;
    }
  }
}

}  // namespace cvo_dev
