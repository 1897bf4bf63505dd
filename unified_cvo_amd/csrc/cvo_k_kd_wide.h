// cvo_k_kd_wide.h -- the spatial (k-d) ordering of a cloud above KD_MAX_POINTS points, across many blocks (ORDER=wide).
// Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.  Host side: wide_plan / enqueue_wide_order
// (cvo_upload.hip).
#pragma once
#include "cvo_k_cloud.h"
#include "cvo_k_prims.h"

namespace cvo_dev {

// ------------------------------------------------------------------------------------------
// The rule is k_kd_order's (tests/np_kd.py): one axis per level from the root box's extents, the `kd_left(points)` smallest
// (coordinate, original index) pairs of every segment go left.  The SHAPE of the tree depends on n alone, so the host lays
// the whole plan out before anything runs (wide_plan): per level the segments of more than `leaf` points with their cut,
// tiles of up to KD_WIDE_TILE positions over them, and the leaves - segments of at most `leaf` points - with the level at
// which they were cut off.  The device keeps no segment bookkeeping above a leaf and nothing comes back between levels.
//
//   k_kd_wide_box / _ext   the root box: per-block fminf / fmaxf partials, combined by one wave (no float atomics); the box
//                          kernel also writes the identity order into buffer 0
//   per global level g     (ids are read from buffer g & 1 and written to buffer (g + 1) & 1, cut segments only)
//     k_kd_wide_hist x 4   radix select of the segment's kd_left-th key, 8 bits a pass from the top: a tile counts the
//                          digits of the keys that match the prefix found so far in LDS and adds its nonzero counts to the
//                          segment's histogram of the pass (integer atomics); every block re-derives the prefix from the
//                          histograms of the earlier passes itself (256 counters and one block scan a pass), so a pass is
//                          one plain launch and nothing waits for another block.  Pass 0 leaves the level's keys in `keys`.
//     k_kd_wide_count      the pivot (all four passes) and, per tile, the keys below it and equal to it
//     k_kd_wide_scatter    the stable partition: a tile adds up the counts of the tiles before it in its segment, ranks its
//                          own keys with a block scan and writes every id to its place
//   k_kd_wide_leaves       one block per leaf: kd_order_levels - k_kd_order's level loop - on segment-local ids from the
//                          leaf's level on, with the extents as halved so far; ids go through the global order on the way out
//
// Ties.  Every partition is stable and buffer 0 starts as the identity, so every segment is in ascending original-index
// order at every level.  "Equal keys by original index" is therefore "equal keys by position": of the keys equal to the
// pivot, the first `rem` (the select's remainder) go left - a prefix count, no second select - and a leaf's local ids
// (positions in its segment) order ties as original indices do.  -0.0 and +0.0 are one key (kd_ordered).
// Everything is integer arithmetic on fixed inputs: the same rows give the same order on every call.
// ------------------------------------------------------------------------------------------
constexpr int KD_WIDE_THREADS = 256;
constexpr int KD_WIDE_TILE = 2048;             // positions per tile: 8 per thread
constexpr int KD_WIDE_PER = KD_WIDE_TILE / KD_WIDE_THREADS;
constexpr int KD_WIDE_BOX_BLOCKS = 256;        // at most, of k_kd_wide_box
constexpr int KD_WIDE_MAX_POINTS = 1 << 24;
constexpr int KD_WIDE_LEAF = 1024;             // the default leaf capacity (WIDE_LEAF), at most KD_MAX_POINTS

struct KdWideSeg {
  int lo, hi, left;  // positions [lo, hi), cut at lo + left
  int tile0;         // its first tile (index into the plan's tiles)
};
struct KdWideTile {
  int start, count;  // positions [start, start + count) of one segment
  int seg;           // index into the plan's segments
};
struct KdWideLeaf {
  int lo, n, NP;     // positions [lo, lo + n), the next power of two >= n (>= KD_THREADS)
  int level;         // the level at which it left the global partitions: its ids are in buffer level & 1
  int sop_off;       // its seg_of_pos scratch begins here
};
struct KdWide {
  int n;
  int seg_stride;              // entries of one of a leaf's two seg_lo tables
  const float4* x4;            // coordinates, ORIGINAL order
  int* buf[2];                 // [n] ids, ping-pong
  unsigned* keys;              // [n] kd_ordered coordinate of the current level, by position
  float* box;                  // [KD_WIDE_BOX_BLOCKS][6] partial minima / maxima, behind them the root extents [3]
  unsigned* hist;              // [segments][4][256], zero when the first level starts
  uint2* tile_cnt;             // per tile: keys below the pivot, keys equal to it
  uint2* seg_piv;              // per segment: the pivot key, how many of its equals go left
  const KdWideSeg* segs;
  const KdWideTile* tiles;
  const KdWideLeaf* leaves;
  unsigned short* seg_of_pos;  // scratch of the leaves' level loops
  unsigned short* seg_lo;      // [leaves][2][seg_stride]
  int* order;                  // out: sorted position -> original index
};

// The axis of `level` from the root extents: strict >, y then z over x, the chosen extent halved per level (k_kd_order's
// rule).  ext comes back as it stands AT that level.
__device__ __forceinline__ int kd_level_axis(float (&ext)[3], int level) {
  for (int l = 0;; l++) {
    int axis = 0;
    if (ext[1] > ext[axis]) axis = 1;
    if (ext[2] > ext[axis]) axis = 2;
    if (l == level) return axis;
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (c == axis) ext[c] *= 0.5f;
  }
}
__device__ __forceinline__ void kd_wide_extents(const KdWide& J, float (&ext)[3]) {
  for (int c = 0; c < 3; c++) ext[c] = J.box[KD_WIDE_BOX_BLOCKS * 6 + c];
}

__global__ __launch_bounds__(KD_WIDE_THREADS) void k_kd_wide_box(KdWide J) {
  __shared__ float s_red[KD_WIDE_THREADS / 64][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int p = blockIdx.x * KD_WIDE_THREADS + tid; p < J.n; p += gridDim.x * KD_WIDE_THREADS) {
    const float4 x = J.x4[p];
    lo[0] = fminf(lo[0], x.x); hi[0] = fmaxf(hi[0], x.x);
    lo[1] = fminf(lo[1], x.y); hi[1] = fmaxf(hi[1], x.y);
    lo[2] = fminf(lo[2], x.z); hi[2] = fmaxf(hi[2], x.z);
    J.buf[0][p] = p;
  }
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o));
    }
  if (lane == 0)
    for (int c = 0; c < 3; c++) {
      s_red[wave][c] = lo[c];
      s_red[wave][3 + c] = hi[c];
    }
  __syncthreads();
  if (tid < 6) {
    float v = s_red[0][tid];
    for (int w = 1; w < KD_WIDE_THREADS / 64; w++) v = tid < 3 ? fminf(v, s_red[w][tid]) : fmaxf(v, s_red[w][tid]);
    J.box[blockIdx.x * 6 + tid] = v;
  }
}

// one wave: the partials of `blocks` blocks -> the root extents (max - min, float32)
__global__ __launch_bounds__(64) void k_kd_wide_ext(KdWide J, int blocks) {
  const int lane = threadIdx.x;
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int b = lane; b < blocks; b += 64)
    for (int c = 0; c < 3; c++) {
      lo[c] = fminf(lo[c], J.box[b * 6 + c]);
      hi[c] = fmaxf(hi[c], J.box[b * 6 + 3 + c]);
    }
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o));
    }
  if (lane == 0)
    for (int c = 0; c < 3; c++) J.box[KD_WIDE_BOX_BLOCKS * 6 + c] = hi[c] - lo[c];
}

// The radix select of one segment after `passes` passes over its histograms hist[pass][256]: prefix = the top 8 * passes
// bits of the key of rank `left` (1-based, ascending), rem = that key's rank among the keys that share the prefix.  Exactly
// one digit of a pass holds the rank (the counts of a pass add up to the keys that matched its prefix, and 1 <= rem <= that).
// part[256], pick[2]: LDS.  Every thread of a block of KD_WIDE_THREADS calls it.
__device__ __forceinline__ void kd_wide_select(const unsigned* hist, int passes, unsigned left, unsigned* part, unsigned* pick,
                                               unsigned& prefix, unsigned& rem) {
  prefix = 0u;
  rem = left;
  for (int q = 0; q < passes; q++) {
    const unsigned c = hist[q * 256 + threadIdx.x];
    const unsigned incl = block_scan_incl<KD_WIDE_THREADS>(part, c);
    if (incl - c < rem && rem <= incl) {
      pick[0] = threadIdx.x;
      pick[1] = rem - (incl - c);
    }
    __syncthreads();
    prefix = (prefix << 8) | pick[0];
    rem = pick[1];
    __syncthreads();
  }
}

// one pass of the select over the tiles [tile0, tile0 + gridDim.x) of level `level`
__global__ __launch_bounds__(KD_WIDE_THREADS) void k_kd_wide_hist(KdWide J, int level, int tile0, int pass) {
  __shared__ unsigned part[KD_WIDE_THREADS], pick[2], s_h[256];
  const int tid = threadIdx.x;
  const KdWideTile T = J.tiles[tile0 + blockIdx.x];
  const KdWideSeg S = J.segs[T.seg];
  unsigned* hist = J.hist + (size_t)T.seg * 1024;
  pick[0] = pick[1] = 0u;
  s_h[tid] = 0u;
  unsigned prefix, rem;
  kd_wide_select(hist, pass, (unsigned)S.left, part, pick, prefix, rem);  // (its barriers publish s_h and pick; pass 0: none needed)
  __syncthreads();
  if (pass == 0) {
    float ext[3];
    kd_wide_extents(J, ext);
    const int axis = kd_level_axis(ext, level);
    const int* src = J.buf[level & 1];
    for (int e = tid; e < T.count; e += KD_WIDE_THREADS) {
      const float4 x = J.x4[min((unsigned)src[T.start + e], (unsigned)J.n - 1u)];  // (an id is < n; clamped, so that no state of the buffers reads outside x4)
      const unsigned key = kd_ordered(axis == 0 ? x.x : (axis == 1 ? x.y : x.z));
      J.keys[T.start + e] = key;
      atomicAdd(&s_h[key >> 24], 1u);
    }
  } else {
    const int top = 32 - 8 * pass;  // 24, 16, 8
    for (int e = tid; e < T.count; e += KD_WIDE_THREADS) {
      const unsigned key = J.keys[T.start + e];
      if ((key >> top) == prefix) atomicAdd(&s_h[(key >> (top - 8)) & 255u], 1u);
    }
  }
  __syncthreads();
  if (s_h[tid]) atomicAdd(&hist[pass * 256 + tid], s_h[tid]);
}

// the block's sum of v (part[256]: LDS)
__device__ __forceinline__ unsigned kd_wide_block_sum(unsigned* part, unsigned v) {
  (void)block_scan_incl<KD_WIDE_THREADS>(part, v);
  const unsigned total = part[KD_WIDE_THREADS - 1];
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(KD_WIDE_THREADS) void k_kd_wide_count(KdWide J, int tile0) {
  __shared__ unsigned part[KD_WIDE_THREADS], pick[2];
  const int tid = threadIdx.x, t = tile0 + blockIdx.x;
  const KdWideTile T = J.tiles[t];
  const KdWideSeg S = J.segs[T.seg];
  pick[0] = pick[1] = 0u;
  unsigned pivot, rem;
  kd_wide_select(J.hist + (size_t)T.seg * 1024, 4, (unsigned)S.left, part, pick, pivot, rem);
  unsigned lt = 0, eq = 0;
  for (int e = tid; e < T.count; e += KD_WIDE_THREADS) {
    const unsigned key = J.keys[T.start + e];
    lt += key < pivot;
    eq += key == pivot;
  }
  const unsigned both = kd_wide_block_sum(part, lt | (eq << 16));  // (a tile holds at most 2048 keys: neither half carries)
  if (tid == 0) {
    J.tile_cnt[t] = make_uint2(both & 0xffffu, both >> 16);
    if (t == S.tile0) J.seg_piv[T.seg] = make_uint2(pivot, rem);
  }
}

__global__ __launch_bounds__(KD_WIDE_THREADS) void k_kd_wide_scatter(KdWide J, int level, int tile0) {
  __shared__ unsigned part[KD_WIDE_THREADS];
  const int tid = threadIdx.x, t = tile0 + blockIdx.x;
  const KdWideTile T = J.tiles[t];
  const KdWideSeg S = J.segs[T.seg];
  const uint2 piv = J.seg_piv[T.seg];
  const unsigned pivot = piv.x, rem = piv.y;
  // keys below / equal to the pivot in the segment's earlier tiles
  unsigned lt0 = 0, eq0 = 0;
  for (int q = S.tile0 + tid; q < t; q += KD_WIDE_THREADS) {
    const uint2 c = J.tile_cnt[q];
    lt0 += c.x;
    eq0 += c.y;
  }
  lt0 = kd_wide_block_sum(part, lt0);
  eq0 = kd_wide_block_sum(part, eq0);
  // this thread's KD_WIDE_PER consecutive positions
  const int e0 = tid * KD_WIDE_PER;
  unsigned key[KD_WIDE_PER];
  unsigned lt = 0, eq = 0;
#pragma unroll
  for (int q = 0; q < KD_WIDE_PER; q++) {
    key[q] = e0 + q < T.count ? J.keys[T.start + e0 + q] : 0xffffffffu;
    if (e0 + q < T.count) {
      lt += key[q] < pivot;
      eq += key[q] == pivot;
    }
  }
  const unsigned mine = lt | (eq << 16);
  const unsigned before = block_scan_incl<KD_WIDE_THREADS>(part, mine) - mine;
  lt = lt0 + (before & 0xffffu);
  eq = eq0 + (before >> 16);
  const int* src = J.buf[level & 1];
  int* dst = J.buf[(level + 1) & 1];
  const unsigned len = (unsigned)(S.hi - S.lo);
#pragma unroll
  for (int q = 0; q < KD_WIDE_PER; q++) {
    if (e0 + q >= T.count) break;
    const unsigned pos = (unsigned)(T.start + e0 + q - S.lo);        // position in the segment
    const unsigned lefts = lt + (eq < rem ? eq : rem);               // of the positions before it, those that go left
    const bool is_lt = key[q] < pivot, is_eq = key[q] == pivot;
    const bool goes_left = is_lt || (is_eq && eq < rem);
    const unsigned at = goes_left ? lefts : (unsigned)S.left + (pos - lefts);
    if (at < len) dst[S.lo + at] = src[T.start + e0 + q];            // (always, for counts that add up: nothing is written outside the segment)
    lt += is_lt;
    eq += is_eq;
  }
}

__global__ __launch_bounds__(KD_THREADS) void k_kd_wide_leaves(KdWide J) {
  extern __shared__ unsigned long long kd_key[];  // [NP of the launch's largest leaf]
  const KdWideLeaf L = J.leaves[blockIdx.x];
  float ext[3];
  kd_wide_extents(J, ext);
  (void)kd_level_axis(ext, L.level);
  const int* src = J.buf[L.level & 1] + L.lo;
  kd_order_levels(kd_key, L.n, L.NP, ext, J.seg_of_pos + L.sop_off, J.seg_lo + (size_t)blockIdx.x * 2 * J.seg_stride, J.seg_stride,
                  [&](unsigned id) { return J.x4[min((unsigned)src[id], (unsigned)J.n - 1u)]; });
  // (clamped like the reads above: k_cloud_gather scatters through `order` unguarded, so whatever the buffers hold, every id
  // that leaves these kernels is one of the cloud's)
  for (int p = threadIdx.x; p < L.n; p += KD_THREADS) J.order[L.lo + p] = (int)min((unsigned)src[kd_key[p] & 0xffffull], (unsigned)J.n - 1u);
}

}  // namespace cvo_dev
