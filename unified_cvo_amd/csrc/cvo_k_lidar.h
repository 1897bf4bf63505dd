// cvo_k_lidar.h -- kernels of the LiDAR front end (cvo_lidar.hip): LeGoLoamPointSelection::cloudHandler of a raw scan on the
// n_scan x horizon_scan range image.  The decisions are the functions of cvo_lidar_math.h, which the CPU twin calls too.
//
//   LidarTransition    predicate of k_compact_count: the 4 -> 1 quadrant transitions, whose inclusive scan is the ring id
//   k_lidar_project    ring id (compact_block_rank<true>), column and range of every point; the LAST point in index order wins
//                      its cell (atomicMax)
//   k_lidar_cells      per cell: range, ground (a gather over the pair below and the pair above), the union-find's start
//   k_lidar_union      4-connected components, columns wrapping: uf_unite (cvo_k_prims.h), the root is the lowest row-major cell
//   k_lidar_flatten    the root of every cell; size and row mask (seed excluded) of a component by atomics on its root
//   k_lidar_valid      the validity rule per cell, the component counts
//   LidarSegKeep       predicate of the ordered compaction that makes the segmented cloud, row-major
//   k_lidar_bounds     segmented points before every ring (a binary search per ring)
//   k_lidar_smooth     curvature and occlusion marks, both stencils over the segmented arrays
//   k_lidar_pick       one block per ring: its six sixths one after another - sort by (curvature, index) in LDS, the greedy
//                      pick with neighbour suppression in one lane, up to 20 edges per sixth in pick order
//   LidarCand, LidarKept   predicates of the two ordered compactions of the thinning: a candidate's rank is its draw
//
// No output depends on the order waves arrive in: max, min, add and or commute; every position comes from an ordered
// compaction; the union-find is uf_find / uf_unite (cvo_k_prims.h).  Part of the kernel set of cvo_kernels.h; compiled only as
// part of cvo_hip.hip.
#pragma once
#include "cvo_k_compact.h"
#include "cvo_lidar_math.h"

namespace cvo_dev {

constexpr int LIDAR_THREADS = 256;
constexpr int LIDAR_PICK_THREADS = 256;
constexpr int LIDAR_SORT_MAX = 1024;                  // a sixth holds at most (LIDAR_MAX_HORIZON - 10) / 6 + 1 = 682 entries
constexpr int LIDAR_FLAG_PAD = 8;                     // suppression reaches 5 past a ring's range on either side
constexpr int LIDAR_FLAGS = LIDAR_MAX_HORIZON + 2 * LIDAR_FLAG_PAD;
enum : unsigned char { LIDAR_EMPTY = 0, LIDAR_GROUND = 1, LIDAR_LIVE = 2 };

struct LidarStats {
  unsigned projected, ground, valid, invalid;
};

struct LidarTransition {
  using Item = int;
  const float4* p;
  __device__ bool flag(int i, int n) const {
    if (i < 1 || i >= n) return false;
    const float4 a = p[i - 1], b = p[i];
    return lidar_quadrant(b.x, b.z) == 1 && lidar_quadrant(a.x, a.z) == 4;
  }
  __device__ bool keep(int i, int n, Item*) const { return flag(i, n); }
  __device__ void write(unsigned, const Item&) const {}
};

__global__ __launch_bounds__(COMPACT_THREADS) void k_lidar_project(int n, LidarTransition tr, LidarConst k, const unsigned* __restrict__ block_offset,
                                                                   int* cellwin) {
  const int i = blockIdx.x * COMPACT_THREADS + (int)threadIdx.x;
  const unsigned ring = compact_block_rank<true>(tr.flag(i, n), block_offset);  // inclusive: the transition point opens its ring
  if (i >= n || ring >= (unsigned)k.R) return;
  const float4 q = tr.p[i];
  const int col = lidar_column(q.x, q.z, k.ang_res_x, k.H);
  if (col < 0 || lidar_range(q.x, q.y, q.z) < k.min_range) return;
  atomicMax(&cellwin[(int)ring * k.H + col], i);
}

__device__ __forceinline__ bool lidar_cell_pair(const float4* __restrict__ p, const int* __restrict__ cellwin, int lo_cell, int up_cell, const LidarConst& k) {
  const int a = cellwin[lo_cell], b = cellwin[up_cell];
  if (a < 0 || b < 0) return false;
  const float4 pa = p[a], pb = p[b];
  const float lo[3] = {pa.x, pa.y, pa.z}, up[3] = {pb.x, pb.y, pb.z};
  return lidar_ground_pair(lo, up, k);
}

__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_cells(LidarConst k, const float4* __restrict__ p, const int* __restrict__ cellwin,
                                                               float* __restrict__ range, unsigned char* __restrict__ state, int* __restrict__ parent,
                                                               LidarStats* stats) {
  const int c = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x, cells = k.R * k.H;
  bool full = false, ground = false;
  if (c < cells) {
    const int w = cellwin[c], row = c / k.H;
    full = w >= 0;
    if (full) {
      const float4 q = p[w];
      range[c] = lidar_range(q.x, q.y, q.z);
      ground = (row < k.ground_rows && lidar_cell_pair(p, cellwin, c, c + k.H, k)) ||
               (row >= 1 && row - 1 < k.ground_rows && lidar_cell_pair(p, cellwin, c - k.H, c, k));
    } else {
      range[c] = FLT_MAX;
    }
    state[c] = !full ? LIDAR_EMPTY : (ground ? LIDAR_GROUND : LIDAR_LIVE);
    parent[c] = full && !ground ? c : -1;
  }
  wave_count_add(full, &stats->projected);
  wave_count_add(ground, &stats->ground);
}

__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_union(LidarConst k, const float* __restrict__ range, const unsigned char* __restrict__ state,
                                                               int* parent) {
  const int c = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x, cells = k.R * k.H;
  if (c >= cells || state[c] != LIDAR_LIVE) return;
  const int row = c / k.H, col = c - row * k.H;
  const int right = row * k.H + (col + 1 == k.H ? 0 : col + 1), down = c + k.H;
  if (right != c && state[right] == LIDAR_LIVE && lidar_connected(range[c], range[right], true, k)) uf_unite(parent, c, right);
  if (row + 1 < k.R && state[down] == LIDAR_LIVE && lidar_connected(range[c], range[down], false, k)) uf_unite(parent, c, down);
}

__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_flatten(LidarConst k, const unsigned char* __restrict__ state, int* parent, int* __restrict__ root,
                                                                 unsigned* size, unsigned* mask) {
  const int c = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x, cells = k.R * k.H;
  if (c >= cells) return;
  if (state[c] != LIDAR_LIVE) {
    root[c] = -1;
    return;
  }
  const int r = uf_find(parent, c);  // (the parents no longer change: k_lidar_union is a launch behind)
  root[c] = r;
  atomicAdd(&size[r], 1u);
  if (r != c) {
    const int row = c / k.H;
    atomicOr(&mask[4 * (size_t)r + (row >> 5)], 1u << (row & 31));
  }
}

__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_valid(LidarConst k, const int* __restrict__ root, const unsigned* __restrict__ size,
                                                               const unsigned* __restrict__ mask, unsigned char* __restrict__ valid, LidarStats* stats) {
  const int c = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x, cells = k.R * k.H;
  bool is_root = false, ok = false;
  if (c < cells) {
    const int r = root[c];
    if (r >= 0) {
      ok = lidar_segment_valid(size[r], &mask[4 * (size_t)r], k);
      is_root = r == c;
    }
    valid[c] = ok ? 1 : 0;
  }
  wave_count_add(is_root && ok, &stats->valid);
  wave_count_add(is_root && !ok, &stats->invalid);
}

struct LidarSegKeep {
  using Item = int;
  int H;
  const unsigned char* valid;
  const float* range;
  const int* cellwin;
  int *seg_cell, *seg_col, *seg_pt;
  float* seg_range;
  __device__ bool keep(int c, int cells, Item* it) const {
    *it = c;
    return c < cells && valid[c] != 0;
  }
  __device__ void write(unsigned at, const Item& c) const {
    seg_cell[at] = c;
    seg_col[at] = c % H;
    seg_pt[at] = cellwin[c];
    seg_range[at] = range[c];
  }
};

// before[i] = segmented points in rows < i, i = 0 .. R
__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_bounds(int R, int H, int S, const int* __restrict__ seg_cell, int* __restrict__ before) {
  const int i = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x;
  if (i > R) return;
  int lo = 0, hi = S;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg_cell[mid] < i * H) lo = mid + 1;
    else hi = mid;
  }
  before[i] = lo;
}

__global__ __launch_bounds__(LIDAR_THREADS) void k_lidar_smooth(int S, const float* __restrict__ seg_range, const int* __restrict__ seg_col,
                                                                float* __restrict__ curv, unsigned char* __restrict__ occluded) {
  const int i = blockIdx.x * LIDAR_THREADS + (int)threadIdx.x;
  if (i >= S) return;
  curv[i] = lidar_curvature(seg_range, i, S);
  occluded[i] = lidar_occluded(seg_range, seg_col, i, S) ? 1 : 0;
}

// One block per ring.  edge_pt[(ring * 6 + j) * 20 + t]: the point of pick t of sixth j; n_edge[ring * 6 + j]: how many.
// cand[k] = 1 for every k of a processed sixth that is not an edge (cand is zero on entry).
__global__ __launch_bounds__(LIDAR_PICK_THREADS) void k_lidar_pick(int S, float edge_thr, const int* __restrict__ before, const float* __restrict__ curv,
                                                                   const unsigned char* __restrict__ occluded, const int* __restrict__ seg_col,
                                                                   const int* __restrict__ seg_pt, int* __restrict__ edge_pt, int* __restrict__ n_edge,
                                                                   unsigned char* __restrict__ cand) {
  __shared__ unsigned long long keys[LIDAR_SORT_MAX];
  __shared__ unsigned char picked[LIDAR_FLAGS], edge[LIDAR_FLAGS];
  const int ring = blockIdx.x, b0 = before[ring], b1 = before[ring + 1], tid = threadIdx.x;
  const int base = b0 - LIDAR_FLAG_PAD;  // picked[k - base]
  for (int t = tid; t < LIDAR_FLAGS; t += LIDAR_PICK_THREADS) {
    const int kk = base + t;
    picked[t] = kk >= 0 && kk < S ? occluded[kk] : 0;
    edge[t] = 0;
  }
  __syncthreads();
  for (int j = 0; j < LIDAR_SIXTHS; j++) {
    int sp, ep;
    lidar_sixth(b0, b1, j, &sp, &ep);
    if (sp >= ep || ep - sp > LIDAR_SORT_MAX) {  // (uniform; the second cannot happen below LIDAR_MAX_HORIZON columns)
      if (tid == 0) n_edge[ring * LIDAR_SIXTHS + j] = 0;
      continue;
    }
    const int len = ep - sp;
    int np2 = 64;
    while (np2 < len) np2 *= 2;
    // an entry that cannot be picked (curvature <= threshold, or a position calculateSmoothness never wrote) is key 0
    for (int t = tid; t < np2; t += LIDAR_PICK_THREADS) {
      const int kk = sp + t;
      unsigned long long key = 0;
      if (t < len && kk >= 5 && kk < S - 5) {
        const float v = curv[kk];
        if (v > edge_thr) key = ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)kk;
      }
      keys[t] = key;
    }
    __syncthreads();
    for (int size = 2; size <= np2; size *= 2)
      for (int stride = size / 2; stride > 0; stride /= 2) {
        for (int t = tid; t < np2 / 2; t += LIDAR_PICK_THREADS) {
          const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
          const bool up = (lo & size) == 0;
          const unsigned long long a = keys[lo], b = keys[hi];
          if ((a > b) == up) {
            keys[lo] = b;
            keys[hi] = a;
          }
        }
        __syncthreads();
      }
    if (tid == 0) {
      int cnt = 0;
      // k = ep first (outside the sorted range, its own entry), then the sorted range from the top
      for (int t = np2; t >= 0; t--) {
        int ind;
        if (t == np2) {
          if (ep < 5 || ep >= S - 5 || !(curv[ep] > edge_thr)) continue;
          ind = ep;
        } else {
          if (keys[t] == 0) break;  // ascending: nothing above the threshold is left
          ind = (int)(unsigned)keys[t];
        }
        if (picked[ind - base]) continue;
        if (++cnt > LIDAR_EDGE_CAP) break;
        edge_pt[(ring * LIDAR_SIXTHS + j) * LIDAR_EDGE_CAP + cnt - 1] = seg_pt[ind];
        edge[ind - base] = 1;
        picked[ind - base] = 1;
        for (int l = 1; l <= 5; l++) {
          if (lidar_col_gap(seg_col, ind + l, ind + l - 1) > 10) break;
          picked[ind + l - base] = 1;
        }
        for (int l = -1; l >= -5; l--) {
          if (lidar_col_gap(seg_col, ind + l, ind + l + 1) > 10) break;
          picked[ind + l - base] = 1;
        }
      }
      n_edge[ring * LIDAR_SIXTHS + j] = cnt > LIDAR_EDGE_CAP ? LIDAR_EDGE_CAP : cnt;
    }
    __syncthreads();
    for (int kk = sp + tid; kk <= ep; kk += LIDAR_PICK_THREADS) cand[kk] = edge[kk - base] ? 0 : 1;
  }
}

// the candidates in ascending segmented index: the rank of one is the draw it gets; quarter[rank] = draw % 4
struct LidarCand {
  using Item = int;
  const unsigned char* cand;
  const unsigned char* quarter;
  unsigned char* kept;
  __device__ bool keep(int k, int S, Item* it) const {
    *it = k;
    return k < S && cand[k] != 0;
  }
  __device__ void write(unsigned at, const Item& k) const { kept[k] = quarter[at] == 0 ? 1 : 0; }
};

struct LidarKept {
  using Item = int;
  const unsigned char* kept;
  const int* seg_pt;
  int *out_k, *out_pt;
  __device__ bool keep(int k, int S, Item* it) const {
    *it = k;
    return k < S && kept[k] != 0;
  }
  __device__ void write(unsigned at, const Item& k) const {
    out_k[at] = k;
    out_pt[at] = seg_pt[k];
  }
};

}  // namespace cvo_dev
