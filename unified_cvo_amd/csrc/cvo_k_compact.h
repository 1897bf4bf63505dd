// cvo_k_compact.h -- ordered compaction, the primitive every front end selects with: the elements a predicate keeps, in
// ascending index, with no atomic deciding a position.
//
//   k_compact_count<P>   keep = P::keep(i); one count per block of 1024 elements (ballot + popcount per wave).
//   k_compact_scan       one block: exclusive scan of the block counts (compact_scan_counts), the total to *total; the voxel grid
//                        has a scan kernel of its own.
//   k_compact_write<P>   recomputes keep; rank = block offset + waves before + lanes before; P::write(rank, item).
//
// A predicate P is a small struct passed by value that holds its inputs and its output pointers:
//   typename P::Item                         what keep() hands to write() of the same lane
//   bool P::keep(int i, int n, Item*) const  false for i >= n
//   void P::write(unsigned at, const Item&) const
// The predicates: VoxelFirst (cvo_k_voxel.h), RgbdCellHit, RgbdKeep (cvo_k_rgbd.h), RgbdKeepScores, RgbdHasDepth (count only;
// cvo_k_rgbd_rows.h), FastAbove (cvo_k_fast.h), StereoKeep
// (cvo_k_stereo.h), LidarTransition (count only; k_lidar_project ranks it inclusively), LidarSegKeep, LidarCand, LidarKept
// (cvo_k_lidar.h).  A kernel that already knows its flag counts with compact_block_count itself (k_rgbd_select).
// Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_k_prims.h"

namespace cvo_dev {

constexpr int COMPACT_THREADS = 1024;          // elements per block
constexpr int COMPACT_MAX_ELEMENTS = 1 << 24;  // (the scan holds COMPACT_MAX_ELEMENTS / COMPACT_THREADS block counts in one block)

// per-block count of `keep` -> block_count[blockIdx.x]; every thread of the block calls it
__device__ __forceinline__ void compact_block_count(bool keep, unsigned* __restrict__ block_count) {
  __shared__ unsigned wcnt[COMPACT_THREADS / 64];
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (unsigned)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = 0;
    for (int v = 0; v < COMPACT_THREADS / 64; v++) c += wcnt[v];
    block_count[blockIdx.x] = c;
  }
}

// block offset + flagged elements of the block before this one (INCL: and this one); every thread of the block calls it.  The
// exclusive form is the position of a kept element in the ordered output, ~0u for the others.  ONCE per kernel and form: no
// barrier follows the last read of wcnt, so a second call of the same instantiation would race with the first.
template <bool INCL>
__device__ __forceinline__ unsigned compact_block_rank(bool keep, const unsigned* __restrict__ block_offset) {
  __shared__ unsigned wcnt[COMPACT_THREADS / 64];
  const unsigned long long m = __ballot(keep);
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wcnt[wv] = (unsigned)__popcll(m);
  __syncthreads();
  if (!INCL && !keep) return ~0u;
  unsigned at = block_offset[blockIdx.x] + (unsigned)__popcll(m & (((INCL ? 2ull : 1ull) << lane) - 1ull));
  for (unsigned v = 0; v < wv; v++) at += wcnt[v];
  return at;
}

// block_count[0 .. nb) -> its exclusive prefix sums, in place; returns the total.  Every thread of ONE block of COMPACT_THREADS
// calls it, thread t takes ceil(nb / 1024) consecutive counts; nb <= COMPACT_MAX_ELEMENTS / COMPACT_THREADS.
__device__ __forceinline__ unsigned compact_scan_counts(int nb, unsigned* block_count) {
  __shared__ unsigned part[COMPACT_THREADS];
  const int per = (nb + COMPACT_THREADS - 1) / COMPACT_THREADS, lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
  unsigned sum = 0;
  for (int b = lo; b < hi; b++) sum += block_count[b];
  unsigned run = block_scan_incl<COMPACT_THREADS>(part, sum) - sum;
  for (int b = lo; b < hi; b++) {
    const unsigned c = block_count[b];
    block_count[b] = run;
    run += c;
  }
  return part[COMPACT_THREADS - 1];
}

template <class P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_count(int n, P pred, unsigned* __restrict__ block_count) {
  typename P::Item item{};
  compact_block_count(pred.keep(blockIdx.x * COMPACT_THREADS + (int)threadIdx.x, n, &item), block_count);
}

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_scan(int nb, unsigned* block_count, unsigned* total) {
  const unsigned t = compact_scan_counts(nb, block_count);
  if (threadIdx.x == COMPACT_THREADS - 1) *total = t;
}

template <class P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_write(int n, P pred, const unsigned* __restrict__ block_offset) {
  typename P::Item item{};
  const bool keep = pred.keep(blockIdx.x * COMPACT_THREADS + (int)threadIdx.x, n, &item);
  const unsigned at = compact_block_rank<false>(keep, block_offset);
  if (at < (unsigned)n) pred.write(at, item);  // (at most n elements are kept: never out of bounds; ~0u of the others fails the test)
}

}  // namespace cvo_dev
