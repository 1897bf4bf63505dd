// cvo_k_compact.h -- ordered compaction, the primitive every front end selects with: the elements a predicate keeps, in
// ascending index, with no atomic deciding a position.
//
//   k_compact_count<P>   keep = P::keep(i); one count per block of 1024 elements (ballot + popcount per wave).
//   k_voxel_scan         (cvo_k_voxel.h) exclusive scan of the block counts, the total to VoxelCtl::n_kept.
//   k_compact_write<P>   recomputes keep; rank = block offset + waves before + lanes before; P::write(rank, item).
//
// A predicate P is a small struct passed by value that holds its inputs and its output pointers:
//   typename P::Item                         what keep() hands to write() of the same lane
//   bool P::keep(int i, int n, Item*) const  false for i >= n
//   void P::write(unsigned at, const Item&) const
// The predicates: VoxelFirst (cvo_k_voxel.h), RgbdCellHit, RgbdKeep (cvo_k_rgbd.h), FastAbove (cvo_k_fast.h), StereoKeep
// (cvo_k_stereo.h), LidarTransition (count only), LidarSegKeep, LidarCand, LidarKept (cvo_k_lidar.h).  A kernel that already knows its flag counts with compact_block_count itself (k_rgbd_select).
// Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_device.h"

namespace cvo_dev {

constexpr int COMPACT_THREADS = 1024;  // elements per block; k_voxel_scan holds one count per block

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

// position of a kept element in the ordered output, or ~0u; every thread of the block calls it
__device__ __forceinline__ unsigned compact_block_place(bool keep, const unsigned* __restrict__ block_offset) {
  __shared__ unsigned wcnt[COMPACT_THREADS / 64];
  const unsigned long long m = __ballot(keep);
  const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wcnt[wv] = (unsigned)__popcll(m);
  __syncthreads();
  if (!keep) return ~0u;
  unsigned at = block_offset[blockIdx.x] + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  for (unsigned v = 0; v < wv; v++) at += wcnt[v];
  return at;
}

template <class P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_count(int n, P pred, unsigned* __restrict__ block_count) {
  typename P::Item item{};
  compact_block_count(pred.keep(blockIdx.x * COMPACT_THREADS + (int)threadIdx.x, n, &item), block_count);
}

template <class P>
__global__ __launch_bounds__(COMPACT_THREADS) void k_compact_write(int n, P pred, const unsigned* __restrict__ block_offset) {
  typename P::Item item{};
  const bool keep = pred.keep(blockIdx.x * COMPACT_THREADS + (int)threadIdx.x, n, &item);
  const unsigned at = compact_block_place(keep, block_offset);
  if (at < (unsigned)n) pred.write(at, item);  // (at most n elements are kept: never out of bounds; ~0u of the others fails the test)
}

}  // namespace cvo_dev
