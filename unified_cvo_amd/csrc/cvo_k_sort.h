// cvo_k_sort.h -- a stable LSD radix sort of (u64 key, u32 value) pairs, 256 per block: eight passes over an 8-bit digit, each
// k_sort_hist / k_sort_scan / k_sort_scatter between two buffers (sort_pairs_u64, cvo_frontend.hip).  Part of the kernel set
// of cvo_kernels.h; compiled only as part of cvo_hip.hip.
#pragma once
#include "cvo_k_prims.h"

namespace cvo_dev {

constexpr int SORT_THREADS = 256;  // pairs per block

// rank of this thread's element among the block's earlier live elements with the same 8-bit digit; leaves the digit counts of
// the block's four waves in wcount
__device__ __forceinline__ unsigned sort_rank(unsigned digit, bool live, unsigned (*wcount)[256]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < (SORT_THREADS / 64) * 256; t += SORT_THREADS) (&wcount[0][0])[t] = 0;
  __syncthreads();
  unsigned long long same = __ballot(live);
  for (int b = 0; b < 8; b++) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bal = __ballot(bit);
    same &= bit ? bal : ~bal;
  }
  const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
  if (live && below == 0) wcount[w][digit] = (unsigned)__popcll(same);
  __syncthreads();
  unsigned r = below;
  for (int q = 0; q < w; q++) r += wcount[q][digit];
  return r;
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(unsigned n, const unsigned long long* key, int shift, unsigned* hist) {
  __shared__ unsigned wcount[SORT_THREADS / 64][256];
  const unsigned e = blockIdx.x * SORT_THREADS + threadIdx.x;
  const bool live = e < n;
  const unsigned digit = live ? (unsigned)(key[e] >> shift) & 255u : 0u;
  (void)sort_rank(digit, live, wcount);
  unsigned c = 0;
  for (int q = 0; q < SORT_THREADS / 64; q++) c += wcount[q][threadIdx.x];
  hist[(size_t)blockIdx.x * 256 + threadIdx.x] = c;
}

// hist[block][digit] -> where the block's elements of that digit start: digits ascending, blocks ascending inside a digit
__global__ __launch_bounds__(256) void k_sort_scan(unsigned nb, unsigned* hist) {
  __shared__ unsigned part[256];
  unsigned total = 0;
  for (unsigned b = 0; b < nb; b++) total += hist[(size_t)b * 256 + threadIdx.x];
  unsigned run = block_scan_incl<256>(part, total) - total;
  for (unsigned b = 0; b < nb; b++) {
    const unsigned c = hist[(size_t)b * 256 + threadIdx.x];
    hist[(size_t)b * 256 + threadIdx.x] = run;
    run += c;
  }
}

__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(unsigned n, const unsigned long long* key, const unsigned* val, int shift,
                                                                const unsigned* hist, unsigned long long* key_out, unsigned* val_out) {
  __shared__ unsigned wcount[SORT_THREADS / 64][256];
  const unsigned e = blockIdx.x * SORT_THREADS + threadIdx.x;
  const bool live = e < n;
  const unsigned long long k = live ? key[e] : 0ull;
  const unsigned digit = (unsigned)(k >> shift) & 255u;
  const unsigned rank = sort_rank(digit, live, wcount);
  if (!live) return;
  const unsigned at = hist[(size_t)blockIdx.x * 256 + digit] + rank;
  key_out[at] = k;
  val_out[at] = val[e];
}

}  // namespace cvo_dev
