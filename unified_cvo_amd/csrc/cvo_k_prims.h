// cvo_k_prims.h -- the device primitives the front ends' kernels share, each with its contract (tests/test_gpu_prims.py runs them
// one by one); the ordered compaction is cvo_k_compact.h, the radix sort cvo_k_sort.h.  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_wave.h"

namespace cvo_dev {

// *to += lanes of the wave with f, one atomic per wave (none for a wave without one).  Every lane of the wave calls it.
__device__ __forceinline__ void wave_count_add(bool f, unsigned* to) {
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(to, (unsigned)__popcll(m));
}
// `want` consecutive places of a bump counter for every lane, in lane order, one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ unsigned wave_alloc(unsigned want, unsigned* counter) {
  const int lane = threadIdx.x & 63, incl = wave_prefix_incl_i32((int)want, lane);
  int base = 0;
  if (lane == 63 && incl) base = (int)atomicAdd(counter, (unsigned)incl);
  base = __builtin_amdgcn_readlane(base, 63);
  return (unsigned)base + (unsigned)incl - want;
}

// part[0 .. THREADS) <- the inclusive prefix sums of the block's v (Hillis-Steele), a barrier behind the last write; returns
// part[thread].  Every thread of a block of THREADS calls it.
template <int THREADS>
__device__ __forceinline__ unsigned block_scan_incl(unsigned* part, unsigned v) {
  part[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < THREADS; d *= 2) {
    const unsigned add = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  return part[threadIdx.x];
}

// Union-find over cells with parent[x] <= x always: a root is the lowest cell of its tree, the final root the lowest cell of
// its component.  Blocks of one launch meet only in what the atomics return; a find after the launch reads settled parents.
__device__ __forceinline__ int uf_find(int* parent, int x) {
  for (;;) {
    const int q = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    x = q;
  }
}
__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    const int hi = max(a, b);
    b = min(a, b);
    const int old = atomicMin(&parent[hi], b);
    if (old == hi) return;
    a = old;
  }
}

// Open-addressing table of 64-bit keys, linear probing, a power of two of slots.  TABLE_EMPTY: a free slot (no key has bit 63).
constexpr unsigned long long TABLE_EMPTY = ~0ull;
constexpr unsigned SLOT_NONE = ~0u;
// home slot: the finaliser of splitmix64 (neighbouring keys differ in a few low bits of one field)
__host__ __device__ inline unsigned long long key_mix(unsigned long long k) {
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}
// Claims or finds `key` from home slot h & mask; returns the slot, *fresh += 1 if this call took it, *visited = slots seen (1:
// the home slot); either pointer may be null.  The decisions are taken on what the compare-and-swap RETURNS, never on a plain
// load of keys[]: another XCD's L2 may hold a stale line of it while the kernel runs.  The table is at most half full: an empty
// slot is always met.  (The counters are locals inside the loop: through the pointers the compiler counts under an exec mask.)
__device__ __forceinline__ unsigned table_insert(unsigned long long* keys, unsigned mask, unsigned h, unsigned long long key,
                                                 unsigned* fresh = nullptr, unsigned* visited = nullptr) {
  unsigned g = h & mask, len = 1, f = fresh ? *fresh : 0u;
  for (;;) {
    const unsigned long long old = atomicCAS(&keys[g], TABLE_EMPTY, key);
    if (old == TABLE_EMPTY) f++;
    if (old == TABLE_EMPTY || old == key) break;
    g = (g + 1) & mask;
    len++;
  }
  if (fresh) *fresh = f;
  if (visited) *visited = len;
  return g;
}
// The slot of `key`, or SLOT_NONE: table_insert's home slot and probing, read-only.  For a table no kernel is writing (the
// launch runs behind every insert on the same stream), so plain loads see every key.  The first empty slot ends the probe -
// the table is at most half full -, and the slot count ends it whatever the table holds.
__device__ __forceinline__ unsigned table_find(const unsigned long long* keys, unsigned mask, unsigned h, unsigned long long key) {
  unsigned g = h & mask;
  for (unsigned seen = 0; seen <= mask; seen++) {
    const unsigned long long at = keys[g];
    if (at == key) return g;
    if (at == TABLE_EMPTY) return SLOT_NONE;
    g = (g + 1) & mask;
  }
  return SLOT_NONE;
}

}  // namespace cvo_dev
