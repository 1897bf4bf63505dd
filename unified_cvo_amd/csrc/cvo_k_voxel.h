// cvo_k_voxel.h -- voxel-grid downsampling of a raw frame (cvo::VoxelMap, VoxelMap_impl.hpp:126-170): one point per occupied
// voxel, the one with the lowest original index, in ascending original index.
//
//   k_voxel_insert   one point per lane: voxel key, open-addressing insert into a table in HBM (table_insert, cvo_k_prims.h),
//                    unsigned min of the point's index on the slot.  Optionally (PRE) the 1024 points of a block first meet
//                    in an LDS table and only the block's lowest index of every voxel goes to HBM.
//   VoxelFirst       the predicate of the ordered compaction (cvo_k_compact.h): keep = "my index is my slot's minimum";
//                    k_compact_count<VoxelFirst> counts per block of 1024 points, k_compact_write<VoxelFirst> writes the
//                    kept indices in ascending order.
//   k_voxel_scan     compact_scan_counts of this selection's block counts and, in the same launch, the sum of k_voxel_insert's
//                    block statistics (one block).
//
// Which slot a voxel lands in depends on the order the waves arrive in; no output does: min commutes and the compaction is
// ordered by index.  Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.
#pragma once
#include "cvo_device.h"
#include "cvo_k_compact.h"

namespace cvo_dev {

constexpr int VOX_THREADS = COMPACT_THREADS;      // points per block of every kernel here
constexpr int VOX_INSERT_BLOCKS = 512;            // most blocks k_voxel_insert is launched with (two per CU; it strides)
constexpr int VOX_LDS_SLOTS = 2048;               // block-local table of the pre-pass: 2 slots per point, never full
constexpr int VOX_KMAX = 1 << 20;                 // |k| < 2^20 per axis: three 21-bit fields, a 63-bit key
enum : unsigned { VOX_BAD_FINITE = 1, VOX_BAD_X = 2, VOX_BAD_Y = 4, VOX_BAD_Z = 8 };

// what a selection leaves for the host: one 48-byte copy
struct VoxelCtl {
  unsigned status;   // OR of VOX_BAD_* over all points; non-zero = refused
  unsigned n_kept;
  unsigned longest;  // longest probe sequence (slots visited by one insert; 1 = the home slot)
  unsigned pad;
  unsigned long long occupied, probes, entered;  // slots taken; slots visited by all inserts; points that reached the HBM table
};

// what one block of k_voxel_insert counted, summed by k_voxel_scan (every wave adding to the ONE VoxelCtl with global atomics
// took 200 of the kernel's 237 us at 307 200 points: profiles/voxel/kernel_trace_wave_atomics.txt)
struct VoxelBlockStats {
  unsigned long long probes, occupied, entered;
  unsigned longest, pad;
};

// Voxel of a point: k = rint(x / s) per axis with the correctly rounded quotient and ties to even (VoxelMap_impl.hpp:170;
// numpy: np.rint(xyz / float32(s))).  Returns VOX_BAD_* bits, or 0 and the key.  The same code runs on the host (CPU twin).
__host__ __device__ inline unsigned vox_key(float x, float y, float z, float s, unsigned long long* key) {
  if (!(fabsf(x) < INFINITY) || !(fabsf(y) < INFINITY) || !(fabsf(z) < INFINITY)) return VOX_BAD_FINITE;
  const float kx = rintf(x / s), ky = rintf(y / s), kz = rintf(z / s);
  const unsigned bad = (fabsf(kx) < (float)VOX_KMAX ? 0u : (unsigned)VOX_BAD_X) | (fabsf(ky) < (float)VOX_KMAX ? 0u : (unsigned)VOX_BAD_Y) |
                       (fabsf(kz) < (float)VOX_KMAX ? 0u : (unsigned)VOX_BAD_Z);
  if (bad) return bad;
  *key = (unsigned long long)((int)kx + VOX_KMAX) | ((unsigned long long)((int)ky + VOX_KMAX) << 21) |
         ((unsigned long long)((int)kz + VOX_KMAX) << 42);
  return 0;
}

// SLOT_NONE: slot[] of a point that did not enter the table, first[] of an empty slot.  Both are read back by the NEXT kernel only.
template <bool PRE>
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_insert(int n, const float* __restrict__ xyz, float s, unsigned mask,
                                                              unsigned long long* keys, unsigned* first, unsigned* __restrict__ slot,
                                                              VoxelCtl* ctl, VoxelBlockStats* __restrict__ block_stats) {
  __shared__ unsigned long long lkeys[PRE ? VOX_LDS_SLOTS : 1];
  __shared__ unsigned lfirst[PRE ? VOX_LDS_SLOTS : 1];
  unsigned probes = 0, longest = 0, fresh = 0, entered = 0, bad = 0, len;
  for (int base = blockIdx.x * VOX_THREADS; base < n; base += gridDim.x * VOX_THREADS) {  // (uniform per block: the barriers below)
    const int i = base + (int)threadIdx.x;
    unsigned long long key = 0;
    bool live = i < n;
    if (live) {
      const unsigned b = vox_key(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], s, &key);
      bad |= b;
      live = b == 0;
    }
    const unsigned long long h = key_mix(key);
    if (PRE) {
      for (int t = threadIdx.x; t < VOX_LDS_SLOTS; t += VOX_THREADS) {
        lkeys[t] = TABLE_EMPTY;
        lfirst[t] = SLOT_NONE;
      }
      __syncthreads();
      unsigned ls = (unsigned)(h >> 40) & (VOX_LDS_SLOTS - 1);
      if (live) {
        ls = table_insert(lkeys, VOX_LDS_SLOTS - 1, ls, key);
        atomicMin(&lfirst[ls], (unsigned)i);
      }
      __syncthreads();
      live = live && lfirst[ls] == (unsigned)i;  // the block's lowest index of this voxel goes on
      __syncthreads();                           // (the next trip clears the table)
    }
    if (live) {
      const unsigned g = table_insert(keys, mask, (unsigned)h, key, &fresh, &len);  // (capacity >= 2 n)
      atomicMin(&first[g], (unsigned)i);
      slot[i] = g;
      probes += len;
      longest = max(longest, len);
      entered++;
    } else if (i < n) {
      slot[i] = SLOT_NONE;
    }
  }
  if (bad) atomicOr(&ctl->status, bad);
  __shared__ unsigned wstat[VOX_THREADS / 64][4];
  probes = wave_sum_u32(probes);
  fresh = wave_sum_u32(fresh);
  entered = wave_sum_u32(entered);
  longest = wave_max_u32(longest);
  if ((threadIdx.x & 63) == 0) {
    unsigned* w = wstat[threadIdx.x >> 6];
    w[0] = probes;
    w[1] = fresh;
    w[2] = entered;
    w[3] = longest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    VoxelBlockStats b{};
    for (int w = 0; w < VOX_THREADS / 64; w++) {
      b.probes += wstat[w][0];
      b.occupied += wstat[w][1];
      b.entered += wstat[w][2];
      b.longest = max(b.longest, wstat[w][3]);
    }
    block_stats[blockIdx.x] = b;
  }
}

__device__ __forceinline__ bool vox_keep(int i, int n, unsigned mask, const unsigned* __restrict__ first, const unsigned* __restrict__ slot) {
  if (i >= n) return false;
  const unsigned g = slot[i];
  return g <= mask && first[g] == (unsigned)i;
}

struct VoxelFirst {
  typedef int Item;  // the point's index
  unsigned mask;
  const unsigned *first, *slot;
  int* kept;
  __device__ bool keep(int i, int n, Item* item) const {
    *item = i;
    return vox_keep(i, n, mask, first, slot);
  }
  __device__ void write(unsigned at, const Item& i) const { kept[at] = i; }
};

// the total -> ctl->n_kept; also sums the n_stats <= VOX_INSERT_BLOCKS block statistics of k_voxel_insert into ctl.  One block.
__global__ __launch_bounds__(VOX_THREADS) void k_voxel_scan(int nb, unsigned* block_count, VoxelCtl* ctl, int n_stats,
                                                            const VoxelBlockStats* __restrict__ block_stats) {
  __shared__ unsigned long long tot[3];
  __shared__ unsigned longest;
  if (threadIdx.x < 3) tot[threadIdx.x] = 0;
  if (threadIdx.x == 3) longest = 0;
  __syncthreads();
  if ((int)threadIdx.x < n_stats) {
    const VoxelBlockStats b = block_stats[threadIdx.x];
    atomicAdd(&tot[0], b.probes);
    atomicAdd(&tot[1], b.occupied);
    atomicAdd(&tot[2], b.entered);
    atomicMax(&longest, b.longest);
  }
  const unsigned total = compact_scan_counts(nb, block_count);
  if (threadIdx.x == VOX_THREADS - 1) {  // (the barriers of the scan lie between the LDS atomics above and these reads)
    ctl->n_kept = total;
    ctl->probes = tot[0];
    ctl->occupied = tot[1];
    ctl->entered = tot[2];
    ctl->longest = longest;
  }
}

}  // namespace cvo_dev
