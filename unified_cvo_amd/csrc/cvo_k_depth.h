// cvo_k_depth.h -- the keyframe depth filter (main_depth_filtering.cpp:245-294) on the device: k_depth_accumulate (one
// frame's association, where its evaluation left it, folded into the keyframe rows' accumulators), k_depth_finish (the
// weighted mean depth of every row, its point moved along its ray, a keep flag) and DepthKept, the predicate the ordered
// compaction of cvo_k_compact.h turns the flags into an ascending index list with.  The arithmetic is cvo_depth_math.h's.
// Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.  Host side: cvo_depth.hip.
#pragma once
#include "cvo_depth_math.h"
#include "cvo_k_compact.h"

namespace cvo_dev {

constexpr int DEPTH_THREADS = 256;

// ------------------------------------------------------------------------------------------
// k_depth_accumulate: the kernel matrix the last evaluation left in pair 0's workspace - what k_irls_gather reads: nnz_row,
// NNZ_DENSE_FLAG / dense_off, ell through ell_index, ell_j, iorig - folded into depth_sum / weight_sum / count of the
// keyframe rows (ORIGINAL index).  One thread per row POSITION walks the row's slots in order, i.e. in ascending original
// target index, so a row's sums are sequential: the order is the statement's without an atomic, and no two threads touch one
// row.  Per entry: the value a, the column j, the target's UNtransformed coordinates y4[j] (original index, as
// IrlsEdge::x2), zj = depth_zj(T_depth row 2, y4[j]), depth_fold.
//
// What each access is.  nnz_row / iorig / dense_off: one dword per lane, consecutive lanes consecutive addresses.  ell_j is
// slot-major [slot][position] for every row class: a slot's columns of a wave are one 256-byte run.  The values of the
// thread-per-row rows are slot-major too (8- or 16-byte entries: a wave reads 512 B or 1 KiB per slot, a quarter or a half
// of it used).  The values of rows the wave-per-row kernels evaluated sit in row-major runs (dense_off >= 0): a lane walks
// its own run, consecutive lanes are a run length apart - one entry per cache line and lane; a wave per such row would read
// them coalesced and is NOT built (the sums of a row would then need an ordered reduction to stay bit for bit).  The target
// gather y4[j] is 16 bytes at a data-dependent address per entry; rows that are neighbours in the spatial order share
// targets, so most of it is served by L2.
// CLAIM (no counter pass has tested it): the kernel is bound by the latency of the dependent chain ell_j -> y4[j] per slot
// - each lane has one gather in flight per trip - not by bandwidth.  Per entry it moves 4 B of ell_j, an 8- or 16-byte value
// and 16 B of y4: 28 - 36 B, i.e. 17 - 21 MB if all 9 284 rows of the probe's keyframe held 64 entries, and 0.7 - 0.9 MB at the
// 2.6 - 4.8 entries per row and frame the probe's clouds really have (1.3 MB at most).  Measured (one kernel-trace pass,
// profiles/depth_filter/depth_kernel_stats.csv): 12.3 us per launch on average (8.7 - 16.6) over the probe's 72 adds, 0.2 % of
// the device time of the calls, next to 5.2 ms per launch of k_assoc_dense - some 100 GB/s, far from the memory system's
// limit, which agrees with the claim and does not prove it.
//
// Bounds: a slot beyond the matrix (ell_cap entries), a column outside [0, M) or a row outside [0, n_rows) is never
// dereferenced: the thread sets *bad and leaves its row as it was.  The host reads the word after every launch and refuses
// the add as the host's own export refuses such a matrix: corrupt.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_accumulate(const PairDesc* __restrict__ D, int K, size_t ell_cap,
                                                                    const float4* __restrict__ y4, int M, DepthRow t, int n_rows,
                                                                    float* __restrict__ depth_sum, float* __restrict__ weight_sum,
                                                                    int* __restrict__ count, unsigned* __restrict__ bad) {
  const int pos = (int)blockIdx.x * DEPTH_THREADS + (int)threadIdx.x;
  const int N = D->N;
  if (pos >= N) return;
  const unsigned v = D->nnz_row[pos];
  const int n = min((int)nnz_count(v), K);
  if (n <= 0) return;
  const int i = D->iorig[pos];
  if ((unsigned)i >= (unsigned)n_rows) {
    *bad = 1u;
    return;
  }
  const int off = (v & NNZ_DENSE_FLAG) ? D->dense_off[pos] : -1;
  const EllEntry* __restrict__ ell = D->ell;
  const int* __restrict__ ell_j = D->ell_j;
  float ds = depth_sum[i], ws = weight_sum[i];
  int c = count[i];
  for (int s = 0; s < n; s++) {
    const size_t e = ell_index(N, s, pos, off);
    const int j = ell_j[(size_t)s * N + pos];
    if (e >= ell_cap || (unsigned)j >= (unsigned)M) {
      *bad = 1u;
      return;
    }
    const float a = ell[e].a;
    const float4 y = y4[j];
    depth_fold(ds, ws, c, depth_zj(t, y.x, y.y, y.z), a);
  }
  depth_sum[i] = ds;
  weight_sum[i] = ws;
  count[i] = c;
}

// ------------------------------------------------------------------------------------------
// k_depth_finish: depth_finish_row of every keyframe row.  One thread per row; xyz is the packed copy k_cloud_unpack made
// (12 bytes per row: three dword loads per lane, consecutive lanes 12 bytes apart - every line read is used whole).  Writes
// the moved point into xyz_out (a row that is not kept keeps its coordinates: the array is whole, the ingest reads only
// kept rows), the refined depth (0 for a row that is not kept) and the flag; rows whose result is not finite are counted
// (one integer atomic per wave that has some: the count does not depend on the order).  The accumulators are only read.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DEPTH_THREADS) void k_depth_finish(int n, int min_count, const float* __restrict__ xyz,
                                                                const float* __restrict__ depth_sum, const float* __restrict__ weight_sum,
                                                                const int* __restrict__ count, float* __restrict__ xyz_out,
                                                                float* __restrict__ depth, unsigned char* __restrict__ flag,
                                                                unsigned* __restrict__ n_nonfinite) {
  const int i = (int)blockIdx.x * DEPTH_THREADS + (int)threadIdx.x;
  int what = DEPTH_DROP;
  if (i < n) {
    const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    float out[3] = {p[0], p[1], p[2]}, d = 0.f;
    what = depth_finish_row(depth_sum[i], weight_sum[i], count[i], min_count, p, out, &d);
    const bool keep = what == DEPTH_KEEP;
    for (int k = 0; k < 3; k++) xyz_out[3 * (size_t)i + k] = keep ? out[k] : p[k];
    depth[i] = keep ? d : 0.f;
    flag[i] = (unsigned char)what;
  }
  const unsigned long long m = __ballot(what == DEPTH_NONFINITE);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(n_nonfinite, (unsigned)__popcll(m));
}

// the kept rows in ascending original index, and their refined depths next to them
struct DepthKept {
  using Item = int;
  const unsigned char* flag;
  const float* depth;
  int* kept;
  float* depth_kept;
  __device__ bool keep(int i, int n, Item* it) const {
    if (i >= n) return false;
    *it = i;
    return flag[i] == DEPTH_KEEP;
  }
  __device__ void write(unsigned at, const Item& it) const {
    kept[at] = it;
    depth_kept[at] = depth[it];
  }
};

}  // namespace cvo_dev
