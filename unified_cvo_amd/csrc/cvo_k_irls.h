// cvo_k_irls.h -- the multi-frame least-squares kernels (CvoBatchIRLS::solve, IRLS.cpp:77-215, without Ceres):
// k_irls_gather (one edge's kernel matrix, where its evaluation left it, into the edge's resident entry list),
// k_irls_eval<true> = k_irls_normal (cost, gradient and Gauss-Newton matrix per edge), k_irls_eval<false> = k_irls_cost
// (cost only, at a candidate pose), k_irls_finish (the ordered per-edge pass over the block partials).
// Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.
#pragma once
#include "cvo_irls_solve.h"
#include "cvo_wave.h"

namespace cvo_dev {

constexpr int IRLS_THREADS = 256;
constexpr int IRLS_PER_THREAD = 16;
constexpr int IRLS_BLOCK_ENTRIES = IRLS_THREADS * IRLS_PER_THREAD;  // entry slots one block walks
using cvo_irls::IRLS_W;  // per edge: cost, g[12], the upper triangle of the 12 x 12 H row by row [78]: the host solver's record

// One stored entry (r, c, w = A.mat) of an edge's kernel matrix: row r of frame 1, column c of frame 2 (ORIGINAL
// indices).  c < 0: an empty slot (the row had fewer than K entries).
struct IrlsEntry {
  int r, c;
  float w, pad;
};
static_assert(sizeof(IrlsEntry) == 16, "IrlsEntry");

// One active edge of a launch.  Blocks [blk0, blk0 + ceil(n / IRLS_BLOCK_ENTRIES)) walk its entry slots.
struct IrlsEdge {
  const float4* x1;  // frame 1, UNtransformed xyz, original index
  const float4* x2;  // frame 2
  const IrlsEntry* ent;
  int n, n1, n2;  // entry slots, points of frame 1 / 2
  int f1, f2;     // frames (12 doubles each in the pose array)
  int blk0;
};

// ------------------------------------------------------------------------------------------
// k_irls_gather: the kernel matrix the last evaluation left in pair 0's workspace (ELL by position: nnz_row, the
// row-major runs of the wave-per-row rows, ell_j, iorig - what fetch_ell / last_xorder read on the host) as the edge's
// entry list, row-major [position][K].  One thread per (position, slot): consecutive lanes write consecutive 16-byte
// entries.  The matrix never leaves the device.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_irls_gather(const PairDesc* __restrict__ D, int K, IrlsEntry* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int N = D->N;
  if (t >= (size_t)N * K) return;
  const int pos = (int)(t / K), s = (int)(t % K);
  const unsigned v = D->nnz_row[pos];
  const int n = min((int)nnz_count(v), K);
  IrlsEntry e{-1, -1, 0.f, 0.f};
  if (s < n) {
    const int off = (v & NNZ_DENSE_FLAG) ? D->dense_off[pos] : -1;
    e.r = D->iorig[pos];
    e.c = D->ell_j[(size_t)s * N + pos];
    e.w = D->ell[ell_index(N, s, pos, off)].a;
  }
  out[t] = e;
}

// ------------------------------------------------------------------------------------------
// k_irls_eval: PairwiseAnalyticalDiffFunctor::Evaluate (IRLS_Cost_CPU.hpp:117-166) on every stored entry of every
// active edge, in fp64, at the poses `poses` (12 doubles per frame, 3x4 row-major):
//   e = T1 p1 - T2 p2,  res = w |e|^2,  cost = 1/2 sum res^2
//   J1 = e^T DT1 * ComputeJacobian(T1) = [a, p1 x a],  a = R1^T e      (local_parameterization_se3.hpp:49-88, delta = (u, w))
//   J2 = -e^T DT2 * ComputeJacobian(T2) = -[b, p2 x b],  b = R2^T e
// (upstream's Jacobian, without the factor 2 w of d res: DESIGN.md section 4).  NORMAL: the block's partial of
// (cost, J^T res, upper(J^T J)); otherwise the cost only.  Deterministic: each thread sums its slots in a fixed order,
// a butterfly per wave, the waves in order - one partial per block in a fixed slot; k_irls_finish sums them in order.
// ------------------------------------------------------------------------------------------
template <bool NORMAL>
__global__ __launch_bounds__(IRLS_THREADS) void k_irls_eval(const IrlsEdge* __restrict__ edges, int n_edges,
                                                            const double* __restrict__ poses, double* __restrict__ part) {
  constexpr int W = NORMAL ? IRLS_W : 1;
  __shared__ double red[IRLS_THREADS / 64][W];
  const int b = blockIdx.x;
  int lo = 0, hi = n_edges - 1;  // the last edge whose first block is <= b (edges without slots have no blocks)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (edges[mid].blk0 <= b) lo = mid;
    else hi = mid - 1;
  }
  const IrlsEdge E = edges[lo];
  const double* P1 = poses + 12 * E.f1;
  const double* P2 = poses + 12 * E.f2;
  double T1[12], T2[12];
  for (int q = 0; q < 12; q++) {
    T1[q] = P1[q];
    T2[q] = P2[q];
  }
  double acc[W];  // stays in registers: every loop that indexes it is unrolled
#pragma unroll
  for (int q = 0; q < W; q++) acc[q] = 0.0;
  const size_t base = (size_t)(b - E.blk0) * IRLS_BLOCK_ENTRIES + threadIdx.x;
  for (int k = 0; k < IRLS_PER_THREAD; k++) {
    const size_t i = base + (size_t)k * IRLS_THREADS;
    if (i >= (size_t)E.n) break;
    const IrlsEntry en = E.ent[i];
    if (en.c < 0 || (unsigned)en.r >= (unsigned)E.n1 || (unsigned)en.c >= (unsigned)E.n2) continue;
    const float4 fa = E.x1[en.r], fb = E.x2[en.c];
    const double p1[3] = {(double)fa.x, (double)fa.y, (double)fa.z};
    const double p2[3] = {(double)fb.x, (double)fb.y, (double)fb.z};
    double e[3];
    for (int r = 0; r < 3; r++) {
      const double q1 = T1[4 * r] * p1[0] + T1[4 * r + 1] * p1[1] + T1[4 * r + 2] * p1[2] + T1[4 * r + 3];
      const double q2 = T2[4 * r] * p2[0] + T2[4 * r + 1] * p2[1] + T2[4 * r + 2] * p2[2] + T2[4 * r + 3];
      e[r] = q1 - q2;
    }
    const double res = (double)en.w * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    acc[0] += 0.5 * (res * res);
    if constexpr (NORMAL) {
      double J[12];
      for (int c = 0; c < 3; c++) {
        J[c] = T1[c] * e[0] + T1[4 + c] * e[1] + T1[8 + c] * e[2];
        J[6 + c] = -(T2[c] * e[0] + T2[4 + c] * e[1] + T2[8 + c] * e[2]);
      }
      // p x a, and -(p2 x b) = p2 x (-b)
      J[3] = p1[1] * J[2] - p1[2] * J[1];
      J[4] = p1[2] * J[0] - p1[0] * J[2];
      J[5] = p1[0] * J[1] - p1[1] * J[0];
      J[9] = p2[1] * J[8] - p2[2] * J[7];
      J[10] = p2[2] * J[6] - p2[0] * J[8];
      J[11] = p2[0] * J[7] - p2[1] * J[6];
#pragma unroll
      for (int q = 0; q < 12; q++) acc[1 + q] += J[q] * res;
#pragma unroll
      for (int q = 0; q < 12; q++)
#pragma unroll
        for (int s = q; s < 12; s++) acc[13 + q * 12 - q * (q - 1) / 2 + (s - q)] += J[q] * J[s];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < W; q++) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // every lane ends with the same sum
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < W; q += IRLS_THREADS) {
    double v = red[0][q];
    for (int w = 1; w < IRLS_THREADS / 64; w++) v += red[w][q];
    part[(size_t)b * W + q] = v;
  }
}

// The ordered pass: out[e][q] = sum of edge e's block partials in block order.  One block per edge.
__global__ __launch_bounds__(128) void k_irls_finish(const IrlsEdge* __restrict__ edges, int n_edges, int n_blocks, int W,
                                                     const double* __restrict__ part, double* __restrict__ out) {
  const int e = blockIdx.x;
  const int b0 = edges[e].blk0, b1 = e + 1 < n_edges ? edges[e + 1].blk0 : n_blocks;
  for (int q = threadIdx.x; q < W; q += 128) {
    double v = 0.0;
    for (int b = b0; b < b1; b++) v += part[(size_t)b * W + q];
    out[(size_t)e * W + q] = v;
  }
}

}  // namespace cvo_dev
