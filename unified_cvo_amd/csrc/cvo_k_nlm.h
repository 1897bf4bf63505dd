// cvo_k_nlm.h -- non-local-means denoising of an 8-bit image (cvo_nlm.hip; the statement: tests/np_nlm.py).
//
// k_nlm<C, TH>: one block makes a tile of NLM_TILE_W(TH) x NLM_TILE_H output pixels of a C-channel image from an LDS copy
// of the tile and its halo of b = TH + sh pixels, reflected at the image border (BORDER_REFLECT_101) while staging, so that
// every source byte leaves memory once per tile that needs it and no patch comparison goes to global memory.
//
// A wave owns NLM_STRIP rows of the tile and one column per lane: lane l holds column l - TH of the tile, so the 64 lanes
// span the tile's NLM_TILE_W = 64 - 2 TH columns and the template's halo.  Per search offset (dy, dx) the (2 TH + 1)^2 patch
// sum is separable running sums, not 49 terms per pixel:
//   1. the lane squares the differences of its column for the NLM_STRIP + 2 TH rows the strip's patches touch (the
//      reference column a() is offset independent and stays in registers: one LDS byte per term);
//   2. a vertical window slides down those: V[r + 1] = V[r] + d2[r + 2 TH + 1] - d2[r];
//   3. the horizontal window is lane shifts of V (__shfl_down, by doubling: 4 for a window of 7): lane l ends with the patch
//      sum of tile column l.
// That is (NLM_STRIP + 2 TH) / NLM_STRIP squared differences per pixel, offset and channel instead of (2 TH + 1)^2: 4
// instead of 49 at TH = 3.  Longer strips share more (1.75 at 8 rows on 2 waves) but leave too few waves to hide the chain
// LDS read -> lane shifts -> table read -> LDS read, and ran at half the speed.
// The weight of dist >> shift comes from the table's nonzero leading part in LDS (dynamic, n_lds entries); an index from
// n_lds on and below n_nonzero is read from global memory (a table too long for NLM_TABLE_LDS: a large h); from n_nonzero
// on it is 0 without a load.  Integers only, no atomics, no exchange between blocks: an output depends on its inputs alone.
//
// Bounds.  The staged region is EW x EH = (64 + 2 sh) x (NLM_TILE_H + 2 TH + 2 sh) pixels whatever the image's size (the
// reflection maps any coordinate into the image), so every LDS read below is of a staged byte: columns sh + l + dx <=
// 63 + 2 sh, rows sh + r0 + k + dy <= NLM_TILE_H + 2 TH + 2 sh - 1.  Only the store is masked by the image's extent.
#pragma once

constexpr int NLM_WAVES = 8;                       // waves per block
constexpr int NLM_STRIP = 2;                       // output rows per wave
constexpr int NLM_TILE_H = NLM_WAVES * NLM_STRIP;  // 16
constexpr int NLM_THREADS = NLM_WAVES * 64;
constexpr int NLM_MAX_TH = 3, NLM_MAX_SH = 10;
constexpr int NLM_TABLE_LDS = 8192;                // entries of the weight table a block may hold in LDS (32 KB)
constexpr int NLM_EXT_BYTES = (64 + 2 * NLM_MAX_SH) * (NLM_TILE_H + 2 * NLM_MAX_TH + 2 * NLM_MAX_SH) * 3;
constexpr int nlm_tile_w(int th) { return 64 - 2 * th; }

struct NlmArgs {
  const unsigned char* src;  // first byte of the plane group: channel c of pixel p at src[p * src_stride + c]
  unsigned char* dst;        // likewise with dst_stride
  int src_stride, dst_stride;
  int rows, cols, sh;
  int tiles_x;               // tiles per row of tiles: block t makes tile (t % tiles_x, t / tiles_x)
  const int* weight;         // n_nonzero entries
  int n_nonzero, n_lds, shift;
};

// BORDER_REFLECT_101, repeated until the index lies in 0 .. n - 1
__device__ __forceinline__ int nlm_reflect(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

// the sum of v over lanes l .. l + 2 TH, by doubling: 2 / 3 / 4 lane shifts for windows of 3 / 5 / 7 (integers: any order)
template <int TH>
__device__ __forceinline__ int nlm_window(int v) {
  if constexpr (TH == 0) return v;
  const int a1 = v + __shfl_down(v, 1);
  if constexpr (TH == 1) return a1 + __shfl_down(v, 2);
  const int a2 = a1 + __shfl_down(a1, 2);
  if constexpr (TH == 2) return a2 + __shfl_down(v, 4);
  return a2 + __shfl_down(a1, 4) + __shfl_down(v, 6);
}

template <int C, int TH>
__global__ __launch_bounds__(NLM_THREADS) void k_nlm(const NlmArgs a) {
  constexpr int TW = 2 * TH + 1, W = nlm_tile_w(TH), NR = NLM_STRIP + 2 * TH;
  __shared__ unsigned char s_ext[NLM_EXT_BYTES];
  extern __shared__ int s_weight[];
  const int sh = a.sh, b = TH + sh;
  const int EW = 64 + 2 * sh, EH = NLM_TILE_H + 2 * b;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;  // (one grid axis: a tall image has more rows of tiles than grid.y allows)
  const int x0 = tx * W, y0 = ty * NLM_TILE_H;

  for (int e = (int)threadIdx.x; e < EW * EH; e += NLM_THREADS) {
    const int ey = e / EW, ex = e - ey * EW;
    const size_t p = (size_t)nlm_reflect(y0 - b + ey, a.rows) * (size_t)a.cols + (size_t)nlm_reflect(x0 - b + ex, a.cols);
#pragma unroll
    for (int c = 0; c < C; c++) s_ext[e * C + c] = a.src[p * (size_t)a.src_stride + c];
  }
  for (int i = (int)threadIdx.x; i < a.n_lds; i += NLM_THREADS) s_weight[i] = a.weight[i];
  __syncthreads();

  const int lane = (int)threadIdx.x & 63, r0 = ((int)threadIdx.x >> 6) * NLM_STRIP;
  // the lane's reference column: rows r0 - TH .. r0 + NLM_STRIP - 1 + TH of the tile, column lane - TH
  const unsigned char* col = s_ext + ((sh + r0) * EW + sh + lane) * C;
  int ref[NR][C];
#pragma unroll
  for (int k = 0; k < NR; k++)
#pragma unroll
    for (int c = 0; c < C; c++) ref[k][c] = col[k * EW * C + c];

  unsigned est[NLM_STRIP][C], ws[NLM_STRIP];
#pragma unroll
  for (int r = 0; r < NLM_STRIP; r++) {
    ws[r] = 0;
#pragma unroll
    for (int c = 0; c < C; c++) est[r][c] = 0;
  }

  for (int dy = -sh; dy <= sh; dy++) {
    for (int dx = -sh; dx <= sh; dx++) {
      const unsigned char* q = col + (dy * EW + dx) * C;
      int d2[NR];
#pragma unroll
      for (int k = 0; k < NR; k++) {
        int s = 0;
#pragma unroll
        for (int c = 0; c < C; c++) {
          const int d = ref[k][c] - (int)q[k * EW * C + c];
          s += d * d;
        }
        d2[k] = s;
      }
      int v = 0;
#pragma unroll
      for (int k = 0; k < TW; k++) v += d2[k];
#pragma unroll
      for (int r = 0; r < NLM_STRIP; r++) {
        if (r > 0) v += d2[r + TW - 1] - d2[r - 1];
        const int dist = nlm_window<TH>(v);
        // (lanes from W on hold sums of fewer columns: they are never stored and feed no other lane's output)
        const int idx = dist >> a.shift;
        unsigned w = 0;
        if (lane < W && idx < a.n_nonzero) w = idx < a.n_lds ? (unsigned)s_weight[idx] : (unsigned)a.weight[idx];
        // the centre of the compared patch: tile row r0 + r + dy, column lane + dx; lanes from W on read column 0's (w = 0)
        const unsigned char* ctr = q + ((TH + r) * EW + (lane < W ? TH : -lane)) * C;
        ws[r] += w;
#pragma unroll
        for (int c = 0; c < C; c++) est[r][c] += w * (unsigned)ctr[c];
      }
    }
  }

  const int x = x0 + lane;
  if (lane >= W || x >= a.cols) return;
#pragma unroll
  for (int r = 0; r < NLM_STRIP; r++) {
    const int y = y0 + r0 + r;
    if (y >= a.rows) break;
    unsigned char* o = a.dst + ((size_t)y * (size_t)a.cols + (size_t)x) * (size_t)a.dst_stride;
#pragma unroll
    for (int c = 0; c < C; c++) {
      const unsigned t = (est[r][c] + ws[r] / 2u) / ws[r];
      o[c] = (unsigned char)(t > 255u ? 255u : t);
    }
  }
}
