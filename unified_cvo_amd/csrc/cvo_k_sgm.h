// cvo_k_sgm.h -- kernels of the stereo matcher (cvo_sgm.hip; the statement: tests/np_sgm.py): semi-global matching over a
// census cost.  The decisions are the functions of cvo_sgm_math.h, which the CPU twin calls too.
//
// k_sgm_census      one block makes the census words of a SGM_TILE_W x SGM_TILE_H tile of the left or the right image
//                   (blockIdx.y) from an LDS copy of the tile and its 4 / 3 pixel halo, clamped to the image while staging;
//                   a wave writes one row of 64 words.
// k_sgm_path<D,DIR> one wave (one block) walks one path line of direction DIR from the border the direction enters from.
//                   Lane l holds the hypotheses d = l + 64 j, j < D / 64, so S, and the 64 right census words a step reads,
//                   are consecutive across the lanes.  The cost is made on the fly from the census words (two 32-bit
//                   popcounts); no cost volume exists.  L(q, d - 1) / L(q, d + 1) come from the neighbouring lanes
//                   (ds_bpermute; lanes 0 / 63 take them from the neighbouring j through a scalar register), min_k L(q, k)
//                   from a DPP reduction.  Lines of one direction share no pixel, so S is a plain read-modify-write; the
//                   first direction stores instead of adding, which spares clearing S.  A step's loads are issued SGM_AHEAD
//                   steps ahead.  The directions are consecutive launches on one stream.
// k_sgm_select<D>   one wave per pixel: the first argmin of S as a wave minimum of (S << 16 | d), the best sum more than
//                   one disparity away, the sub-pixel term, and - with the left-right check - the first argmin of the
//                   right image's pixel u - d*, read from the diagonal S(v, x + d, d).
// No kernel waits for another block or polls memory; integers only but for sgm_subpixel's division and addition; no scratch
// (every per-lane array is indexed by unrolled constants).
//
// Bounds.  census: the staged coordinates are clamped into the image, LDS reads stay inside the (64 + 8) x (8 + 6) region,
// the store is masked by the image's extent.  path: a line's pixels are inside the image by sgm_line; the right word of d is
// read only for u - d >= 0, the same row.  select: the diagonal reads x + d < cols of the pixel's own row.
#pragma once
#include "cvo_sgm_math.h"
#include "cvo_wave.h"

namespace cvo_dev {

constexpr int SGM_TILE_W = 64, SGM_TILE_H = 8;
constexpr int SGM_CENSUS_THREADS = SGM_TILE_W * SGM_TILE_H;
constexpr int SGM_SELECT_WAVES = 4;  // pixels per block of k_sgm_select
constexpr int SGM_AHEAD = 4;         // steps by which k_sgm_path's loads run ahead of its arithmetic

struct SgmCensusArgs {
  const unsigned char* left;
  const unsigned char* right;
  unsigned long long* census_left;
  unsigned long long* census_right;
  int rows, cols, tiles_x;  // block t makes tile (t % tiles_x, t / tiles_x)
};

__global__ __launch_bounds__(SGM_CENSUS_THREADS) void k_sgm_census(const SgmCensusArgs a) {
  constexpr int EW = SGM_TILE_W + 2 * SGM_HALO_X, EH = SGM_TILE_H + 2 * SGM_HALO_Y;
  __shared__ unsigned char s_img[EW * EH];
  const unsigned char* img = blockIdx.y ? a.right : a.left;
  unsigned long long* out = blockIdx.y ? a.census_right : a.census_left;
  const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
  const int x0 = tx * SGM_TILE_W, y0 = ty * SGM_TILE_H;
  for (int e = (int)threadIdx.x; e < EW * EH; e += SGM_CENSUS_THREADS) {
    const int ey = e / EW, ex = e - ey * EW;
    const int y = min(max(y0 - SGM_HALO_Y + ey, 0), a.rows - 1), x = min(max(x0 - SGM_HALO_X + ex, 0), a.cols - 1);
    s_img[e] = img[(size_t)y * (size_t)a.cols + (size_t)x];
  }
  __syncthreads();
  const int lx = (int)threadIdx.x & (SGM_TILE_W - 1), ly = (int)threadIdx.x >> 6;
  const unsigned char* c = s_img + (ly + SGM_HALO_Y) * EW + lx + SGM_HALO_X;
  const int centre = *c;
  unsigned long long word = 0;
#pragma unroll
  for (int dy = -SGM_HALO_Y; dy <= SGM_HALO_Y; dy++)
#pragma unroll
    for (int dx = -SGM_HALO_X; dx <= SGM_HALO_X; dx++)
      if (dy != 0 || dx != 0) word = (word << 1) | (unsigned long long)((int)c[dy * EW + dx] < centre ? 1 : 0);
  const int x = x0 + lx, y = y0 + ly;
  if (x < a.cols && y < a.rows) out[(size_t)y * (size_t)a.cols + (size_t)x] = word;
}

struct SgmPathArgs {
  const unsigned long long* census_left;
  const unsigned long long* census_right;
  unsigned short* S;  // rows x cols x D
  int rows, cols, p1, p2, n_lines;
  int accumulate;     // 0: the first direction stores
};

// what a step of k_sgm_path reads from memory: the left census word of its pixel, the right words of the lane's hypotheses
// and their sums so far
template <int NH>
struct SgmStepInput {
  unsigned long long cl, cr[NH];
  int sum[NH];
};

template <int D>
__device__ __forceinline__ void sgm_fetch(const SgmPathArgs& a, int v, int u, int lane, SgmStepInput<D / 64>& in) {
  const size_t p = (size_t)v * (size_t)a.cols + (size_t)u;
  in.cl = a.census_left[p];
#pragma unroll
  for (int j = 0; j < D / 64; j++) {
    const int d = lane + 64 * j;
    in.cr[j] = u - d >= 0 ? a.census_right[p - (size_t)d] : 0ull;
    in.sum[j] = a.accumulate ? (int)a.S[p * (size_t)D + (size_t)d] : 0;
  }
}

template <int D, int DIR>
__global__ __launch_bounds__(64) void k_sgm_path(const SgmPathArgs a) {
  constexpr int NH = D / 64;
  const int lane = (int)threadIdx.x;
  if ((int)blockIdx.x >= a.n_lines) return;
  int v, u, len;
  sgm_line(DIR, (int)blockIdx.x, a.rows, a.cols, &v, &u, &len);
  const int dv = sgm_dv(DIR), du = sgm_du(DIR);
  int L[NH];
  int m = 0;
  // The loads of step s + SGM_AHEAD are issued before the arithmetic of step s: the recurrence is a dependent chain with one
  // wave per line, and nothing else would hide the memory latency of a step.  A pixel SGM_AHEAD steps
  // on is written neither by the steps in between nor by any other line of this direction.  The ring is indexed by the
  // unrolled k only: registers.
  SgmStepInput<NH> ring[SGM_AHEAD];
#pragma unroll
  for (int k = 0; k < SGM_AHEAD; k++)
    if (k < len) sgm_fetch<D>(a, v + k * dv, u + k * du, lane, ring[k]);
  for (int s = 0; s < len; s += SGM_AHEAD) {
#pragma unroll
    for (int k = 0; k < SGM_AHEAD; k++) {
      if (s + k >= len) break;
      const SgmStepInput<NH> in = ring[k];
      if (s + k + SGM_AHEAD < len) sgm_fetch<D>(a, v + SGM_AHEAD * dv, u + SGM_AHEAD * du, lane, ring[k]);
      int c[NH];
#pragma unroll
      for (int j = 0; j < NH; j++) c[j] = sgm_cost(in.cl, in.cr[j], u - (lane + 64 * j) >= 0);
      if (s + k == 0) {
#pragma unroll
        for (int j = 0; j < NH; j++) L[j] = c[j];
      } else {
        int next[NH];
#pragma unroll
        for (int j = 0; j < NH; j++) {
          int lo = __shfl_up(L[j], 1), hi = __shfl_down(L[j], 1);
          if (j > 0) {
            const int seam = __builtin_amdgcn_readlane(L[j > 0 ? j - 1 : 0], 63);
            lo = lane == 0 ? seam : lo;
          }
          if (j < NH - 1) {
            const int seam = __builtin_amdgcn_readlane(L[j < NH - 1 ? j + 1 : j], 0);
            hi = lane == 63 ? seam : hi;
          }
          const int d = lane + 64 * j;
          next[j] = sgm_step(c[j], L[j], lo, d > 0, hi, d < D - 1, m, a.p1, a.p2);
        }
#pragma unroll
        for (int j = 0; j < NH; j++) L[j] = next[j];
      }
      int least = L[0];
#pragma unroll
      for (int j = 1; j < NH; j++) least = min(least, L[j]);
      m = (int)wave_min_u32((unsigned)least);
      unsigned short* sp = a.S + ((size_t)v * (size_t)a.cols + (size_t)u) * (size_t)D;
#pragma unroll
      for (int j = 0; j < NH; j++) sp[lane + 64 * j] = (unsigned short)(in.sum[j] + L[j]);
      v += dv;
      u += du;
    }
  }
}

struct SgmSelectArgs {
  const unsigned short* S;
  float* disparity;
  int rows, cols, uniqueness, lr_max_diff;
};

template <int D>
__global__ __launch_bounds__(64 * SGM_SELECT_WAVES) void k_sgm_select(const SgmSelectArgs a) {
  constexpr int NH = D / 64;
  const int lane = (int)threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SGM_SELECT_WAVES + ((int)threadIdx.x >> 6));
  if (p >= a.rows * a.cols) return;
  const int v = p / a.cols, u = p - v * a.cols;
  const unsigned short* sp = a.S + (size_t)p * (size_t)D;
  unsigned s[NH], key = ~0u;
#pragma unroll
  for (int j = 0; j < NH; j++) {
    s[j] = sp[lane + 64 * j];
    key = min(key, (s[j] << 16) | (unsigned)(lane + 64 * j));
  }
  key = wave_min_u32(key);
  const int d = (int)(key & 0xFFFFu), s1 = (int)(key >> 16);
  unsigned far = SGM_NO_COST;
#pragma unroll
  for (int j = 0; j < NH; j++) {
    const int dd = lane + 64 * j;
    if (dd < d - 1 || dd > d + 1) far = min(far, s[j]);
  }
  const int s2 = (int)wave_min_u32(far);
  bool valid = !sgm_ambiguous(s1, s2, a.uniqueness);
  const int sm = d > 0 ? (int)sp[d - 1] : 0, sn = d < D - 1 ? (int)sp[d + 1] : 0;
  const float disp = sgm_subpixel(d, D, sm, s1, sn);
  if (a.lr_max_diff >= 0) {
    const int x = u - d;  // (wave-uniform, as d is)
    if (x < 0) {
      valid = false;
    } else {
      const unsigned short* row = a.S + (size_t)v * (size_t)a.cols * (size_t)D;
      unsigned rkey = ~0u;
#pragma unroll
      for (int j = 0; j < NH; j++) {
        const int dd = lane + 64 * j;
        if (x + dd < a.cols) rkey = min(rkey, ((unsigned)row[(size_t)(x + dd) * (size_t)D + (size_t)dd] << 16) | (unsigned)dd);
      }
      rkey = wave_min_u32(rkey);
      if (sgm_lr_differs(d, (int)(rkey & 0xFFFFu), a.lr_max_diff)) valid = false;
    }
  }
  if (lane == 0) a.disparity[p] = valid ? disp : SGM_INVALID;
}

}  // namespace cvo_dev
