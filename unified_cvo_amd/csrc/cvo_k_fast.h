// cvo_k_fast.h -- the FAST-9/16 corner detector as cv::FAST(gray, keypoints, t, nonmax = false) defines it, for EVERY
// threshold at once (select_points_from_image's CV_FAST branch re-runs the detector per threshold, CvoPointCloud.cpp:273-312).
//
//   k_fast_score    one pixel per lane.  With d_k = I_k - I_p over the 16 ring pixels, the score s(p) is the maximum over the
//                   16 cyclic arcs of 9 and the two signs of the minimum of +-d_k over the arc: p is a corner at t iff
//                   s(p) > t.  Writes max(s, 0) as one byte per pixel (0: a corner at no threshold) and adds the block's
//                   257-bin histogram of clamp(s, -1, 255) - built in LDS - to the frame's (integer atomics: counts only).
//                   Pixels outside 3 <= x < w - 3, 3 <= y < h - 3 score -1.  The suffix sums of the histogram are the
//                   detector's keypoint counts at all 256 thresholds, so the host replays the threshold schedule on 257
//                   numbers.  TILE: the block's 64 x 16 pixels and their 3-pixel halo go through LDS (a BGR image is
//                   converted once per pixel, not 17 times); otherwise every lane reads its ring through the cache.
//   FastAbove       predicate of the ordered (row-major) compaction (cvo_k_compact.h): the pixels with score > t.
//
// All integer arithmetic: nothing to round.  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_k_rgbd.h"

namespace cvo_dev {

constexpr int FAST_BINS = 257;                  // s = -1 .. 255
constexpr int FAST_TILE_W = 64, FAST_TILE_H = RGBD_THREADS / 64;  // pixels of a block: one wave per row
constexpr int FAST_HALO = 3;
constexpr int FAST_LDS_W = FAST_TILE_W + 2 * FAST_HALO, FAST_LDS_H = FAST_TILE_H + 2 * FAST_HALO;

// the Bresenham circle of radius 3 in OpenCV's order: (dx, dy) of ring pixel k
#define CVO_FAST_RING_DX {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1}
#define CVO_FAST_RING_DY {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3}

// s(p) of the 16 differences d_k = I_k - I_p: max over arcs and signs of the min of +-d_k over 9 contiguous ring pixels.
// min over an arc of 9 = min(min of 8 by doubling, the ninth); the dark sign is -(max over the arc).
__host__ __device__ inline int fast_score16(const int (&d)[16]) {
  int lo[16], hi[16], lo2[16], hi2[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    lo[k] = min(d[k], d[(k + 1) & 15]);
    hi[k] = max(d[k], d[(k + 1) & 15]);
  }
#pragma unroll
  for (int k = 0; k < 16; k++) {
    lo2[k] = min(lo[k], lo[(k + 2) & 15]);
    hi2[k] = max(hi[k], hi[(k + 2) & 15]);
  }
  int best = -256;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int l9 = min(min(lo2[k], lo2[(k + 4) & 15]), d[(k + 8) & 15]);
    const int h9 = max(max(hi2[k], hi2[(k + 4) & 15]), d[(k + 8) & 15]);
    best = max(best, max(l9, -h9));
  }
  return best;
}

// s(p) clamped to -1 .. 255 at pixel (x, y) of a plane read through `at(x, y)`; -1 outside the interior
template <class At>
__host__ __device__ inline int fast_score_at(int w, int h, int x, int y, At at) {
  if (x < FAST_HALO || y < FAST_HALO || x >= w - FAST_HALO || y >= h - FAST_HALO) return -1;
  constexpr int dx[16] = CVO_FAST_RING_DX, dy[16] = CVO_FAST_RING_DY;
  const int c = at(x, y);
  int d[16];
#pragma unroll
  for (int k = 0; k < 16; k++) d[k] = at(x + dx[k], y + dy[k]) - c;
  return max(-1, fast_score16(d));
}

template <bool TILE>
__global__ __launch_bounds__(RGBD_THREADS) void k_fast_score(int w, int h, int channels, const unsigned char* __restrict__ img,
                                                            unsigned char* __restrict__ score, unsigned* __restrict__ hist) {
  __shared__ unsigned bins[FAST_BINS];
  __shared__ unsigned char tile[TILE ? FAST_LDS_H * FAST_LDS_W : 1];
  const int nbx = (w + FAST_TILE_W - 1) / FAST_TILE_W;  // (a 1-D grid of nbx x ceil(h / FAST_TILE_H) blocks, row-major)
  const int x0 = ((int)blockIdx.x % nbx) * FAST_TILE_W, y0 = ((int)blockIdx.x / nbx) * FAST_TILE_H;
  for (int b = threadIdx.x; b < FAST_BINS; b += RGBD_THREADS) bins[b] = 0;
  if (TILE)
    for (int i = threadIdx.x; i < FAST_LDS_H * FAST_LDS_W; i += RGBD_THREADS) {
      const int gx = x0 - FAST_HALO + i % FAST_LDS_W, gy = y0 - FAST_HALO + i / FAST_LDS_W;
      tile[i] = (gx >= 0 && gy >= 0 && gx < w && gy < h) ? (unsigned char)rgbd_gray(img, channels, (size_t)gy * w + gx) : 0;
    }
  __syncthreads();
  const int x = x0 + ((int)threadIdx.x & (FAST_TILE_W - 1)), y = y0 + ((int)threadIdx.x >> 6);
  if (x < w && y < h) {
    int s;
    if (TILE)
      s = fast_score_at(w, h, x, y, [&](int xx, int yy) { return (int)tile[(yy - y0 + FAST_HALO) * FAST_LDS_W + (xx - x0 + FAST_HALO)]; });
    else
      s = fast_score_at(w, h, x, y, [&](int xx, int yy) { return rgbd_gray(img, channels, (size_t)yy * w + xx); });
    score[(size_t)y * w + x] = (unsigned char)max(s, 0);
    atomicAdd(&bins[s + 1], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < FAST_BINS; b += RGBD_THREADS)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

struct FastAbove {
  typedef int Item;  // the pixel
  const unsigned char* score;
  int t;
  int* out;
  __device__ bool keep(int p, int n, Item* item) const {
    *item = p;
    return p < n && (int)score[p] > t;
  }
  __device__ void write(unsigned at, const Item& p) const { out[at] = p; }
};

}  // namespace cvo_dev
