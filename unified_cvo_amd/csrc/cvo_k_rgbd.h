// cvo_k_rgbd.h -- RGB-D front end: from a colour image, a depth image and a calibration to the candidate points of
// CvoPointCloud(ImageRGBD, Calibration, FULL / DSO_EDGES) (CvoPointCloud.cpp:459-553, CvoPixelSelector.cpp:51-474).
//
//   k_rgbd_gray_grad    gray level (given plane, or OpenCV 3's 8-bit BGR2GRAY) and g2 = dx^2 + dy^2 of the central
//                       differences x 0.5 (RawImage.cpp:55-82), one pixel per lane.
//   k_rgbd_hist         one block per 32 x 32 image block: histogram of int(sqrtf(g2)) capped at 48 in LDS (a wave adds
//                       each distinct bin once), its 0.5 quantile + 7 (makeHists, :83-117).
//   k_rgbd_smooth       3 x 3 mean over existing neighbours, squared (:119-143).  One block.
//   k_rgbd_select       one lane per pot x pot cell, for EVERY potential the schedule can ask for (2 .. 7) in one launch:
//                       the first pixel in row-major order with the largest g2 strictly above its threshold.  Cells are
//                       enumerated in the reference's nesting (blocks of 4 pot, 2 pot, pot, each row-major), padded to whole
//                       4 pot blocks, so an ORDERED compaction (k_compact_scan over the block counts it writes itself,
//                       k_compact_write<RgbdCellHit>) gives output_uv of select() (:270-426) for each potential.  No atomic
//                       decides a position.
//   RgbdKeep            predicate of the ordered compaction (cvo_k_compact.h) over a pixel list - FULL's column-major order
//                       or a selected list -: depth test (dep != 0 && !isnan(dep)) and exclusion byte; writes the pixel
//                       index and xyz of the survivors.
//   k_rgbd_gather       out[i] = pixel[kept[i]]: only the survivors' pixel indices go back to the host.
//
// Every value here is exact or correctly rounded: g2 is a multiple of 0.25 below 2^16, the root is an integer root of
// 4 g2, the divisions of the back-projection are IEEE (no fast-math).  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_device.h"
#include "cvo_k_voxel.h"

namespace cvo_dev {

constexpr int RGBD_THREADS = COMPACT_THREADS;  // (k_rgbd_select counts per block for the ordered compaction)
constexpr int RGBD_POT_MIN = 2, RGBD_POT_MAX = 7, RGBD_POTS = RGBD_POT_MAX - RGBD_POT_MIN + 1;
constexpr int RGBD_THS_SLACK = 100;        // thsSmoothed has (w/32)(h/32) + 100 entries (CvoPixelSelector.cpp:63)
enum : int { RGBD_DEPTH_U16 = 0, RGBD_DEPTH_F32 = 1 };

// where the cells of every potential start in the concatenated cell list (each segment padded to whole blocks of
// RGBD_THREADS, so no block of k_rgbd_select straddles two potentials)
struct RgbdCells {
  int start[RGBD_POTS + 1];
};

__host__ __device__ inline int rgbd_gray(const unsigned char* img, int channels, size_t p) {
  if (channels == 1) return img[p];
  return (1868 * (int)img[3 * p] + 9617 * (int)img[3 * p + 1] + 4899 * (int)img[3 * p + 2] + 8192) >> 14;
}

// int(sqrtf(g2)) for g2 a non-negative multiple of 0.25: floor(sqrt(4 g2)) / 2 in integers (no device sqrtf is trusted
// at the perfect squares)
__host__ __device__ inline int rgbd_root(float g2) {
  const int m = (int)(4.0f * g2);
  int r = (int)sqrtf((float)m);
  while (r * r > m) r--;
  while ((r + 1) * (r + 1) <= m) r++;
  return r >> 1;
}

// g2 of pixel (x, y) from the gray levels of its four neighbours; zero on the first / last row and column
__host__ __device__ inline float rgbd_g2(const unsigned char* img, int channels, int w, int h, int x, int y) {
  if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return 0.f;
  const size_t p = (size_t)y * w + x;
  const float dx = 0.5f * ((float)rgbd_gray(img, channels, p + 1) - (float)rgbd_gray(img, channels, p - 1));
  const float dy = 0.5f * ((float)rgbd_gray(img, channels, p + w) - (float)rgbd_gray(img, channels, p - w));
  return dx * dx + dy * dy;
}

__global__ __launch_bounds__(RGBD_THREADS) void k_rgbd_gray_grad(int w, int h, int channels, const unsigned char* __restrict__ img,
                                                                 float* __restrict__ g2) {
  const int p = blockIdx.x * RGBD_THREADS + (int)threadIdx.x;
  if (p >= w * h) return;
  g2[p] = rgbd_g2(img, channels, w, h, p % w, p / w);
}

// computeHistQuantil (CvoPixelSelector.cpp:72-80) at 0.5 over bins[0 .. 49) of `count` pixels; the reference scans 90 bins,
// of which those from 49 on are never written
__host__ __device__ inline int rgbd_quantile(const unsigned* bins, unsigned count) {
  int th = (int)((float)count * 0.5f + 0.5f);
  for (int i = 0; i < 90; i++) {
    th -= i < 49 ? (int)bins[i] : 0;
    if (th < 0) return i;
  }
  return 90;
}

__global__ __launch_bounds__(RGBD_THREADS) void k_rgbd_hist(int w, int h, const float* __restrict__ g2, float* __restrict__ ths) {
  __shared__ unsigned bins[50];  // [49]: the number of pixels counted
  const int w32 = w / 32, bx = blockIdx.x % w32, by = blockIdx.x / w32;
  if (threadIdx.x < 50) bins[threadIdx.x] = 0;
  __syncthreads();
  const int it = 32 * bx + ((int)threadIdx.x & 31), jt = 32 * by + ((int)threadIdx.x >> 5);
  const bool valid = !(it > w - 2 || jt > h - 2 || it < 1 || jt < 1);
  const int bin = valid ? min(48, rgbd_root(g2[(size_t)jt * w + it])) : -1;
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  if (lane == 0 && todo) atomicAdd(&bins[49], (unsigned)__popcll(todo));
  while (todo) {  // (wave-uniform) a flat block puts all its pixels into one bin: one LDS atomic per wave, not 64
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __shfl(bin, leader);
    const unsigned long long same = __ballot(bin == lb);
    if (lane == leader) atomicAdd(&bins[lb], (unsigned)__popcll(same));
    todo &= ~same;
  }
  __syncthreads();
  if (threadIdx.x == 0) ths[blockIdx.x] = (float)(rgbd_quantile(bins, bins[49]) + 7);
}

// thsSmoothed of block (x, y) (CvoPixelSelector.cpp:119-143); the thresholds are small integers, any order of the sum is exact
__host__ __device__ inline float rgbd_smooth_one(const float* ths, int w32, int h32, int x, int y) {
  float sum = 0.f, num = 0.f;
  for (int yy = y - 1; yy <= y + 1; yy++)
    for (int xx = x - 1; xx <= x + 1; xx++)
      if (xx >= 0 && xx < w32 && yy >= 0 && yy < h32) {
        num += 1.f;
        sum += ths[xx + yy * w32];
      }
  const float m = sum / num;
  return m * m;
}

__global__ __launch_bounds__(RGBD_THREADS) void k_rgbd_smooth(int w32, int h32, const float* __restrict__ ths, float* __restrict__ sm) {
  for (int b = threadIdx.x; b < w32 * h32; b += RGBD_THREADS) sm[b] = rgbd_smooth_one(ths, w32, h32, b % w32, b / w32);
}

// The pixel cell `c` of potential `pot` keeps, or -1.  c counts the cells of the image padded to whole 4 pot blocks in
// the reference's nesting: 16 cells per block - (y3, x3) the 2 pot quadrant, (y2, x2) the cell in it -, blocks row-major.
// sm: thsSmoothed, read at (x >> 5) + (y >> 5) * (w / 32) literally (the host has checked that this stays inside it).
__host__ __device__ inline int rgbd_cell_best(int c, int pot, int w, int h, const float* g2, const float* sm) {
  const int nbx = (w + 4 * pot - 1) / (4 * pot), b4 = c >> 4;
  const int x0 = (b4 % nbx) * 4 * pot + ((c >> 2) & 1) * 2 * pot + (c & 1) * pot;
  const int y0 = (b4 / nbx) * 4 * pot + ((c >> 3) & 1) * 2 * pot + ((c >> 1) & 1) * pot;
  if (x0 >= w || y0 >= h) return -1;
  const int x1 = min(x0 + pot, w), y1 = min(y0 + pot, h), step = w / 32;
  int best = -1;
  float best_val = 0.f;
  for (int y = y0; y < y1; y++)
    for (int x = x0; x < x1; x++) {
      if (x < 4 || x >= w - 5 || y < 4 || y > h - 4) continue;
      const float a = g2[(size_t)y * w + x];
      if (a > sm[(x >> 5) + (y >> 5) * step] && a > best_val) {
        best_val = a;
        best = y * w + x;
      }
    }
  return best;
}

// number of cells of the padded image at potential pot
__host__ __device__ inline int rgbd_cells(int pot, int w, int h) {
  return ((w + 4 * pot - 1) / (4 * pot)) * ((h + 4 * pot - 1) / (4 * pot)) * 16;
}

__global__ __launch_bounds__(RGBD_THREADS) void k_rgbd_select(int w, int h, RgbdCells cells, const float* __restrict__ g2,
                                                              const float* __restrict__ sm, int* __restrict__ hit,
                                                              unsigned* __restrict__ block_count) {
  const int gid = blockIdx.x * RGBD_THREADS + (int)threadIdx.x;
  int k = 0, first = 0;
#pragma unroll
  for (int j = 1; j < RGBD_POTS; j++)  // (uniform per block; constant indices keep the argument in registers)
    if (gid >= cells.start[j]) {
      k = j;
      first = cells.start[j];
    }
  const int pot = RGBD_POT_MIN + k, c = gid - first;
  const int best = c < rgbd_cells(pot, w, h) ? rgbd_cell_best(c, pot, w, h, g2, sm) : -1;
  hit[gid] = best;
  compact_block_count(best >= 0, block_count);
}

// the write side of k_rgbd_select's compaction: hit[] in order, without the cells that hit nothing
struct RgbdCellHit {
  typedef int Item;  // the cell's pixel
  const int* hit;
  int* out;
  __device__ bool keep(int i, int n, Item* v) const {
    *v = i < n ? hit[i] : -1;
    return *v >= 0;
  }
  __device__ void write(unsigned at, const Item& v) const { out[at] = v; }
};

// the depth of pixel p in metres x scaling factor, and whether the reference keeps it: dep != 0 && !isnan(dep)
__host__ __device__ inline bool rgbd_depth(const void* depth, int depth_type, size_t p, float* dep) {
  if (depth_type == RGBD_DEPTH_U16) {
    const unsigned short d = ((const unsigned short*)depth)[p];
    *dep = (float)d;
    return d != 0;
  }
  const float d = ((const float*)depth)[p];
  *dep = d;
  return d != 0.f && d == d;
}

struct RgbdCalib {
  float fx, fy, cx, cy, scale;
};

// CvoPointCloud.cpp:491-498, float32 in this order of operations
__host__ __device__ inline void rgbd_backproject(const RgbdCalib& k, int u, int v, float dep, float* xyz) {
  const float z = dep / k.scale;
  xyz[0] = (((float)u - k.cx) * z) / k.fx;
  xyz[1] = (((float)v - k.cy) * z) / k.fy;
  xyz[2] = z;
}

// candidate i of a pass: pixel list[i], or - list == nullptr, FULL - the i-th pixel in column-major order
__device__ __forceinline__ bool rgbd_candidate(int i, int n, const int* __restrict__ list, int w, int h, const void* __restrict__ depth,
                                               int depth_type, const unsigned char* __restrict__ excl, int* pix, float* dep) {
  if (i >= n) return false;
  const int p = list ? list[i] : (i % h) * w + i / h;
  *pix = p;
  if ((unsigned)p >= (unsigned)(w * h)) return false;
  return rgbd_depth(depth, depth_type, (size_t)p, dep) && !(excl && excl[p]);
}

struct RgbdKeep {
  struct Item {
    int pix;
    float dep;
  };
  const int* list;
  int w, h;
  const void* depth;
  int depth_type;
  const unsigned char* excl;
  RgbdCalib calib;
  int* pix_out;
  float* xyz;
  __device__ bool keep(int i, int n, Item* c) const { return rgbd_candidate(i, n, list, w, h, depth, depth_type, excl, &c->pix, &c->dep); }
  __device__ void write(unsigned at, const Item& c) const {
    float p[3];
    rgbd_backproject(calib, c.pix % w, c.pix / w, c.dep, p);
    pix_out[at] = c.pix;
    xyz[3 * (size_t)at] = p[0];
    xyz[3 * (size_t)at + 1] = p[1];
    xyz[3 * (size_t)at + 2] = p[2];
  }
};

__global__ __launch_bounds__(RGBD_THREADS) void k_rgbd_gather(int n, int n_src, const int* __restrict__ kept, const int* __restrict__ pix,
                                                              int* __restrict__ out) {
  const int i = blockIdx.x * RGBD_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const int k = kept[i];
  out[i] = (unsigned)k < (unsigned)n_src ? pix[k] : -1;
}

}  // namespace cvo_dev
