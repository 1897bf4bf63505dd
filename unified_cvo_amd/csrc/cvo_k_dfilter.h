// cvo_k_dfilter.h -- kernels of the disparity post-filter (cvo_dfilter.hip; the statement: tests/np_dfilter.py): libelas's
// removeSmallSegments, gapInterpolation and adaptiveMean on a float map whose invalid pixels are negative.  The decisions are
// the functions of cvo_dfilter_math.h, which the CPU twin calls too.
//
// Every kernel but k_dfilter_gap runs one thread per pixel in blocks of DFILTER_TILE_W x DFILTER_TILE_H pixels, a wave per tile
// row, so the 64 lanes of a wave are 64 consecutive pixels of one image row.
//
// Speckle: connected components of the valid pixels (4-neighbours within `sim`) by uf_find / uf_unite of cvo_k_prims.h.
// k_dfilter_label   parent[p] = the first pixel of p's horizontal run inside its wave (a ballot, no atomics): the horizontal
//                   links cost nothing and leave trees of depth 1; size[p] = 0.
// k_dfilter_unite   the links k_dfilter_label could not see: to the left across a wave's first lane, and downwards - the
//                   downward link is skipped where the left neighbour's downward link and the two horizontal links imply it
//                   (inside a flat region: all but the first column of a wave).
// k_dfilter_roots   root[p] = find(p), -1 for an invalid pixel; a wave adds each run of equal roots to size[root] with ONE
//                   atomic, so a segment that covers the image takes one add per wave, not one per pixel.
// k_dfilter_mask    the map with segments below speckle_size, and every negative value, as -10; counts segments and removed pixels.
// Labels are minimum indices and sizes integer sums: the result does not depend on the order the waves run in.
//
// k_dfilter_gap     one wave per line (a row, or a column by its strides): a forward pass in steps of 64 pixels leaves the
//                   index of the last valid pixel before every pixel (a ballot per step, the carry between steps uniform),
//                   a backward pass finds the next valid one the same way and fills.  Valid pixels never change, so the
//                   passes read the input only; any gap width works.
// k_dfilter_mean_h / _v   one pixel per thread from an LDS copy of the tile and its halo (4 before, 3 after, along the pass).
//
// Bounds.  A thread outside the image takes part in ballots and shuffles with an invalid value and writes nothing.  unite
// reads p - 1 only for x > 0 and p + cols only for y + 1 < rows.  gap: indices j < len of line < n_lines; prev / next are
// indices of valid pixels of the same line or -1 / len, tested before use.  mean: the staged coordinates are clamped into
// the image, a window is read only where libelas's loops reach (it lies inside the image there), LDS reads stay in the
// (64 + 7) x 4 or 64 x (4 + 7) region.
#pragma once
#include "cvo_dfilter_math.h"
#include "cvo_k_prims.h"

namespace cvo_dev {

constexpr int DFILTER_TILE_W = 64, DFILTER_TILE_H = 4;
constexpr int DFILTER_THREADS = DFILTER_TILE_W * DFILTER_TILE_H;
constexpr int DFILTER_HALO = DFILTER_MEAN_BEFORE + DFILTER_MEAN_AFTER;

struct DFilterCounters {
  unsigned segments, removed, filled_rows, filled_cols;
};

// the pixel of a thread: block t covers tile (t % tiles_x, t / tiles_x)
struct DFilterPixel {
  int x0, y0, lx, ly, x, y;
  bool in;
  size_t p;
};

__device__ __forceinline__ DFilterPixel dfilter_pixel(int rows, int cols, int tiles_x) {
  DFilterPixel q;
  const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
  q.x0 = tx * DFILTER_TILE_W;
  q.y0 = ty * DFILTER_TILE_H;
  q.lx = (int)threadIdx.x & 63;
  q.ly = (int)threadIdx.x >> 6;
  q.x = q.x0 + q.lx;
  q.y = q.y0 + q.ly;
  q.in = q.x < cols && q.y < rows;
  q.p = q.in ? (size_t)q.y * (size_t)cols + (size_t)q.x : 0;
  return q;
}

struct DFilterSpeckleArgs {
  const float* src;
  float* out;
  int* parent;
  int* root;
  unsigned* size;
  DFilterCounters* counters;
  int rows, cols, tiles_x, speckle_size;
  float sim;
};

__device__ __forceinline__ bool dfilter_linked(float a, float b, float sim) {
  return dfilter_valid(a) && dfilter_valid(b) && dfilter_similar(a, b, sim);
}

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_label(const DFilterSpeckleArgs a) {
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  const float v = q.in ? a.src[q.p] : DFILTER_INVALID;
  const float left = __shfl_up(v, 1);
  const bool link = q.lx > 0 && dfilter_linked(v, left, a.sim);
  const unsigned long long heads = __ballot(!link);  // (lane 0 is always one)
  if (!q.in) return;
  const int start = 63 - __clzll(heads & (~0ull >> (63 - q.lx)));
  a.parent[q.p] = (int)q.p - (q.lx - start);
  a.size[q.p] = 0u;
}

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_unite(const DFilterSpeckleArgs a) {
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  const bool has_down = q.in && q.y + 1 < a.rows;
  const float v = q.in ? a.src[q.p] : DFILTER_INVALID;
  const float down = has_down ? a.src[q.p + (size_t)a.cols] : DFILTER_INVALID;
  const float left = __shfl_up(v, 1), down_left = __shfl_up(down, 1);
  if (!q.in || !dfilter_valid(v)) return;
  const int p = (int)q.p;
  if (q.lx == 0 && q.x > 0 && dfilter_linked(v, a.src[q.p - 1], a.sim)) uf_unite(a.parent, p, p - 1);
  if (dfilter_linked(v, down, a.sim)) {
    const bool implied = q.lx > 0 && dfilter_linked(v, left, a.sim) && dfilter_linked(left, down_left, a.sim) && dfilter_linked(down_left, down, a.sim);
    if (!implied) uf_unite(a.parent, p, p + a.cols);
  }
}

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_roots(const DFilterSpeckleArgs a) {
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  int r = -1;
  if (q.in && dfilter_valid(a.src[q.p])) r = uf_find(a.parent, (int)q.p);  // (the parents no longer change: a launch behind)
  if (q.in) a.root[q.p] = r;
  const int before = __shfl_up(r, 1);
  const bool head = q.lx == 0 || before != r;
  const unsigned long long heads = __ballot(head);
  if (head && r >= 0) {
    const unsigned long long above = q.lx < 63 ? heads >> (q.lx + 1) : 0ull;
    atomicAdd(&a.size[r], (unsigned)(above ? __ffsll((long long)above) : 64 - q.lx));
  }
}

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_mask(const DFilterSpeckleArgs a) {
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  const int r = q.in ? a.root[q.p] : -1;
  const bool keep = r >= 0 && a.size[r] >= (unsigned)a.speckle_size;
  if (q.in) a.out[q.p] = keep ? a.src[q.p] : DFILTER_INVALID;
  wave_count_add(r >= 0 && r == (int)q.p, &a.counters->segments);
  wave_count_add(r >= 0 && !keep, &a.counters->removed);
}

struct DFilterGapArgs {
  const float* in;
  float* out;
  int* prev;         // scratch, one int per pixel
  unsigned* filled;  // pixels filled, added to
  int n_lines, len, line_stride, elem_stride, width;
};

__global__ __launch_bounds__(64) void k_dfilter_gap(const DFilterGapArgs a) {
  const int lane = (int)threadIdx.x, line = (int)blockIdx.x;
  if (line >= a.n_lines) return;
  const size_t base = (size_t)line * (size_t)a.line_stride, es = (size_t)a.elem_stride;
  int carry = -1;  // the last valid pixel before the step
  for (int b = 0; b < a.len; b += 64) {
    const int j = b + lane;
    const bool in = j < a.len;
    const bool valid = in && dfilter_valid(a.in[base + (size_t)j * es]);
    const unsigned long long m = __ballot(valid);
    const unsigned long long below = lane ? m & (~0ull >> (64 - lane)) : 0ull;
    if (in) a.prev[base + (size_t)j * es] = below ? b + 63 - __clzll(below) : carry;
    if (m) carry = b + 63 - __clzll(m);
  }
  int next = a.len;  // the first valid pixel after the step
  unsigned filled = 0;
  for (int b = (a.len - 1) / 64 * 64; b >= 0; b -= 64) {
    const int j = b + lane;
    const bool in = j < a.len;
    const float v = in ? a.in[base + (size_t)j * es] : DFILTER_INVALID;
    const bool valid = in && dfilter_valid(v);
    const unsigned long long m = __ballot(valid);
    const unsigned long long above = lane < 63 ? m >> (lane + 1) : 0ull;
    const int nx = above ? j + __ffsll((long long)above) : next;
    bool fill = false;
    float o = v;
    if (in && !valid) {
      const int pv = a.prev[base + (size_t)j * es];  // (this lane wrote it)
      if (pv >= 0 && nx < a.len && nx - pv - 1 <= a.width) {
        o = dfilter_fill(a.in[base + (size_t)pv * es], a.in[base + (size_t)nx * es]);
        fill = true;
      }
    }
    if (in) a.out[base + (size_t)j * es] = o;
    filled += (unsigned)__popcll(__ballot(fill));
    if (m) next = b + __ffsll((long long)m) - 1;
  }
  if (lane == 0 && filled) atomicAdd(a.filled, filled);
}

struct DFilterMeanArgs {
  const float* in;   // the map the mean starts from
  const float* tmp;  // _v: the horizontal pass's result
  float* out;        // _h: tmp
  int rows, cols, tiles_x;
};

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_mean_h(const DFilterMeanArgs a) {
  constexpr int EW = DFILTER_TILE_W + DFILTER_HALO;
  __shared__ float s[DFILTER_TILE_H * EW];
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  for (int e = (int)threadIdx.x; e < DFILTER_TILE_H * EW; e += DFILTER_THREADS) {
    const int ey = e / EW, ex = e - ey * EW;
    const int y = min(q.y0 + ey, a.rows - 1), x = min(max(q.x0 - DFILTER_MEAN_BEFORE + ex, 0), a.cols - 1);
    const float v = a.in[(size_t)y * (size_t)a.cols + (size_t)x];
    s[e] = dfilter_valid(v) ? v : DFILTER_INVALID;
  }
  __syncthreads();
  if (!q.in) return;
  const float* win = s + q.ly * EW + q.lx;  // coordinate x - 4
  const float cur = win[DFILTER_MEAN_BEFORE];
  float o = cur, d;
  if (q.y >= 3 && q.y <= a.rows - 4 && q.x >= 4 && q.x <= a.cols - 4 && dfilter_mean(win, 1, q.x - DFILTER_MEAN_BEFORE, cur, &d)) o = d;
  a.out[q.p] = o;
}

__global__ __launch_bounds__(DFILTER_THREADS) void k_dfilter_mean_v(const DFilterMeanArgs a) {
  constexpr int EH = DFILTER_TILE_H + DFILTER_HALO;
  __shared__ float s[EH * DFILTER_TILE_W];
  const DFilterPixel q = dfilter_pixel(a.rows, a.cols, a.tiles_x);
  for (int e = (int)threadIdx.x; e < EH * DFILTER_TILE_W; e += DFILTER_THREADS) {
    const int ey = e >> 6, ex = e & 63;
    const int y = min(max(q.y0 - DFILTER_MEAN_BEFORE + ey, 0), a.rows - 1), x = min(q.x0 + ex, a.cols - 1);
    s[e] = a.tmp[(size_t)y * (size_t)a.cols + (size_t)x];
  }
  __syncthreads();
  if (!q.in) return;
  const float* win = s + q.ly * DFILTER_TILE_W + q.lx;  // coordinate y - 4
  float o = a.in[q.p], d;
  if (q.x >= 3 && q.x <= a.cols - 4 && q.y >= 4 && q.y <= a.rows - 4 &&
      dfilter_mean(win, DFILTER_TILE_W, q.y - DFILTER_MEAN_BEFORE, win[DFILTER_MEAN_BEFORE * DFILTER_TILE_W], &d))
    o = d;
  a.out[q.p] = o;
}

}  // namespace cvo_dev
