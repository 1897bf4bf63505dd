// cvo_k_rgbd_rows.h -- RGB-D front end, the rows of the kept pixels: the ONE copy of the row and exclusion arithmetic
// (CvoPointCloud.cpp:501-545, :614-618, :1237-1239) for the host routes, the CPU twin cvo_rgbd_frame_rows_host and the
// kernels of a frame whose planes are already in device memory (cvo_cloud_from_rgbd_device, cvo_rgbd.hip).
//
//   rgbd_excluded       the first maximum over a pixel's class scores is class 10; the scores are STRIDED (row, pixel and
//                       class stride in bytes), which covers H x W x C, C x H x W and a column slice of a wider tensor.
//   rgbd_gradient_at    gradient_[j] of the interleaved (dx, dy) array, computed where it is asked for.
//   rgbd_features       the channels + 2 features of the image constructor; rgbd_recipe_row: the drivers' recipe row.
//   RgbdKeepScores      RgbdKeep with the exclusion rule evaluated in keep(), for the candidates only: no exclusion plane.
//   RgbdHasDepth        count-only predicate of the ordered compaction: pixels with dep != 0 && !isnan(dep) (`with_depth`
//                       when semantics hide some pixels from the FULL pass's count) - k_compact_count's block reduction,
//                       k_compact_scan's sum in block order.
//   k_rgbd_rows         one block per 256 kept pixels: xyz, 5 features and the geometric type are computed by the pixel's
//                       lane, staged in LDS and written with consecutive lanes on consecutive floats; the 19 label floats
//                       of the block's rows (76 bytes a point) the same way, each read a gather through the pixel list.
//                       The arrays are the ones k_cloud_ingest reads (strides 12 / 20 / 76 / 8 bytes).
//
// Every value is exact or correctly rounded: the colour and the gradient are divided in DOUBLE and rounded to float once,
// int(f * 255) is a float product truncated; no statement here may contract into a multiply-add (the library is built
// with contraction off, the device divides in IEEE).  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_k_rgbd.h"

namespace cvo_dev {

constexpr int RGBD_ROW_THREADS = 256;
constexpr int RGBD_EXCLUDED_CLASS = 10;  // "unlabeled" (CvoPointCloud.cpp:501-507)

// the plane the gradient is taken of: the caller's gray plane, a 1-channel image, or the BGR image (gray per access)
struct GrayView {
  const unsigned char* p;
  int channels;
};

// class scores of a frame: the score of class c at pixel (v, u) is the float at base + v * row + u * pixel + c * cls
struct RgbdScores {
  const char* base;
  size_t row, pixel, cls;  // bytes
  int classes, w;
};

__host__ __device__ inline const char* rgbd_scores_at(const RgbdScores& s, size_t p) { return s.base + (p / (size_t)s.w) * s.row + (p % (size_t)s.w) * s.pixel; }
__host__ __device__ inline float rgbd_score(const char* at, const RgbdScores& s, int c) { return *(const float*)(at + (size_t)c * s.cls); }

// first maximum is class 10 (CvoPointCloud.cpp:501-507): `row[c] > row[best]` from best = 0, so a NaN never wins and equal
// scores keep the earlier class
__host__ __device__ inline bool rgbd_excluded(const RgbdScores& s, size_t p) {
  if (s.classes <= RGBD_EXCLUDED_CLASS) return false;  // (class 10 cannot win; no score is read)
  const char* at = rgbd_scores_at(s, p);
  int best = 0;
  float row_best = rgbd_score(at, s, 0);
  for (int c = 1; c < s.classes; c++) {
    const float v = rgbd_score(at, s, c);
    if (v > row_best) {
      best = c;
      row_best = v;
    }
  }
  return best == RGBD_EXCLUDED_CLASS;
}

// gradient_[j] of the interleaved (dx, dy) array (RawImage.cpp:55-82), computed where it is asked for
__host__ __device__ inline float rgbd_gradient_at(const GrayView& g, int w, int h, size_t j) {
  const size_t p = j >> 1;
  const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w);
  if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return 0.f;
  const size_t d = (j & 1) ? (size_t)w : 1;
  return 0.5f * ((float)rgbd_gray(g.p, g.channels, p + d) - (float)rgbd_gray(g.p, g.channels, p - d));
}

// what a row is made of: the planes (host pointers for the host routes and the twin, device pointers for the kernels)
struct RgbdRowFrame {
  int w, h, channels;
  const unsigned char* image;
  GrayView gray;
  const void* depth;
  int depth_type;
  RgbdCalib calib;
  RgbdScores scores;
};

__host__ __device__ inline void rgbd_xyz(const RgbdRowFrame& f, int p, float* xyz) {
  float dep = 0.f;
  (void)rgbd_depth(f.depth, f.depth_type, (size_t)p, &dep);
  rgbd_backproject(f.calib, p % f.w, p / f.w, dep, xyz);
}

// the channels + 2 features of the image constructor (CvoPointCloud.cpp:527-545).  The reference reads the interleaved
// gradient array at the PIXEL index (v w + u, v w + u + 1): reproduced.
__host__ __device__ inline void rgbd_features(const RgbdRowFrame& f, int p, float* out) {
  const int ch = f.channels;
  for (int c = 0; c < ch; c++) out[c] = (float)((double)(float)f.image[(size_t)p * ch + c] / 255.0);
  out[ch] = (float)((double)rgbd_gradient_at(f.gray, f.w, f.h, (size_t)p) / 500.0 + 0.5);
  out[ch + 1] = (float)((double)rgbd_gradient_at(f.gray, f.w, f.h, (size_t)p + 1) / 500.0 + 0.5);
}

// a row of the drivers' recipe: the first three image-constructor features through export_to_pcd's bytes
// (min(255, int(f * 255)), CvoPointCloud.cpp:1237-1239) and back through the (XYZRGB, GeometryType) constructor (:614-618);
// xyz may be null (a stereo frame has its coordinates already)
__host__ __device__ inline void rgbd_recipe_row(const RgbdRowFrame& f, int p, bool edge, float* xyz, float* feat5, float* geo) {
  float ft[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  rgbd_features(f, p, ft);
  if (xyz) rgbd_xyz(f, p, xyz);
  for (int c = 0; c < 3; c++) {
    const int i255 = (int)(ft[c] * 255);
    const int byte = i255 < 255 ? i255 : 255;
    feat5[c] = (float)((double)(float)byte / 255.0);
  }
  feat5[3] = feat5[4] = 0.f;
  geo[0] = edge ? 1.f : 0.f;
  geo[1] = edge ? 0.f : 1.f;
}

// which rows: the image constructor's (geometric type (t0, t1) of its method) or the recipe's
struct RgbdRowKind {
  int recipe;
  float t0, t1;
};

// one row as a resident cloud holds it: 5 features (a mono frame's 3 zero-padded)
__host__ __device__ inline void rgbd_row5(const RgbdRowFrame& f, const RgbdRowKind& k, int p, bool edge, float* xyz, float* feat5, float* geo) {
  if (k.recipe) {
    rgbd_recipe_row(f, p, edge, xyz, feat5, geo);
    return;
  }
  for (int c = 0; c < 5; c++) feat5[c] = 0.f;
  rgbd_features(f, p, feat5);  // (channels + 2 <= 5)
  rgbd_xyz(f, p, xyz);
  geo[0] = k.t0;
  geo[1] = k.t1;
}

// RgbdKeep for a frame whose class scores are on the device: the rule is evaluated for the candidates that have a depth
struct RgbdKeepScores {
  typedef RgbdKeep::Item Item;
  RgbdKeep base;  // (excl: nullptr)
  RgbdScores scores;
  __device__ bool keep(int i, int n, Item* c) const { return base.keep(i, n, c) && !rgbd_excluded(scores, (size_t)c->pix); }
  __device__ void write(unsigned at, const Item& c) const { base.write(at, c); }
};

// count only: the pixels with a depth
struct RgbdHasDepth {
  typedef int Item;
  const void* depth;
  int depth_type;
  __device__ bool keep(int i, int n, Item*) const {
    float dep;
    return i < n && rgbd_depth(depth, depth_type, (size_t)i, &dep);
  }
  __device__ void write(unsigned, const Item&) const {}
};

struct RgbdRowsOut {
  float *xyz, *feat, *label, *geo;  // n x 3, n x FD, n x NC (nullptr: a frame without classes), n x 2
};

// rows of the pixels pix[0 .. n): the first n_edge of a recipe are its edges.  A pixel outside the image (the compactions
// never write one) gives a row of zeros: nothing is read through it.
__global__ __launch_bounds__(RGBD_ROW_THREADS) void k_rgbd_rows(int n, int n_edge, const int* __restrict__ pix, RgbdRowFrame f, RgbdRowKind kind,
                                                                RgbdRowsOut o) {
  __shared__ int s_pix[RGBD_ROW_THREADS];
  __shared__ float s_xyz[3 * RGBD_ROW_THREADS], s_feat[FD * RGBD_ROW_THREADS], s_geo[2 * RGBD_ROW_THREADS];
  const int t = (int)threadIdx.x, i0 = blockIdx.x * RGBD_ROW_THREADS, i = i0 + t;
  const int rows = min(RGBD_ROW_THREADS, n - i0);
  int p = -1;
  float xyz[3] = {0.f, 0.f, 0.f}, ft[FD] = {0.f, 0.f, 0.f, 0.f, 0.f}, geo[2] = {0.f, 0.f};
  if (i < n) {
    p = pix[i];
    if ((unsigned)p >= (unsigned)(f.w * f.h)) p = -1;
    if (p >= 0) rgbd_row5(f, kind, p, i < n_edge, xyz, ft, geo);
  }
  s_pix[t] = p;
  for (int c = 0; c < 3; c++) s_xyz[3 * t + c] = xyz[c];
  for (int c = 0; c < FD; c++) s_feat[FD * t + c] = ft[c];
  s_geo[2 * t] = geo[0];
  s_geo[2 * t + 1] = geo[1];
  __syncthreads();
  for (int e = t; e < 3 * rows; e += RGBD_ROW_THREADS) o.xyz[3 * (size_t)i0 + e] = s_xyz[e];
  for (int e = t; e < FD * rows; e += RGBD_ROW_THREADS) o.feat[FD * (size_t)i0 + e] = s_feat[e];
  for (int e = t; e < 2 * rows; e += RGBD_ROW_THREADS) o.geo[2 * (size_t)i0 + e] = s_geo[e];
  if (!o.label) return;
  for (int e = t; e < NC * rows; e += RGBD_ROW_THREADS) {
    const int r = e / NC, c = e - NC * r, q = s_pix[r];
    o.label[NC * (size_t)i0 + e] = (q >= 0 && c < f.scores.classes) ? rgbd_score(rgbd_scores_at(f.scores, (size_t)q), f.scores, c) : 0.f;
  }
}

}  // namespace cvo_dev
