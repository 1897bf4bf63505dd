// cvo_k_stereo.h -- stereo front end: from candidate pixels and a disparity map to the points of
// CvoPointCloud(ImageStereo, Calibration, method) (CvoPointCloud.cpp:680-773, StaticStereo.cpp:84-107, is_good_point :39-49).
//
//   StereoKeep          predicate of the ordered compaction (cvo_k_compact.h): the keep predicate and the back-projection
//                       over a pixel list - FAST's row-major list, a DSO selection - or over FULL's column-major order
//                       (list == nullptr); writes the pixel index and xyz of the survivors.  The candidates come from
//                       cvo_k_fast.h / cvo_k_rgbd.h.
//
// stereo_point IS the contract's arithmetic, shared with the CPU twin: every product and sum is rounded on its own (the
// translation unit is compiled with -ffp-contract=off, and the pragma below holds where it is not), the division is IEEE,
// and `norm >= 55` is decided on the squared norm against the smallest float whose correctly rounded root reaches 55
// (StereoCalib::far2, found on the host), so no device sqrtf takes part.  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_k_rgbd.h"

namespace cvo_dev {

// Eigen 3.3's size-3 cofactor inverse of K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (the entries that are not zero), the
// product |baseline| fx, and far2 (see above); stereo_calib (cvo_stereo.hip) fills it
struct StereoCalib {
  float k00, k11, k02, k12, k22, bf, far2;
};

constexpr float STEREO_MIN_DISPARITY = 0.05f;  // `disparity <= 0.05` in double rejects exactly disparity < 0.05f
constexpr int STEREO_TOP = 100, STEREO_BOTTOM = 30;  // is_good_point keeps 100 <= v <= h - 30: nothing in a frame of fewer than 130 rows

// whether the reference keeps pixel (u, v) with disparity disp, and its xyz.  A NaN disparity passes every test.
__host__ __device__ inline bool stereo_point(const StereoCalib& k, int u, int v, int w, int h, float disp, float* xyz) {
#pragma clang fp contract(off)
  if (u < 1 || u > w - 2 || v < 1 || v > h - 2) return false;  // pt_depth_from_disparity: OOB
  if (disp < STEREO_MIN_DISPARITY) return false;                // ... OUTLIER
  if (u < 2 || u > w - 2 || v < STEREO_TOP || v > h - STEREO_BOTTOM) return false;  // is_good_point
  const float depth = k.bf / disp;
  const float x = (k.k00 * (float)u + k.k02) * depth, y = (k.k11 * (float)v + k.k12) * depth, z = k.k22 * depth;
  if ((x * x + y * y) + z * z >= k.far2) return false;
  xyz[0] = x;
  xyz[1] = y;
  xyz[2] = z;
  return true;
}

// candidate i of a pass: pixel list[i], or - list == nullptr, FULL - the i-th pixel in column-major order
__device__ __forceinline__ bool stereo_candidate(int i, int n, const int* __restrict__ list, int w, int h, const float* __restrict__ disparity,
                                                 const unsigned char* __restrict__ excl, const StereoCalib& k, int* pix, float* xyz) {
  if (i >= n) return false;
  const int p = list ? list[i] : (i % h) * w + i / h;
  *pix = p;
  if ((unsigned)p >= (unsigned)(w * h)) return false;
  return stereo_point(k, p % w, p / w, w, h, disparity[p], xyz) && !(excl && excl[p]);
}

struct StereoKeep {
  struct Item {
    int pix;
    float p[3];
  };
  const int* list;
  int w, h;
  const float* disparity;
  const unsigned char* excl;
  StereoCalib calib;
  int* pix_out;
  float* xyz;
  __device__ bool keep(int i, int n, Item* c) const { return stereo_candidate(i, n, list, w, h, disparity, excl, calib, &c->pix, c->p); }
  __device__ void write(unsigned at, const Item& c) const {
    pix_out[at] = c.pix;
    xyz[3 * (size_t)at] = c.p[0];
    xyz[3 * (size_t)at + 1] = c.p[1];
    xyz[3 * (size_t)at + 2] = c.p[2];
  }
};

}  // namespace cvo_dev
