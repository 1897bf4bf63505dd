// cvo_dfilter_math.h -- the arithmetic of the disparity post-filter (libelas's removeSmallSegments, gapInterpolation and
// adaptiveMean, full-resolution branch) that decides something: one copy, compiled for the host (the CPU twin of
// cvo_dfilter.hip) and for the device (the kernels of cvo_k_dfilter.h), restated operation by operation in tests/np_dfilter.py.
// Every float operation is a single IEEE subtraction, addition, multiplication or division (the tree compiles with
// -ffp-contract=off, so no multiply is fused into the add that follows it).  Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_device.h"

namespace cvo_dev {

constexpr float DFILTER_INVALID = -10.f;          // libelas's marker, the matcher's too (SGM_INVALID)
constexpr float DFILTER_DISCONTINUITY = 3.f;      // gapInterpolation's discon_threshold
constexpr unsigned DFILTER_ABS_BITS = 0x4F000000u;  // the bit pattern of (float)0x7FFFFFFF: adaptiveMean's "absolute mask"
constexpr int DFILTER_MEAN_BEFORE = 4, DFILTER_MEAN_AFTER = 3;  // the window: centre - 4 .. centre + 3

// the run-time constants of a call, from cvo_dfilter_config_t
struct DFilterConst {
  int rows, cols;
  float sim;
  int speckle_size, gap_width, mean;
};

__host__ __device__ inline bool dfilter_valid(float v) { return v >= 0.f; }

// speckle: a 4-neighbour of a valid pixel joins its segment (equality joins)
__host__ __device__ inline bool dfilter_similar(float a, float b, float sim) { return __builtin_fabsf(a - b) <= sim; }

// gap: the value a run bounded by d1 (before) and d2 (after) is filled with
__host__ __device__ inline float dfilter_fill(float d1, float d2) {
  if (__builtin_fabsf(d1 - d2) < DFILTER_DISCONTINUITY) return (d1 + d2) / 2.f;
  return d2 < d1 ? d2 : d1;
}

// mean: the weight of a window value against the centre's.  The mask keeps five exponent bits and no mantissa bit, so the
// masked difference is 0 or a power of two: the weight is 4 below |val - cur| = 2, 2 in [2, 8) and 0 from 8 on (until the
// exponent's bit 5 comes into play, at 2^33).
__host__ __device__ inline float dfilter_weight(float val, float cur) {
  const float t = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, val - cur) & DFILTER_ABS_BITS);
  const float w = 4.f - t;
  return w > 0.f ? w : 0.f;
}

// mean: one output.  win[o * stride], o = 0 .. 7, is the value at coordinate first + o along the pass (first = centre - 4);
// cur is the centre's.  libelas keeps the window in a ring indexed by coordinate mod 8 and adds slot k to slot k + 4 before the
// four lanes are summed from the left, so the order of the additions depends on the coordinate.  False: nothing is written.
__host__ __device__ inline bool dfilter_mean(const float* win, int stride, int first, float cur, float* d) {
  float wl[4], fl[4];
  for (int k = 0; k < 4; k++) {
    const int oa = (k - first) & 7, ob = (oa + 4) & 7;  // where the values of slots k and k + 4 are
    const float va = win[oa * stride], vb = win[ob * stride];
    const float wa = dfilter_weight(va, cur), wb = dfilter_weight(vb, cur);
    const float fa = va * wa, fb = vb * wb;
    wl[k] = wa + wb;
    fl[k] = fa + fb;
  }
  const float weight_sum = ((wl[0] + wl[1]) + wl[2]) + wl[3];
  const float factor_sum = ((fl[0] + fl[1]) + fl[2]) + fl[3];
  if (!(weight_sum > 0.f)) return false;
  const float q = factor_sum / weight_sum;
  if (!(q >= 0.f)) return false;
  *d = q;
  return true;
}

}  // namespace cvo_dev
