// cvo_depth_math.h -- the arithmetic of the keyframe depth filter (the last loops of main_depth_filtering.cpp:245-294) that
// the CPU twin (cvo_depth.hip: cvo_depth_filter_accumulate_host / _finish_host) and the kernels (cvo_k_depth.h) share, so
// that the two cannot drift: the depth of an associated point in the keyframe's frame, the fold of one observation into a
// row's accumulators, and the finish of one row.  tests/np_depthfilter.py states the same in numpy float32.  Everything here is
// plain float arithmetic, every product and sum rounded on its own (the build compiles with -ffp-contract=off; the division
// is IEEE's: hipcc's default for float), in the order the statement fixes.
#pragma once

namespace cvo_dev {

enum : int { DEPTH_DROP = 0, DEPTH_KEEP = 1, DEPTH_NONFINITE = 2 };  // what depth_finish_row says of a row

// row 2 of the 4x4 T_depth (column-major as every transform of the C-ABI): the only part of it the filter reads
struct DepthRow {
  float m0, m1, m2, m3;
};
__host__ __device__ inline DepthRow depth_row(const float T_colmajor[16]) {
  return DepthRow{T_colmajor[2], T_colmajor[6], T_colmajor[10], T_colmajor[14]};
}

// zj = T(2,0) x + T(2,1) y + T(2,2) z + T(2,3): CvoPointCloud::transform's expression for the third coordinate, three
// products added left to right
__host__ __device__ inline float depth_zj(const DepthRow& t, float x, float y, float z) {
  const float px = t.m0 * x, py = t.m1 * y, pz = t.m2 * z;
  return ((px + py) + pz) + t.m3;
}

// one observation (depth zj, weight a) into a row's accumulators: depths[idx1].push_back / weights[idx1].push_back, summed
// in push order
__host__ __device__ inline void depth_fold(float& depth_sum, float& weight_sum, int& count, float zj, float a) {
  const float p = zj * a;
  depth_sum = depth_sum + p;
  weight_sum = weight_sum + a;
  count = count + 1;
}

// The finish of one row with the keyframe point p: DEPTH_DROP - count <= min_count, nothing is written; else *d = the
// refined depth and out = (p / p.z) * d, DEPTH_KEEP when all four are finite, DEPTH_NONFINITE otherwise (p.z == 0, a zero
// weight: upstream's text pins nothing there; the library drops the row and counts it).
__host__ __device__ inline int depth_finish_row(float depth_sum, float weight_sum, int count, int min_count, const float p[3],
                                                float out[3], float* d) {
  if (!(count > min_count)) return DEPTH_DROP;
  const float z0 = p[2];
  const float wbar = weight_sum / (float)count;
  const float zw = z0 * wbar;
  float dd = depth_sum + zw;
  const float w = weight_sum + wbar;
  dd = dd / w;
  bool ok = __builtin_isfinite(dd);
  for (int k = 0; k < 3; k++) {
    const float q = p[k] / z0;
    out[k] = q * dd;
    ok = ok && __builtin_isfinite(out[k]);
  }
  *d = dd;
  return ok ? DEPTH_KEEP : DEPTH_NONFINITE;
}

}  // namespace cvo_dev
