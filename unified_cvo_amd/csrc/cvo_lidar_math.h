// cvo_lidar_math.h -- the arithmetic of the LiDAR front end that decides something: one copy, compiled for the host (the CPU
// twin of cvo_lidar.hip) and for the device (the kernels of cvo_k_lidar.h), restated operation by operation in
// tests/np_lidar.py.  No libm call decides anything here: the one angle a decision needs (the column of a return) comes from
// lidar_atan2_deg, built from IEEE add / multiply / divide in double in a fixed order (the tree compiles with
// -ffp-contract=off); every other angle test of LeGoLoamPointSelection.cpp is cross-multiplied against constants that
// cvo_lidar_config_derive computes once (LidarConst).  Part of the kernel set of cvo_kernels.h.
#pragma once
#include <cfloat>

#include "cvo_device.h"

namespace cvo_dev {

constexpr int LIDAR_MAX_SCAN = 128;       // rows of the range image: a component's row mask is 128 bits
constexpr int LIDAR_MAX_HORIZON = 4096;   // columns: a ring's suppression flags and a sixth's sort live in LDS
constexpr int LIDAR_MAX_POINTS = 1 << 24;
constexpr int LIDAR_SIXTHS = 6;           // sectionsTotal
constexpr int LIDAR_EDGE_CAP = 20;        // edge picks per sixth
constexpr int LIDAR_BIG_SEGMENT = 30;     // a component of this many cells is valid whatever its rows

// the run-time constants of a call, from cvo_lidar_config_t (doubles: cvo_lidar_config_derive)
struct LidarConst {
  int R, H, ground_rows, valid_points, valid_lines;
  float ang_res_x, min_range, edge_thr;
  double tan_theta, sin_ax, cos_ax, sin_ay, cos_ay, tan_g_lo, tan_g_hi, tan_s_lo, tan_s_hi;
};

// LeGoLoamPointSelection::get_quadrant of (x, z) in upstream's axes: u = z, v = -x
__host__ __device__ inline int lidar_quadrant(float x, float z) {
  const float u = z, v = -x;
  if (u > 0 && v >= 0) return 1;
  if (u <= 0 && v > 0) return 2;
  if (u < 0 && v <= 0) return 3;
  if (u >= 0 && v < 0) return 4;
  return 0;
}

// atan2(y, x) in degrees.  |error| < 1e-7 degrees (truncation of the series < 2.6e-8 degrees at |t| <= tan(pi/8), the
// roundings of ~20 double operations far below that); exact on the axes; (0, 0) is 0.  a = min / max of the magnitudes
// in [0, 1]; above tan(pi/8) the argument is folded with atan a = pi/4 + atan((a - 1) / (a + 1)); the odd Taylor series
// to t^19 in Horner form; then the octant.
__host__ __device__ inline double lidar_atan2_deg(double y, double x) {
  const double ay = y < 0 ? -y : y, ax = x < 0 ? -x : x;
  const double hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
  if (hi == 0.0) return 0.0;
  const double a = lo / hi;
  double t = a, base = 0.0;
  if (a > 0.41421356237309503) {
    t = (a - 1.0) / (a + 1.0);
    base = 45.0;
  }
  const double s = t * t;
  double p = -1.0 / 19.0;
  p = p * s + 1.0 / 17.0;
  p = p * s + -1.0 / 15.0;
  p = p * s + 1.0 / 13.0;
  p = p * s + -1.0 / 11.0;
  p = p * s + 1.0 / 9.0;
  p = p * s + -1.0 / 7.0;
  p = p * s + 1.0 / 5.0;
  p = p * s + -1.0 / 3.0;
  p = p * s + 1.0;
  double d = base + (p * t) * 57.295779513082323;  // atan(lo / hi) in degrees, 0 .. 45
  if (ay > ax) d = 90.0 - d;
  if (x < 0) d = 180.0 - d;
  return y < 0 ? -d : d;
}

// the square root of a float, correctly rounded: through the double root, whose second rounding is harmless (53 >= 2 * 24 + 2)
__host__ __device__ inline float lidar_sqrtf(float v) { return (float)sqrt((double)v); }

__host__ __device__ inline float lidar_range(float x, float y, float z) { return lidar_sqrtf(x * x + y * y + z * z); }

// projectPointCloud's column: horizonAngle = float(atan2(z, -x) in degrees), -round((h - 90) / ang_res_x) + H / 2, wrapped
// once; -1: outside the image.  round() is half away from zero.
__host__ __device__ inline int lidar_column(float x, float z, float ang_res_x, int H) {
  const float h = (float)lidar_atan2_deg((double)z, (double)(-x));
  const double q = ((double)h - 90.0) / (double)ang_res_x;
  const double r = q < 0 ? -floor(-q + 0.5) : floor(q + 0.5);
  double c = -r + (double)(H / 2);
  if (c >= (double)H) c -= (double)H;
  if (!(c >= 0.0) || c >= (double)H) return -1;
  return (int)c;
}

// groundRemoval's test of a column's cells in rows i (lower) and i + 1 (upper): the slope between them within 10 degrees of
// the mount angle and the lower return itself more than 3 degrees off it, as tangents: tan_lo * h <= dy <= tan_hi * h
__host__ __device__ inline bool lidar_ground_pair(const float* lo, const float* up, const LidarConst& k) {
  const float dx = up[0] - lo[0], dy = up[1] - lo[1], dz = up[2] - lo[2];
  const double h = sqrt((double)(dx * dx + dz * dz));
  const bool slope = (double)dy <= k.tan_g_hi * h && (double)dy >= k.tan_g_lo * h;
  const double hs = sqrt((double)(lo[0] * lo[0] + lo[2] * lo[2]));
  const bool self_off = (double)lo[1] > k.tan_s_hi * hs || (double)lo[1] < k.tan_s_lo * hs;
  return slope && self_off;
}

// labelComponents' neighbour criterion, atan2(d2 sin a, d1 - d2 cos a) > theta with d1 >= d2 > 0 the two ranges, as
// y > tan(theta) x for x > 0; x <= 0 with y > 0 is true, y <= 0 with x <= 0 false.  Symmetric in the ranges.
__host__ __device__ inline bool lidar_connected(float ra, float rb, bool same_row, const LidarConst& k) {
  const double d1 = (double)(ra > rb ? ra : rb), d2 = (double)(ra > rb ? rb : ra);
  const double y = d2 * (same_row ? k.sin_ax : k.sin_ay), x = d1 - d2 * (same_row ? k.cos_ax : k.cos_ay);
  if (x > 0.0) return y > k.tan_theta * x;
  return y > 0.0;
}

// a component of `size` cells whose members other than its seed lie in the rows of mask[4]
__host__ __device__ inline bool lidar_segment_valid(unsigned size, const unsigned* mask, const LidarConst& k) {
  if (size >= (unsigned)LIDAR_BIG_SEGMENT) return true;
  if (size < (unsigned)k.valid_points) return false;
  int rows = 0;
  for (int w = 0; w < 4; w++) {
    unsigned m = mask[w];
    for (; m; m &= m - 1) rows++;
  }
  return rows >= k.valid_lines;
}

// calculateSmoothness: cloudCurvature[i], 0 outside [5, S - 5) (never written upstream)
__host__ __device__ inline float lidar_curvature(const float* r, int i, int S) {
  if (i < 5 || i >= S - 5) return 0.f;
  const float d = r[i - 5] + r[i - 4] + r[i - 3] + r[i - 2] + r[i - 1] - r[i] * 10.f + r[i + 1] + r[i + 2] + r[i + 3] + r[i + 4] + r[i + 5];
  return d * d;
}

// markOccludedPoints as a gather: what iteration i of its loop writes, asked of position k
__host__ __device__ inline int lidar_col_gap(const int* col, int a, int b) {
  const int d = col[a] - col[b];
  return d < 0 ? -d : d;
}
__host__ __device__ inline bool lidar_occluded(const float* r, const int* col, int k, int S) {
  const int lo = 5, hi = S - 6;  // i in [lo, hi)
  for (int i = (k > lo ? k : lo); i <= k + 5 && i < hi; i++)  // depth1 - depth2 > 0.3 marks i - 5 .. i
    if (lidar_col_gap(col, i + 1, i) < 10 && (double)(r[i] - r[i + 1]) > 0.3) return true;
  for (int i = (k - 6 > lo ? k - 6 : lo); i <= k - 1 && i < hi; i++)  // else depth2 - depth1 > 0.3 marks i + 1 .. i + 6
    if (lidar_col_gap(col, i + 1, i) < 10 && !((double)(r[i] - r[i + 1]) > 0.3) && (double)(r[i + 1] - r[i]) > 0.3) return true;
  if (k >= lo && k < hi) {
    const float d1 = fabsf(r[k - 1] - r[k]), d2 = fabsf(r[k + 1] - r[k]);
    if ((double)d1 > 0.02 * (double)r[k] && (double)d2 > 0.02 * (double)r[k]) return true;
  }
  return false;
}

// extractFeatures' range of sixth j of a ring whose segmented points are [before, after): start = before + 4,
// end = after - 6, C's truncating division
__host__ __device__ inline void lidar_sixth(int before, int after, int j, int* sp, int* ep) {
  const int s = before + 4, e = after - 6;
  *sp = (s * (6 - j) + e * j) / 6;
  *ep = (s * (5 - j) + e * (j + 1)) / 6 - 1;
}

}  // namespace cvo_dev
