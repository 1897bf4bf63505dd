// cvo_sgm_math.h -- the arithmetic of the stereo matcher (semi-global matching over a census cost) that decides something: one
// copy, compiled for the host (the CPU twin of cvo_sgm.hip) and for the device (the kernels of cvo_k_sgm.h), restated
// operation by operation in tests/np_sgm.py.  Integers throughout; the sub-pixel term's one float division and one float
// addition are the only float operations (the tree compiles with -ffp-contract=off, and both are IEEE on either side).
// Part of the kernel set of cvo_kernels.h.
#pragma once
#include "cvo_device.h"

namespace cvo_dev {

constexpr int SGM_CENSUS_W = 9, SGM_CENSUS_H = 7;  // the window: 62 neighbours, one 64-bit word per pixel
constexpr int SGM_HALO_X = SGM_CENSUS_W / 2, SGM_HALO_Y = SGM_CENSUS_H / 2;
constexpr int SGM_CENSUS_BITS = SGM_CENSUS_W * SGM_CENSUS_H - 1;  // the cost of a hypothesis whose right pixel is outside
constexpr int SGM_MAX_P2 = 255 - SGM_CENSUS_BITS;                  // 193: L <= 62 + p2 stays a byte
constexpr int SGM_MAX_PATHS = 8;
constexpr float SGM_INVALID = -10.f;                               // libelas's marker; cvo_stereo_points rejects it
constexpr unsigned SGM_NO_COST = 0xFFFFu;                          // above any S (<= 8 x 255 = 2040)

// the run-time constants of a call, from cvo_sgm_config_t
struct SgmConst {
  int rows, cols, D, p1, p2, uniqueness, lr_max_diff, paths;
};

// the directions (dv, du), in the order the contract numbers them
__host__ __device__ inline int sgm_dv(int dir) { return dir < 2 ? 0 : (dir == 2 || dir == 4 || dir == 5) ? 1 : -1; }
__host__ __device__ inline int sgm_du(int dir) { return dir == 0 ? 1 : dir == 1 ? -1 : dir < 4 ? 0 : (dir == 4 || dir == 6) ? 1 : -1; }

// lines of a direction: every pixel of the border the direction enters from starts one
__host__ __device__ inline int sgm_line_count(int dir, int rows, int cols) { return dir < 2 ? rows : dir < 4 ? cols : rows + cols - 1; }

// line i of a direction: its first pixel (v0, u0) and its length.  Horizontal: row i from the left / right edge; vertical:
// column i from the top / bottom edge; diagonal: i < cols starts in column i of the top / bottom row, the others in the
// left / right column, one row further in each.
__host__ __device__ inline void sgm_line(int dir, int i, int rows, int cols, int* v0, int* u0, int* len) {
  const int dv = sgm_dv(dir), du = sgm_du(dir);
  int v, u;
  if (dv == 0) {
    v = i;
    u = du > 0 ? 0 : cols - 1;
  } else if (du == 0 || i < cols) {
    v = dv > 0 ? 0 : rows - 1;
    u = i;
  } else {
    const int k = i - cols + 1;
    v = dv > 0 ? k : rows - 1 - k;
    u = du > 0 ? 0 : cols - 1;
  }
  const int nv = dv == 0 ? rows + cols : dv > 0 ? rows - v : v + 1;
  const int nu = du == 0 ? rows + cols : du > 0 ? cols - u : u + 1;
  *v0 = v;
  *u0 = u;
  *len = nv < nu ? nv : nu;
}

__host__ __device__ inline int sgm_popcount64(unsigned long long x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// C(v, u, d) from the two census words; in_image: u - d >= 0
__host__ __device__ inline int sgm_cost(unsigned long long cl, unsigned long long cr, bool in_image) {
  return in_image ? sgm_popcount64(cl ^ cr) : SGM_CENSUS_BITS;
}

// L(p, d) from the predecessor's L(q, d), L(q, d - 1), L(q, d + 1) (has_lo / has_hi: the neighbour exists) and m = min_k L(q, k)
__host__ __device__ inline int sgm_step(int c, int lq, int lq_lo, bool has_lo, int lq_hi, bool has_hi, int m, int p1, int p2) {
  int best = lq < m + p2 ? lq : m + p2;
  if (has_lo && lq_lo + p1 < best) best = lq_lo + p1;
  if (has_hi && lq_hi + p1 < best) best = lq_hi + p1;
  return c + best - m;
}

// the uniqueness rule: s1 the winner's sum, s2 the best sum more than one disparity away
__host__ __device__ inline bool sgm_ambiguous(int s1, int s2, int uniqueness) { return s2 * (100 - uniqueness) < s1 * 100; }

// the disparity of winner d with sums sm = S(d - 1), s1 = S(d), sp = S(d + 1) (sm, sp read only for 0 < d < D - 1)
__host__ __device__ inline float sgm_subpixel(int d, int D, int sm, int s1, int sp) {
  if (d <= 0 || d >= D - 1) return (float)d;
  const int den = sm + sp - 2 * s1;
  if (den <= 0) return (float)d;
  return (float)d + (float)(sm - sp) / (float)(2 * den);
}

__host__ __device__ inline bool sgm_lr_differs(int d_left, int d_right, int lr_max_diff) {
  const int diff = d_left > d_right ? d_left - d_right : d_right - d_left;
  return diff > lr_max_diff;
}

}  // namespace cvo_dev
