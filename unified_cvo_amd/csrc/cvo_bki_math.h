// cvo_bki_math.h -- the arithmetic of the semantic voxel map (semantic_bki::SemanticBKIOctoMap under its counting sensor
// model, block_depth = 1) that the CPU twin (cvo_bki_twin.h) and the kernels (cvo_k_bki.h) share, so that the two cannot drift:
// the block index of a coordinate, the closed float box of a block, the beam samples of a hit, the class of a label row, the
// state of a voxel and the rows of the cloud read out - and, for the sparse kernel, the weight with its own sin / cos routine
// and the neighbour slots.  tests/np_bki.py and tests/np_bki_sparse.py state the same in numpy.  Everything here is plain
// float / double arithmetic without fused multiply-adds (the build compiles with -ffp-contract=off).  A host compiler takes
// this header too (for cvo_bki_twin.h; cvo_host_attrs.h).
#pragma once
#include <cmath>

#include "cvo_host_attrs.h"

namespace cvo_dev {

constexpr int BKI_KOFF = 524288;                // block index 524288 is the block centred on 0
constexpr double BKI_K0_LO = 1.0;               // k0 in [1, 2^20 - 2]: k0 - 1 .. k0 + 1 fit the key's 20-bit fields
constexpr double BKI_K0_HI = 1048575.0;         // (exclusive bound of the double before it is truncated)
constexpr int BKI_MAX_CLASSES = 19;             // C of the configuration: 0 .. 19 (a cloud's label row)
constexpr int BKI_FEAT = 5;
// training points of ONE insert (hits that max_range keeps, their beam samples, the origin): below 2^24 every class count of
// an insert is an exact float and a beam's running sum d always grows
constexpr long long BKI_MAX_TRAINING = 1ll << 24;
constexpr int BKI_MAX_RAY = 65536;              // ... and l / free_resolution of one hit stays below this (a lane walks a beam alone)
enum : int { BKI_FREE = 0, BKI_OCCUPIED = 1, BKI_UNKNOWN = 2 };
enum : unsigned { BKI_BAD_RANGE = 1, BKI_BAD_TOO_MANY = 2, BKI_BAD_INTERNAL = 4 };

struct BkiConst {
  float size, half;  // Block::size = resolution at block_depth 1; half = size / 2.0f
  float prior, free_thresh, occupied_thresh, free_resolution, max_range;
  int C;       // classes of a label row; 0: clouds without labels (the extension: every hit is class 1)
  int nclass;  // classes of the map: max(C, 1) + 1, class 0 = free space
};

// k0 = int64(p / (double)size + 524288.5); false: outside [1, 2^20 - 2] (p is finite)
__host__ __device__ inline bool bki_k0(float p, float size, long long* k0) {
  const double q = (double)p / (double)size + 524288.5;
  if (!(q >= BKI_K0_LO && q < BKI_K0_HI)) return false;
  *k0 = (long long)q;
  return true;
}

// upstream's closed box of block k on one axis: c - h <= p <= c + h in float, c = float(k - 524288) * size
__host__ __device__ inline float bki_centre(long long k, float size) { return (float)(k - BKI_KOFF) * size; }
__host__ __device__ inline bool bki_holds(long long k, float p, float size, float half) {
  const float c = bki_centre(k, size);
  return c - half <= p && p <= c + half;
}

// the centre of block `key` on one axis, its 20-bit index unpacked (THE place that knows the key's layout backwards), and on all three
__host__ __device__ inline float bki_key_centre1(unsigned long long key, int axis, float size) {
  return bki_centre((long long)(axis == 0 ? key >> 40 : (axis == 1 ? (key >> 20) & 0xFFFFFull : key & 0xFFFFFull)), size);
}
__host__ __device__ inline void bki_key_centre(unsigned long long key, float size, float out[3]) {
  out[0] = bki_key_centre1(key, 0, size);
  out[1] = bki_key_centre1(key, 1, size);
  out[2] = bki_key_centre1(key, 2, size);
}

// the blocks of k0 - 1, k0, k0 + 1 that hold p on one axis, ascending; returns how many (0: p lies in a rounding gap)
__host__ __device__ inline int bki_axis(float p, long long k0, float size, float half, unsigned ks[3]) {
  int n = 0;
  for (long long k = k0 - 1; k <= k0 + 1; k++)
    if (bki_holds(k, p, size, half)) ks[n++] = (unsigned)k;
  return n;
}

__host__ __device__ inline unsigned long long bki_key(unsigned kx, unsigned ky, unsigned kz) {
  return ((unsigned long long)kx << 40) | ((unsigned long long)ky << 20) | (unsigned long long)kz;
}

// f(key) for every block that holds (x, y, z), x-major then y then z, each axis ascending.  Returns the number of blocks, or
// -1 when a k0 leaves its range (nothing is visited then).
template <class F>
__host__ __device__ inline int bki_members(const BkiConst& k, float x, float y, float z, F&& f) {
  long long k0x, k0y, k0z;
  if (!bki_k0(x, k.size, &k0x) || !bki_k0(y, k.size, &k0y) || !bki_k0(z, k.size, &k0z)) return -1;
  unsigned ax[3], ay[3], az[3];
  const int nx = bki_axis(x, k0x, k.size, k.half, ax), ny = bki_axis(y, k0y, k.size, k.half, ay), nz = bki_axis(z, k0z, k.size, k.half, az);
  for (int a = 0; a < nx; a++)
    for (int b = 0; b < ny; b++)
      for (int c = 0; c < nz; c++) f(bki_key(ax[a], ay[b], az[c]));
  return nx * ny * nz;
}

// float sum of squares of the float differences, left to right
__host__ __device__ inline float bki_dist2(const float p[3], const float o[3]) {
  const float dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
  return dx * dx + dy * dy + dz * dz;
}

// max_range > 0 drops a hit when sqrt((double)s) > max_range, s = bki_dist2.  Decided without a square root: for a float s
// and a float R the double R * R is exact (48 bits), and a float s that differs from it differs by more than the 2^-52
// relative width within which the rounded double root could still equal R - so the rounded root exceeds R exactly when s
// exceeds R * R.
__host__ __device__ inline bool bki_in_range(const BkiConst& k, const float p[3], const float o[3]) {
  if (!(k.max_range > 0.f)) return true;
  return !((double)bki_dist2(p, o) > (double)k.max_range * (double)k.max_range);
}

// The training points of one kept hit, in upstream's order: f(x, y, z, true) for the hit, then f(x, y, z, false) for each
// of its beam samples - d the running float sum fr, fr + fr, ... while d < l, then one more at l - fr when l > fr; each
// sample origin + n * d with a separate multiply and add.  f returns false to stop.  Returns false when the ray would need
// BKI_MAX_RAY samples or more (nothing is visited then), or when f stopped.  l = 0 (hit == origin): no samples, the
// NaN direction is never used.
template <class F>
__host__ __device__ inline bool bki_hit_points(const BkiConst& k, const float p[3], const float o[3], unsigned* too_many, F&& f) {
  const float fr = k.free_resolution;
  const float l = sqrtf(bki_dist2(p, o));  // (the double root rounded to float is the same number)
  if (!(l / fr < (float)BKI_MAX_RAY)) return *too_many = 1, false;
  if (!f(p[0], p[1], p[2], true)) return false;
  const float nx = (p[0] - o[0]) / l, ny = (p[1] - o[1]) / l, nz = (p[2] - o[2]) / l;
  for (float d = fr; d < l; d += fr)
    if (!f(o[0] + nx * d, o[1] + ny * d, o[2] + nz * d, false)) return false;
  if (l > fr) {
    const float d = l - fr;
    if (!f(o[0] + nx * d, o[1] + ny * d, o[2] + nz * d, false)) return false;
  }
  return true;
}

// class of a hit: 1 + the first maximum of its label row (C = 0: 1)
__host__ __device__ inline int bki_class(const float* label, int C) {
  int best = 0;
  for (int c = 1; c < C; c++)
    if (label[c] > label[best]) best = c;
  return 1 + best;
}

// sequential float sum of ms[from .. nclass)
__host__ __device__ inline float bki_sum(const float* ms, int from, int nclass) {
  float s = 0.f;
  for (int c = from; c < nclass; c++) s += ms[c];
  return s;
}

// the state, a function of ms alone: probs = ms / sum(ms); first maximum class 0 -> FREE; else p = 1 - probs[0]:
// OCCUPIED above occupied_thresh, FREE below free_thresh, UNKNOWN between
__host__ __device__ inline int bki_state(const BkiConst& k, const float* ms) {
  const float sum = bki_sum(ms, 0, k.nclass);
  const float p0 = ms[0] / sum;
  float best = p0;
  bool free_wins = true;
  for (int c = 1; c < k.nclass; c++) {
    const float pc = ms[c] / sum;
    if (pc > best) best = pc, free_wins = false;
  }
  if (free_wins) return BKI_FREE;
  const float p = 1.f - p0;
  return p > k.occupied_thresh ? BKI_OCCUPIED : (p < k.free_thresh ? BKI_FREE : BKI_UNKNOWN);
}

// the row of an occupied voxel in the cloud read out: its centre, fs / sum(ms[1:]), ms[1 .. C] / sum(ms)
__host__ __device__ inline void bki_row(const BkiConst& k, unsigned long long key, const float* ms, const float* fs, float* xyz, float* feat, float* label) {
  if (xyz) bki_key_centre(key, k.size, xyz);
  if (feat) {
    const float occ = bki_sum(ms, 1, k.nclass);
    for (int c = 0; c < BKI_FEAT; c++) feat[c] = fs[c] / occ;
  }
  if (label) {
    const float sum = bki_sum(ms, 0, k.nclass);
    for (int c = 1; c <= k.C; c++) label[c - 1] = ms[c] / sum;
  }
}

// ---- the sparse kernel (SemanticBKInference::predict / covSparse, get_extended_block; tests/np_bki_sparse.py) ----

// memberships (work records) of ONE insert under the sparse kernel: the device sorts that many (key, record) pairs
constexpr long long BKI_SPARSE_MAX_RECORDS = 1ll << 24;
constexpr int BKI_SPARSE_SLOTS = 7;         // a voxel's neighbour slots: self, +x, -x, +y, -y, +z, -z
constexpr float BKI_SPARSE_PI = 3.1415926f;  // upstream's constant
constexpr float BKI_SPARSE_FAR = 1.5f;      // from this distance on (in units of ell) the weight is 0 without being evaluated

// the block in neighbour slot j of `key`, get_extended_block's order; false: the index leaves the key's 20-bit field
__host__ __device__ inline bool bki_sparse_slot(unsigned long long key, int j, unsigned long long* out) {
  if (j == 0) return *out = key, true;
  const int shift = 40 - 20 * ((j - 1) / 2);
  const long long k = (long long)((key >> shift) & 0xFFFFFull) + ((j & 1) ? 1 : -1);
  if (k < 0 || k > 0xFFFFFll) return false;
  *out = (key & ~(0xFFFFFull << shift)) | ((unsigned long long)k << shift);
  return true;
}

// sin and cos of a in [0, 3 pi), the statement's routine operation for operation: the quarter turn q nearest to a, r = a - q pi/2
// in three steps (the first two exact), a polynomial each in z = r * r on |r| <= pi/4 by Horner's rule with separate
// multiplies and adds, the quadrant's signs and swap.  cos 0 = 1 and sin 0 = 0 exactly.
__host__ __device__ inline void bki_sparse_sincos(float a, float* s, float* c) {
  const int q = (int)(a * 0.63661977f + 0.5f);
  const float fq = (float)q;
  float r = a - fq * 1.5703125f;
  r = r - fq * 4.837512969970703125e-4f;
  r = r - fq * 7.54978995489188216e-8f;
  const float z = r * r;
  const float ps = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
  const float pc = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z - 0.5f * z + 1.0f;
  const float s0 = (q & 1) ? pc : ps, c0 = (q & 1) ? ps : pc;
  *s = (q & 2) ? -s0 : s0;
  *c = ((q + 1) & 2) ? -c0 : c0;
}

// covSparse of one (voxel centre, training point) pair: d = |centre / ell - p / ell|, the squares summed left to right,
// k = ((2 + cos 2 pi d)(1 - d) / 3 + sin 2 pi d / (2 pi)) sf2, negative values 0
__host__ __device__ inline float bki_sparse_k(const float centre[3], const float p[3], float sf2, float ell) {
  const float dx = centre[0] / ell - p[0] / ell, dy = centre[1] / ell - p[1] / ell, dz = centre[2] / ell - p[2] / ell;
  const float d = sqrtf(dx * dx + dy * dy + dz * dz);
  if (d >= BKI_SPARSE_FAR) return 0.f;
  const float a = d * 2.0f * BKI_SPARSE_PI;
  float s, c;
  bki_sparse_sincos(a, &s, &c);
  const float k = ((2.0f + c) * (1.0f - d) / 3.0f + s / (2.0f * BKI_SPARSE_PI)) * sf2;
  return k < 0.f ? 0.f : k;
}

// ---- the read side (tests/np_bki_query.py): a voxel as upstream's node getters answer for it (SemanticBKIOctoMap::search,
// Semantics::get_probs / get_vars / get_features), and the library's own ray walk ----

enum : int { BKI_Q_ABSENT = 0, BKI_Q_FOUND = 1, BKI_Q_OUTSIDE = 2 };  // `found` of a point query
enum : unsigned { BKI_BIT_FREE = 1, BKI_BIT_OCCUPIED = 2, BKI_BIT_UNKNOWN = 4, BKI_BIT_ABSENT = 8 };  // a voxel in a stop mask
enum : int { BKI_RAY_END = 0, BKI_RAY_STOPPED = 1, BKI_RAY_TOO_LONG = 2, BKI_RAY_OUTSIDE = 3 };
constexpr int BKI_RAY_MAX_STEPS = 1 << 20;      // voxels of one ray
constexpr long long BKI_RENDER_MAX_PIXELS = 1ll << 24;
constexpr unsigned long long BKI_NO_KEY = ~0ull;  // the key of a ray that walked nothing

// the one NaN the read side writes (the centre of a point outside the key range, of a ray that walked nothing)
__host__ __device__ inline float bki_nan() { return __builtin_bit_cast(float, 0x7fc00000u); }
// ... and the centre a read answers with: the voxel's, or that NaN three times
__host__ __device__ inline void bki_key_centre_or_nan(bool valid, unsigned long long key, float size, float out[3]) {
  out[0] = valid ? bki_key_centre1(key, 0, size) : bki_nan();
  out[1] = valid ? bki_key_centre1(key, 1, size) : bki_nan();
  out[2] = valid ? bki_key_centre1(key, 2, size) : bki_nan();
}

// the voxel of a point: the key of its k0 per axis (block_to_hash_key); false: not finite, or a k0 outside [1, 2^20 - 2]
__host__ __device__ inline bool bki_point_key(float x, float y, float z, float size, unsigned long long* key) {
  long long kx, ky, kz;
  if (!bki_k0(x, size, &kx) || !bki_k0(y, size, &ky) || !bki_k0(z, size, &kz)) return false;  // (NaN and infinity fail both comparisons)
  *key = bki_key((unsigned)kx, (unsigned)ky, (unsigned)kz);
  return true;
}

// get_probs / get_vars of one class, sum = bki_sum(ms, 0, nclass): every operation on its own, in upstream's written order
__host__ __device__ inline float bki_prob(float m, float sum) { return m / sum; }
__host__ __device__ inline float bki_var(float m, float sum) {
  const float p = m / sum;
  return (p - p * p) / (sum + 1.f);
}

// max_element over get_probs: the first maximum (all NaN: 0).  ms(c): the voxel's ms, or the prior for the default node.
template <class M>
__host__ __device__ inline int bki_semantics(M&& ms, float sum, int nclass) {
  int best = 0;
  float pb = ms(0) / sum;
  for (int c = 1; c < nclass; c++) {
    const float pc = ms(c) / sum;
    if (pc > pb) pb = pc, best = c;
  }
  return best;
}

// the stop-mask bit of a stored voxel
__host__ __device__ inline unsigned bki_state_bit(const BkiConst& k, const float* ms) { return 1u << bki_state(k, ms); }

// parameter of the i-th crossing (i = 1 .. N) on one axis of the segment o -> e, from block k0 in direction s: the boundary
// b = ((k0 - 524288) + s (i - 0.5)) resolution and t = (b - o) / (e - o) in double, one rounding per operation (the sum
// in front of the resolution is exact)
__host__ __device__ inline double bki_ray_t(long long k0, int s, long long i, double res, float o, float e) {
  const double b = ((double)(k0 - BKI_KOFF) + (double)s * ((double)i - 0.5)) * res;
  return (b - (double)o) / ((double)e - (double)o);
}

struct BkiRay {
  int status, steps;       // BKI_RAY_*; voxels visited
  unsigned long long key;  // the last voxel visited (the stopping voxel; the end's on BKI_RAY_END), BKI_NO_KEY: nothing walked
  float t;                 // the cast of the parameter at which the walk entered it; 0 in the origin's voxel
  double td;               // ... the parameter itself (cvo_map_render's depth is (float)(td * (double)z_far))
};

// The library's own walk over the voxels the segment o -> e passes through, face by face (NOT upstream's RayCaster): exactly
// 1 + N[x] + N[y] + N[z] voxels, N the distance of the two k0 per axis, known before the first step; each step crosses the
// axis whose next crossing has the smallest t, ties to the lowest axis.  look(key) -> BKI_BIT_* of the voxel; the walk stops
// at the first voxel, the origin's included, whose bit is in stop_mask.  Both counts bound the loop: it cannot run away.
template <class Look>
__host__ __device__ inline BkiRay bki_ray_walk(float size, const float o[3], const float e[3], unsigned stop_mask, int max_steps, Look&& look) {
  BkiRay r{BKI_RAY_OUTSIDE, 0, BKI_NO_KEY, 0.f, 0.0};
  long long k0x, k0y, k0z, k1x, k1y, k1z;
  if (!bki_k0(o[0], size, &k0x) || !bki_k0(o[1], size, &k0y) || !bki_k0(o[2], size, &k0z)) return r;
  if (!bki_k0(e[0], size, &k1x) || !bki_k0(e[1], size, &k1y) || !bki_k0(e[2], size, &k1z)) return r;
  const long long dx = k1x - k0x, dy = k1y - k0y, dz = k1z - k0z;
  const long long nx = dx < 0 ? -dx : dx, ny = dy < 0 ? -dy : dy, nz = dz < 0 ? -dz : dz;
  const int sx = dx > 0 ? 1 : (dx < 0 ? -1 : 0), sy = dy > 0 ? 1 : (dy < 0 ? -1 : 0), sz = dz > 0 ? 1 : (dz < 0 ? -1 : 0);
  const long long total = 1 + nx + ny + nz;
  if (total > (long long)max_steps) return r.status = BKI_RAY_TOO_LONG, r;
  const double res = (double)size;
  long long ix = 1, iy = 1, iz = 1, kx = k0x, ky = k0y, kz = k0z;
  double tx = nx ? bki_ray_t(k0x, sx, 1, res, o[0], e[0]) : 0.0;
  double ty = ny ? bki_ray_t(k0y, sy, 1, res, o[1], e[1]) : 0.0;
  double tz = nz ? bki_ray_t(k0z, sz, 1, res, o[2], e[2]) : 0.0;
  double t = 0.0;
  for (long long step = 1; step <= total; step++) {
    r.key = bki_key((unsigned)kx, (unsigned)ky, (unsigned)kz);
    r.steps = (int)step;
    r.t = (float)t;
    r.td = t;
    if (look(r.key) & stop_mask) return r.status = BKI_RAY_STOPPED, r;
    if (step == total) break;
    // the axis with crossings left whose next one comes first; ties: the lowest axis
    int a = -1;
    double tb = 0.0;
    if (ix <= nx) a = 0, tb = tx;
    if (iy <= ny && (a < 0 || ty < tb)) a = 1, tb = ty;
    if (iz <= nz && (a < 0 || tz < tb)) a = 2, tb = tz;
    if (a == 0) {
      kx += sx, t = tx, ix++;
      if (ix <= nx) tx = bki_ray_t(k0x, sx, ix, res, o[0], e[0]);
    } else if (a == 1) {
      ky += sy, t = ty, iy++;
      if (iy <= ny) ty = bki_ray_t(k0y, sy, iy, res, o[1], e[1]);
    } else {
      if (a < 0) break;  // (no axis has a crossing left: the count says this cannot be)
      kz += sz, t = tz, iz++;
      if (iz <= nz) tz = bki_ray_t(k0z, sz, iz, res, o[2], e[2]);
    }
  }
  return r.status = BKI_RAY_END, r;
}

// the camera-frame end point of pixel (u, v): (((u - cx) / fx) z_far, ((v - cy) / fy) z_far, z_far), each operation on its own
__host__ __device__ inline void bki_pixel_end(int u, int v, float fx, float fy, float cx, float cy, float z_far, float out[3]) {
  out[0] = (((float)u - cx) / fx) * z_far;
  out[1] = (((float)v - cy) / fy) * z_far;
  out[2] = z_far;
}

}  // namespace cvo_dev
