// cvo_k_bki_stage.h -- k_bki_stage: the rows of ONE resident cloud, in ORIGINAL order, as the hits of one insert into the
// semantic voxel map (cvo_map_insert_cloud).  It writes the insert scratch in exactly the layout k_bki_count ... k_bki_long
// read (BkiInsertArgs, cvo_k_bki.h): xyz n x 3, feat n x 5, label n x C, all packed, so the six insert kernels run unchanged
// behind it - and, on a map of the host side, the three arrays are what the twin's insert takes once they are copied down.
//
// The addressing is k_cloud_unpack's (cvo_k_merge.h) for one job: row i has its coordinates in x4[i] - under the pose
// transform_point_pose_vec(pose, x4[i]), the function cvo_cloud_transformed and cvo_map_insert_posed's host loop share;
// without a pose the stored BITS, nothing is multiplied - and its attributes at position inv[i] of the cloud's packed
// spatial-order arrays: colour in the first 5 floats of the 8 at feat[2 inv[i]], the label row in the first C floats of the
// 20 at label[5 inv[i]] (the inverse of the zero padding the map's read-out applies).  What differs from k_cloud_unpack is
// that the rows go out UNPADDED, 5 and C floats: a row is no longer a whole number of float4, so every array moves as dwords.
//
// How the lanes share a tile of 256 rows.  Every array of the tile is ONE flat run of dwords - 768, 1280, 256 C - and thread
// t takes elements t, t + 256 ...: consecutive lanes store consecutive dwords, every store instruction writes whole cache
// lines (256 B per wave).  The loads of a row's 5 / C lanes fall into one 32- / 80-byte run, the rows themselves are
// scattered by inv - a gather, served by L2 for clouds of this size; the lanes of a row read the same inv[i] and x4[i] (one
// address, one fetch).  No LDS.  An inv outside [0, n) - it cannot be one of a cloud the library made - is clamped to n - 1
// before it is used: no gather leaves the cloud's arrays.
//
// The host route refuses a coordinate that is not finite before either side runs (bki_validate_insert); here the moved
// coordinates exist only on the device, so the kernel leaves the LOWEST row with a non-finite moved coordinate in the
// control block (BkiCtl::nonfinite, ~0u: none) and the host refuses with the host route's text and code.
//
// Traffic per point of a cloud with colour and 19 classes: 16 + 4 + 32 + 80 = 132 B read (20 + 4 C + 36 in general), 12 + 20
// + 4 C <= 108 B written.  9 284 points are 1.2 MB + 1.0 MB, 16 686 are 2.2 MB + 1.8 MB: under a microsecond at HBM speed,
// no arithmetic to speak of - the launch is bound by its latency.  Part of the kernel set of
// cvo_kernels.h; compiled only as part of cvo_hip.hip.  Host side: cvo_bki.hip (the twin: cvo_bki_twin.h).
#pragma once
#include "cvo_k_bki.h"

namespace cvo_dev {

constexpr int BKI_STAGE_THREADS = 256;      // threads of a block = rows of a tile
constexpr int BKI_STAGE_MAX_BLOCKS = 1024;  // (four per CU; a block strides over the tiles)

struct BkiStageArgs {
  int n;                // rows (>= 1)
  int C;                // label columns staged: the map's classes (0: none)
  int has_pose, pad;
  float pose[12];       // 3x4 row-major (has_pose != 0)
  const float4* x4;     // coordinates, original order
  const int* inv;       // original index -> sorted position
  const float* feat;    // 8 floats per sorted position (ofeat != null)
  const float* label;   // 20 floats per sorted position (olabel != null)
  float* xyz;           // n x 3
  float* ofeat;         // n x 5, or null: the cloud holds no colour
  float* olabel;        // n x C, or null: C == 0
  BkiCtl* ctl;
};

__global__ __launch_bounds__(BKI_STAGE_THREADS) void k_bki_stage(BkiStageArgs a) {
  const int tid = threadIdx.x;
  const unsigned last = (unsigned)a.n - 1u;
  const int tiles = (a.n + BKI_STAGE_THREADS - 1) / BKI_STAGE_THREADS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int row0 = tile * BKI_STAGE_THREADS, cnt = min(BKI_STAGE_THREADS, a.n - row0);
    // ---- coordinates: a dword per element
    unsigned* xyz = reinterpret_cast<unsigned*>(a.xyz) + 3 * (size_t)row0;
    for (int e = tid; e < cnt * 3; e += BKI_STAGE_THREADS) {
      const int r = e / 3, c = e - 3 * r, row = row0 + r;
      const float4 p = a.x4[row];
      float v = c == 0 ? p.x : (c == 1 ? p.y : p.z);
      if (a.has_pose) {
        const V3 t = transform_point_pose_vec(a.pose, p.x, p.y, p.z);
        v = c == 0 ? t.x : (c == 1 ? t.y : t.z);
      }
      const unsigned bits = __float_as_uint(v);
      if ((bits & 0x7f800000u) == 0x7f800000u) atomicMin(&a.ctl->nonfinite, (unsigned)row);  // (infinity or NaN)
      xyz[e] = bits;
    }
    // ---- colour: five dwords per row
    if (a.ofeat) {
      float* dst = a.ofeat + BKI_FEAT * (size_t)row0;
      for (int e = tid; e < cnt * BKI_FEAT; e += BKI_STAGE_THREADS) {
        const int r = e / BKI_FEAT, c = e - BKI_FEAT * r;
        const unsigned s = min((unsigned)a.inv[row0 + r], last);
        dst[e] = a.feat[(size_t)FD_PAD * s + c];
      }
    }
    // ---- class distributions: the first C dwords of a row
    if (a.olabel) {
      float* dst = a.olabel + (size_t)a.C * row0;
      for (int e = tid; e < cnt * a.C; e += BKI_STAGE_THREADS) {
        const int r = e / a.C, c = e - a.C * r;
        const unsigned s = min((unsigned)a.inv[row0 + r], last);
        dst[e] = a.label[(size_t)NC_PAD * s + c];
      }
    }
  }
}

}  // namespace cvo_dev
