// cvo_k_merge.h -- k_cloud_unpack: resident clouds back into rows in ORIGINAL order, moved by a pose per cloud, concatenated.
// The first step of cvo_cloud_merge (the multi-frame drivers' merge_transformed_pc, main_covisMap_test.cpp:183-215) and, with
// one job and no pose, all of cvo_cloud_download.  Part of the kernel set of cvo_kernels.h; compiled only as part of
// cvo_hip.hip.  Host side: cvo_merge.hip.
#pragma once
#include "cvo_k_cloud.h"

namespace cvo_dev {

// ------------------------------------------------------------------------------------------
// k_cloud_unpack: ONE launch over a job table, a job per non-empty input cloud.  Output row job.base + i is point i of the
// job's cloud: its coordinates x4[i] - under the job's pose transform_point_pose_vec(pose, x4[i]), the function
// k_transform_pose calls; without one the stored BITS (no multiply by an identity: -0.0f, infinities and NaN payloads
// survive) - and its attributes from position inv[i] of the cloud's packed spatial-order arrays.  An attribute the output
// holds and the cloud lacks (a null pointer in the job) is written as zeros.
//
// The output keeps the packed arrays' padded rows, so that every attribute moves as whole float4 / float2:
//   xyz    3 floats per row (what k_voxel_insert reads; an ingest stride of 12)
//   feat   2 float4 per row: FD = 5 floats + 3 of padding (stride 32)
//   label  5 float4 per row: NC = 19 floats + 1 of padding (stride 80)
//   geo    1 float2 per row (stride 8)
//
// How the lanes share a tile of 256 rows.  Every array of the tile is ONE flat run of elements - 768 dwords, 512 / 1280
// float4, 256 float2 - and thread t takes elements t, t + 256 ...: consecutive lanes store consecutive elements, so every
// store instruction writes whole cache lines (1 KiB per wave for the float4 arrays).  The loads are 16 bytes each at
// feat[2 inv[i] + h] / label[5 inv[i] + h]: the 2 / 5 lanes of a row read one 32- / 80-byte run, the rows themselves are
// scattered by inv (original order against spatial order) - a gather, served by L2 for clouds of this size.  The three
// lanes of a row's coordinates load the same x4[i] (one address, one fetch) and each keeps its component.
//
// Which cloud a row belongs to: the jobs' first rows, ascending (the host leaves empty clouds out, so they are strictly
// ascending), sit in LDS - the kernel's only use of it - and every element finds the last job whose first row is not above
// its own by bisection: at most 12 steps for UNPACK_MAX_JOBS, 3 to 4 for the 8 to 16 frames of a window.
//
// Traffic per point of a cloud with every attribute: 16 + 4 + 32 + 80 + 8 = 140 B read, 12 + 32 + 80 + 8 = 132 B written.
// 16 frames of 21 429 points = 48 MB + 45 MB; at HBM speed that is some 20 us, 8 x 10 000 colour points (4.2 + 3.5 MB) are
// under 2 us: the launch is bound by its latency.
// ------------------------------------------------------------------------------------------
constexpr int UNPACK_THREADS = 256;      // threads of a block = rows of a tile
constexpr int UNPACK_MAX_BLOCKS = 1024;  // (four per CU; a block strides over the tiles)
constexpr int UNPACK_MAX_JOBS = 4096;    // the jobs' first rows in LDS: 16 KB
struct UnpackJob {
  int n;                // points (>= 1)
  int base;             // its first output row
  int has_pose, pad;
  float pose[12];       // 3x4 row-major (has_pose != 0)
  const float4* x4;     // coordinates, original order
  const int* inv;       // original index -> sorted position
  const float4* feat;   // 2 float4 per sorted position, or null: zeros
  const float4* label;  // 5 float4 per sorted position, or null
  const float2* geo;    // or null
};
struct UnpackOut {
  int n_jobs, total;  // jobs, rows (the jobs' n summed)
  float* xyz;         // total x 3
  float4* feat;       // total x 2, or null: not wanted
  float4* label;      // total x 5, or null
  float2* geo;        // total, or null
};

// the job of output row `row`: the last one whose first row is <= row (s_base[0] == 0 <= row)
__device__ __forceinline__ int unpack_job_of(const int* s_base, int n_jobs, int row) {
  int lo = 0, hi = n_jobs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s_base[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(UNPACK_THREADS) void k_cloud_unpack(const UnpackJob* __restrict__ jobs, UnpackOut out) {
  __shared__ int s_base[UNPACK_MAX_JOBS];
  const int tid = threadIdx.x, n_jobs = out.n_jobs;
  for (int j = tid; j < n_jobs; j += UNPACK_THREADS) s_base[j] = jobs[j].base;
  __syncthreads();
  const int tiles = (out.total + UNPACK_THREADS - 1) / UNPACK_THREADS;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int row0 = tile * UNPACK_THREADS, cnt = min(UNPACK_THREADS, out.total - row0);
    // ---- coordinates: a dword per element
    unsigned* xyz = reinterpret_cast<unsigned*>(out.xyz) + 3 * (size_t)row0;
    for (int e = tid; e < cnt * 3; e += UNPACK_THREADS) {
      const int r = e / 3, c = e - 3 * r, row = row0 + r;
      const int j = unpack_job_of(s_base, n_jobs, row);
      const UnpackJob& J = jobs[j];
      const float4 p = J.x4[row - s_base[j]];
      unsigned bits = __float_as_uint(c == 0 ? p.x : (c == 1 ? p.y : p.z));
      if (J.has_pose) {
        const V3 t = transform_point_pose_vec(J.pose, p.x, p.y, p.z);
        bits = __float_as_uint(c == 0 ? t.x : (c == 1 ? t.y : t.z));
      }
      xyz[e] = bits;
    }
    // ---- colour: two float4 per row
    if (out.feat) {
      float4* dst = out.feat + 2 * (size_t)row0;
      for (int e = tid; e < cnt * 2; e += UNPACK_THREADS) {
        const int r = e >> 1, h = e & 1, row = row0 + r;
        const int j = unpack_job_of(s_base, n_jobs, row);
        const UnpackJob& J = jobs[j];
        dst[e] = J.feat ? J.feat[2 * (size_t)J.inv[row - s_base[j]] + h] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // ---- class distributions: five float4 per row
    if (out.label) {
      float4* dst = out.label + 5 * (size_t)row0;
      for (int e = tid; e < cnt * 5; e += UNPACK_THREADS) {
        const int r = e / 5, h = e - 5 * r, row = row0 + r;
        const int j = unpack_job_of(s_base, n_jobs, row);
        const UnpackJob& J = jobs[j];
        dst[e] = J.label ? J.label[5 * (size_t)J.inv[row - s_base[j]] + h] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // ---- geometric types: a float2 per row
    if (out.geo && tid < cnt) {
      const int row = row0 + tid;
      const int j = unpack_job_of(s_base, n_jobs, row);
      const UnpackJob& J = jobs[j];
      out.geo[row] = J.geo ? J.geo[J.inv[row - s_base[j]]] : make_float2(0.f, 0.f);
    }
  }
}

}  // namespace cvo_dev
