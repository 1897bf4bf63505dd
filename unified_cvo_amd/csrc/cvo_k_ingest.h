// cvo_k_ingest.h -- k_cloud_ingest (a caller's rows, already in device memory, into a cloud's slab) and k_cloud_gather
// (the slab's raw arrays into spatial order under an ordering made on the host); the exact one-hot rule both upload routes use.
// Part of the kernel set of cvo_kernels.h; compiled only as part of cvo_hip.hip.  Host side: cvo_ingest.hip.
#pragma once
#include "cvo_k_cloud.h"

namespace cvo_dev {

// THE one-hot rule of a label row (upload_host_cloud on the host, k_cloud_ingest on the device): the class id when exactly
// one entry == 1.0f and every other == 0.0f (-0.0f included), -1 otherwise (a soft distribution, two ones, a NaN, no one).
__host__ __device__ inline int label_onehot_class(const float* l) {
  int hot = -1, ones = 0;
  for (int c = 0; c < NC; c++) {
    if (l[c] == 1.0f) {
      hot = c;
      ones++;
    } else if (!(l[c] == 0.0f)) {
      ones = 2;  // (neither 0 nor 1: a soft distribution)
    }
  }
  return ones == 1 ? hot : -1;
}

// ------------------------------------------------------------------------------------------
// k_cloud_ingest: what upload_host_cloud does on the calling thread - gather the rows, pack x4 and the raw attribute
// arrays, detect one-hot label rows, flag non-finite coordinates, sum the centroid, find the largest |p|^2 - for rows that
// are in device memory already.  Grid (blocks, cloud): block b of cloud q works on the 256-point tiles b, b + gridDim.x ...
//
// How the lanes share a record.  Records are only 4-byte aligned (a 76-byte label row, a 192-byte AoS record at offset
// 44), so no load wider than a dword is legal.  One lane per POINT would make every load instruction touch 64 records
// (64 x 76 B: 38 cache lines per instruction, 19 instructions per row - each line fetched 19 times from L1).  Instead a
// tile's attribute is ONE flat array of 256 x W dwords: lane t takes elements t, t + 256 ..., element e is dword e % W of
// point e / W.  Consecutive lanes read consecutive dwords of a record and step to the next record (contiguous for packed
// rows, 192 B on for AoS records), so every instruction reads 256 B of whole cache lines once; the packed destination is
// lane-contiguous (base + 4 e).  The tile's label dwords also go to LDS, [256][19]: the one-hot rule then runs one lane
// per point on ds_read_b32 at a stride of 19 dwords - odd, so the 32 lanes of a group fall on 32 different banks.
//
// Per-cloud results go to the cloud's control block: three "clear on event" words (preset to ~0 by the host) and one
// partial per block.  Sum order, fixed for a given grid: thread t adds its points t + 256 * tile in ascending tile order
// (doubles), the 64 lanes of a wave combine by the xor butterfly 32, 16 ... 1 (every lane ends with the same bits), lane 0
// of wave 0 adds the four waves in order 0 .. 3 and writes partial[b] = {sx, sy, sz, r2max}; the host adds the partials in
// block order.  r2max follows the host's rule: the largest px*px + py*py + pz*pz in double, a NaN sticks - a maximum, so
// it equals the host's bit for bit whatever the order.
//
// Traffic: (12 + 20 + 76 + 8) B in and (16 + 20 + 76 + 8 + 4) B out per point; 10k points = 1.16 MB + 1.24 MB, at
// HBM speed under a microsecond - the launch is bound by its latency, not by bytes.
// ------------------------------------------------------------------------------------------
constexpr int INGEST_THREADS = 256;
constexpr int INGEST_MAX_BLOCKS = 256;  // blocks per cloud (one per CU): bounds the control block
struct IngestFlags {
  unsigned onehot;   // cleared by a label row that is not an exact one-hot
  unsigned finite;   // cleared by a non-finite coordinate
  unsigned bad_pos;  // the first position whose rows[] entry is outside [0, n_records) (atomic minimum; ~0: none)
  unsigned pad;
};
struct IngestPartial {
  double sx, sy, sz, r2max;
};
struct IngestJob {
  int n, n_records;
  const char* xyz;   unsigned xyz_stride;    // 3 floats at xyz + r * stride (bytes)
  const char* feat;  unsigned feat_stride;   // FD floats, or null
  const char* label; unsigned label_stride;  // NC floats, or null
  const char* geo;   unsigned geo_stride;    // 2 floats, or null
  const int* rows;                           // point i is record rows[i], or null: record i
  float4* x4;                                // out: coordinates, original order, w = 0
  float* raw_feat;                           // out: n x FD packed            } null where the
  float* raw_label;                          // out: n x NC packed            } source is
  float* raw_geo;                            // out: n x 2 packed             }
  int* raw_lid;                              // out: class id per point (-1: not a one-hot row), or null (no labels / NO_ONEHOT)
  IngestFlags* flags;                        // the cloud's control block: the flag words ...
  IngestPartial* partial;                    // ... and gridDim.x partials behind them
};

// one attribute of a tile: W dwords per point from the strided records into the tile's packed rows dst (global memory or
// LDS) and, lds != null, into LDS as well
template <int W>
__device__ __forceinline__ void ingest_rows(const char* __restrict__ src, unsigned stride, const int* s_rec, int cnt, float* dst,
                                            float* lds) {
  for (int e = threadIdx.x; e < cnt * W; e += INGEST_THREADS) {
    const int p = e / W, c = e - p * W;
    const float v = *reinterpret_cast<const float*>(src + (size_t)s_rec[p] * stride + 4 * c);
    dst[e] = v;
    if (lds) lds[e] = v;
  }
}

// NaN sticks, otherwise the larger (the host's `if (m == m && !(r2 <= m)) m = r2` as a combine of two partial results)
__device__ __forceinline__ double ingest_r2_combine(double a, double b) { return a != a ? a : (b != b ? b : (a >= b ? a : b)); }

__global__ __launch_bounds__(INGEST_THREADS) void k_cloud_ingest(const IngestJob* __restrict__ jobs) {
  __shared__ int s_rec[INGEST_THREADS];
  __shared__ float s_xyz[INGEST_THREADS * 3];
  __shared__ float s_lab[INGEST_THREADS * NC];
  __shared__ double s_red[INGEST_THREADS / 64][4];
  const IngestJob J = jobs[blockIdx.y];
  const int n = J.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double sx = 0, sy = 0, sz = 0, r2max = 0;
  for (long long base = (long long)blockIdx.x * INGEST_THREADS; base < n; base += (long long)gridDim.x * INGEST_THREADS) {
    const int cnt = (int)min((long long)INGEST_THREADS, n - base);
    __syncthreads();  // (the previous tile's LDS has been read)
    if (tid < cnt) {
      int r = (int)base + tid;
      if (J.rows) {
        r = J.rows[base + tid];
        if (r < 0 || r >= J.n_records) {  // clamped BEFORE any load through it: nothing out of bounds is read
          atomicMin(&J.flags->bad_pos, (unsigned)(base + tid));
          r = 0;
        }
      }
      s_rec[tid] = r;
    }
    __syncthreads();
    ingest_rows<3>(J.xyz, J.xyz_stride, s_rec, cnt, s_xyz, nullptr);
    if (J.feat) ingest_rows<FD>(J.feat, J.feat_stride, s_rec, cnt, J.raw_feat + (size_t)base * FD, nullptr);
    if (J.label) ingest_rows<NC>(J.label, J.label_stride, s_rec, cnt, J.raw_label + (size_t)base * NC, J.raw_lid ? s_lab : nullptr);
    if (J.geo) ingest_rows<2>(J.geo, J.geo_stride, s_rec, cnt, J.raw_geo + (size_t)base * 2, nullptr);
    __syncthreads();
    if (tid < cnt) {
      const float x = s_xyz[3 * tid], y = s_xyz[3 * tid + 1], z = s_xyz[3 * tid + 2];
      J.x4[base + tid] = make_float4(x, y, z, 0.f);
      if (!(isfinite(x) && isfinite(y) && isfinite(z))) J.flags->finite = 0u;
      const double px = x, py = y, pz = z;
      sx += px;
      sy += py;
      sz += pz;
      const double r2 = px * px + py * py + pz * pz;
      if (r2max == r2max && !(r2 <= r2max)) r2max = r2;
      if (J.raw_lid) {
        const int hot = label_onehot_class(s_lab + NC * tid);
        J.raw_lid[base + tid] = hot;
        if (hot < 0) J.flags->onehot = 0u;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sx += __shfl_xor(sx, o);
    sy += __shfl_xor(sy, o);
    sz += __shfl_xor(sz, o);
    r2max = ingest_r2_combine(r2max, __shfl_xor(r2max, o));
  }
  if (lane == 0) {
    s_red[wave][0] = sx;
    s_red[wave][1] = sy;
    s_red[wave][2] = sz;
    s_red[wave][3] = r2max;
  }
  __syncthreads();
  if (tid == 0) {
    IngestPartial P{s_red[0][0], s_red[0][1], s_red[0][2], s_red[0][3]};
    for (int w = 1; w < INGEST_THREADS / 64; w++) {
      P.sx += s_red[w][0];
      P.sy += s_red[w][1];
      P.sz += s_red[w][2];
      P.r2max = ingest_r2_combine(P.r2max, s_red[w][3]);
    }
    J.partial[blockIdx.x] = P;
  }
}

// ------------------------------------------------------------------------------------------
// k_cloud_gather: the output pass of k_kd_order for a cloud whose ordering was made on the host (fewer than 8 or more than
// KD_MAX_POINTS points, non-finite coordinates, NO_SORT, ORDER=host / virtual): `order` has been uploaded, the raw arrays
// are where k_cloud_ingest left them - the attributes never leave the device.  Grid (blocks, cloud), grid-stride loops; the
// job is the KdJob of the cloud (seg_of_pos / seg_lo unused).
// ------------------------------------------------------------------------------------------
constexpr int GATHER_THREADS = 256;
__global__ __launch_bounds__(GATHER_THREADS) void k_cloud_gather(const KdJob* __restrict__ jobs) {
  const KdJob J = jobs[blockIdx.y];
  const int n = J.n, t0 = blockIdx.x * GATHER_THREADS + threadIdx.x, step = gridDim.x * GATHER_THREADS;
  for (int p = t0; p < n; p += step) {
    const int id = J.order[p];
    J.inv[id] = p;
    J.xs4[p] = J.x4[id];
    if (J.raw_lid) J.lid[p] = J.raw_lid[id];
    if (J.raw_geo) J.geo[p] = make_float2(J.raw_geo[2 * (size_t)id], J.raw_geo[2 * (size_t)id + 1]);
  }
  if (J.raw_feat)
    for (int q = t0; q < n * 2; q += step) {  // two float4 per point: 5 floats + 3 zeros
      const int r = q >> 1, h = q & 1;
      const float* src = J.raw_feat + (size_t)J.order[r] * FD;
      J.feat[q] = h == 0 ? make_float4(src[0], src[1], src[2], src[3]) : make_float4(src[4], 0.f, 0.f, 0.f);
    }
  if (J.raw_label)
    for (long long q = t0; q < (long long)n * 5; q += step) {  // five float4 per point: 19 floats + 1 zero
      const int r = (int)(q / 5), h = (int)(q - 5ll * r);
      const float* src = J.raw_label + (size_t)J.order[r] * NC + 4 * h;
      J.label[q] = make_float4(src[0], src[1], src[2], h < 4 ? src[3] : 0.f);
    }
}

}  // namespace cvo_dev
