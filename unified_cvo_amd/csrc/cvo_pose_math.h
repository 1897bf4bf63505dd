// cvo_pose_math.h -- a 3x4 ROW-major pose times (x, y, z, 1), THE expression of transform_point_pose_vec (cvo_device.h, which
// says where it comes from): fma(T0, x, T1 * y) + fma(T2, z, T3) per row.  On its own so that the kernels and every host
// loop that must equal them - cvo_map_insert_posed, the host side of cvo_map_query_cloud, the voxel map's CPU twin
// (cvo_bki_twin.h) - evaluate one text.  A host compiler takes this header too (cvo_host_attrs.h).
#pragma once
#include "cvo_host_attrs.h"

namespace cvo_dev {

__host__ __device__ inline void pose_point(const float* T, float x, float y, float z, float out[3]) {
  out[0] = __builtin_fmaf(T[0], x, T[1] * y) + __builtin_fmaf(T[2], z, T[3]);
  out[1] = __builtin_fmaf(T[4], x, T[5] * y) + __builtin_fmaf(T[6], z, T[7]);
  out[2] = __builtin_fmaf(T[8], x, T[9] * y) + __builtin_fmaf(T[10], z, T[11]);
}

}  // namespace cvo_dev
