// cvo_hip.hip -- host side of the C-ABI declared in include/cvo_hip.h: contexts, HBM-resident
// clouds, workspace layout, and the enqueue-only optimiser loop (hipGraph replays of
// [k_scan, k_assoc, k_coeff, k_update, k_prep] with a device-side status word; no host round trip per
// iteration, unlike the ~15 blocking syncs per iteration of CvoGPU.cu:1387-1533).
//
// ONE translation unit, in sections.  The kernels are templates in headers (cvo_kernels.h) that share __device__ globals
// (g_phase_ticks ...) and are launched from several sections; without -fgpu-rdc every translation unit would get its own
// copy of those globals and of every kernel instantiation it touches, so the sections below are compiled together, in
// dependency order.  Each of them reads on its own next to cvo_internal.h:
//   cvo_ctx.hip     contexts, stream pool, options, workspace          cvo_upload.hip  resident clouds
//   cvo_launch.hip  every kernel launch of the solver                  cvo_sched.hip   setup, chunk graphs, cvo_align_batch
//   cvo_queue.hip   the batch queue                                    cvo_eval.hip    inner products, single evaluations
//   cvo_export.hip  association / ELL exports                          cvo_debug.hip   test and profiling hooks
//   cvo_irls.hip    multi-frame align (the outer loop of CvoBatchIRLS and its device workspace; the trust-region solve itself is
//                   cvo_irls_solve.h, plain C++ that host/cvo_irls_solve_check runs without a device)
//   cvo_frontend.hip  what the front ends below share: scratch regions, the ordered-compaction launcher, the route rule, the entry frame
//   cvo_ingest.hip  resident clouds from rows that are already in device memory: checks, k_cloud_ingest, the route rule, k_cloud_gather
//   cvo_voxel.hip   voxel-grid downsampling: selection on the device or the host, upload of the survivors
//   cvo_merge.hip   resident clouds merged under their poses into one (k_cloud_unpack, then the two sections above) and read back
//   cvo_rgbd.hip    RGB-D front end: depth + colour frame to candidate points and to a resident cloud
//   cvo_fast.hip    the CV_FAST point selection: FAST-9/16 scores, the reference's threshold schedule
//   cvo_stereo.hip  stereo front end: left frame + disparity to candidate points and to a resident cloud
//   cvo_lidar.hip   LiDAR front end: raw scan to the LOAM selection's indices and to a resident cloud
//   cvo_nlm.hip     non-local-means denoising of an 8-bit image: RawImage's first statement
//   cvo_sgm.hip     the stereo matcher: left + right gray planes to the left disparity (semi-global matching over census)
//   cvo_dfilter.hip the disparity post-filter: libelas's speckle, gap and adaptive-mean passes on the matcher's or a caller's map
//   cvo_stereo_pair.hip  the entry points that chain matcher, filter and stereo front end under one lock
//   cvo_bki.hip     the semantic voxel map: posed clouds (host rows or resident) fused into a persistent table, its occupied voxels read out as a cloud,
//                   point queries, ray casts and rendered views of it (the handle, the side rule and the device side; the CPU twin is
//                   cvo_bki_twin.h, plain C++ that a host compiler builds without a device)
//   cvo_depth.hip   the keyframe depth filter: a resident keyframe refined from resident frames (the non-isotropic association where its
//                   evaluation left it, k_depth_accumulate, k_depth_finish, the ordered compaction, the ingest of cvo_ingest.hip)
#include "cvo_internal.h"

#include "cvo_ctx.hip"
#include "cvo_launch.hip"
#include "cvo_upload.hip"
#include "cvo_frontend.hip"
#include "cvo_ingest.hip"
#include "cvo_voxel.hip"
#include "cvo_merge.hip"
#include "cvo_rgbd.hip"
#include "cvo_fast.hip"
#include "cvo_stereo.hip"
#include "cvo_lidar.hip"
#include "cvo_nlm.hip"
#include "cvo_sgm.hip"
#include "cvo_dfilter.hip"
#include "cvo_stereo_pair.hip"
#include "cvo_bki.hip"
#include "cvo_sched.hip"
#include "cvo_queue.hip"
#include "cvo_eval.hip"
#include "cvo_export.hip"
#include "cvo_irls.hip"
#include "cvo_depth.hip"
#include "cvo_debug.hip"
