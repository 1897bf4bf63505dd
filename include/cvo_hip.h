/*
 * cvo_hip.h -- C-ABI of the MI355X (gfx950) backend for unified_cvo's pairwise
 * CvoGPU::align() / inner_product_gpu() / function_angle() hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  The C++
 * classes in include/UnifiedCvo/ (cvo::CvoGPU, cvo::CvoPointCloud, cvo::CvoParams) are a
 * thin veneer over these entry points, and a maintainer of the reference binds them as
 * shown in INTEGRATION.md.  Each entry point cites the reference interface it replaces
 * (file:line relative to the upstream repository).
 *
 * Conventions
 *   * 4x4 transforms are 16 floats, COLUMN-major (the memory layout of Eigen::Matrix4f).
 *   * `init_T` is the reference's T_target_frame_to_source_frame argument; it is taken as
 *     the running (R, T) directly (CvoGPU.cu:1363-1364).  `out_T` is the returned
 *     `transform` = [R^T | -R^T T] (CvoGPU.cu:94-112, 1562).
 *   * Return codes: 0 = ok, -1 = "flow vanished" exactly as the reference (CvoGPU.cu:1454-1458),
 *     <= -2 = argument / HIP errors (CVO_E_*); never exit().  cvo_last_error() gives text.
 *   * A context is bound to one HIP device and owns one stream; it is not thread-safe,
 *     distinct contexts are independent.
 */
#ifndef CVO_HIP_H
#define CVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVO_FEATURE_DIMENSIONS 5 /* CMakeLists.txt:498 (cvo_gpu_img_lib) */
#define CVO_NUM_CLASSES 19       /* CMakeLists.txt:498 */

#define CVO_OK 0
#define CVO_RET_FLOW_VANISHED (-1)
#define CVO_E_INVALID (-2)
#define CVO_E_HIP (-3)
#define CVO_E_NOMEM (-4)
#define CVO_E_UNSUPPORTED (-5)
#define CVO_E_VERIFY (-6) /* CVO_VERIFY_LISTS=1: a row derived from the cached candidate lists differed from the literal scan */

/* Layout-identical to cvo::CvoParams (include/UnifiedCvo/cvo/CvoParams.hpp:12-73): same
 * members, same order, same types, so a reference build can pass &params unchanged. */
typedef struct cvo_params_t {
  float ell_init_first_frame;
  float ell_init;
  float ell_min;
  int min_ell_iter_limit;
  float ell_max;
  double dl;
  double dl_step;
  float sigma;
  float sp_thres;
  float c;
  float d;
  float c_ell;
  float c_sigma;
  float s_ell;
  float s_sigma;
  int MAX_ITER;
  float eps;
  float eps_2;
  float min_step;
  float max_step;
  float step;
  int nearest_neighbors_max;
  float ell_decay_rate;
  float ell_decay_rate_first_frame;
  int ell_decay_start;
  int ell_decay_start_first_frame;
  int indicator_window_size;
  float indicator_stable_threshold;
  int is_pcl_visualization_on;
  int is_using_least_square;
  int is_ell_adaptive;
  int is_full_ip_matrix;
  int is_using_geometry;
  int is_using_intensity;
  int is_using_semantics;
  int is_using_range_ell;
  int is_using_kdtree;
  int is_exporting_association;
  int is_using_geometric_type;
  int multiframe_using_cpu;
  int multiframe_max_iters;
  float multiframe_ell_init;
  float multiframe_ell_min;
  int multiframe_iter_per_ell;
  float multiframe_ell_decay_rate;
  int multiframe_iterations_per_ell;
  int multiframe_iterations_per_solve;
  int multiframe_expected_points;
  float multiframe_downsample_voxel_size;
  int multiframe_num_neighbors;
  int multiframe_least_squares_num_threads;
  int multiframe_min_nonzeros;
} cvo_params_t;

/* Fills *p with the defaults of CvoParams::CvoParams() (CvoParams.hpp:75-126).  max_step and
 * step, which the reference leaves uninitialised, are set to 0.8 and 0 (documented in DESIGN.md). */
void cvo_params_default(cvo_params_t* p);

typedef struct cvo_ctx cvo_ctx;     /* device + stream + cached scratch */
typedef struct cvo_cloud cvo_cloud; /* a point cloud resident in HBM */

/* One record per optimiser iteration, written by the device when tracing is requested. */
typedef struct cvo_trace_t {
  int k;
  int K;
  float ell;
  float step;
  unsigned int nnz;
  unsigned int max_nnz;
  float omega[3];
  float v[3];
  double B, C, D, E;
  double dist;
  float R[9]; /* running R after the update, row-major */
  float T[3];
} cvo_trace_t;

/* Per-call outputs beyond the transform. */
typedef struct cvo_align_info_t {
  int iterations;        /* value of k when the loop ended ("cvo # of iterations", CvoGPU.cu:1545) */
  int ret;               /* 0 or -1, as CvoGPU::align returns (batch queue results: CVO_E_HIP if the pair was ended by a device-side synchronisation time-out) */
  float final_ell;
  int final_num_neighbors;
  double seconds;        /* registration_seconds: hipEvent time of the loop (CvoGPU.cu:1534-1560) */
} cvo_align_info_t;

/* Optional controls for cvo_align_ex / cvo_align_batch_ex (all zero = reference behaviour). */
typedef struct cvo_align_opts_t {
  int max_iterations;    /* >0: stop after this many iterations (parity tests, benchmarks) */
  int override_state;    /* 1: start from ell0 / K0 below instead of ell_init / nearest_neighbors_max */
  float ell0;
  int K0;
  cvo_trace_t* trace;    /* host array, or NULL */
  int trace_capacity;    /* rows available per pair */
  int trace_dense;       /* record every iteration k < trace_dense ... */
  int trace_every;       /* ... and every k % trace_every == 0 (0 = none) */
  int* n_trace;          /* out: rows written (per pair) */
  int iters_per_launch;  /* iterations enqueued per host check (0 = default) */
  int use_graph;         /* 0 = default (on), 1 = force plain launches, 2 = force graph */
  int kernel_clock;      /* 1: this call runs the instrumented instantiation of the per-iteration kernels, which time
                            every launch on the device clock (read back with cvo_debug_kernel_clock; ~3 % slower);
                            0 = follow the CVO_KERNEL_CLOCK environment switch */
} cvo_align_opts_t;

/* ---- context ------------------------------------------------------------------------ */
int cvo_ctx_create(int device, cvo_ctx** out);
void cvo_ctx_destroy(cvo_ctx* ctx);
const char* cvo_last_error(const cvo_ctx* ctx);
/* Hardware queues.  A batch (cvo_align_batch, CvoGPUSharded) runs on four sub-batch HIP streams that must sit on four
 * different hardware queues; HIP deals streams onto GPU_MAX_HW_QUEUES queues (default 4, read once at the process's
 * first HIP call) and the upload stream, RCCL and the host application bring streams of their own.
 * cvo_process_hint_hw_queues() returns the number of hardware queues in force (4 when the variable is unset); the
 * library never changes it: that is the host's (or the machine's) choice, made before the process's first HIP call.
 * If the variable says less than 8,
 * cvo_ctx_create leaves an advisory text in cvo_ctx_advice() ("" = nothing to report) and prints it once per process
 * on stderr (CVO_QUIET=1 silences the print).  Nothing but speed depends on it. */
int cvo_process_hint_hw_queues(void);
const char* cvo_ctx_advice(const cvo_ctx* ctx);
/* Destroys the HIP streams pooled from destroyed contexts (they are kept across contexts so that a later context finds
 * its sub-batch streams on the hardware queues the first one was given).  Optional, e.g. before unloading the library. */
void cvo_shutdown(void);
/* Tuning / diagnostic switches of a context (none changes a result; the list is in unified_cvo_amd/csrc/cvo_options.h,
 * kOptions, and INTEGRATION.md).  A context reads CVO_<NAME> from the environment ONCE, in cvo_ctx_create; afterwards
 * only this call changes them (value NULL = back to the default), so no library call depends on the process environment while it
 * runs.  `name` with or without the CVO_ prefix.  Unknown names: CVO_E_INVALID. */
int cvo_ctx_set_option(cvo_ctx* ctx, const char* name, const char* value);
/* HIP stream of the context as an opaque pointer (hipStream_t). */
void* cvo_ctx_stream(cvo_ctx* ctx);
int cvo_ctx_synchronize(cvo_ctx* ctx);

/* ---- clouds: replaces CvoPointCloud_to_gpu (CvoGPU_impl.cu:206-285) ------------------
 * xyz: n x 3.  feat: n x 5 row-major or NULL.  label: n x 19 row-major or NULL.
 * geotype: n x 2 or NULL.  Missing arrays read as zeros, as the reference leaves the
 * default-constructed CvoPoint fields (PointSegmentedDistribution.hpp:40-56); they are neither uploaded nor allocated
 * until a call needs them.  Uploads of one context serialise on its upload stream (cvo_cloud_upload_many is the
 * parallel form); they never wait for, nor delay, a solve in flight.  A cloud handed to an align / inner-product
 * call may get a zeroed attribute slab attached by that call (see above): do not share ONE cvo_cloud between
 * concurrent calls of different contexts' threads. */
int cvo_cloud_upload(cvo_ctx* ctx, int n, const float* xyz, const float* feat, const float* label,
                     const float* geotype, cvo_cloud** out);
/* Replaces pcl_PointCloud_to_gpu (CvoGPU_impl.cu:287-362): n records of the 192-byte AoS
 * CvoPoint = pcl::PointSegmentedDistribution<5,19> (PointSegmentedDistribution.hpp:17-99). */
int cvo_cloud_upload_aos192(cvo_ctx* ctx, int n, const void* cvo_points, cvo_cloud** out);
/* n_clouds clouds at once from a pool of `threads` host threads (0 = default): the per-cloud work of cvo_cloud_upload -
 * spatial ordering, one allocation, one copy on the thread's own stream - runs in parallel.  n / xyz: per-cloud sizes and
 * pointers; feat / label / geotype: arrays of per-cloud pointers, the arrays or single entries may be NULL.
 * out: n_clouds handles (all NULL on error). */
int cvo_cloud_upload_many(cvo_ctx* ctx, int n_clouds, const int* n, const float* const* xyz, const float* const* feat,
                          const float* const* label, const float* const* geotype, int threads, cvo_cloud** out);
/* ---- clouds from rows that are already in device memory (no reference counterpart: upstream builds every cloud on the host) ----
 * A caller whose points are in HBM - a network's class scores in a tensor, its own HIP pre-processing - hands them over
 * without a host copy.  Point i of the cloud is record r = rows ? rows[i] : i of strided arrays: 3 floats at
 * xyz + r * xyz_stride, 5 at feat, 19 at label, 2 at geotype (strides in bytes; feat / label / geotype may be NULL and then
 * read as zeros, as in cvo_cloud_upload).
 * Contract: every pointer is device memory of the context's device, complete when the call is made (the caller synchronises
 * its producer stream).  The library enqueues on its upload stream and returns after it has synchronised that stream; the
 * arrays are only read, the cloud owns a copy and may outlive them.  The cloud is interchangeable with the one
 * cvo_cloud_upload makes of the same rows: same spatial order (cvo_debug_cloud_order), same one-hot detection, bit-identical
 * results of every solver, score, association, export, cvo_cloud_transformed and multi-frame call.  Non-finite coordinates
 * are no error here either: such a cloud is ordered on the host and refused by the solvers.
 * CVO_E_INVALID, nothing allocated, *out NULL - decided on the host before any launch: n < 0; xyz NULL with n > 0;
 * n_records < 1, or < n without rows; a stride below the row's size or no multiple of 4; a pointer that is not 4-byte
 * aligned, that hipPointerGetAttributes does not report as device memory of this context's device (host, pinned and
 * managed memory, other devices), or whose n_records rows do not fit the allocation behind it.  No pointer is read
 * through before it is classified.  Found by the ingest kernel: a rows[] entry outside [0, n_records) - the read is
 * clamped, nothing out of bounds is loaded, and cvo_last_error names the first bad position. */
typedef struct {
  int n;                 /* points of the cloud */
  int n_records;         /* records the arrays hold (>= 1 when n > 0); without `rows` it must be >= n */
  const void* xyz;     size_t xyz_stride;      /* 3 floats at xyz + r * stride */
  const void* feat;    size_t feat_stride;     /* 5 floats, or NULL */
  const void* label;   size_t label_stride;    /* 19 floats, or NULL */
  const void* geotype; size_t geotype_stride;  /* 2 floats, or NULL */
  const int* rows;       /* device, optional: point i is record rows[i]; duplicates allowed */
} cvo_device_rows_t;
int cvo_cloud_from_device(cvo_ctx* ctx, const cvo_device_rows_t* rows, cvo_cloud** out);
/* n_clouds clouds with one ingest launch, one read-back and one ordering launch.  out: n_clouds handles (all NULL on error). */
int cvo_cloud_from_device_many(cvo_ctx* ctx, int n_clouds, const cvo_device_rows_t* rows, cvo_cloud** out);
/* The device twin of cvo_cloud_upload_aos192: n 192-byte CvoPoint records in device memory, same byte offsets. */
int cvo_cloud_from_device_aos192(cvo_ctx* ctx, int n, const void* d_pts, cvo_cloud** out);
/* ---- voxel-grid downsampling: replaces cvo::VoxelMap<PointT> as the drivers use it (VoxelMap.hpp, VoxelMap_impl.hpp:126-170) ----
 * Voxel of a point: k = (lrint(x / s), lrint(y / s), lrint(z / s)) with the correctly rounded float quotient and ties to
 * even.  Of every occupied voxel ONE point is kept, the one with the lowest index (upstream draws a member at random);
 * kept[] holds the kept points' indices in ascending order, *n_kept their number.  CVO_E_INVALID, nothing written: a voxel
 * size that is not finite or <= 0, a non-finite coordinate, |k| >= 2^20 on any axis (cvo_last_error names the point, the axis
 * and the extent).  CVO_E_UNSUPPORTED: n > 2^24.  n = 0 is an empty selection.  The selection runs on the context's upload
 * stream: like an upload it neither waits for nor delays a solve in flight.  Frames of fewer than 4096 points take the CPU
 * twin, which is faster there; switch VOXEL_HOST=1 / 0: the CPU twin / the kernels for every size. */
/* one point per occupied voxel of side voxel_size (VoxelMap.hpp / VoxelMap_impl.hpp:126-149, deterministic: lowest index) */
int cvo_voxel_select(cvo_ctx* ctx, int n, const float* xyz, float voxel_size, int* kept /* n ints */, int* n_kept);
int cvo_voxel_select_host(int n, const float* xyz, float voxel_size, int* kept, int* n_kept);   /* CPU twin, no context */
/* Selection + upload: only the coordinates cross to the device for the selection; the cloud returned is the one
 * cvo_cloud_upload makes of the kept rows (same spatial order, one-hot detection, lazily attached zero slabs). */
int cvo_cloud_upload_voxel(cvo_ctx* ctx, int n, const float* xyz, const float* feat, const float* label,
                           const float* geotype, float voxel_size, cvo_cloud** out,
                           int* kept /* n ints or NULL */, int* n_kept /* or NULL */);
/* ---- RGB-D front end: replaces CvoPointCloud(ImageRGBD<T>, Calibration, PointSelectionMethod) (CvoPointCloud.cpp:459-553,
 * CvoPixelSelector.cpp:51-474, RawImage.cpp:55-82) and the per-frame block of the multi-frame RGB-D drivers
 * (main_multi_frame_irls_tum.cpp:279-335) ----
 * A frame: the colour image AS RawImage HOLDS IT AFTER ITS DENOISING (cvo_nlm_denoise / cvo_nlm_denoise_lab below),
 * rows x cols x channels bytes, BGR order for 3 channels; optionally the 8-bit gray plane the gradient is taken
 * of (NULL: 1-channel images as they are, 3-channel ones through OpenCV 3's 8-bit COLOR_BGR2GRAY,
 * (1868 B + 9617 G + 4899 R + 8192) >> 14; OpenCV 4 differs by one level at rare pixels, so parity with a given OpenCV
 * needs the caller's plane); the depth image, uint16_t or float; the calibration; optionally num_classes floats per pixel. */
#define CVO_DEPTH_U16 0
#define CVO_DEPTH_F32 1
/* cvo::CvoPointCloud::PointSelectionMethod (CvoPointCloud.hpp:39-49), same values; the two that are built */
#define CVO_SELECT_DSO_EDGES 2
#define CVO_SELECT_FULL 8
typedef struct cvo_rgbd_frame_t {
  int rows, cols, channels;    /* channels: 1 or 3 */
  const uint8_t* image;        /* rows x cols x channels */
  const uint8_t* gray;         /* rows x cols, or NULL */
  const void* depth;           /* rows x cols of depth_type */
  int depth_type;              /* CVO_DEPTH_U16 / CVO_DEPTH_F32 */
  float fx, fy, cx, cy;        /* Calibration::intrinsic() */
  float scaling_factor;        /* Calibration::scaling_factor(): z = depth / scaling_factor */
  int num_classes;             /* 0 = no semantics */
  const float* semantic;       /* rows x cols x num_classes, or NULL */
} cvo_rgbd_frame_t;
/* The points of the reference constructor, in its order.  FULL: every pixel, COLUMN-major (u outer, v inner), geometric type
 * (0.5, 0.5).  DSO_EDGES: the pixels of dso_select_pixels(num_want = 10000) - per 32 x 32 block the 0.5 quantile of
 * int(sqrtf(g2)) + 7, smoothed 3 x 3 and squared, read at (x >> 5) + (y >> 5) * (cols / 32) literally (aliasing when cols
 * or rows is no multiple of 32); per pot x pot cell the first pixel with the largest g2 above it; potential schedule 3, then
 * 4 .. 7 while more than 10 000, then once 3 + times - 2 if fewer than 6666 - type (0.9, 0.1).  A pixel is kept iff
 * depth != 0 && !isnan(depth), and - with semantics - its first-maximum class is not 10.  z = depth / scaling_factor,
 * x = ((u - cx) z) / fx, y = ((v - cy) z) / fy in float.  pixel[i] = v * cols + u of point i (room for
 * rows x cols ints: no method yields more); the row outputs may be NULL: xyz n x 3, feat n x (channels + 2) - the channels
 * / 255.0, then gradient_[v cols + u] / 500.0 + 0.5 and gradient_[v cols + u + 1] / 500.0 + 0.5, the reference's indexing of
 * its interleaved (dx, dy) array by the PIXEL index -, label n x num_classes, geotype n x 2.
 * CVO_E_INVALID, nothing written: rows / cols < 1, channels not 1 or 3, a missing pointer, fx / fy / scaling_factor not
 * finite or <= 0.  CVO_E_UNSUPPORTED: the other selection methods (OpenCV detectors, rand()), more than 2^24 pixels, an
 * image shape whose literal threshold index leaves the reference's allocation.  Images under 32 pixels on a side are
 * valid (no whole block: every threshold is zero).  Runs on the upload stream like a voxel selection; switch RGBD_HOST=1 / 0:
 * the CPU twin / the kernels for every size (unset: frames under 32768 pixels take the CPU twin). */
int cvo_rgbd_points(cvo_ctx* ctx, const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                    float* label, float* geotype);
int cvo_rgbd_points_host(const cvo_rgbd_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                         float* label, float* geotype);   /* CPU twin, no context */
/* The drivers' recipe in one call: the DSO_EDGES points through a voxel grid of side leaf / edge_divisor, the FULL points
 * through one of side leaf (the cvo_voxel_select contract and its refusals); every survivor as export_to_pcd<PointXYZRGB> and
 * the (XYZRGB, GeometryType) constructor leave it - F = 5: the first three features through min(255, int(f * 255)) and back
 * over 255.0 (the identity on the colour bytes), 0, 0; type EDGE (1, 0) / SURFACE (0, 1); no labels -, edge rows first.  The cloud
 * is the one cvo_cloud_upload makes of those rows.  pixel / is_edge (optional, room for 2 x rows x cols
 * entries): pixel index and set of every point; *n their number.  leaf, edge_divisor: finite and > 0. */
int cvo_cloud_upload_rgbd(cvo_ctx* ctx, const cvo_rgbd_frame_t* frame, float leaf, float edge_divisor, cvo_cloud** out,
                          int* pixel, unsigned char* is_edge, int* n);
/* ---- RGB-D frames that are already in device memory: the counterpart of cvo_cloud_from_device for frames ----
 * A network's class scores in a tensor, a rendered view, an image the caller's own HIP code produced: image, depth and scores
 * go in where they are, a RESIDENT cloud comes out.  No plane and no row crosses to the host, no host thread touches a pixel.
 * image / gray / depth are DENSE (no strides): rows x cols x channels bytes, rows x cols bytes, rows x cols uint16_t or float.
 * The score of class c at pixel (v, u) is the float at semantic + v * row_stride + u * pixel_stride + c * class_stride (bytes):
 * H x W x C is (4 C cols, 4 C, 4), C x H x W is (4 cols, 4, 4 rows cols), a column slice of a wider tensor has larger ones.
 * Contract (cvo_cloud_from_device's): every pointer is device memory of the context's device, complete when the call is made
 * (the caller synchronises its producer stream).  The library enqueues on its upload stream and returns after it has
 * synchronised that stream; the planes are only read - in place, nothing is staged -, the cloud owns what it keeps and may
 * outlive them.  With f the host copy of the frame (scores brought to H x W x C): cvo_cloud_from_rgbd_device's cloud is
 * interchangeable with cvo_cloud_upload of cvo_rgbd_points(f, method)'s rows, features zero-padded to 5 and classes to 19 (no
 * label array without classes); cvo_cloud_from_rgbd_device_recipe's with cvo_cloud_upload_rgbd(f, leaf, edge_divisor)'s - the
 * same n, n_edge and pixel order, the same rows on cvo_cloud_download, the same cvo_debug_cloud_order and one-hot detection,
 * bit-identical scores and solves.  cvo_debug_rgbd_stats reports what the host-frame device route reports for f.
 * Device frames ALWAYS take the kernels: RGBD_HOST and its crossover do not apply to them.  ORDER / NO_SORT / NO_ONEHOT act
 * through the ingest as for cvo_cloud_from_device.  pixel (HOST memory, optional): the pixel index of every point, room for
 * rows x cols (recipe: 2 x rows x cols) ints; NULL saves the copy and a synchronisation.
 * CVO_E_INVALID, nothing allocated, *out NULL, decided on the host before any launch: cvo_rgbd_points' refusals of shape,
 * channels, a missing plane, fx / fy / scaling_factor (and cvo_cloud_upload_rgbd's of leaf / edge_divisor), with the same
 * messages; a semantic stride that is 0 or no multiple of 4; a plane that is not aligned (float depth and scores 4 bytes,
 * uint16_t depth 2), that hipPointerGetAttributes does not report as device memory of this context's device (host, pinned
 * and managed memory, other devices), or whose extent does not fit the allocation behind it.  No pointer is read through
 * before it is classified.  CVO_E_UNSUPPORTED: the other selection methods, more than 2^24 pixels, a shape whose literal
 * threshold index leaves the reference's allocation, num_classes > 19 (a resident cloud holds 19 class columns). */
typedef struct cvo_rgbd_device_frame_t {
  int rows, cols, channels;          /* channels: 1 or 3 */
  const void* image;                 /* device, rows x cols x channels bytes, dense (BGR for 3): what RawImage holds after denoising */
  const void* gray;                  /* device, rows x cols bytes, dense, or NULL (then as in cvo_rgbd_frame_t) */
  const void* depth; int depth_type; /* device, rows x cols, dense; CVO_DEPTH_U16 / CVO_DEPTH_F32 */
  float fx, fy, cx, cy, scaling_factor;
  int num_classes;                   /* 0 .. 19; 0 = no semantics */
  const void* semantic;              /* device floats, strided as above; NULL without classes */
  size_t semantic_row_stride, semantic_pixel_stride, semantic_class_stride;   /* bytes */
} cvo_rgbd_device_frame_t;
/* CvoPointCloud(ImageRGBD, Calibration, method), method DSO_EDGES or FULL, as a resident cloud; *n (optional): its points */
int cvo_cloud_from_rgbd_device(cvo_ctx* ctx, const cvo_rgbd_device_frame_t* frame, int method, cvo_cloud** out, int* n, int* pixel);
/* the drivers' recipe, cvo_cloud_upload_rgbd's cloud; *n_edge (optional): the first n_edge points are the edges */
int cvo_cloud_from_rgbd_device_recipe(cvo_ctx* ctx, const cvo_rgbd_device_frame_t* frame, float leaf, float edge_divisor,
                                      cvo_cloud** out, int* n, int* n_edge, int* pixel);
/* CPU twin of the row and exclusion arithmetic, no context: `frame` holds HOST pointers with the same strides.  The rows of the
 * n given pixels (v * cols + u, each inside the image) as the resident cloud holds them - recipe 0: the constructor's rows of
 * `method` (features zero-padded to 5), recipe 1: the recipe's rows, is_edge[i] != 0 an edge row (required) - xyz n x 3,
 * feat n x 5, label n x 19 (zero-padded; may be NULL), geotype n x 2; excluded (optional): 1 where the pixel's first-maximum
 * class is 10.  Any output may be NULL.  CVO_E_INVALID: what cvo_cloud_from_rgbd_device refuses of the frame's fields, n < 0,
 * a pixel outside the image; CVO_E_UNSUPPORTED: num_classes > 19, another method. */
int cvo_rgbd_frame_rows_host(const cvo_rgbd_device_frame_t* frame, int recipe, int method, int n, const int* pixel,
                             const unsigned char* is_edge, float* xyz, float* feat, float* label, float* geotype,
                             unsigned char* excluded);
/* ---- CV_FAST point selection: replaces select_points_from_image's CV_FAST branch (CvoPointCloud.cpp:273-312) ----
 * cv::FAST(gray, keypoints, t, nonmax = false), TYPE_9_16: a pixel with 3 <= x < cols - 3, 3 <= y < rows - 3 is a corner at t
 * iff 9 cyclically contiguous pixels of its radius-3 ring are all brighter than I_p + t or all darker than I_p - t (strict;
 * t clamped to 0 .. 255); keypoints in row-major order.  The reference's schedule, literally: the first call is ALWAYS at 5;
 * while more than num_want keypoints, ++thresh and call again, stopping at break_thresh; then while fewer than num_min,
 * --thresh and call again, stopping at 0; the keypoints of the LAST call stand (with no loop taken: those at 5, not at
 * thresh).  One departure: a lowering loop that would pass below 0 ends there.  pixel: v * cols + u of every keypoint
 * (room for rows x cols ints); *threshold_used (optional): the last call's threshold.  Images under 7 pixels on a side are
 * valid and have no corners.  CVO_E_INVALID, nothing written: rows / cols < 1, a missing pointer, a schedule with a negative
 * field, thresh > 255 or num_min > num_want.  CVO_E_UNSUPPORTED: more than 2^24 pixels.  Runs on the upload stream; switch
 * STEREO_HOST as for the stereo front end below.  RGB-D users get upstream's CV_FAST pixels with CVO_FAST_RGBD. */
#define CVO_SELECT_CV_FAST 0
typedef struct cvo_fast_schedule_t {
  int thresh, num_want, num_min, break_thresh;
} cvo_fast_schedule_t;
#define CVO_FAST_RGBD {9, 15000, 12000, 13}
#define CVO_FAST_STEREO {4, 24000, 15000, 50}
#define CVO_FAST_STEREO_SEMANTIC {4, 28000, 15000, 50}   /* a stereo frame with classes */
int cvo_fast_select(cvo_ctx* ctx, int rows, int cols, const uint8_t* gray, const cvo_fast_schedule_t* schedule,
                    int* pixel /* rows*cols */, int* n, int* threshold_used);
int cvo_fast_select_host(int rows, int cols, const uint8_t* gray, const cvo_fast_schedule_t* schedule, int* pixel, int* n,
                         int* threshold_used);   /* CPU twin, no context */
/* ---- stereo front end: replaces CvoPointCloud(ImageStereo, Calibration, PointSelectionMethod) (CvoPointCloud.cpp:680-773,
 * StaticStereo.cpp:84-107, is_good_point :39-49) FROM A GIVEN DISPARITY MAP (upstream computes it with libelas, which is not
 * part of this library - cvo_stereo_disparity below is the library's own matcher, another algorithm; the invalid marker -10 of
 * both is rejected like every disparity below 0.05) and the per-frame block of the
 * multi-frame KITTI driver (main_multi_frame_irls_kitti.cpp:235-292) ----
 * image / gray / semantic: as in cvo_rgbd_frame_t (the LEFT image, after RawImage's denoising: cvo_nlm_denoise). */
typedef struct cvo_stereo_frame_t {
  int rows, cols, channels;    /* channels: 1 or 3 */
  const uint8_t* image;        /* rows x cols x channels */
  const uint8_t* gray;         /* rows x cols, or NULL */
  const float* disparity;      /* rows x cols, left disparity in pixels */
  float fx, fy, cx, cy;        /* Calibration::intrinsic() */
  float baseline;              /* Calibration::baseline(); its absolute value is used */
  int num_classes;             /* 0 = no semantics */
  const float* semantic;       /* rows x cols x num_classes, or NULL */
} cvo_stereo_frame_t;
/* The points of the reference constructor, in its order.  Candidates: CV_FAST - cvo_fast_select with CVO_FAST_STEREO
 * (CVO_FAST_STEREO_SEMANTIC with classes), type (1, 0); DSO_EDGES and FULL - exactly cvo_rgbd_points' candidates, types
 * (0.9, 0.1) and (0.5, 0.5).  A candidate (u, v) is kept iff 1 <= u <= cols - 2 && 1 <= v <= rows - 2; its disparity is not
 * below 0.05f (0.05f itself is kept; a NaN passes this and every later test, as upstream); 2 <= u <= cols - 2 &&
 * 100 <= v <= rows - 30 (a frame with fewer than 130 rows yields no points); !(|xyz| >= 55); and - with semantics - its
 * first-maximum class is not 10.  In float, every operation rounded on its own: depth = |baseline| fx / disparity,
 * xyz = (Kinv (u, v, 1)) depth with Eigen 3.3's cofactor inverse (invdet = 1 / (fx fy), Kinv00 = fy invdet, Kinv11 =
 * fx invdet, Kinv02 = -(cx fy) invdet, Kinv12 = -(fx cy) invdet, Kinv22 = (fx fy) invdet), |xyz| = sqrtf((x x + y y) + z z).
 * Outputs as cvo_rgbd_points: pixel (room for rows x cols ints), xyz, feat n x (channels + 2), label, geotype.
 * CVO_E_INVALID, nothing written: rows / cols < 1, channels not 1 or 3, a missing pointer, fx / fy / baseline not finite
 * or zero.  CVO_E_UNSUPPORTED: the other selection methods, more than 2^24 pixels, for DSO_EDGES an image shape whose
 * literal threshold index leaves the reference's allocation.  Runs on the upload stream; switch STEREO_HOST=1 / 0: the CPU
 * twin / the kernels for every size (unset: frames under 10000 pixels take the CPU twin; the recipe below: under 24000). */
int cvo_stereo_points(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                      float* label, float* geotype);
int cvo_stereo_points_host(const cvo_stereo_frame_t* frame, int method, int* pixel, int* n, float* xyz, float* feat,
                           float* label, float* geotype);   /* CPU twin, no context */
/* The pairwise driver's cloud (main_cvo_gpu_align_raw_image.cpp:61-91): the constructor's rows through cvo_cloud_upload -
 * the channels + 2 features zero-padded to 5 (a mono frame has 3), labels padded or cut to 19 classes.  Rows with a
 * non-finite coordinate (NaN disparity) are treated as cvo_cloud_upload treats them.  pixel (optional), *n (optional). */
int cvo_cloud_upload_stereo(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, int method, cvo_cloud** out, int* pixel, int* n);
/* The multi-frame KITTI driver's block: cvo_cloud_upload_rgbd's recipe on the stereo points - DSO_EDGES points through a voxel
 * grid of side leaf / edge_divisor (the driver's divisor is 5), FULL points through one of side leaf, rows F = 5 colour
 * bytes, types EDGE / SURFACE, edge first.  The voxel contract's refusals pass through (a NaN disparity inside the kept
 * region is one: a non-finite coordinate).  pixel / is_edge: room for 2 x rows x cols entries. */
int cvo_cloud_upload_stereo_recipe(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, float leaf, float edge_divisor, cvo_cloud** out,
                                   int* pixel, unsigned char* is_edge, int* n);
/* ---- LiDAR front end: replaces CvoPointCloud(PointCloud<PointXYZI>::Ptr, target_num_points, beam_num, LOAM) and its
 * semantic twin (CvoPointCloud.cpp:964-1136): LidarPointSelector::edge_detection, then LeGoLoamPointSelection::cloudHandler
 * (ring ids from the 4 -> 1 quadrant transitions, range image, ground, components with the validity rule, the segmented
 * cloud, smoothness, occlusion marks, up to 20 edges per sixth of a ring, the std::rand() % 4 thinning of the rest) ----
 * The statement of what is computed, departures from upstream's text included, is tests/np_lidar.py. */
typedef struct cvo_lidar_scan_t {
  int n;                       /* points, in the order the sensor returned them */
  const float* xyzi;           /* n x 4: x, y, z, intensity in upstream's axes (x = -raw.y, y = -raw.z, z = raw.x) */
  const int* semantic;         /* n class ids, -1 = unlabelled; NULL = no semantics */
  int num_classes;             /* 0 without semantics */
} cvo_lidar_scan_t;
typedef struct cvo_lidar_config_t {
  int n_scan, horizon_scan;    /* the range image: at most 128 x 4096 */
  float ang_res_x;             /* degrees per column */
  int ground_scan_ind;         /* rows 0 .. ground_scan_ind are tested for ground; below n_scan */
  float sensor_min_range, sensor_mount_angle /* degrees, |.| <= 45 */;
  float segment_theta, segment_alpha_x, segment_alpha_y;   /* radians, in (0, pi / 2) */
  int segment_valid_point_num, segment_valid_line_num;
  float edge_threshold, surf_threshold;
  double intensity_bound, depth_bound, distance_bound;     /* edge_detection's */
  int beam_num;                /* edge_detection's ring limit */
  /* derived by cvo_lidar_config_derive, the only libm calls of the front end: tan(segment_theta), sin / cos of the two
   * alphas, tan(mount -/+ 10 degrees), tan(mount -/+ 3 degrees).  Every angle test is a cross-multiplication with these. */
  double tan_theta, sin_alpha_x, cos_alpha_x, sin_alpha_y, cos_alpha_y, tan_ground_lo, tan_ground_hi, tan_self_lo, tan_self_hi;
} cvo_lidar_config_t;
/* glibc's default rand() (the additive-feedback TYPE_3 generator), restated: the stream extractFeatures draws from. */
typedef struct cvo_lidar_rand_t {
  unsigned int r[31];
  int front, rear;
} cvo_lidar_rand_t;
/* The HDL-64 values of LeGoLoamPointSelection.hpp:296-341 and the constructors' bounds (distance 40, semantic: 75), derived
 * fields included.  cvo_lidar_config_derive recomputes the derived fields after a change of the angles. */
void cvo_lidar_config_default(cvo_lidar_config_t* cfg, int semantic);
void cvo_lidar_config_derive(cvo_lidar_config_t* cfg);
/* srand(seed): seed 1 is the stream of a process that never called srand. */
void cvo_lidar_rand_seed(cvo_lidar_rand_t* state, unsigned int seed);
/* One draw, as rand() returns it: the stepping function the library's calls use. */
unsigned int cvo_lidar_rand_next(cvo_lidar_rand_t* state);
/* The indices of the selected points: edge_detection's list, then LeGO-LOAM's - per ring and sixth the edges in pick order,
 * then the thinned rest ascending -, duplicates kept (a point can be in both lists).  is_edge (optional): 1 for
 * edge_detection's points and LeGO-LOAM's edges, 0 for thinned points.  With semantics, unlabelled points are in neither
 * list (their draws are still consumed).  index / is_edge: room for 2 x n entries.  `rand` advances by exactly the draws
 * upstream would make (one per non-edge point of every sixth), so a driver chains frames with one state.
 * CVO_E_INVALID, nothing written and no draw consumed: a missing pointer, n < 1, a config field that is not positive or out
 * of range (n_scan > 128, horizon_scan > 4096, ground_scan_ind >= n_scan, ...), derived fields that do not match the
 * angles, a label outside -1 .. num_classes - 1, a coordinate that is not finite or not below 1e15 in magnitude.
 * CVO_E_UNSUPPORTED: more than 2^24 points.  cvo_lidar_select runs on the upload stream; switch LIDAR_HOST=1 / 0: the CPU
 * twin / the kernels for every size (unset: scans under 12000 points take the CPU twin). */
int cvo_lidar_select_host(const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand, int* index,
                          unsigned char* is_edge, int* n);   /* CPU twin, no context */
int cvo_lidar_select(cvo_ctx* ctx, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand,
                     int* index, unsigned char* is_edge, int* n);
/* The constructor's cloud: the selected points through cvo_cloud_upload with F = 1 (intensity, zero-padded to 5), type
 * (1, 0) and - with semantics - one-hot labels, padded or cut to 19 classes.  index (optional), *n (optional). */
int cvo_cloud_upload_lidar(cvo_ctx* ctx, const cvo_lidar_scan_t* scan, const cvo_lidar_config_t* cfg, cvo_lidar_rand_t* rand,
                           cvo_cloud** out, int* index, int* n);
/* ---- non-local-means denoising: replaces RawImage's first statement (RawImage.cpp:21-24),
 * cv::fastNlMeansDenoising(image, image, 10, 7, 21) for gray frames and the middle of
 * cv::fastNlMeansDenoisingColored(image, image, 10, 10, 7, 21) for colour ones ----
 * OpenCV's FastNlMeansDenoisingInvoker for 8-bit images with the squared distance, restated from OpenCV's published
 * algorithm (parity with a given OpenCV binary is unpinned: OpenCV is not part of this library's tests); the statement is
 * tests/np_nlm.py.  th = template_window / 2, sh = search_window / 2, tw = 2 th + 1, sw = 2 sh + 1 (an even size grows by
 * one), b = th + sh.  The image is extended by b on every side with BORDER_REFLECT_101 (repeated on images smaller than
 * b + 1).  mult = INT_MAX / (sw sw 255); shift: the smallest p with (1 << p) >= tw tw; m = (1 << shift) / (tw tw);
 * weight[d] = lrint(mult exp(-(d m) / hh)) in double, ties to even, for d < int(255 255 channels / m + 1), hh = h h channels
 * evaluated in float, entries under 0.001 mult set to 0.  For every pixel and every offset of [-sh, sh]^2: dist = the sum
 * over the tw x tw template and the channels of the squared differences of the two patches, w = weight[dist >> shift];
 * out[c] = min(255, (sum w q[c] + sum w / 2) / sum w) in unsigned 32-bit arithmetic, q the offset pixel.
 * channels: 1, 2 or 3, interleaved; 3 is OpenCV's fastNlMeansDenoising of a CV_8UC3 image, NOT the Colored call.
 * dst == src (in place) is allowed.  CVO_E_INVALID, nothing written: a missing pointer, rows / cols < 1, channels outside
 * 1 .. 3, h / h_color not finite or <= 0 (upstream's h = 0 branch is not reproduced), a window < 1.  CVO_E_UNSUPPORTED, on
 * both routes: th > 3 or sh > 10 (upstream only ever asks for 7 / 21), more than 2^24 pixels.  cvo_nlm_denoise runs on the
 * context's upload stream like the front ends: it neither waits for nor delays a solve.  Switch NLM_HOST=1 / 0: the CPU twin
 * (one thread) / the kernel of cvo_k_nlm.h for every size (unset: images under 256 pixels take the CPU twin). */
typedef struct cvo_nlm_config_t {
  float h;
  int template_window, search_window;
} cvo_nlm_config_t;
void cvo_nlm_config_default(cvo_nlm_config_t* cfg);   /* 10, 7, 21: RawImage's call */
/* The one place the table is built (double, the host's exp); the twin and the device route take it from here.  Writes the
 * first min(capacity, *n_table) entries to weight (NULL: the sizes only); *n_nonzero: the length of the nonzero leading run.
 * Any output pointer may be NULL.  Refusals as above. */
int cvo_nlm_weights(const cvo_nlm_config_t* cfg, int channels, int* weight, int capacity, int* n_table, int* n_nonzero,
                    int* mult, int* shift);
int cvo_nlm_denoise_host(int rows, int cols, int channels, const uint8_t* src, const cvo_nlm_config_t* cfg,
                         uint8_t* dst);   /* CPU twin, no context */
int cvo_nlm_denoise(cvo_ctx* ctx, int rows, int cols, int channels, const uint8_t* src, const cvo_nlm_config_t* cfg,
                    uint8_t* dst);
/* The middle of fastNlMeansDenoisingColored: plane 0 of a rows x cols x 3 Lab image denoised as a 1-channel image with
 * cfg->h, planes 1-2 as one 2-channel image with h_color, the same windows, re-interleaved; on the device one upload, one
 * download, one synchronisation.  BGR <-> Lab stays the caller's (cv::cvtColor with COLOR_LBGR2Lab / COLOR_Lab2LBGR):
 * OpenCV's 8-bit Lab is table-driven fixed point that differs between versions - the position `gray` takes for BGR -> gray. */
int cvo_nlm_denoise_lab_host(int rows, int cols, const uint8_t* lab, const cvo_nlm_config_t* cfg, float h_color,
                             uint8_t* dst);   /* CPU twin, no context */
int cvo_nlm_denoise_lab(cvo_ctx* ctx, int rows, int cols, const uint8_t* lab, const cvo_nlm_config_t* cfg, float h_color,
                        uint8_t* dst);
/* ---- stereo matcher: what cvo::ImageStereo(left, right) needs a disparity from.  NOT upstream's matcher: upstream computes
 * the left disparity with libelas (StaticStereo::disparity), whose support-point triangulation and filters are not restated;
 * this is the library's own semi-global matching over a census cost, so poses from its map differ from poses from libelas's,
 * and parity with any other SGM implementation is unpinned.  The statement is tests/np_sgm.py; the CPU twin and the kernels of
 * cvo_k_sgm.h equal it exactly.  left / right: rectified 8-bit gray planes of rows x cols.
 * Census: 9 wide x 7 high, coordinates clamped to the image, bit = neighbour < centre for the 62 neighbours in row-major window
 * order, first neighbour most significant.  Cost: C(v, u, d) = popcount(cL[v, u] ^ cR[v, u - d]) for u - d >= 0, else 62, for d
 * in [0, max_disparity).  Paths (dv, du) in the order (0,1) (0,-1) (1,0) (-1,0) (1,1) (1,-1) (-1,1) (-1,-1), the first `paths`
 * of them: with q = p - r inside the image and m = min_k L(q, k), L(p, d) = C(p, d) + min(L(q, d), L(q, d - 1) + p1,
 * L(q, d + 1) + p1, m + p2) - m (terms outside [0, max_disparity) left out), else L(p, d) = C(p, d); S = sum of the L (a
 * byte each, 16 bits the sum).  Winner d* = first argmin S, s1 its sum, s2 = min S over |d - d*| > 1; invalid when
 * s2 (100 - uniqueness) < 100 s1.  Sub-pixel for 0 < d* < max_disparity - 1 and den = S(d* - 1) + S(d* + 1) - 2 s1 > 0:
 * (float)d* + (float)(S(d* - 1) - S(d* + 1)) / (float)(2 den), else (float)d*.  Left-right check (lr_max_diff >= 0): dR(v, x) =
 * first argmin_d S(v, x + d, d) over x + d < cols; invalid when u - d* < 0 or |dR(v, u - d*) - d*| > lr_max_diff.  Invalid
 * pixels are written as -10.f, the marker cvo_stereo_points rejects.  The matcher itself filters nothing; libelas's three
 * post-passes are cvo_disparity_filter below (cvo_stereo_disparity_filtered runs both).
 * CVO_E_INVALID, nothing written: a missing pointer, rows / cols < 1, max_disparity not 64 / 128 / 256, not 0 <= p1 <= p2 <= 193,
 * uniqueness outside 0 .. 99, paths not 4 or 8.  CVO_E_UNSUPPORTED: more than 2^24 pixels, rows x cols x max_disparity x 2 bytes
 * of sums above 2 GiB.  cols < max_disparity and 1 x 1 frames are valid.  cvo_stereo_disparity runs on the context's upload
 * stream like the front ends.  Switch SGM_HOST=1 / 0: the CPU twin (one thread) / the kernels for every size (unset: frames
 * under 128 pixels take the CPU twin: measured, profiles/sgm/crossover.txt). */
typedef struct cvo_sgm_config_t {
  int max_disparity;           /* 64, 128 or 256 */
  int p1, p2;                  /* 0 <= p1 <= p2 <= 193 */
  int uniqueness;              /* percent, 0 .. 99 */
  int lr_max_diff;             /* < 0: no left-right check */
  int paths;                   /* 4 or 8 */
} cvo_sgm_config_t;
void cvo_sgm_config_default(cvo_sgm_config_t* cfg);   /* 128, 10, 120, 5, 1, 8 */
int cvo_stereo_disparity_host(int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* cfg,
                              float* disparity);   /* CPU twin, no context */
int cvo_stereo_disparity(cvo_ctx* ctx, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* cfg,
                         float* disparity);
/* "Two images in, cloud out": cvo_stereo_disparity of (the frame's gray plane - frame->gray, a 1-channel image, or the BGR
 * image through the front end's own gray formula -, right_gray), downloaded, then cvo_cloud_upload_stereo exactly as it is
 * on a copy of the frame that carries the map.  frame->disparity is not read and may be NULL.  Refusals: the matcher's, then
 * cvo_cloud_upload_stereo's. */
int cvo_cloud_upload_stereo_pair(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, const uint8_t* right_gray, const cvo_sgm_config_t* cfg,
                                 int method, cvo_cloud** out, int* pixel, int* n);
/* ---- disparity post-filter: the three passes libelas runs on the left map after matching (StaticStereo::disparity, ROBOTICS
 * parameters, postprocess_only_left) - removeSmallSegments, gapInterpolation, adaptiveMean, in that order - on any float map
 * whose invalid pixels are negative (the matcher's -10 included).  The statement is tests/np_dfilter.py, restated from
 * elas.cpp; the CPU twin and the kernels of cvo_k_dfilter.h equal it exactly, and it equals libelas's own compiled passes
 * exactly (tests/golden/dfilter_elas.npz) outside the pixels where libelas's result depends on uninitialised memory: its
 * adaptiveMean reads the never-written part of a malloc'ed buffer, which reaches column 3 and rows 4 - 6 and rows - 6 .. rows - 4
 * of its output; here that buffer starts as a copy of the map.  Built: the full-resolution branch.  NOT built, because
 * upstream never turns them on: param.subsampling, the add_corners extrapolation, the median filter; libelas's matcher is
 * not built either, and the filtered map is downloaded and uploaded again before the front end reads it.
 * Speckle: 4-connected segments of valid (>= 0) pixels, neighbours joined when fabsf(a - b) <= speckle_sim_threshold; segments
 * of fewer than speckle_size pixels, and every negative value, become -10.f; speckle_size <= 1: no-op.  Gap: rows, then
 * columns on the rows' result: a run of 1 .. ipol_gap_width invalid pixels with a valid pixel on both sides inside the line
 * is filled with (d1 + d2) / 2 when fabsf(d1 - d2) < 3, else min(d1, d2); width 0: no-op.  Adaptive mean (adaptive_mean != 0):
 * a horizontal, then a vertical 8-tap pass (centre - 4 .. centre + 3) whose weights are max(0, 4 - masked |difference|) with
 * libelas's mask as compiled (the bit pattern 0x4F000000: 4 below a difference of 2, 2 in [2, 8), 0 from 8) and whose sums
 * run in libelas's ring order, which depends on the coordinate mod 8; invalid pixels enter as -10.
 * CVO_E_INVALID, nothing written: a missing pointer, rows / cols < 1, speckle_sim_threshold not finite or negative,
 * speckle_size or ipol_gap_width < 0, a value that is not finite, a negative value that is not < -speckle_sim_threshold
 * (libelas's result would depend on its seed order).  CVO_E_UNSUPPORTED: more than 2^24 pixels.  out == in is allowed.
 * cvo_disparity_filter runs on the context's upload stream like the front ends.  Switch DFILTER_HOST=1 / 0: the CPU twin (one
 * thread) / the kernels for every size (unset: maps under 32768 pixels take the CPU twin: measured, profiles/dfilter/crossover.txt). */
typedef struct cvo_dfilter_config_t {
  float speckle_sim_threshold; /* finite, >= 0 */
  int speckle_size;            /* >= 0; <= 1: no speckle pass */
  int ipol_gap_width;          /* >= 0; 0: no gap pass */
  int adaptive_mean;           /* 0: no mean pass */
} cvo_dfilter_config_t;
void cvo_dfilter_config_default(cvo_dfilter_config_t* cfg);   /* 1, 200, 3, 1: libelas's ROBOTICS setting */
int cvo_disparity_filter_host(int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, float* out);   /* CPU twin, no context */
int cvo_disparity_filter(cvo_ctx* ctx, int rows, int cols, const float* in, const cvo_dfilter_config_t* cfg, float* out);
/* cvo_stereo_disparity, then cvo_disparity_filter of its map: the map stays on the device between the two, one download at
 * the end.  Refusals: the matcher's, then the filter's configuration (a speckle_sim_threshold of 10 or more included: the
 * matcher's -10 would not lie below it). */
int cvo_stereo_disparity_filtered(cvo_ctx* ctx, int rows, int cols, const uint8_t* left, const uint8_t* right, const cvo_sgm_config_t* sgm_cfg,
                                  const cvo_dfilter_config_t* dfilter_cfg, float* disparity);
/* cvo_cloud_upload_stereo_pair with cvo_stereo_disparity_filtered in the place of cvo_stereo_disparity. */
int cvo_cloud_upload_stereo_pair_filtered(cvo_ctx* ctx, const cvo_stereo_frame_t* frame, const uint8_t* right_gray,
                                          const cvo_sgm_config_t* sgm_cfg, const cvo_dfilter_config_t* dfilter_cfg, int method,
                                          cvo_cloud** out, int* pixel, int* n);
/* ---- semantic voxel map: posed clouds fused into a voxel map, its occupied voxels read out as a cloud.  It is upstream's
 * bki_mapping_lib as its driver main_local_mapping.cpp uses it - semantic_bki::SemanticBKIOctoMap::insert_pointcloud_csm under the
 * counting sensor model with free-space beam samples, block_depth 1, and CvoPointCloud(const SemanticBKIOctoMap*, num_classes).
 * The statement is tests/np_bki.py; the CPU twin and the kernels of cvo_k_bki.h equal it bit for bit (shared arithmetic:
 * cvo_bki_math.h).  Its choices where upstream's text pins nothing - feature rows summed in ascending hit index, the cloud in
 * ascending key order - and its departures are listed there and in DESIGN.md section 4; parity with upstream's binary is
 * unpinned.  num_classes = 0 is an extension: every hit is class 1 of a two-class map and the cloud has no label rows.
 * A map of a context lives on ONE side, taken at its first insert and kept: switch BKI_HOST=1 / 0 the CPU twin (one thread) /
 * the device; unset, a map whose first insert has fewer than 2129 training points takes the twin (measured: profiles/bki/bki_probe.txt).  Inserts and read-outs of a device map run on the
 * context's upload stream, like a voxel selection; the table grows by itself (k_bki_rehash) before an insert could take it
 * past half full.  Close every map before its context is destroyed.
 * Refusals leave the map as it was.  CVO_E_INVALID: resolution or free_resolution not finite or <= 0, a threshold outside
 * [0, 1], prior negative or not finite, num_classes outside 0 .. 19 (cvo_map_open); a coordinate or origin that is not finite,
 * a hit, beam sample or origin whose block index leaves [1, 2^20 - 2] on an axis, label rows missing on a map with classes
 * (insert; cvo_last_error names the hit).  CVO_E_UNSUPPORTED: block_depth != 1; 2^24 training points or more in one insert
 * (hits kept, their beam samples, the origin); a hit with 65536 beam samples or more; a table beyond 2^30 slots. */
typedef struct cvo_map cvo_map;
typedef struct cvo_map_config_t {
  float resolution;      /* voxel edge, > 0 */
  int block_depth;       /* 1 */
  int num_classes;       /* C: classes of a label row, 0 .. 19; the map has C + 1, class 0 = free space */
  float sf2, ell;        /* the sparse kernel's scale and length (cvo_map_set_kernel); the counting kernel ignores them, as upstream's */
  float prior;           /* ms of a new voxel, >= 0 */
  float var_thresh;      /* accepted, changes nothing */
  float free_thresh, occupied_thresh; /* in [0, 1] */
  float ds_resolution;   /* accepted, changes nothing */
  float free_resolution; /* distance between beam samples, > 0 */
  float max_range;       /* > 0: hits farther from the origin are dropped; <= 0: off */
} cvo_map_config_t;
void cvo_map_config_default(cvo_map_config_t* cfg);   /* main_local_mapping.cpp: 0.05, 1, 0, 1, 1, 0, 1, 0.65, 0.9, -1, 1, -1 */
int cvo_map_open(cvo_ctx* ctx, const cvo_map_config_t* cfg, long long initial_voxels, cvo_map** out);
void cvo_map_close(cvo_map* map);
/* n hits already in the map frame: xyz n x 3, feat n x 5 or NULL (zeros), label n x num_classes (NULL only with 0 classes) */
int cvo_map_insert(cvo_map* map, int n, const float* xyz, const float* feat, const float* label, const float origin[3]);
/* the rows moved by a 3x4 row-major pose as cvo_cloud_transformed moves them, the pose's translation as origin */
int cvo_map_insert_posed(cvo_map* map, int n, const float* xyz, const float* feat, const float* label, const float pose12[12]);
int cvo_map_size(cvo_map* map, long long* voxels, long long* occupied);   /* either pointer may be NULL; host maps too */
/* The OCCUPIED voxels in ascending key order: *n rows; xyz / feat / label (n x 3 / 5 / num_classes, each optional) are written
 * when capacity >= *n (CVO_E_INVALID otherwise, *n set).  resident != NULL: the cloud cvo_cloud_upload makes of exactly those
 * rows (label rows of fewer than 19 classes followed by zeros), to align a new frame against. */
int cvo_map_cloud(cvo_map* map, long long capacity, float* xyz, float* feat, float* label, long long* n, cvo_cloud** resident);
/* A resident cloud in, a resident cloud out: on a map of the device side no row of either passes through the host.
 * The rows of a resident cloud, in ORIGINAL order, as the hits of one insert.
 * pose12 (3x4 row-major float, or NULL): the rows moved as cvo_cloud_transformed moves them
 *   (transform_point_pose_vec).  NULL: the stored bits, nothing is multiplied.
 * origin (3 floats, or NULL): NULL means the pose's translation, as cvo_map_insert_posed.
 *   pose12 == NULL && origin == NULL is refused.
 * The map is afterwards bit for bit what cvo_map_insert_posed (a pose, no origin) or cvo_map_insert of the moved rows leaves
 * when given the rows cvo_cloud_download returns: a hit's label row is the first num_classes of the cloud's 19 columns, a
 * cloud that holds no features inserts as feat == NULL does, n == 0 inserts the origin alone.  The hits are staged on the
 * device (k_bki_stage); the side rule is the map's: an undecided map with BKI_HOST unset takes the host side when the device
 * counts fewer than 2129 training points, and a map of the host side has the staged rows copied down for the twin.
 * Refusals leave the map as it was, cvo_last_error begins "cvo_map_insert_cloud:".  CVO_E_INVALID: a NULL handle, a map of
 * cvo_map_open_host, a cloud of another context, both pointers NULL, a pose or origin that is not finite, a moved coordinate
 * that is not finite (the text names the hit), label rows missing on a map with classes, a block index outside
 * [1, 2^20 - 2]; CVO_E_UNSUPPORTED: as cvo_map_insert. */
int cvo_map_insert_cloud(cvo_map* map, const cvo_cloud* cloud, const float pose12[12], const float origin[3]);
/* The OCCUPIED voxels, ascending key order, as a resident cloud; no row comes down to the host.
 * *n (optional): their number.  Interchangeable with the cloud cvo_map_cloud(..., &resident) returns: the same rows, order,
 * one-hot detection, scores and solves; the rows go from k_bki_rows to cvo_cloud_from_device's ingest where they are, so its
 * route rule orders them (ORDER=wide above 16 384 voxels).  A map of the host side uploads the twin's rows. */
int cvo_map_cloud_resident(cvo_map* map, cvo_cloud** out, long long* n);
/* The kernel of the inserts that follow, on a map of either side or of cvo_map_open_host, between any two inserts; it applies
 * to cvo_map_insert, _insert_posed, _insert_cloud and _insert_host alike.  CVO_MAP_KERNEL_CSM, the default: the counting
 * sensor model above.  CVO_MAP_KERNEL_SPARSE: SemanticBKInference::predict with covSparse over get_extended_block's seven
 * blocks, at block_depth 1 - every training point, beam samples and origin included, votes into the voxels of its blocks and
 * of their face neighbours with the weight ((2 + cos 2 pi d)(1 - d) / 3 + sin 2 pi d / (2 pi)) sf2 of its distance d (in
 * units of ell) to the voxel's centre, 0 from d = 1 on; every touched block and every face neighbour of one is stored.
 * The statement is tests/np_bki_sparse.py (its own sin / cos routine, sums in ascending training order, slot by slot); the
 * twin and the kernels of cvo_k_bki_sparse.h equal it bit for bit, and the same insert gives the same bits on every run.
 * The side rule is unchanged.  One more cap: 2^24 block memberships or more in one sparse insert are CVO_E_UNSUPPORTED,
 * nothing written.  CVO_E_INVALID, the map and its kernel as they were, cvo_last_error begins "cvo_map_set_kernel:": a NULL
 * handle, an unknown kernel, SPARSE on a map whose sf2 or ell is not finite and > 0. */
#define CVO_MAP_KERNEL_CSM 0
#define CVO_MAP_KERNEL_SPARSE 1
int cvo_map_set_kernel(cvo_map* map, int kernel);
/* the CPU twin on a map without a context */
int cvo_map_open_host(const cvo_map_config_t* cfg, cvo_map** out);
void cvo_map_close_host(cvo_map* map);
int cvo_map_insert_host(cvo_map* map, int n, const float* xyz, const float* feat, const float* label, const float origin[3]);
int cvo_map_cloud_host(cvo_map* map, long long capacity, float* xyz, float* feat, float* label, long long* n);
/* ---- the read side of the map: what is at this point, what does this segment meet first, what does the map look like from
 * this pose.  The statement is tests/np_bki_query.py; the CPU twin and the kernels of cvo_k_bki_query.h equal it bit for bit
 * (shared arithmetic: cvo_bki_math.h).  A query only reads: the table (keys, ms, fs, counters) is bit for bit what it was.
 * It runs where the map lives - a map of the device side on the context's upload stream, ordered behind every insert and
 * synchronised on return; a map of the host side, and a map without an insert, which stays undecided, through the twin.
 *
 * cvo_map_query is upstream's SemanticBKIOctoMap::search(x, y, z) over n points (xyz n x 3, map frame) with the node's
 * getters.  A point's voxel is the key of its k0 = int64(p / (double)resolution + 524288.5) per axis (block_to_hash_key) -
 * ONE voxel, not the up to 8 closed boxes an inserted hit belongs to: a point on a face was stored in two voxels and is found
 * in one.  Every output pointer may be NULL:
 *   found      1: a stored voxel has this key; 0: none; 2: "outside" - a coordinate is not finite or a k0 leaves [1, 2^20 - 2]
 *   state      0 FREE, 1 OCCUPIED, 2 UNKNOWN: get_state, for a stored voxel the read-out's rule on its ms
 *   semantics  get_semantics: the first maximum of ms / sum in float (Semantics::update's max_element over get_probs)
 *   probs      n x (max(num_classes, 1) + 1): get_probs, ms[c] / sum
 *   vars       as probs: get_vars, ((ms[c] / sum) - (ms[c] / sum) * (ms[c] / sum)) / (sum + 1), each operation a float operation
 *   feat       n x 5: get_features, fs / (sum of ms[1:])
 *   centre     n x 3: float(k0 - 524288) * resolution per axis
 * A point without a stored voxel is answered by upstream's default node Semantics(): found 0, state UNKNOWN, ms = prior in
 * every class and fs = 0 pushed through the same float expressions (prior 0: NaN probabilities, as upstream's), semantics -1
 * (upstream leaves the member uninitialised; -1 is this library's choice).  A point "outside" is answered the same way with
 * found 2 and a NaN centre - a deliberate difference from the inserts, which refuse such a coordinate: a query is read-only,
 * and one bad pixel must not fail a frame.
 * Refused, CVO_E_INVALID, cvo_last_error begins with the function's name: a NULL map, n < 0, xyz NULL with n > 0 (n == 0 is
 * accepted); a map of cvo_map_open_host given to cvo_map_query or a map of a context given to cvo_map_query_host.
 * cvo_map_query_cloud: the rows of a resident cloud, in ORIGINAL order, moved as cvo_cloud_transformed moves them
 * (transform_point_pose_vec; pose12 NULL: the stored bits); on a map of the device side no row passes through the host
 * (k_bki_query reads x4[i] as k_bki_stage does).  The results equal cvo_map_query of cvo_cloud_download's coordinates moved
 * on the host with the same float arithmetic, bit for bit.  Also refused: a NULL cloud, a cloud of another context, a map of
 * cvo_map_open_host, a pose that is not finite. */
typedef struct cvo_map_query_out_t {
  uint8_t* found;
  uint8_t* state;
  int32_t* semantics;
  float* probs;
  float* vars;
  float* feat;
  float* centre;
} cvo_map_query_out_t;
int cvo_map_query(cvo_map* map, int n, const float* xyz, const cvo_map_query_out_t* out);
int cvo_map_query_cloud(cvo_map* map, const cvo_cloud* cloud, const float pose12[12], const cvo_map_query_out_t* out);
int cvo_map_query_host(cvo_map* map, int n, const float* xyz, const cvo_map_query_out_t* out);
/* cvo_map_raycast: n_rays segments origin[i] -> end[i] (3 floats each, map frame).  This is the library's own walk over
 * the map's voxels, written for this library; it is NOT upstream's RayCaster and is not compared with it.  RayCaster has no
 * caller upstream, and its text stands against restating it: its diagonal branch takes three from the step count for two
 * steps; a ray whose start block is not stored sees nothing at all; and with xy_error > 0 and xz_error == 0 (or xy_error < 0
 * and yz_error == 0) none of its four branches applies, so the same voxel is returned until the count runs out.
 * The walk visits every voxel the segment passes through, face by face.  k0[a], k1[a]: the k0 of origin and end per axis;
 * N[a] = |k1[a] - k0[a]|, s[a] its sign.  The walk has exactly 1 + N[x] + N[y] + N[z] voxels.  The i-th crossing on axis a
 * (i = 1 .. N[a]) lies at b = ((k0[a] - 524288) + s[a] (i - 0.5)) * (double)resolution, its parameter is
 * t = (b - (double)o[a]) / ((double)e[a] - (double)o[a]), every operation one IEEE double operation.  Each step takes the
 * axis whose next crossing has the smallest t, ties go to the lowest axis (a corner is two or three face steps).  At every
 * voxel, the origin's included, the stored state is looked up - FREE is bit 1, OCCUPIED 2, UNKNOWN 4, no stored voxel 8 - and
 * the walk stops at the first voxel whose bit is in stop_mask (0 is valid: the walk reaches the end).
 * Per ray, every pointer optional:
 *   status     0: reached the end's voxel without stopping; 1: stopped; 2: more than max_steps voxels, nothing walked;
 *              3: an endpoint not finite or outside the key range, nothing walked
 *   key        (kx << 40) | (ky << 20) | kz of the last voxel visited - the stopping voxel, on status 0 the end's; ~0 when
 *              nothing was walked (centre then NaN, t 0, steps 0, state UNKNOWN, semantics -1)
 *   centre     3 floats, t: the float cast of the entering crossing's double t (0 in the origin's voxel), steps: voxels visited
 *   state, semantics   of that voxel, as cvo_map_query answers (not stored: UNKNOWN, -1)
 * max_steps lies in 1 .. 2^20.  Refused, CVO_E_INVALID: a NULL map, n_rays < 0, origin or end NULL with n_rays > 0,
 * max_steps outside its range, stop_mask above 15, the wrong kind of map for the entry point. */
typedef struct cvo_map_ray_out_t {
  uint8_t* status;
  uint64_t* key;
  float* centre;
  float* t;
  int32_t* steps;
  uint8_t* state;
  int32_t* semantics;
} cvo_map_ray_out_t;
#define CVO_MAP_STOP_FREE 1u
#define CVO_MAP_STOP_OCCUPIED 2u
#define CVO_MAP_STOP_UNKNOWN 4u
#define CVO_MAP_STOP_ABSENT 8u
int cvo_map_raycast(cvo_map* map, int n_rays, const float* origin, const float* end, unsigned stop_mask, int max_steps,
                    const cvo_map_ray_out_t* out);
int cvo_map_raycast_host(cvo_map* map, int n_rays, const float* origin, const float* end, unsigned stop_mask, int max_steps,
                         const cvo_map_ray_out_t* out);
/* cvo_map_render: one ray of cvo_map_raycast per pixel of a pinhole camera at pose12 (3x4 row-major, camera to map).  Pixel
 * (u, v) - column, row - has the camera-frame end point (((u - cx) / fx) * z_far, ((v - cy) / fy) * z_far, z_far) in float,
 * each operation rounded on its own, moved by the pose with transform_point_pose_vec; the origin is the pose's translation.
 * The rays are made on the device.  Every plane is optional, rows x cols row-major:
 *   depth      (float)(t * (double)z_far) of the stopping voxel's entering crossing: a z-depth; 0: no stop
 *   semantics  of the stopping voxel; -1: no stop (or a stop at a voxel that is not stored, with bit 8 in the mask)
 *   feat       x 5: get_features; zeros without a stop
 *   label      x num_classes: get_occupied_probs, the layout cvo_rgbd_frame_t::semantic takes; zeros without a stop
 * max_steps is 2^20: a ray that would need more voxels, or whose end leaves the key range, renders as no stop.
 * Refused: CVO_E_INVALID - a NULL map or pose, rows or cols < 1, fx, fy or z_far not finite or <= 0, cx or cy not finite, a
 * pose that is not finite, stop_mask above 15; CVO_E_UNSUPPORTED - more than 2^24 pixels. */
typedef struct cvo_map_render_out_t {
  float* depth;
  int32_t* semantics;
  float* feat;
  float* label;
} cvo_map_render_out_t;
int cvo_map_render(cvo_map* map, const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far,
                   unsigned stop_mask, const cvo_map_render_out_t* out);
int cvo_map_render_host(cvo_map* map, const float pose12[12], float fx, float fy, float cx, float cy, int rows, int cols, float z_far,
                        unsigned stop_mask, const cvo_map_render_out_t* out);
int cvo_cloud_size(const cvo_cloud* c);
void cvo_cloud_free(cvo_cloud* c);

/* ---- CvoGPU::align (CvoGPU.cu:1574-1632) --------------------------------------------- */
int cvo_align(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source, const cvo_cloud* target,
              const float init_T[16], float out_T[16], cvo_align_info_t* info);
int cvo_align_ex(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source, const cvo_cloud* target,
                 const float init_T[16], float out_T[16], cvo_align_info_t* info,
                 const cvo_align_opts_t* opts);

/* New (not in the reference): n independent frame pairs solved concurrently on the
 * context's device.  init_T / out_T: n x 16.  infos: n entries or NULL.  Returns CVO_OK or
 * a CVO_E_* code; the per-pair 0 / -1 results are in infos[i].ret. */
int cvo_align_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_pairs, const cvo_cloud* const* sources,
                    const cvo_cloud* const* targets, const float* init_T, float* out_T,
                    cvo_align_info_t* infos, const cvo_align_opts_t* opts);
/* Copies the n x 16 result transforms of the last cvo_align_batch to DEVICE memory `dst`
 * on the context's stream (so a caller can hand them to an RCCL all-gather without a host
 * round trip). */
int cvo_batch_poses_to_device(cvo_ctx* ctx, void* dst_device, int n_pairs);

/* ---- batch queue (new, not in the reference): a STREAM of frame pairs through a fixed number of in-flight slots --------
 * cvo_align_batch takes a fixed set of pairs.  The reference's real use is a frame stream (one align() per frame, warm
 * starts, very different iteration counts: main_cvo_gpu_align_raw_image.cpp:100-170): here a pair that finishes hands its
 * slice of the workspace to the next submitted pair at the next chunk boundary, so `slots` pairs stay in flight however
 * long each of them runs.  Every pose is bit-identical to a solo cvo_align of the same pair.
 *   cvo_batch_open    sizes the workspace for `slots` pairs of up to max_source_points x max_target_points
 *                     (min_source_points: the smallest source cloud that will be submitted, 0 = same as max - small
 *                     clouds split their coefficient pass over more blocks and the launches must provide for it).
 *                     opts: only max_iterations is honoured.  While a queue is open the context's other align /
 *                     evaluation calls are refused.
 *   cvo_batch_submit  queues one pair (the clouds must stay alive until its result has been delivered); *ticket = its
 *                     number in submission order, from 0.  max_iterations > 0: this pair's own iteration limit (a warm
 *                     start that needs a few hundred iterations among cold starts that need thousands), at most the
 *                     queue's.
 *   cvo_batch_poll    drives the queue and delivers finished pairs IN SUBMISSION ORDER (a result is held back until
 *                     every earlier ticket has been delivered).  wait = 0: make progress, do not wait for results;
 *                     1: until at least one result can be delivered (or nothing is pending); 2: until everything
 *                     submitted so far has finished (or `capacity` results are ready).
 *   cvo_batch_pending submitted pairs not yet delivered.  cvo_batch_close waits for the device and releases the queue
 *                     (undelivered results are dropped).
 *   While a queue is open the context refuses cvo_align* / inner products / cvo_ctx_set_option (CVO_E_INVALID).
 *   cvo_ctx_destroy on a context with an open queue drains the queue's streams, releases its device side and ORPHANS the
 *   handle: every later call on it returns CVO_E_INVALID, cvo_batch_close then only frees the host object. */
typedef struct cvo_batch_queue cvo_batch_queue;
typedef struct cvo_batch_result_t {
  long long ticket;
  float transform[16]; /* column-major 4x4, as out_T of cvo_align */
  cvo_align_info_t info; /* info.seconds: wall time from the pair's placement into a slot to its retirement */
} cvo_batch_result_t;
int cvo_batch_open(cvo_ctx* ctx, const cvo_params_t* params, int slots, int max_source_points, int max_target_points,
                   int min_source_points, const cvo_align_opts_t* opts, cvo_batch_queue** out);
int cvo_batch_submit(cvo_batch_queue* q, const cvo_cloud* source, const cvo_cloud* target, const float init_T[16],
                     int max_iterations, long long* ticket);
int cvo_batch_poll(cvo_batch_queue* q, int wait, int capacity, cvo_batch_result_t* results, int* n_results);
int cvo_batch_pending(const cvo_batch_queue* q);
/* chunks launched (all sub-batches), how many of them were full graphs, slots filled so far (statistics) */
int cvo_batch_stats(const cvo_batch_queue* q, unsigned long long* chunks, unsigned long long* full_chunks,
                    unsigned long long* refills);
void cvo_batch_close(cvo_batch_queue* q);

/* ---- the Association align() exports (CvoGPU.cu:1552-1556 -> gpu_association_to_cpu, CvoGPU_impl.cu:366-427) -------
 * What `align(..., Association*)` returns when params.is_exporting_association is set: the kernel matrix of the LAST
 * EXECUTED iteration of the loop (pose before that iteration's update, that iteration's ell and num_neighbors), of
 * pair `pair` of the last cvo_align / cvo_align_ex / cvo_align_batch call on this context.  CSR as cvo_association:
 * row_ptr n_source + 1 ints; col / val up to `capacity` entries (NULL / 0 to size: CVO_E_NOMEM with *nnz_out set).
 * Stride: upstream reads its row-major buffers with the value num_neighbors has AFTER the loop.  After a `break`
 * (eps / eps_2) that is the stride they were written with.  When the loop ran out of iterations num_neighbors had
 * already been advanced (CvoGPU.cu:1529) and, if it changed, the buffers are read with another stride than they were
 * written with; that re-striding is reproduced here wherever it stays inside the part of the buffer the last iteration
 * defined (new stride <= old stride); beyond it upstream returns leftovers of earlier iterations, here the row ends
 * (see DESIGN.md "Association export").  *stride_written / *stride_read (optional) report the two values. */
int cvo_align_association(cvo_ctx* ctx, int pair, int* row_ptr, int* col, float* val, size_t capacity, size_t* nnz_out,
                          int* stride_written, int* stride_read);

/* ---- inner_product_gpu / function_angle (CvoGPU.cu:1780-1873) ------------------------
 * A_sum of fill_in_A_mat_gpu's matrix (first nearest_neighbors_max pairs of a row in ascending target index, a > sp_thres),
 * accumulated in double.  With a geometric cut-off the evaluation is ONE kernel launch over the resident clouds (no candidate
 * structure; up to three pairs - exact function_angle - in the same launch); a call in which a row finds more than
 * nearest_neighbors_max pairs, a call without geometry, or a context with option "IP_CHAIN" set runs the loop's
 * candidate-list chain instead.  Same pairs, same values; the two orders of summation agree in all but the last bits of
 * the double sum. */
int cvo_inner_product(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source,
                      const cvo_cloud* target, const float T[16], float ell, float* out);
int cvo_function_angle(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source,
                       const cvo_cloud* target, const float T[16], float ell, int is_approximate,
                       float* out);

/* New (not in the reference): n_jobs scores in one call - what the reference's drivers compute pair by pair
 * (main_indicator_in_sequence.cpp, main_evaluate_indicator.cpp, the multi-frame drivers' function_angle checks).
 * Job k = (sources[k], targets[k], T[16k .. 16k+15], ell[k]); out[k] = what cvo_inner_product / cvo_function_angle
 * returns for it, bit for bit.  The whole call is validated first (on an error nothing is written to out); n_jobs == 0
 * is accepted; a job with an empty cloud yields 0.  The jobs go through k_overlap_table in chunks, one launch and one
 * synchronisation per chunk (no job-count limit); void jobs (a row beyond nearest_neighbors_max) and chain-only calls run
 * the list chain as the single call does.  The exact function_angle evaluates <X, X> / <Y, Y> once per distinct cloud and
 * lengthscale of the call. */
int cvo_inner_product_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_jobs, const cvo_cloud* const* sources,
                            const cvo_cloud* const* targets, const float* T, const float* ell, float* out);
int cvo_function_angle_batch(cvo_ctx* ctx, const cvo_params_t* params, int n_jobs, const cvo_cloud* const* sources,
                             const cvo_cloud* const* targets, const float* T, const float* ell, int is_approximate,
                             float* out);
/* ---- compute_association_gpu(float lengthscale) (CvoGPU.cu:1876-1911) -----------------
 * CSR of Association::pairs (row = source index, col = target index, ascending).
 * row_ptr: n_source + 1 ints.  col/val: capacity entries.  *nnz_out = pairs found (may
 * exceed capacity, in which case only row_ptr is complete and CVO_E_NOMEM is returned). */
int cvo_association(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source,
                    const cvo_cloud* target, const float T[16], float ell, int* row_ptr, int* col,
                    float* val, size_t capacity, size_t* nnz_out);

/* ---- compute_association_gpu(..., const Eigen::Matrix3f& non_isotropic_kernel) (CvoGPU.cu:1913-1995) ---------
 * Association under a Mahalanobis distance d^T kernel^-1 d (fill_in_A_mat_gpu_dense_mat_kernel, CvoGPU.cu:217-327):
 * no geometric cut-off, geometric types off, K = nearest_neighbors_max.  kernel: 9 floats in Eigen::Matrix3f
 * (column-major) layout.  Output as cvo_association. */
int cvo_association_non_isotropic(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* source,
                                  const cvo_cloud* target, const float T[16], const float kernel_colmajor[9],
                                  int* row_ptr, int* col, float* val, size_t capacity, size_t* nnz_out);

/* ---- multi-frame edge kernel: BinaryStateGPU::update_inner_product (IRLS_State_GPU.cu:43-79) -------------
 * A frame is a resident cloud under a pose (3x4 ROW-major floats, CvoFrameGPU.cu:7-61).
 * cvo_cloud_transformed = CvoFrameGPU::transform_pointcloud (transform_point_pose_vec, CvoGPU_impl.cu:85-185):
 * a new resident cloud with every point moved by the pose (features / labels / geometric types copied).
 * cvo_edge_kernel_matrix = fill_in_A_mat_gpu(frame1, frame2, num_neighbors, ell) + compute_nonzeros +
 * copy_internal_SparseKernelMat_gpu_to_cpu: mat / ind row-major [n1 x num_neighbors] in the reference's cleared
 * layout (0 / -1 beyond a row's entries), nonzeros [n1], *nonzero_sum = their sum (what the caller hands to
 * Ceres).  Any of the output pointers may be NULL. */
int cvo_cloud_transformed(cvo_ctx* ctx, const cvo_cloud* in, const float pose_3x4_rowmajor[12], cvo_cloud** out);
int cvo_edge_kernel_matrix(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* frame1_transformed,
                           const cvo_cloud* frame2_transformed, float ell, int num_neighbors, float* mat, int* ind,
                           unsigned int* nonzeros, unsigned int* nonzero_sum);

/* ---- multi-frame align: CvoGPU::align(frames, frames_to_hold_const, edges, registration_seconds)
 * (CvoGPU.cu:1637-1683 -> CvoBatchIRLS::solve, IRLS.cpp:77-215) ---------------------------------------------------
 * n_frames clouds (the frames' UNtransformed points) under poses[12 * f .. 12 * f + 11] (3x4 ROW-major doubles,
 * CvoFrame::pose_vec), hold_const[f] != 0: frame f never moves (NULL = none held).  Edge k = (edges[2k], edges[2k+1]) =
 * (frame1, frame2) is one BinaryStateGPU with K = multiframe_num_neighbors and ell = multiframe_ell_init.
 * The outer loop is upstream's; each solve is a Levenberg-Marquardt trust-region loop with the Ceres defaults upstream
 * does not override, on the device-reduced normal equations of the free frames.  The edge state
 * is always the device one: multiframe_using_cpu (upstream's BinaryStateCPU, a nanoflann radius search) is ignored.
 * The whole call is validated first; on any error nothing is written.  CVO_E_INVALID: a null cloud, a frame index out
 * of range, a self-edge, an empty cloud in an edge.  CVO_E_UNSUPPORTED: n_frames > 64 or n_edges > 2048 (caps that keep
 * the dense host system at most 384 x 384).  n_edges == 0: the poses stay as given.
 * info (optional): totals of the call.  trace (optional): one row per outer iteration, up to trace_capacity rows;
 * *n_trace = rows written.  termination: 0 = no solve (ell decayed or loop ended), 1 = function tolerance, 2 = gradient
 * tolerance, 3 = parameter tolerance, 4 = minimum radius, 5 = iteration cap, 6 = too many invalid steps. */
#define CVO_MULTIFRAME_MAX_FRAMES 64
#define CVO_MULTIFRAME_MAX_EDGES 2048
typedef struct cvo_multiframe_info_t {
  int outer_iterations, solves, steps, accepted_steps; /* totals over the call */
  float final_ell;
  unsigned int last_total_nonzeros;
  double seconds; /* registration_seconds (CvoGPU.cu:1676-1680) */
} cvo_multiframe_info_t;
typedef struct cvo_multiframe_trace_t { /* one row per outer iteration */
  int iter, n_active_edges, solved, steps, accepted, termination;
  float ell;
  unsigned int total_nonzeros;
  double cost_initial, cost_final;
} cvo_multiframe_trace_t;
int cvo_multiframe_align(cvo_ctx* ctx, const cvo_params_t* params, int n_frames, const cvo_cloud* const* clouds,
                         double* poses, const int* hold_const, int n_edges, const int* edges,
                         cvo_multiframe_info_t* info, cvo_multiframe_trace_t* trace, int trace_capacity, int* n_trace);

/* ---- posed resident clouds merged into one, and a resident cloud read back: what the multi-frame drivers do right after
 * the solve (merge_transformed_pc + a VoxelMap of side leaf / 2, main_covisMap_test.cpp:183-215, 464-534), without a host
 * copy of any frame ----
 * cvo_cloud_merge: the rows of clouds[0], clouds[1] ... in their ORIGINAL order, concatenated; global row = the rows of the
 * clouds before it + the point's index.  poses: 12 doubles per cloud (3x4 ROW-major, what cvo_multiframe_align leaves),
 * each cast to float and applied as cvo_cloud_transformed applies it (transform_point_pose_vec); NULL: no row is moved at
 * all (the stored bits: -0.0f and non-finite values survive).  voxel_size == 0: the concatenation; voxel_size > 0: of
 * every occupied voxel of that side the row with the lowest global index, as cvo_voxel_select chooses over the moved rows.
 * kept (optional, room for every row): the global indices of the result's points, ascending (0, 1 ... when voxel_size ==
 * 0); *n_kept (optional): their number.  An attribute is present in the result iff some non-empty input holds it; inputs
 * without it contribute zeros.
 * The result is interchangeable with the cloud cvo_cloud_upload_voxel (voxel_size == 0: cvo_cloud_upload) makes of the
 * same moved, concatenated rows on the host: same spatial order, same one-hot detection, bit-identical results of every
 * later call.  Everything stays on the device - rows, moved coordinates, kept indices - except what the ordering route of
 * the result brings down today (cvo_cloud_from_device's rule).  Runs on the upload stream, synchronised on return.  The
 * inputs are only read; one handle may appear several times.
 * Refused on the host, before any launch or allocation: CVO_E_INVALID - n_clouds < 1, a NULL handle, a cloud of another
 * context, a voxel size that is negative or not finite; CVO_E_UNSUPPORTED - n_clouds > 4096, more than 2^24 rows in
 * total.  Refused by the selection (CVO_E_INVALID), as by cvo_voxel_select: a non-finite moved coordinate or |k| >= 2^20
 * when voxel_size > 0.  On any error *out is NULL and nothing is kept.  All inputs empty: an empty cloud.
 * cvo_cloud_download: the cloud's rows in ORIGINAL order, bit for bit what was uploaded (for a cloud of
 * cvo_cloud_transformed: the moved coordinates): xyz n x 3, feat n x 5, label n x 19, geotype n x 2 floats; any pointer
 * may be NULL.  *present (optional): CVO_CLOUD_HAS_* bits of the attributes the cloud really holds (0 for an empty cloud);
 * the others are written as zeros. */
#define CVO_CLOUD_HAS_FEAT 1
#define CVO_CLOUD_HAS_LABEL 2
#define CVO_CLOUD_HAS_GEOTYPE 4
int cvo_cloud_merge(cvo_ctx* ctx, int n_clouds, const cvo_cloud* const* clouds,
                    const double* poses /* 12 per cloud, 3x4 row-major, or NULL */, float voxel_size, cvo_cloud** out,
                    int* kept /* or NULL */, int* n_kept /* or NULL */);
int cvo_cloud_download(cvo_ctx* ctx, const cvo_cloud* cloud, float* xyz, float* feat, float* label, float* geotype,
                       int* present);

/* ---- keyframe depth filtering: the last loops of main_depth_filtering.cpp (208-298), frames in, cloud out -------------
 * A keyframe's depths refined from later frames with known poses.  Per frame the driver runs compute_association_gpu(kf,
 * frame, T_t2s, non_isotropic_kernel) and collects, for every keyframe row, the depth of each associated point moved into
 * the keyframe's frame (row 2 of T_s2t applied as CvoPointCloud::transform applies it) and its weight a_ij; rows with more
 * than three observations get a weighted mean depth and are re-projected along their ray, the others are dropped.  Here the
 * keyframe and the frames are resident clouds and nothing of it comes down: the association stays where its evaluation left
 * it, the accumulators and the moved rows live in a region the filter owns, the result is built from device rows.
 * tests/np_depthfilter.py is the statement (numpy float32); the kernels and the CPU twin equal it bit for bit.
 *
 *   state per keyframe row (original order): depth_sum (float), weight_sum (float), count (int), zero at open;
 *   add:    for the row's entries j in ascending target index: zj = T_depth(2,0) x_j + T_depth(2,1) y_j + T_depth(2,2) z_j +
 *           T_depth(2,3) (three rounded products added left to right, no fused multiply-add), depth_sum += zj * a,
 *           weight_sum += a, count += 1.  Frames in call order: the order upstream's depths[idx1] / weights[idx1] fill in;
 *   finish: rows with count > min_count (upstream: 3; the comparison is strict): wbar = weight_sum / float(count),
 *           d = (depth_sum + z0 wbar) / (weight_sum + wbar), xyz' = (xyz / z0) * d per component; features, labels and
 *           geometric types copied; rows in ascending original index.  A row whose d or xyz' is not finite (z0 == 0, a zero
 *           weight sum) is dropped and counted in *n_nonfinite: upstream's text pins nothing there, this is the library's
 *           choice.  Finish leaves the state as it is: more frames may follow it.
 * Departures from the driver's text: both matrices come from the caller (the driver derives T_t2s = T_t^-1 T_s and T_s2t =
 * T_s^-1 T_t with Eigen's 4x4 float inverse); nearest_neighbors_max truncates a row's entries per frame, as upstream's
 * kernel does; geometric types are off in the association (inner_product_non_isotropic_impl forces that).
 *
 * cvo_depth_filter_open: the filter COPIES what it needs of the keyframe - its rows in original order (k_cloud_unpack) and a
 * resident cloud built from them, interchangeable with the keyframe - so the caller's handle may be freed as soon as open
 * returns and is never dereferenced again.  The context must outlive the filter (close it before cvo_ctx_destroy).
 * cvo_depth_filter_add: T and kernel_colmajor are exactly cvo_association_non_isotropic's (source = the keyframe, target =
 * the frame); T_depth is 16 floats, column-major like T.  The frame is only read and may be freed on return.  Uses the
 * context's pair workspace and stream like cvo_association (refused while a batch queue is open).
 * cvo_depth_filter_state: the accumulators in original row order (cvo_depth_filter_size rows); any pointer may be NULL.
 * cvo_depth_filter_finish: *out = the refined keyframe as a resident cloud, the cloud cvo_cloud_upload makes of the
 * statement's rows (same spatial order and ordering route, same one-hot detection, bit-identical results of every later
 * call); kept / depth (optional, room for every row): original indices and refined depths of its points; *n_kept,
 * *n_nonfinite (optional).  Runs on the upload stream, synchronised on return.
 * cvo_depth_filter: open, add for every frame (T / T_depth: 16 floats per frame), finish, close in one call.
 * An empty keyframe or frame is accepted: add is a no-op, finish yields an empty cloud.  Every call is validated before
 * anything is written (CVO_E_INVALID: a NULL argument, a cloud of another context, a non-finite T_depth, min_count < 0;
 * CVO_E_UNSUPPORTED: a keyframe of more than 2^24 rows); on an error *out is NULL and the state is unchanged.  One error is
 * found on the device: an add whose kernel matrix names a row, slot or column out of range is refused with CVO_E_HIP, as the
 * association export refuses such a matrix; the filter's state is then lost and every later call but close is refused.
 * Not built: several frames' associations in one launch; a fused kernel that never materialises the association (the
 * ordered truncation at nearest_neighbors_max stands in the way); deriving the two matrices from world poses.
 *
 * The CPU twin needs no context: pure arithmetic over an association the caller already has, rows = keyframe rows in
 * original order, columns ascending (the CSR cvo_association_non_isotropic returns).  _accumulate_host adds one frame to the
 * caller's accumulators (CVO_E_INVALID, nothing written: row_ptr not ascending from 0, a column outside [0, n_target));
 * _finish_host writes the kept rows' moved coordinates (n_kept x 3), indices and depths; any output pointer may be NULL. */
typedef struct cvo_depth_filter_s cvo_depth_filter_t;
int cvo_depth_filter_open(cvo_ctx* ctx, const cvo_cloud* keyframe, cvo_depth_filter_t** out);
int cvo_depth_filter_add(cvo_depth_filter_t* df, const cvo_params_t* params, const cvo_cloud* frame, const float T[16],
                         const float T_depth[16], const float kernel_colmajor[9]);
int cvo_depth_filter_size(const cvo_depth_filter_t* df);
int cvo_depth_filter_state(cvo_depth_filter_t* df, float* depth_sum, float* weight_sum, int* count);
int cvo_depth_filter_finish(cvo_depth_filter_t* df, int min_count, cvo_cloud** out, int* kept /* or NULL */,
                            float* depth /* or NULL */, int* n_kept /* or NULL */, int* n_nonfinite /* or NULL */);
void cvo_depth_filter_close(cvo_depth_filter_t* df);
int cvo_depth_filter(cvo_ctx* ctx, const cvo_params_t* params, const cvo_cloud* keyframe, int n_frames,
                     const cvo_cloud* const* frames, const float* T /* 16 per frame */, const float* T_depth /* 16 per frame */,
                     const float kernel_colmajor[9], int min_count, cvo_cloud** out, int* kept, float* depth, int* n_kept,
                     int* n_nonfinite);
int cvo_depth_filter_accumulate_host(int n_rows, const int* row_ptr, const int* col, const float* val, int n_target,
                                     const float* target_xyz, const float T_depth[16], float* depth_sum, float* weight_sum,
                                     int* count);
int cvo_depth_filter_finish_host(int n_rows, const float* xyz, const float* depth_sum, const float* weight_sum,
                                 const int* count, int min_count, float* xyz_out, int* kept, float* depth, int* n_kept,
                                 int* n_nonfinite);

const char* cvo_version(void);

#ifdef __cplusplus
}
#endif
#endif
