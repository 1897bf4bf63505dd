/*
 * cvo_hip_debug.h -- test and profiling hooks of the MI355X backend.  NOT part of the drop-in boundary
 * (include/cvo_hip.h): nothing here replaces a reference interface; tests/, bench.py and scripts/ use these entry
 * points to look inside a context (last ELL matrix, kernel timings, candidate-list statistics, the device's scalar
 * routines on caller inputs).
 */
#ifndef CVO_HIP_DEBUG_H
#define CVO_HIP_DEBUG_H

#include "cvo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- test / profiling hooks ---------------------------------------------------------- */
/* Dumps the ELL kernel matrix of the LAST iteration executed by cvo_align_ex (row stride K):
 * mat/ind sized n_source*K, nonzeros sized n_source; K = the num_neighbors of that iteration. */
int cvo_debug_last_ell(cvo_ctx* ctx, int K, float* mat, int* ind, unsigned int* nonzeros);
/* A batch is enqueued as n_groups sub-batches (one stream each) of pairs_per_group pairs: these are the
 * launches a profiler sees. */
int cvo_debug_last_geometry(cvo_ctx* ctx, int* n_groups, int* pairs_per_group);
/* Re-issues the k_scan launches of one optimiser iteration (one per sub-batch) `reps` times on the final
 * state of the last call, timed with HIP events on the context's stream (bench.py's roofline leg).
 * *ms = average milliseconds per k_scan launch (of pairs_per_group pairs). */
int cvo_debug_time_scan(cvo_ctx* ctx, int reps, float* ms);
/* Tile-culling statistics of the last align call (all pairs, all iterations): number of fine tiles
 * the scan executed and the tile shape; executed pair tests = tiles * rows_per_tile * targets_per_tile. */
int cvo_debug_scan_stats(cvo_ctx* ctx, unsigned long long* tiles, int* rows_per_tile, int* targets_per_tile);
/* Re-issues the two per-iteration kernels (k_assoc; k_coeff including its update tail) one launch per sub-batch,
 * `reps` times, on the state the last call left behind and without writing anything back; timed with HIP events on
 * the context's stream.  *ms_* = average milliseconds per launch (of pairs_per_group pairs). */
int cvo_debug_time_kernels(cvo_ctx* ctx, int reps, float* ms_assoc, float* ms_coeff);
/* Kernel durations inside the optimiser loop itself.  With CVO_KERNEL_CLOCK set in the environment when the context is
 * created, the first block of a pair in k_assoc (lean graph) / k_coeff stamps its entry on the device's constant-rate counter
 * (s_memrealtime) and the block that finishes the pair's work in the launch (twist reduction / update) closes the
 * interval; the per-pair sums are part of the state.  Returns the averages of the last align call in ms - first
 * block in to last block out per pair and launch, the quantity rocprofv3 --kernel-trace --stats averages per launch -
 * and the number of k_coeff intervals behind them.  The counter's rate is calibrated against HIP events. */
int cvo_debug_kernel_clock(cvo_ctx* ctx, float* ms_assoc, float* ms_coeff, unsigned long long* launches);
/* Candidate-list reuse of the last align call, summed over the pairs: how many times the candidate bitmap was
 * (re)built by k_scan, the optimiser iterations run, and the candidate pairs k_assoc evaluated exactly. */
int cvo_debug_list_builds(cvo_ctx* ctx, unsigned long long* builds, unsigned long long* iterations,
                          unsigned long long* candidate_evaluations);
/* How the last list build of pair `pair` of the last align call classed its rows: rows beyond the 64-entry candidate
 * lists (served by k_assoc_dense), those of them beyond a long list as well (literal scan of all targets), and whether
 * the pair ended in the dense regime (no lists at all). */
int cvo_debug_row_classes(cvo_ctx* ctx, int pair, int* overflow_rows, int* scanned_rows, int* dense_regime);
/* The speculative update of pair `pair` of the last align call: iterations whose scalar tail was adopted from the speculative
 * run on the predicted step (update_speculate), and the iterations run.  0 adopted for traced calls and CVO_NO_SPECULATE. */
int cvo_debug_speculation(cvo_ctx* ctx, int pair, int* adopted, int* iterations);
/* Number of candidate pairs in the bitmap the last iteration used (superset of nnz). */
int cvo_debug_last_candidates(cvo_ctx* ctx, unsigned long long* out);
/* Runs the device's scalar restatements of the reference's host-side maths (cubic roots of poly_solver_order3,
 * the step selection of compute_step_size, Exp_SEK3, ||SE3 log||, update_tf, the indicator windows) on caller-supplied
 * inputs, so that the device code itself can be pinned against numpy / scipy.  ops and layouts: k_scalar_math in
 * unified_cvo_amd/csrc/cvo_kernels.h.  in / out: host arrays of 16 doubles per item (op 7: one item of 2 + n / n). */
int cvo_debug_scalar_math(cvo_ctx* ctx, int op, int n, const double* in, double* out);
/* Runs ONE shared device primitive of the front ends' kernels (unified_cvo_amd/csrc/cvo_k_prims.h, cvo_k_compact.h,
 * cvo_k_sort.h) on caller-supplied host arrays, which are copied up, worked on in place and copied back: k64 (n64 64-bit
 * words), a (na 32-bit words), b (nb 32-bit words).  Arrays too small for the op's n and m are refused.
 *   op 0  scan           a[n] block counts -> their exclusive offsets, b[0] = the total (k_compact_scan; n <= 16384)
 *   op 1  radix sort     k64[2 n], a[2 n]: n (key, value) pairs in the first halves -> sorted by key, stable, in the first
 *                        halves; the second halves and b[256 * ceil(n / 256)] are the sort's scratch
 *   op 2  wave_alloc     ceil(n / 256) blocks of 256 lanes: a[i] = want of lane i -> the first of its places; b[0]: the counter
 *   op 3  table_insert   k64[n + m]: n keys, behind them the table of m = 2^k >= 2 n slots (cleared here, returned);
 *                        a[i] = slot of key i; b[1 + i] = 2 * slots visited + fresh; b[0] += fresh lanes (wave_count_add)
 *   op 4  uf_unite       n cells, m edges a[2 e], a[2 e + 1]; b[n]: the parents (every cell its own, set here); a second
 *                        launch leaves k64[c] = uf_find(c)
 *   op 5  block ranks    blocks of 1024: a[i] != 0 flags element i, b[block] = block offset; k64[i] = inclusive rank << 32 |
 *                        exclusive rank (~0u where the flag is not set) */
int cvo_debug_prim(cvo_ctx* ctx, int op, int n, int m, unsigned long long* k64, size_t n64, unsigned* a, size_t na, unsigned* b,
                   size_t nb);
/* CVO_VERIFY_LISTS=1 (environment, read when a call starts): rows k_verify re-derived with the literal scan during the
 * last align call, summed over pairs and iterations (0 when the check was off). */
int cvo_debug_verified_rows(cvo_ctx* ctx, unsigned long long* rows);
/* The spatial (k-d) ordering of a resident cloud: out[r] = original index of the point at sorted position r (n entries).
 * Computed on the device at upload for clouds of 8 .. 16384 finite points (k_kd_order) and, under CVO_ORDER=wide, of up to
 * 2^24 (the multi-block ordering, cvo_k_kd_wide.h); on the host otherwise and under CVO_ORDER=host / virtual / CVO_NO_SORT.
 * No result depends on it. */
int cvo_debug_cloud_order(const cvo_cloud* cloud, int* out);
/* What ordered this cloud: 0 = the host, 1 = k_kd_order, 2 = the multi-block ordering of CVO_ORDER=wide (a cloud made by
 * cvo_cloud_transformed: what ordered its input). */
int cvo_debug_cloud_order_route(const cvo_cloud* cloud);
/* The route rule itself, which every upload path calls: the value above for a cloud of n points, all finite or not, under
 * the text order_value of the ORDER switch (NULL: unset) and NO_SORT set or not.  No context, no device. */
int cvo_debug_order_route_rule(int n, int finite, const char* order_value, int no_sort);
/* The host's plan of the multi-block ordering of n points (0 .. 2^24): *W = the leaf capacity of a default context, *n_rows
 * = the cuts of segments of more than W points, rows = (level, lo, hi, left) of the first `capacity` of them, level by
 * level and by position inside a level.  No context, no device.  W may be NULL. */
int cvo_debug_wide_plan(int n, int* W, int* rows /* level, lo, hi, left */, int capacity, int* n_rows);
/* ... with leaves of at most `leaf` points, what a context with CVO_WIDE_LEAF=leaf uploads: the cuts of segments of more than
 * `leaf` points.  CVO_E_INVALID for a leaf outside 1024 .. 16384. */
int cvo_debug_wide_plan_at(int n, int leaf, int* rows /* level, lo, hi, left */, int capacity, int* n_rows);
/* The select of the multi-block ordering, as the device computed it when `cloud` was uploaded by a context with
 * CVO_WIDE_RECORD=1: for every cut of the cloud's plan, in plan order (cvo_debug_wide_plan_at's rows), pivot = the kd_ordered
 * key of the segment's left-th smallest coordinate along the level's axis, rem = how many of the keys equal to it go left.
 * *n_segments = the cuts, of which the first `capacity` are written.  CVO_E_INVALID for a cloud that was not ordered by the
 * multi-block ordering itself (route != 2, or made by cvo_cloud_transformed) or was ordered without the switch. */
int cvo_debug_cloud_wide_pivots(const cvo_cloud* cloud, int capacity, unsigned* pivot, unsigned* rem, int* n_segments);
/* What the last score call did - cvo_inner_product / cvo_function_angle (one job) or their _batch forms: evaluations summed
 * by k_overlap (the exact function_angle's <X, X> / <Y, Y> once per distinct cloud and lengthscale), evaluations repeated
 * or run by the list chain (void jobs, chain-only calls), and launches (k_overlap chunks + chain sub-batches).  E.g.
 * (1, 0, 1) for an inner product no row voids, (3, 0, 1) for an exact function_angle of two distinct clouds.  A call that
 * returns before any device work (a single call with an empty cloud) leaves the previous values.  Any pointer may be NULL. */
int cvo_debug_last_score_batch(const cvo_ctx* ctx, int* overlap_evals, int* chain_evals, int* launches);
/* The tile records every cull of k_overlap trusts (k_tile_spheres): for each 64 consecutive sorted positions of a resident
 * cloud, out[8 t .. 8 t + 7] = centre x, y, z, radius, box half extents x, y, z, 0; *n_tiles = ceil(n / 64).  `out` holds
 * 8 floats per tile.  The records are made on the stream of the scores when no score has read the cloud yet, and kept: a
 * score before the call equals the score after it.  CVO_E_INVALID for a null pointer, an empty cloud, a cloud of another
 * context. */
int cvo_debug_cloud_tiles(cvo_ctx* ctx, const cvo_cloud* cloud, float* out /* n_tiles x 8 */, int* n_tiles);
/* Free / total bytes of the context's device (hipMemGetInfo), for leak checks without a second HIP runtime in the process. */
int cvo_debug_device_memory(cvo_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
/* Device arrays for the tests of cvo_cloud_from_device, without a second HIP runtime in the process.  *d == NULL: allocates
 * `bytes` of device memory on the context's device into *d; then, host_src != NULL, copies `bytes` from host_src to *d
 * (synchronously) - with *d given, that overwrites an earlier buffer of at least `bytes`.  _release frees one. */
int cvo_debug_device_buffer(cvo_ctx* ctx, size_t bytes, const void* host_src, void** d);
int cvo_debug_device_release(cvo_ctx* ctx, void* d);
/* k_irls_normal on its own: the kernel matrix of the last evaluation on this context (cvo_edge_kernel_matrix) as edge
 * (frame1, frame2) - the UNtransformed clouds the evaluated ones were moved from - at the poses pose1 / pose2 (3x4
 * row-major doubles).  out[91] = cost, g[12], the upper triangle of the 12 x 12 H row by row (78). */
int cvo_debug_irls_normal(cvo_ctx* ctx, const cvo_cloud* frame1, const cvo_cloud* frame2, const double pose1[12],
                          const double pose2[12], double* out);
/* k_irls_eval / k_irls_finish on a caller-made launch table: resident UNtransformed clouds (n_frames of them), poses
 * (12 doubles per frame, 3x4 row-major), n_edges edges (edge_frames: frame1, frame2 per edge) whose entry slots are
 * [slot_off[e], slot_off[e + 1]) of ent_r / ent_c / ent_w (row of frame 1, column of frame 2, weight; c < 0: an empty
 * slot).  The table (first block per edge, block count) is built by the builder cvo_multiframe_align uses, over every
 * edge given, zero-slot edges included.  out: n_edges x 91 doubles (cost, g[12], upper H[78]) when normal != 0, else
 * n_edges costs.  Everything is checked on the host before any launch: frames in range, slot_off non-decreasing,
 * 0 <= r < n1 and c < n2 for every stored entry (CVO_E_INVALID otherwise). */
int cvo_debug_irls_eval(cvo_ctx* ctx, int n_frames, const cvo_cloud* const* clouds, const double* poses, int n_edges,
                        const int* edge_frames, const int* slot_off, const int* ent_r, const int* ent_c, const float* ent_w,
                        int normal, double* out);
/* k_irls_gather on the matrix of the last evaluation on this context (cvo_edge_kernel_matrix) at its neighbour budget K
 * (CVO_E_INVALID for another K): the N x K entry slots, row-major by sorted position, as r / c / w arrays. */
int cvo_debug_irls_gather(cvo_ctx* ctx, int K, int* r, int* c, float* w);
/* The context's last voxel selection (cvo_voxel_select / cvo_cloud_upload_voxel) on the device: slots of the hash table,
 * slots taken (= voxels), slots visited by all inserts, the longest probe sequence of one insert (1 = its home slot), and the
 * points that reached the table in HBM (all of them without the block-local pre-pass).  All 0 after a selection on the host
 * (VOXEL_HOST=1, or fewer than 4096 points by default) or of an empty cloud.  Any pointer may be NULL. */
int cvo_debug_voxel_stats(cvo_ctx* ctx, unsigned long long* capacity, unsigned long long* occupied,
                          unsigned long long* probes_total, unsigned long long* probe_longest, unsigned long long* entered);
/* The context's last cvo_rgbd_points / cvo_cloud_upload_rgbd: the potentials the selector's schedule tried (*n_tried <= 6 of
 * them) and the pixels selected at each; pixels of the standing selection, how many of them became points (depth, class),
 * the FULL pass's points, the frame's pixels with a depth (FULL passes only), and whether the kernels ran (0: CPU twin).
 * Parts a call did not compute are 0.  Any pointer may be NULL. */
int cvo_debug_rgbd_stats(cvo_ctx* ctx, int* n_tried, int* potentials /* 8 */, int* counts /* 8 */,
                         unsigned long long* edge_selected, unsigned long long* edge_points,
                         unsigned long long* surface_points, unsigned long long* with_depth, int* on_device);
/* What the context's last selection on the device left in its region - a cvo_rgbd_points / cvo_stereo_points(DSO_EDGES) or a
 * recipe that took the device route; CVO_E_INVALID after a call on the host route, a FULL-only call, any later call that
 * lays the region out again, or no call -: the frame's shape; counts[6], the pixels selected at the potentials 2 .. 7,
 * tried by the schedule or not; g2 (rows x cols); ths and sm, the block thresholds and their smoothed squares, each with
 * all (cols / 32)(rows / 32) + 100 entries; selected: the six selections one after the other (counts[0] + .. + counts[5]
 * pixel indices v cols + u), each in the order the compaction left it.  Any pointer may be NULL: a first call with the
 * arrays NULL sizes them.  Tests use it to name the first stage that differs from the statement without
 * running anything again; the production path launches, copies and waits for nothing on its behalf. */
int cvo_debug_rgbd_readback(cvo_ctx* ctx, int* rows, int* cols, int* counts /* 6 */, float* g2, float* ths, float* sm,
                            int* selected);
/* The context's last cvo_fast_select / cvo_stereo_points / cvo_cloud_upload_stereo / _recipe: the thresholds (CV_FAST) or
 * potentials (DSO_EDGES) the selector's schedule evaluated - *n_tried of them, the first `capacity` written - and the pixels
 * at each; the FAST threshold whose keypoints stand (-1: no FAST selection ran); the 257 pixel counts per FAST score
 * -1 .. 255; the pixels the keep predicate saw and the points it kept (the recipe: both passes); whether the kernels ran.
 * Any pointer may be NULL. */
int cvo_debug_stereo_stats(cvo_ctx* ctx, int capacity, int* n_tried, int* thresholds, int* counts, int* threshold_used,
                           unsigned* histogram /* 257 */, unsigned long long* candidates, unsigned long long* kept, int* on_device);
/* The context's last cvo_lidar_select / cvo_cloud_upload_lidar, counts[9]: range-image cells that hold a point, ground
 * cells, valid components, invalid components, segmented points, LeGO-LOAM edge picks, draws consumed, thinned points kept,
 * edge_detection's points; whether the kernels ran.  Any pointer may be NULL. */
int cvo_debug_lidar_stats(cvo_ctx* ctx, unsigned long long* counts /* 9 */, int* on_device);
/* lidar_atan2_deg of cvo_lidar_math.h - the one copy the CPU twin and the kernels compile - on n pairs, on the host:
 * out[i] = atan2(y[i], x[i]) in degrees.  No context. */
int cvo_debug_lidar_atan2(int n, const double* y, const double* x, double* out);
/* The context's last cvo_nlm_denoise / cvo_nlm_denoise_lab: whether the kernel ran; mult, shift and the length of the
 * table's nonzero leading run (of the chroma pass for _lab); the kernel's tile (0 x 0 on the CPU twin); whether every
 * pass held its whole nonzero run in LDS.  Any pointer may be NULL. */
int cvo_debug_nlm_stats(cvo_ctx* ctx, int* on_device, int* mult, int* shift, int* n_nonzero, int* tile_w, int* tile_h,
                        int* table_in_lds);
/* The context's last cvo_stereo_disparity (cvo_cloud_upload_stereo_pair's included): whether the kernels ran; max_disparity and
 * paths; the lines launched per direction (8 ints, 0 for a direction not run and on the CPU twin); the frame's shape; the
 * census kernel's tile (0 x 0 on the CPU twin).  Any pointer may be NULL. */
int cvo_debug_sgm_stats(cvo_ctx* ctx, int* on_device, int* max_disparity, int* paths, int* lines /* 8 */, int* rows, int* cols,
                        int* tile_w, int* tile_h);
/* What that call left in the context's region, if it ran on the device (CVO_E_INVALID otherwise): the census planes (rows x
 * cols 64-bit words each) and S (rows x cols x max_disparity 16-bit sums).  Any pointer may be NULL.  Tests use it to find
 * the first stage that differs from the statement without running anything again. */
int cvo_debug_sgm_readback(cvo_ctx* ctx, unsigned long long* census_left, unsigned long long* census_right, unsigned short* S);
/* The context's last cvo_disparity_filter (the _filtered entry points' included): whether the kernels ran; the map's shape;
 * the kernels' tile (0 x 0 on the CPU twin); counts[3]: segments of valid pixels the speckle pass found, valid pixels it
 * removed, pixels the gap pass filled (rows + columns).  after_speckle / after_gap / mean_tmp: the maps a call that ran on
 * the device left in the context's region after the speckle pass, after the gap pass and after the mean's horizontal pass
 * (rows x cols floats each; CVO_E_INVALID when the call ran on the host, or for mean_tmp when the mean did not run, for the
 * others when no stage up to theirs ran).  Any pointer may be NULL.  Tests use the maps to name the first stage that differs
 * from the statement without running anything again. */
int cvo_debug_dfilter_stats(cvo_ctx* ctx, int* on_device, int* rows, int* cols, int* tile_w, int* tile_h,
                            unsigned long long* counts /* 3 */, float* after_speckle, float* after_gap, float* mean_tmp);

/* The last insert of a map (either kind): on_device; counts[8] = training points, block memberships, the longest run of hits in
 * one voxel, the table's capacity (slots of a device map; voxels of a host map), growths of the table so far, the longest probe
 * of that insert, voxels stored, classes of the map.  keys / ms / fs (capacity x 1 / classes / 5, each optional): the raw
 * table, ~0 the key of a free slot, so that a test can name the first voxel that differs from the statement. */
int cvo_debug_map_stats(cvo_map* map, int* on_device, unsigned long long* counts /* 8 */, unsigned long long* keys, float* ms, float* fs);

/* How the rows of the matrix a filter's last add accumulated were stored (by position, read from pair 0's workspace): rows
 * with no entry; rows the thread-per-row kernel wrote into the slot-major matrix; rows the wave-per-row kernels wrote
 * slot-major (NNZ_DENSE_FLAG, dense_off < 0) and as row-major runs (dense_off >= 0); rows that hold exactly the neighbour
 * budget K (cut there, or just full); the longest row; K; the rows k_assoc_dense evaluated with a whole block (wide rows:
 * more than 256 and at most 1216 candidates, in a launch of the wide instantiation with a block per overflow row).
 * CVO_E_INVALID unless the context's last evaluation is this filter's last add (its call serial).  Any pointer may be NULL.
 * Tests use it to assert that the row classes they mean to cover are populated. */
int cvo_debug_depth_filter_rows(cvo_depth_filter_t* df, int* n_empty, int* n_list, int* n_dense_slot, int* n_run, int* n_full,
                                int* max_nnz, int* K, int* n_wide);

#ifdef __cplusplus
}
#endif
#endif
