// cvo_internal.h -- what the sections of the host side (cvo_ctx.hip, cvo_upload.hip, cvo_launch.hip, cvo_sched.hip,
// cvo_queue.hip, cvo_eval.hip, cvo_export.hip, cvo_frontend.hip, cvo_ingest.hip, cvo_voxel.hip, cvo_merge.hip, cvo_rgbd.hip, cvo_lidar.hip, cvo_nlm.hip, cvo_sgm.hip, cvo_dfilter.hip, cvo_stereo_pair.hip, cvo_bki.hip, cvo_depth.hip, cvo_debug.hip) share: the context, a resident cloud, the typed walk that lays
// out EVERY device region (ScratchLayout: a pair's workspace, the front ends' scratch, the map's table, a cloud's slabs, the control block, the score blocks), the owner of
// EVERY device and pinned allocation (Region: move-only, frees in its destructor, ONE grow rule - drain, free, allocate, tell the caller it moved), graph keys and the error helpers.  The context's switches: cvo_options.h.  Included once, by cvo_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <memory_resource>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "cvo_kernels.h"

using namespace cvo_dev;

#include "cvo_options.h"

#define CVO_VERSION_STRING "unified_cvo_amd 0.1 (gfx950)"

// The arrays of a cloud's slab (upload_host_cloud's list): a cloud's own, and the same list over the staging buffer the slab
// is uploaded from.  An array the caller did not supply stays null.
struct CloudArrays {
  float4* x4 = nullptr;
  float4* xs4 = nullptr;    // x4 permuted into the spatial order
  float4* feat = nullptr;   // 2 float4 per point      } in SPATIAL order (position r = point order[r]): the kernels
  float4* label = nullptr;  // 5 float4 per point      } index them by sorted position, like the coordinates they
  float2* geo = nullptr;    //                         } gather per candidate
  int* lid = nullptr;       // class id per point, spatial order: only when EVERY label row is an exact one-hot (a single
                            // 1.0f, the rest 0.0f) - the semantic kernel then needs 4 bytes per candidate, not 80
  int* order = nullptr;        // spatial (k-d) order: sorted position -> original index
  int* inv = nullptr;          // its inverse: original index -> sorted position
  // a cloud ordered on the device: the caller's rows in ORIGINAL order and the scratch of k_kd_order, null otherwise
  float *raw_feat = nullptr, *raw_label = nullptr, *raw_geo = nullptr;
  int* raw_lid = nullptr;
  unsigned short *seg_of_pos = nullptr, *seg_lo = nullptr;
};

namespace {

// The chunk a sub-batch runs next (launch_chunk; chosen by choose_chunk, cvo_sched.hip).  Full: a rebuild opportunity and
// k_assoc_dense in every iteration; full without dense: the same minus k_assoc_dense; lean / short lean: a rebuild
// opportunity every `period` iterations; calm: one per chunk.  The lean kinds run k_assoc_dense too when `dense` is set.
enum class ChunkKind { Full, FullNoDense, Lean, ShortLean, Calm };
static const char* const kChunkNames[] = {"full", "full-nodense", "lean", "short", "calm"};

struct ChunkPlan {
  ChunkKind kind = ChunkKind::Full;
  bool dense = false;
  int U = 0;       // iterations
  int period = 0;  // lean kinds: iterations per rebuild opportunity (the calm chunk's is U)
  bool every_iteration() const { return kind == ChunkKind::Full || kind == ChunkKind::FullNoDense; }  // a rebuild opportunity
};

// Where the workspaces of a launch's pairs are (kernel arguments of the row-block kernels, see row_off_*)
struct ArenaArg {
  const char* base;    // workspace of the launch's first pair
  unsigned stride256;  // bytes / 256 between consecutive pairs
  int Npad;
};

// What a cached graph was captured with: the chunk plan and every field of LaunchGeom its launches read, except k_verify's
// grid (the kernel loops over the rows, so a graph captured at another N verifies the same rows).  The list chain
// (run_ip_chain) leaves the plan, csplit, horizon_cap and verify at their defaults: it launches no k_coeff, k_verify or
// lean iteration.  Device pointers of the context are not in it: reallocating them drops every graph (drop_graphs).
struct GraphKey {
  ChunkPlan plan;
  int n_pairs = 0, p0 = 0, T = 0, gx = 0, gy = 0, npb = 0, nbl = 0, nba = 0, csplit = 0, dense_blocks = 0, horizon_cap = 0, feat = 0;
  bool idx16 = false, wide = false, instr = false, verify = false;
  ArenaArg arena{};
  auto fields() const {
    return std::tie(plan.kind, plan.dense, plan.U, plan.period, n_pairs, p0, T, gx, gy, npb, nbl, nba, csplit, dense_blocks,
                    horizon_cap, feat, idx16, wide, instr, verify, arena.base, arena.stride256, arena.Npad);
  }
  bool operator==(const GraphKey& o) const { return fields() == o.fields(); }
};

// Sizes a workspace is laid out for (make_dims)
struct Dims {
  int Mpad, nchunks, rbw_max, nblk_assoc, NG, NGpad, Npad;
};

// What the launches of a sub-batch are (plan_batch, group_geom)
struct LaunchGeom {
  int n_pairs, p0, T, gx, gy, nba, npb, csplit;
  int nbl, nbv;  // blocks of k_list (LIST_THREADS rows each) and k_verify (grid x) for the largest source cloud
  int dense_blocks = DENSE_BLOCKS_MIN;  // k_assoc_dense grid x = PairDesc::dense_blocks of every pair of the launch
  int horizon_cap = 1 << 20;  // the lean graph's period (DevParams::lean_U)
  bool idx16, instr, verify;
  bool wide;  // k_assoc_dense's wide-row instantiation (dense_wide)
  int feat = FEAT_GEO;  // which instantiation of the association kernels the call needs (call_feat)
  hipStream_t stream;
  ArenaArg arena;  // of pair p0
};

// A call's sizes, workspace layout and launch geometry (plan_batch); N / M: its largest source / target cloud
struct BatchSetup {
  int N, M, G;
  bool long_lists = false;
  Dims d;
  size_t slot_bytes;  // one pair's workspace (place_regions): pair p's begins at arena + p * slot_bytes
  LaunchGeom geom;
};

struct CachedGraph {
  hipGraphExec_t exec = nullptr;
  GraphKey key;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

// what cvo_debug_rgbd_stats reports of the context's last RGB-D call (cvo_rgbd.hip)
struct RgbdStatsAcc {
  int n_tried = 0, tried[8] = {}, count[8] = {};  // the selector's schedule: potentials tried, pixels selected at each
  unsigned long long edge_selected = 0, edge_points = 0, surface_points = 0, with_depth = 0;
  int on_device = 0;
};

// where cvo_debug_rgbd_readback finds the stages of the context's last selection on the device (rgbd_device_select, cvo_rgbd.hip):
// host-side facts only.  The stages stay in rgbd_scratch until the region is laid out again (rgbd_device_stage), which ends
// `valid`, as does an RGB-D call on the host route.
struct RgbdSelectionAcc {
  bool valid = false;
  int w = 0, h = 0;
  RgbdCells cells{};
  std::vector<unsigned> sel_offset;  // exclusive offsets of the selection's blocks, the total last
  const float *g2 = nullptr, *ths = nullptr, *sm = nullptr;
  const int* sel = nullptr;
};

// what cvo_debug_stereo_stats reports of the context's last stereo / FAST call (cvo_fast.hip, cvo_stereo.hip)
struct StereoStatsAcc {
  std::vector<int> tried, count;  // the selector's schedule: FAST thresholds (CV_FAST) or potentials (DSO_EDGES) tried, pixels at each
  int threshold_used = -1;        // the FAST threshold whose keypoints stand; -1: no FAST selection ran
  unsigned hist[257] = {};        // FAST: pixels per score -1 .. 255
  unsigned long long candidates = 0, kept = 0;  // pixels the keep predicate saw (FULL: every pixel), points it kept
  int on_device = 0;
};

// what cvo_debug_lidar_stats reports of the context's last LiDAR call (cvo_lidar.hip)
struct LidarStatsAcc {
  unsigned long long projected = 0, ground = 0, valid = 0, invalid = 0, segmented = 0, edges = 0, draws = 0, thinned = 0, edge_detected = 0;
  int on_device = 0;
};

// what cvo_debug_nlm_stats reports of the context's last denoising call (cvo_nlm.hip)
struct NlmStatsAcc {
  int on_device = 0, mult = 0, shift = 0, n_nonzero = 0, tile_w = 0, tile_h = 0, table_in_lds = 0;
};

// what cvo_debug_sgm_stats reports of the context's last cvo_stereo_disparity (cvo_sgm.hip), and where cvo_debug_sgm_readback
// finds the census planes and S of a call that ran on the device
struct SgmStatsAcc {
  SgmStatsAcc() = default;
  explicit SgmStatsAcc(const SgmConst& k) : rows(k.rows), cols(k.cols), D(k.D), paths(k.paths) {}
  int on_device = 0, rows = 0, cols = 0, D = 0, paths = 0, tile_w = 0, tile_h = 0;
  int lines[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // lines launched per direction
  size_t o_census_left = 0, o_census_right = 0, o_S = 0, o_disparity = 0;
};

// what cvo_debug_dfilter_stats reports of the context's last disparity filter (cvo_dfilter.hip), and where it finds the maps
// after each stage of a call that ran on the device (a stage that did not run: its input's)
struct DFilterStatsAcc {
  DFilterStatsAcc() = default;
  explicit DFilterStatsAcc(const DFilterConst& k) : rows(k.rows), cols(k.cols) {}
  int on_device = 0, rows = 0, cols = 0, tile_w = 0, tile_h = 0;
  unsigned long long segments = 0, removed = 0, filled = 0;  // speckle: segments of valid pixels, valid pixels removed; gap: pixels filled
  size_t o_speckle = 0, o_gap = 0, o_tmp = 0;
  bool speckle_resident = false, gap_resident = false, tmp_resident = false;
};

// THE walk over the buffers of one allocation (a pair's workspace slot, a front end's scratch region, the map's table, a
// cloud's slab and its staging copy): a layout is ONE list of take(pointer, count) lines, and this is the only code that
// turns "offset, align, cast" into a pointer.  Every buffer begins on a multiple of 256 bytes from `base`; `off` ends as the
// bytes to allocate, so sizing a region is the same list walked from base 0 into pointers nobody reads.
struct ScratchLayout {
  uintptr_t base;
  size_t off = 0;
  explicit ScratchLayout(const void* at = nullptr) : base((uintptr_t)at) {}
  // one walk of a list(ScratchLayout&) from `base`: its pointers bound there; returns the bytes its buffers need
  template <class List>
  size_t walk(List&& list) { return list(*this), off; }
  // a fixed position (row_off_*), or - offset == off - where the next buffer will begin
  template <class T>
  void at(T*& ptr, size_t offset) const { ptr = reinterpret_cast<T*>(base + offset); }
  // `count` elements of type E behind a pointer of another type: the void* fields, and a byte count that is no multiple
  // of the pointer's element
  template <class E, class T>
  void take_as(T*& ptr, size_t count) {
    at(ptr, off);
    off = align_up(off + sizeof(E) * count, 256);
  }
  // `count` elements of the pointer's own type
  template <class T>
  void take(T*& ptr, size_t count) { take_as<T>(ptr, count); }
};

// THE list of a cloud slab's arrays, for both upload routes (upload_host_cloud in cvo_upload.hip, ingest_device_clouds in cvo_ingest.hip):
// `a` is whatever names these arrays - a CloudArrays (the cloud itself, the staging buffer's view) or the KdJob of the
// ordering kernel.  *up_bytes: the prefix a host upload stages and copies (the caller's rows when the device orders them,
// everything otherwise).
struct SlabShape {
  size_t nn;  // max(n, 1)
  int NP;     // k_kd_order's padded size
  bool feat, label, geo, lid;
  bool raw;   // the caller's rows in ORIGINAL order are part of the slab (a cloud ordered on the device; every device-built cloud)
  bool kd;    // ... and k_kd_order's scratch
};
template <class A>
inline auto cloud_slab_list(A& a, const SlabShape& s, size_t* up_bytes) {
  return [&a, s, up_bytes](ScratchLayout& l) {
    l.take(a.x4, s.nn);
    if (s.raw && s.feat) l.take(a.raw_feat, FD * s.nn);
    if (s.raw && s.label) l.take(a.raw_label, NC * s.nn);
    if (s.raw && s.geo) l.take(a.raw_geo, 2 * s.nn);
    if (s.raw && s.lid) l.take(a.raw_lid, s.nn);
    if (s.raw) *up_bytes = l.off;
    l.take(a.xs4, s.nn);
    l.take(a.order, s.nn);
    l.take(a.inv, s.nn);
    if (s.feat) l.take(a.feat, 2 * s.nn);
    if (s.label) l.take(a.label, 5 * s.nn);
    if (s.geo) l.take(a.geo, s.nn);
    if (s.lid) l.take(a.lid, s.nn);
    if (s.kd) l.take(a.seg_of_pos, (size_t)s.NP);
    if (s.kd) l.take(a.seg_lo, 2 * KD_MAX_SEGS);
    if (!s.raw) *up_bytes = l.off;
  };
}

// THE owner of an allocation: every device and pinned region of the library is a member or a local of this type, and nothing
// else calls hipMalloc / hipHostMalloc / hipFree / hipHostFree (but cvo_debug_device_buffer / _release, which hand a raw
// pointer to the caller by contract).  Move-only; the destructor frees.  Defined below cvo_ctx.
enum class Mem { Device, Pinned, Mapped };  // hipMalloc | hipHostMallocDefault | hipHostMallocMapped + Coherent (what the device writes there needs no cache maintenance to be seen)
template <Mem K>
struct Region {
  char* p = nullptr;
  size_t bytes = 0;
  Region() = default;
  Region(Region&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  Region& operator=(Region&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~Region() { release(); }
  void release() {
    if (p) (void)(K == Mem::Device ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
  // Room for `need` bytes, grow-only: a region that is too small is given back once `drain` - the stream that may still
  // read it, nullptr: none - has been synchronised, and allocated anew.  A failed allocation leaves the owner empty and is
  // CVO_E_NOMEM "<what> hipMalloc: ...".  *moved (optional) is set when the region is a new one: whatever holds a pointer
  // into it, or relies on its contents, acts on that.
  int reserve(cvo_ctx* ctx, size_t need, const char* what, hipStream_t drain, bool* moved = nullptr);
  // Room for the buffers of `list(ScratchLayout&)`, then the list's pointers bound to them: the list sizes the region from
  // base 0 and is walked again from where the region is AFTER reserve, so no pointer outlives a reallocation.
  template <class List>
  int lay_out(cvo_ctx* ctx, const char* what, List list, hipStream_t drain, bool* moved = nullptr) {
    const int rc = reserve(ctx, ScratchLayout().walk(list), what, drain, moved);
    if (rc != CVO_OK) return rc;
    ScratchLayout(p).walk(list);
    return CVO_OK;
  }
  // ... of a front end: laid out anew by every call and used on upload_stream under upload_mutex
  template <class List>
  int lay_out(cvo_ctx* ctx, const char* what, List list);
};
using DeviceRegion = Region<Mem::Device>;
using DeviceScratch = DeviceRegion;  // (the front ends' name for theirs)
using PinnedRegion = Region<Mem::Pinned>;
using MappedRegion = Region<Mem::Mapped>;

struct cvo_cloud : CloudArrays {
  cvo_ctx* ctx = nullptr;  // identity check only: never dereferenced after upload (the context may be gone)
  int device = 0;
  int n = 0;
  DeviceRegion slab;  // the one device allocation behind the arrays
  // Attributes the caller did not supply are zeros (what the reference leaves in the default-constructed CvoPoint).
  // They are not uploaded: a zeroed slab is allocated the first time a call needs them (colour / semantic /
  // geometric-type kernels on a cloud without those arrays), see ensure_attributes.
  mutable DeviceRegion zero_slab;
  // bounding spheres of the 64-point tiles of xs4 (k_tile_spheres), made the first time k_overlap reads this cloud
  mutable DeviceRegion tiles;
  mutable float4* tile4 = nullptr;  // (typed view of `tiles`)
  std::vector<int> h_order;  // host copy (the ELL is stored by sorted row; exports map it back)
  int order_route = 0;       // who made it (order_route, cvo_upload.hip): 0 the host, 1 k_kd_order, 2 the wide ordering
  std::vector<unsigned> h_wide_piv;  // WIDE_RECORD=1, route 2: (pivot key, rem) of every planned segment (KdWide::seg_piv), else empty
  float cx = 0, cy = 0, cz = 0;  // centroid (used only as the cull centre)
  float rmax = 0;                // largest |p| (bounds the motion of any point under a pose change)
};

// THE list of the control block [DevParams | status words: per sub-batch status[n_g], want[n_g] | PairDesc[n] | PairState[n]],
// walked once over the device block and once over its pinned staging copy
inline auto control_block_list(DevParams*& params, int*& status, PairDesc*& descs, PairState*& states, size_t n) {
  return [&params, &status, &descs, &states, n](ScratchLayout& l) {
    l.take(params, 1);
    l.take(status, 2 * n);
    l.take(descs, n);
    l.take(states, n);
  };
}


struct cvo_ctx {
  int device = 0;
  CtxOptions opt;                          // the switches (cvo_options.h)
  std::mutex upload_mutex;                 // cvo_cloud_upload / _aos192 share upload_stream and the error string
  std::mutex kd_mutex;                     // the ordering launches of concurrent uploads share upload_stream and d_kd_jobs
  DeviceRegion d_kd_jobs;                  // job descriptors of the running k_kd_order launch and of the wide clouds' k_cloud_gather
  DeviceRegion d_kd_wide;                  // scratch of the wide ordering (wide_region_list), grown on demand, under kd_mutex too
  hipStream_t stream = nullptr;
  hipStream_t upload_stream = nullptr;  // cvo_cloud_upload copies here (never waits for, nor delays, the solver's streams)
  std::string err;
  std::string advice;  // performance-relevant observations about the process set-up (cvo_ctx_advice), "" = none
  // workspace
  DeviceRegion arena;
  PairDesc* d_descs = nullptr;
  PairState* d_states = nullptr;
  int* d_status = nullptr;
  DevParams* d_params = nullptr;
  // descriptors, states, status words and the parameter block live in ONE device allocation with a pinned staging copy
  // of the same layout: a call uploads its control state with one copy (four copies cost every cvo_align ~10 us and
  // an inner product a third of its time)
  DeviceRegion d_ctl;
  PinnedRegion h_ctl;
  DevParams* s_params = nullptr;  // the staging copy's parts (control_block_list over h_ctl, as d_params .. d_states over d_ctl)
  int* s_status = nullptr;
  PairDesc* s_descs = nullptr;
  PairState* s_states = nullptr;
  int cap_pairs = 0;
  std::vector<PairDesc> h_descs;
  std::vector<PairState> h_states;
  // scores (cvo_inner_product / cvo_function_angle and their batches, k_overlap): per-job gate words (zero between
  // launches) + row-tile partials and the pinned results, sized on first use and grown (see score_ws_reserve); the device
  // job table + tile starts of k_overlap_table and its pinned staging, made by the first call that launches it
  DeviceRegion d_sb, d_sb_table;
  PinnedRegion h_sb;      // staging of the job table (one copy per k_overlap_table launch)
  MappedRegion h_sb_res;  // results: a double and a void flag per job (written by the device)
  int last_score_overlap = 0, last_score_chain = 0, last_score_launches = 0;  // cvo_debug_last_score_batch
  MappedRegion h_status[2];  // [0]: the live host mirror of the status / want words the device writes
                             // (PairDesc::status_host / want_host), [1]: a double per pair, the sum a single
                             // evaluation leaves for the host (PairDesc::asum_host, read by score_batch)
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  // A batch is split into up to MAX_GROUPS sub-batches, each enqueued on its own stream: the pairs are
  // independent, so one group's latency-bound kernels (k_update: one wave per pair) and launch tails
  // overlap the other groups' wide kernels.  Group 0 runs on `stream`.
  static constexpr int MAX_GROUPS = MAX_STREAMS;
  hipStream_t gstream[MAX_GROUPS] = {};
  hipEvent_t ev_chk[2][MAX_GROUPS] = {};
  hipEvent_t ev_fork = nullptr, ev_join[MAX_GROUPS] = {};
  // graph cache: per group, one entry per chunk-graph slot (graph_slot: the eight chunks x instrumented kernels
  // (CVO_KERNEL_CLOCK / CVO_PHASE_TICKS) or not x the three chunk lengths, so that a caller can time single steps of a
  // loop without re-capturing), each replaced when its key changes; and the list chain of run_ip_chain
  static constexpr int GRAPH_SLOTS = 48;
  CachedGraph graphs[MAX_GROUPS][GRAPH_SLOTS];
  CachedGraph chain_graph;
  int last_chunks = 0, last_lean_launches = 0, last_full_launches = 0;
  // The last call, as commit_batch made it (debug hooks, exports, the IRLS readers): its pairs (0 = no workspace of the
  // last call can be read), setup, parameters and pair 0's source order (sorted row -> original row)
  int last_pairs = 0;
  BatchSetup last{};
  DevParams last_params{};
  std::vector<int> last_xorder;
  bool queue_open = false;  // a cvo_batch_queue owns the workspace: the other align / evaluation calls are refused meanwhile
  cvo_batch_queue* queue = nullptr;  // ... that queue (cvo_ctx_destroy releases its device side, see queue_release)
  // voxel selection (cvo_voxel.hip): one growable device region - coordinates, table, per-point slots, block counts, kept
  // indices, VoxelCtl -; the last selection's table size and counters
  DeviceScratch vox_scratch;
  unsigned long long vox_capacity = 0;  // 0: the last selection ran on the host (or none has run)
  VoxelCtl vox_last{};
  // RGB-D front end (cvo_rgbd.hip): one growable device region - image, depth, exclusion bytes, g2, thresholds, cell hits,
  // candidate pixels and their coordinates (the recipes use both regions at once)
  DeviceScratch rgbd_scratch;
  DeviceScratch rgbd_rows;  // the rows k_rgbd_rows writes of a device frame's kept pixels, until the ingest has read them (sized by the points kept, not by the frame)
  std::vector<unsigned char> rgbd_excl;  // staging of the exclusion bytes of a semantic frame
  RgbdStatsAcc rgbd_last{};
  RgbdSelectionAcc rgbd_sel{};
  StereoStatsAcc stereo_last{};  // (the stereo front end and cvo_fast_select share the RGB-D region)
  // LiDAR front end (cvo_lidar.hip): one growable device region - the scan, the range image's per-cell arrays, the
  // segmented cloud's arrays, the picks
  DeviceScratch lidar_scratch;
  LidarStatsAcc lidar_last{};
  // denoising (cvo_nlm.hip): one growable device region - the image, the denoised image, the weight tables
  DeviceScratch nlm_scratch;
  NlmStatsAcc nlm_last{};
  // stereo matcher (cvo_sgm.hip): one growable device region - the two gray planes, their census planes, the sums S of
  // rows x cols x max_disparity hypotheses (16 bits each), the disparity map
  DeviceScratch sgm_scratch;
  SgmStatsAcc sgm_last{};
  // disparity post-filter (cvo_dfilter.hip): one growable device region - the map, the union-find arrays, the gap scan's
  // indices, the map after each stage, the result with its counters
  DeviceScratch dfilter_scratch;
  // ... and its pinned host staging, kept between calls: the map on its way up, the result with its counters on its way down
  // (a pageable 1.9 MB copy either way, into fresh pages every call, cost the call tens of milliseconds: DESIGN.md section 3)
  PinnedRegion dfilter_staging;
  DFilterStatsAcc dfilter_last{};
  // clouds from device rows (cvo_ingest.hip): one growable device region - the jobs of k_cloud_ingest / k_cloud_gather and a
  // control block per cloud (flag words + per-block partials), read back with one copy
  DeviceScratch ingest_scratch;
  // merged and downloaded clouds (cvo_merge.hip): one growable device region - the jobs of k_cloud_unpack and the rows it
  // writes (coordinates packed, attributes in padded rows), read by the voxel selection, the ingest and the copies down
  DeviceScratch merge_scratch;
  double clock_ms_per_tick = 0.0;  // s_memrealtime, calibrated on first use (cvo_debug_kernel_clock)
};

namespace {

int fail(cvo_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess)                                                                       \
      return fail(ctx, CVO_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));           \
  } while (0)

}  // namespace

template <Mem K>
int Region<K>::reserve(cvo_ctx* ctx, size_t need, const char* what, hipStream_t drain, bool* moved) {
  if (need <= bytes) return CVO_OK;
  if (drain) HIP_TRY(ctx, hipStreamSynchronize(drain));
  release();
  void* q = nullptr;
  const hipError_t e = K == Mem::Device ? hipMalloc(&q, need)
                                        : hipHostMalloc(&q, need, K == Mem::Pinned ? hipHostMallocDefault : hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return fail(ctx, CVO_E_NOMEM, std::string(what) + " hipMalloc: " + hipGetErrorString(e));
  p = static_cast<char*>(q);
  bytes = need;
  if (moved) *moved = true;
  return CVO_OK;
}

template <Mem K>
template <class List>
int Region<K>::lay_out(cvo_ctx* ctx, const char* what, List list) {
  return lay_out(ctx, what, list, ctx->upload_stream);
}
