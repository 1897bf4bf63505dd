// cvo_options.h -- the tuning / diagnostic switches of a context (none changes a result): their typed values with the
// defaults (CtxOptions), and the ONE table that names them and says how their text is read (kOptions).  A context reads
// CVO_<NAME> from the environment once, when it is created; cvo_ctx_set_option changes a switch afterwards.  Those two are
// the only code that parses text (parse_option); every reader is a member access.  INTEGRATION.md documents the same names
// (tests/test_option_names.py).  Included by cvo_internal.h.
#pragma once

namespace {

constexpr int MAX_STREAMS = 8;    // sub-batch streams of a context (cvo_ctx::MAX_GROUPS)
constexpr float SKIN_MIN = 0.05f;  // lower clamp of the skin (DevParams::skin_min), a fraction of the cut-off radius

enum class CloudOrder { Device, Host, Virtual, Wide };  // who computes the spatial ordering of an upload (CVO_ORDER; the rule: order_route, cvo_upload.hip)

struct CtxOptions {
  // ---- list reuse / graphs (scripts/skin_sweep.py, early_sweep.py, first_chunk_sweep.sh) ----
  // List-reuse knobs, re-tuned in round 4 (scripts/skin_sweep.py, profiles/r4/skin_sweep.txt): the linear "outlives the
  // next h iterations at the current speed" predictions are pessimistic once the pose jitters around its optimum (the
  // allowance used since a build stays at a few percent while every iteration moves ~10 % of it), so thinner skins and
  // a smaller margin win on every configuration: headline batch 62.05 -> 60.6 ms, config 3 single pair 21.5 -> 18.8 us
  // per iteration.  (Round-2 values: 2.0 / 1.3 / 1.25.)
  float skin = 1.0f;  // 0 = rebuild every iteration
  float lean_skin = 0.5f;
  float horizon_margin = 0.3f;
  // (0.25 until round 6; re-swept on the un-aligned shrink rebuilds: 0.25 / 0.3 / 0.35 / 0.4 / 0.5 -> 55.55 / 55.22 / 55.06 /
  // 55.19 / 55.25 ms for the 64-pair step, 16 pairs -1.3 %, config 3 batch +0.3 %, single pairs unchanged: profiles/r6/shrink_align.txt)
  float skin_max = 0.35f;
  // (Round 4 made the optional shrink rebuilds of a batch wait for iteration counts that are multiples of 64 so that the pairs
  // of a sub-batch share a pass of the rebuild kernels: -1.7 % then.  Re-measured in round 6, with cheaper rebuild kernels and
  // a shorter serial tail: the stale lists' extra candidates cost more than the shared passes save - 64 x 10k geometric 56.55 ->
  // 55.67 ms, 64 x config 3 163.5 -> 158.1, 64 clustered scenes 793 -> 779, 16 / 32 pairs 0 / -1.6 % (profiles/r6/shrink_align.txt).
  // The mask stays as a switch.)
  int shrink_align = 0;
  int lean_U = 8;  // iterations between two rebuild opportunities of the lean graph
  bool no_lean = false, no_dense_regime = false, fixed_chunks = false;
  int first_U = 0;       // iterations of a call's first chunks; 0 = a quarter of the chunk length (cvo_align_batch)
  int first_chunks = 2;  // ... and how many of them there are
  int streams = 0;       // sub-batches of a call; 0 = by the number of pairs (plan_batch)
  int queue_admit = 4;   // the share of free slots - 1 / queue_admit - at which a settled sub-batch of a queue takes newcomers
  // ---- A/B switches of the tests: every one of them leaves the results bit-identical ----
  bool no_sort = false, no_long_lists = false, no_onehot = false, ip_chain = false, keep_columns = false, no_speculate = false;
  CloudOrder order = CloudOrder::Device;
  int wide_leaf = KD_WIDE_LEAF;  // ORDER=wide: the largest segment one block orders in LDS (cvo_k_kd_wide.h)
  int wide_record = 0;           // ORDER=wide, tests only: 1 = an upload keeps the select's pivots (cvo_debug_cloud_wide_pivots)
  int row_max = ASSOC_CAP16;  // DevParams::row_max_cap; ASSOC_CAP16 = off
  int voxel_host = -1;        // cvo_voxel_select / cvo_cloud_upload_voxel: 1 = the CPU twin, 0 = the kernels, -1 = by size (cvo_voxel.hip)
  int rgbd_host = -1;         // cvo_rgbd_points / cvo_cloud_upload_rgbd: 1 = the CPU twin, 0 = the kernels, -1 = by size (cvo_rgbd.hip)
  int stereo_host = -1;       // cvo_stereo_points / cvo_cloud_upload_stereo* / cvo_fast_select: as rgbd_host (cvo_fast.hip)
  int lidar_host = -1;        // cvo_lidar_select / cvo_cloud_upload_lidar: as rgbd_host (cvo_lidar.hip)
  int nlm_host = -1;          // cvo_nlm_denoise / cvo_nlm_denoise_lab: as rgbd_host (cvo_nlm.hip)
  int sgm_host = -1;          // cvo_stereo_disparity / cvo_cloud_upload_stereo_pair's matcher: as rgbd_host (cvo_sgm.hip)
  int dfilter_host = -1;      // cvo_disparity_filter / the filter of the _filtered entry points: as rgbd_host (cvo_dfilter.hip)
  int bki_host = -1;          // the side a cvo_map takes at its first insert: 1 = the CPU twin, 0 = the kernels, -1 = by size (cvo_bki.hip)
  int fast_tile = 1;          // k_fast_score reads the ring from an LDS tile with a 3-pixel halo; 0: through the cache
  int voxel_prepass = 1;      // k_voxel_insert resolves a block's duplicates in LDS first
  // ---- diagnostics ----
  int verbose = 0;  // 0 silent, 1 / 2 / 3: INTEGRATION.md
  bool kernel_clock = false, phase_ticks = false, verify_lists = false, debug_no_motion_bound = false;
  int debug_drop_partial = 0;
};

// How the text of a switch is read.  Flag: on unless unset or a number equal to 0 ("1", "" and "yes" are on).  Level: a flag
// whose number, when it has one above 1, is kept.  Integer / Real: atoi / atof (text without a number is 0), then the clamp.
// Order: "host" / "virtual" / "wide", anything else is the device's ordering.
enum class OptKind { Flag, Level, Integer, Real, Order };

struct OptionSpec {
  const char* name;  // without the CVO_ prefix
  OptKind kind;
  bool CtxOptions::*flag;
  int CtxOptions::*integer;
  float CtxOptions::*real;
  double lo, hi;  // clamp of an Integer / Real, applied to what the text parses to
};
constexpr OptionSpec opt_flag(const char* name, bool CtxOptions::*m) { return {name, OptKind::Flag, m, nullptr, nullptr, 0, 0}; }
constexpr OptionSpec opt_int(const char* name, int CtxOptions::*m, double lo = INT_MIN, double hi = INT_MAX) { return {name, OptKind::Integer, nullptr, m, nullptr, lo, hi}; }
constexpr OptionSpec opt_real(const char* name, float CtxOptions::*m, double lo) { return {name, OptKind::Real, nullptr, nullptr, m, lo, HUGE_VAL}; }

constexpr OptionSpec kOptions[] = {
    opt_real("SKIN", &CtxOptions::skin, 0.0),
    opt_real("SKIN_MAX", &CtxOptions::skin_max, SKIN_MIN),
    opt_real("LEAN_SKIN", &CtxOptions::lean_skin, 0.1),
    opt_real("HORIZON_MARGIN", &CtxOptions::horizon_margin, 0.0),
    opt_int("SHRINK_ALIGN", &CtxOptions::shrink_align, 0),
    opt_int("LEAN_U", &CtxOptions::lean_U, 1),
    opt_flag("NO_LEAN", &CtxOptions::no_lean),
    opt_flag("NO_DENSE_REGIME", &CtxOptions::no_dense_regime),
    opt_flag("FIXED_CHUNKS", &CtxOptions::fixed_chunks),
    opt_int("FIRST_U", &CtxOptions::first_U, 1),  // (and at most the call's chunk length: cvo_align_batch)
    opt_int("FIRST_CHUNKS", &CtxOptions::first_chunks, 0),
    opt_int("STREAMS", &CtxOptions::streams, 1, MAX_STREAMS),  // (and at most the call's pairs: plan_batch)
    opt_int("QUEUE_ADMIT", &CtxOptions::queue_admit, 1),
    opt_flag("NO_SORT", &CtxOptions::no_sort),
    {"ORDER", OptKind::Order, nullptr, nullptr, nullptr, 0, 0},
    opt_int("WIDE_LEAF", &CtxOptions::wide_leaf, KD_THREADS, KD_MAX_POINTS),
    opt_int("WIDE_RECORD", &CtxOptions::wide_record, 0, 1),
    opt_flag("NO_LONG_LISTS", &CtxOptions::no_long_lists),
    opt_int("ROW_MAX", &CtxOptions::row_max, 1, ASSOC_CAP16),
    opt_flag("NO_ONEHOT", &CtxOptions::no_onehot),
    opt_flag("IP_CHAIN", &CtxOptions::ip_chain),
    opt_flag("KEEP_COLUMNS", &CtxOptions::keep_columns),
    opt_flag("NO_SPECULATE", &CtxOptions::no_speculate),
    opt_int("VOXEL_HOST", &CtxOptions::voxel_host, -1, 1),
    opt_int("VOXEL_PREPASS", &CtxOptions::voxel_prepass, 0, 1),
    opt_int("RGBD_HOST", &CtxOptions::rgbd_host, -1, 1),
    opt_int("STEREO_HOST", &CtxOptions::stereo_host, -1, 1),
    opt_int("LIDAR_HOST", &CtxOptions::lidar_host, -1, 1),
    opt_int("NLM_HOST", &CtxOptions::nlm_host, -1, 1),
    opt_int("SGM_HOST", &CtxOptions::sgm_host, -1, 1),
    opt_int("DFILTER_HOST", &CtxOptions::dfilter_host, -1, 1),
    opt_int("BKI_HOST", &CtxOptions::bki_host, -1, 1),
    opt_int("FAST_TILE", &CtxOptions::fast_tile, 0, 1),
    {"VERBOSE", OptKind::Level, nullptr, &CtxOptions::verbose, nullptr, 0, 0},
    opt_flag("KERNEL_CLOCK", &CtxOptions::kernel_clock),
    opt_flag("PHASE_TICKS", &CtxOptions::phase_ticks),
    opt_flag("VERIFY_LISTS", &CtxOptions::verify_lists),
    opt_flag("DEBUG_NO_MOTION_BOUND", &CtxOptions::debug_no_motion_bound),
    opt_int("DEBUG_DROP_PARTIAL", &CtxOptions::debug_drop_partial),
};

// Sets the switch `s` of `o` from `text`; nullptr = back to its default
inline void parse_option(CtxOptions& o, const OptionSpec& s, const char* text) {
  const CtxOptions def;
  char* end = nullptr;
  const bool on = text && !(std::strtol(text, &end, 10) == 0 && end != text);
  switch (s.kind) {
    case OptKind::Flag: o.*s.flag = on; break;
    case OptKind::Level: o.*s.integer = on ? std::max(1, atoi(text)) : 0; break;
    case OptKind::Integer: o.*s.integer = text ? std::max((int)s.lo, std::min(atoi(text), (int)s.hi)) : def.*s.integer; break;
    case OptKind::Real: o.*s.real = text ? std::max((float)s.lo, std::min((float)atof(text), (float)s.hi)) : def.*s.real; break;
    case OptKind::Order: o.order = !text ? def.order : (!std::strcmp(text, "host") ? CloudOrder::Host : (!std::strcmp(text, "virtual") ? CloudOrder::Virtual : (!std::strcmp(text, "wide") ? CloudOrder::Wide : CloudOrder::Device))); break;
  }
}

}  // namespace
