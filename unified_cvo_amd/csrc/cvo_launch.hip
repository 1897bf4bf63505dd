// cvo_launch.hip -- every kernel launch of the solver: scan geometry, the launch wrappers of the row-block kernels, the flag words of an iteration (iteration_words), one iteration (launch_core) and one chunk of iterations (launch_chunk) as the graphs capture them.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
#ifndef CVO_COEFF_DENSE_MULTI_FROM
#define CVO_COEFF_DENSE_MULTI_FROM 8  // pairs per launch from which k_coeff_dense takes eight rows per wave
#endif

namespace {

void choose_scan_config(const cvo_ctx* ctx, int n_pairs, int NG, int Mpad, int* T_out, int* gpb_out) {
  const int T = 2;  // (1 / 4 / 8 were swept in round 2: the k_scan<T> instantiations remain)
  // Measured on MI355X (64 x 10k x 10k, T = 2): one row segment per wave (5120 waves) beats 128-group
  // blocks by 1.4x; a single pair needs the row range split to fill the chip.  Rule: the fewest
  // segments that still give ~4096 waves.
  const long slices = Mpad / (64 * T);
  const int ngr = (int)align_up((size_t)NG, 64);
  int gpb = ngr;
  while (gpb > 64) {
    const long waves = slices * ((ngr + gpb - 1) / gpb) * n_pairs;
    if (waves >= 4096) break;
    gpb = (int)align_up((size_t)gpb / 2, 64);
  }
  *T_out = T;
  *gpb_out = gpb;
}

// force: scan the pairs whose lists are current too (cvo_debug_time_scan); otherwise a pair is scanned when its list expired
void launch_scan(hipStream_t s, int T, dim3 grid, const PairDesc* descs, const DevParams* dp, const PairState* st, bool force) {
  switch (T) {
    case 1: hipLaunchKernelGGL(k_scan<1>, grid, dim3(256), 0, s, descs, dp, st, force); break;
    case 2: hipLaunchKernelGGL(k_scan<2>, grid, dim3(256), 0, s, descs, dp, st, force); break;
    case 4: hipLaunchKernelGGL(k_scan<4>, grid, dim3(256), 0, s, descs, dp, st, force); break;
    default: hipLaunchKernelGGL(k_scan<8>, grid, dim3(256), 0, s, descs, dp, st, force); break;
  }
}

// 1-D grid of the XCD-aware row-block kernels (see pair_block)
inline dim3 row_grid(int nblk, int n_pairs) { return dim3((unsigned)(nblk * ((n_pairs + 7) / 8 * 8))); }

void launch_list(hipStream_t s, bool idx16, int nblk, int n_pairs, const PairDesc* descs, const DevParams* dp,
                 const PairState* st) {
  const dim3 blk(LIST_THREADS), grid = row_grid(nblk, n_pairs);
  if (idx16)
    hipLaunchKernelGGL((k_list<unsigned short, ASSOC_CAP16>), grid, blk, 0, s, descs, dp, st, nblk, n_pairs);
  else
    hipLaunchKernelGGL((k_list<int, ASSOC_CAP32>), grid, blk, 0, s, descs, dp, st, nblk, n_pairs);
}

// instr: the instantiation with time stamps (CVO_KERNEL_CLOCK / CVO_PHASE_TICKS); the production kernels have none
template <typename IdxT, int CAP, int FEAT>
void launch_assoc_t(hipStream_t s, bool instr, dim3 grid, const PairDesc* descs, const DevParams* dp, const PairState* st,
                    const ArenaArg& A, int packed) {
  const dim3 blk(ASSOC_THREADS);
  if (instr)
    hipLaunchKernelGGL((k_assoc<IdxT, CAP, FEAT, true>), grid, blk, 0, s, descs, dp, st, A.base, packed, A.stride256, A.Npad);
  else
    hipLaunchKernelGGL((k_assoc<IdxT, CAP, FEAT, false>), grid, blk, 0, s, descs, dp, st, A.base, packed, A.stride256, A.Npad);
}

// feat: FEAT_GEO / FEAT_ALL / FEAT_COL / FEAT_HOT (cvo_pair_math.h), chosen per call by call_feat()
void launch_assoc(hipStream_t s, bool idx16, int feat, bool instr, int nblk, int n_pairs, const PairDesc* descs,
                  const DevParams* dp, const PairState* st, const ArenaArg& A, int flags) {
  const dim3 grid = row_grid(nblk, n_pairs);
  const int packed = pack_assoc_word(flags, nblk, n_pairs);  // (setup_batch bounds both)
#define CVO_ASSOC_CASE(F)                                                                              \
  case F:                                                                                              \
    if (idx16)                                                                                         \
      launch_assoc_t<unsigned short, ASSOC_CAP16, F>(s, instr, grid, descs, dp, st, A, packed);        \
    else                                                                                               \
      launch_assoc_t<int, ASSOC_CAP32, F>(s, instr, grid, descs, dp, st, A, packed);                   \
    break;
  switch (feat) {
    CVO_ASSOC_CASE(FEAT_GEO)
    CVO_ASSOC_CASE(FEAT_COL)
    CVO_ASSOC_CASE(FEAT_HOT)
    default:
      CVO_ASSOC_CASE(FEAT_ALL)
  }
#undef CVO_ASSOC_CASE
}

void launch_coeff(hipStream_t s, bool instr, int nblk, int split, int n_pairs, const PairDesc* descs, const DevParams* dp,
                  PairState* st, const ArenaArg& A, int flags) {
  const int packed = pack_coeff_word(nblk, split, n_pairs);  // (setup_batch bounds nblk and n_pairs)
  if (instr)
    hipLaunchKernelGGL(k_coeff<true>, row_grid(nblk * split + 1, n_pairs), dim3(ASSOC_THREADS), 0, s, descs, dp, st, A.base, flags,
                       packed, A.stride256, A.Npad);
  else  // (+ 1 block per pair: the speculative run of the update, update_speculate)
    hipLaunchKernelGGL(k_coeff<false>, row_grid(nblk * split + 1, n_pairs), dim3(ASSOC_THREADS), 0, s, descs, dp, st, A.base, flags,
                       packed, A.stride256, A.Npad);
}

// CVO_VERIFY_LISTS: literal re-derivation of every row after the association of an iteration (k_verify)
void launch_verify(hipStream_t s, int feat, int nblk, int n_pairs, const PairDesc* descs, const DevParams* dp, const int* st,
                   int flags) {
  const dim3 grid((unsigned)nblk, (unsigned)n_pairs);
  // (the self-check always takes the general form of the semantic kernel: one-hot rows through the row arithmetic)
  if (feat != FEAT_GEO)
    hipLaunchKernelGGL(k_verify<FEAT_ALL>, grid, dim3(256), 0, s, descs, dp, st, flags);
  else
    hipLaunchKernelGGL(k_verify<FEAT_GEO>, grid, dim3(256), 0, s, descs, dp, st, flags);
}

// a small pair solved alone has a block per overflow row (dense_blocks_for): k_assoc_dense's instantiation with the wide-row phase
inline bool dense_wide(int N, int n_pairs) { return n_pairs <= 1 && N <= DENSE_BLOCKS_MAX / 2; }

void launch_dense(hipStream_t s, int feat, bool wide, int n_pairs, int dense_blocks, const PairDesc* descs, const DevParams* dp,
                  const PairState* st) {
  const dim3 grid(dense_blocks, n_pairs);
#define CVO_LAUNCH_DENSE(F)                                                                                  \
  do {                                                                                                       \
    if (wide)                                                                                                \
      hipLaunchKernelGGL((k_assoc_dense<F, 4, true>), grid, dim3(256), 0, s, descs, dp, st);                 \
    else                                                                                                     \
      hipLaunchKernelGGL((k_assoc_dense<F, 4, false>), grid, dim3(256), 0, s, descs, dp, st);                \
  } while (0)
  switch (feat) {  // (4 waves per block: dense_waves_for)
    case FEAT_GEO: CVO_LAUNCH_DENSE(FEAT_GEO); break;
    case FEAT_COL: CVO_LAUNCH_DENSE(FEAT_COL); break;
    case FEAT_HOT: CVO_LAUNCH_DENSE(FEAT_HOT); break;
    default: CVO_LAUNCH_DENSE(FEAT_ALL); break;
  }
#undef CVO_LAUNCH_DENSE
}

// which instantiation of the association kernels a call needs (FEAT_*, cvo_pair_math.h)
inline int call_feat(const DevParams& dp, bool all_one_hot) {
  if (dp.mode == CALL_NONISO) return FEAT_ALL;
  if (!(dp.use_col || dp.use_sem || dp.use_geotype)) return FEAT_GEO;
  if (!dp.use_sem) return FEAT_COL;
  return all_one_hot ? FEAT_HOT : FEAT_ALL;
}

// What an iteration slot of a graph is.  iteration_words turns it into the flag words of its kernels; no other host code
// writes a flag value.
struct IterSlot {
  bool lean = false;             // a lean graph's slot: a pair that needs the rebuild kernels or k_assoc_dense waits
  bool lean_dense = false;       // ... a lean slot that runs k_assoc_dense all the same
  bool idx32 = false;            // 32-bit candidate lists (a LaunchGeom without idx16)
  bool rebuild_follows = false;  // the rebuild kernels run right after this iteration
  int horizon = 0;               // iterations the list has to survive without another rebuild opportunity (0: full graph)
  bool replay = false;           // timing replay of cvo_debug_time_kernels: nothing is written back
  bool asum_only = false;        // a single evaluation whose association only posts A_sum (run_ip_chain)
};
struct IterWords {
  int assoc;  // AssocFlags of k_assoc / k_verify
  int iter;   // IterFlags of k_coeff / k_update
};
inline IterWords iteration_words(const IterSlot& s) {
  const bool lean_dense = s.lean && s.lean_dense;
  return {(s.lean ? ASSOC_LEAN : 0) | (s.replay ? ASSOC_REPLAY : 0) | (lean_dense ? ASSOC_LEAN_DENSE : 0) |
              (s.asum_only ? ASSOC_ASUM_ONLY : 0),
          (s.lean ? ITER_LEAN : 0) | (s.rebuild_follows ? ITER_REBUILD_FOLLOWS : 0) | (s.replay ? ITER_REPLAY : 0) |
              (lean_dense ? ITER_LEAN_DENSE : 0) | (s.idx32 ? ITER_IDX32 : 0) | (s.horizon << ITER_HORIZON_SHIFT)};
}

void launch_init(cvo_ctx* c, const LaunchGeom& g) {
  hipLaunchKernelGGL(k_update<true>, dim3(g.n_pairs), dim3(64), 0, g.stream, c->d_descs + g.p0, c->d_params,
                     c->d_status + 2 * g.p0, iteration_words({}).iter);
}

// The rebuild kernels: no-ops (early exit) unless k_update flagged the pair's candidate list as expired.
void launch_rebuild(cvo_ctx* c, const LaunchGeom& g) {
  const PairDesc* descs = c->d_descs + g.p0;
  const PairState* states = c->d_states + g.p0;
  hipLaunchKernelGGL(k_prep, dim3(g.npb, g.n_pairs), dim3(PREP_THREADS), 0, g.stream, descs, c->d_params, states);
  launch_scan(g.stream, g.T, dim3(g.gx, g.gy, g.n_pairs), descs, c->d_params, states, false);
  launch_list(g.stream, g.idx16, g.nbl, g.n_pairs, descs, c->d_params, states);
}

// One optimiser iteration over the current lists: association, [overflow rows], coefficients + update (the last
// block of k_coeff).  Lean: no k_assoc_dense, pairs with overflow rows or an expired list wait - unless the slot is
// lean_dense (pairs with overflow rows / in the dense regime that need no rebuild opportunity in every iteration).
void launch_core(cvo_ctx* c, const LaunchGeom& g, const IterSlot& slot) {
  const PairDesc* descs = c->d_descs + g.p0;
  const int* st = c->d_status + 2 * g.p0;  // the sub-batch's status words (see setup_batch)
  const IterWords w = iteration_words(slot);
  const bool dense = !slot.lean || slot.lean_dense;
  // rows beyond their cached lists first (a wave per row; per-row results), then every row's reduction in k_assoc
  if (dense) launch_dense(g.stream, g.feat, g.wide, g.n_pairs, g.dense_blocks, descs, c->d_params, c->d_states + g.p0);
  launch_assoc(g.stream, g.idx16, g.feat, g.instr, g.nba, g.n_pairs, descs, c->d_params, c->d_states + g.p0, g.arena, w.assoc);
  if (g.verify) launch_verify(g.stream, g.feat, g.nbv, g.n_pairs, descs, c->d_params, st, w.assoc);
  // ... their coefficient sums likewise (k_coeff_dense leaves per-row sums, k_coeff picks them up)
  if (dense)
    // (7 waves per SIMD against k_assoc_dense's 4: twice the blocks, so that a lone pair's rows get a wave each - the kernel
    // then lasts as long as its longest row, not as two)
    hipLaunchKernelGGL((k_coeff_dense<4>), dim3(g.n_pairs <= 4 ? std::min(2 * g.dense_blocks, (int)DENSE_BLOCKS_MAX) : g.dense_blocks, g.n_pairs), dim3(256), 0, g.stream, descs,
                       c->d_params, c->d_states + g.p0, g.n_pairs >= CVO_COEFF_DENSE_MULTI_FROM ? 8 : 1);
  launch_coeff(g.stream, g.instr, g.nba, g.csplit, g.n_pairs, descs, c->d_params, c->d_states + g.p0, g.arena, w.iter);
}

// A chunk (see ChunkPlan).  Full: every iteration can rebuild its candidate list and serve overflow rows.  Full without
// dense: a rebuild opportunity in every iteration with the full graph's rebuild rule (no horizon), but a pair whose rows
// overflow their lists waits (and asks for the dense kernel: want = 4); large clouds run their fast first iterations
// here: the dense kernel, launched for nothing, is 5 us + a launch gap.  Lean kinds: rebuild opportunities only every
// `period` iterations; pairs that need more wait for a full chunk.
void launch_chunk(cvo_ctx* c, const LaunchGeom& g, const ChunkPlan& p) {
  if (p.every_iteration()) {
    const IterSlot slot{.lean = p.kind == ChunkKind::FullNoDense, .idx32 = !g.idx16, .rebuild_follows = true};
    for (int u = 0; u < p.U; u++) {
      launch_rebuild(c, g);
      launch_core(c, g, slot);
    }
    return;
  }
  for (int u = 0; u < p.U; u++) {
    if (u % p.period == 0) launch_rebuild(c, g);
    const bool last = (u % p.period == p.period - 1) || u == p.U - 1;
    // (horizon of the rebuild rule: the lean graph's period even in a calm chunk, whose one opportunity per chunk is a bet
    // on the list outliving the linear prediction - a pair that loses it waits for the next chunk)
    launch_core(c, g, {.lean = true, .lean_dense = p.dense, .idx32 = !g.idx16, .rebuild_follows = last,
                       .horizon = std::min(p.period, g.horizon_cap)});
  }
}

GraphKey graph_key(const LaunchGeom& g, const ChunkPlan& plan) {
  return {plan, g.n_pairs, g.p0, g.T, g.gx, g.gy, g.npb, g.nbl, g.nba, g.csplit, g.dense_blocks, g.horizon_cap, g.feat,
          g.idx16, g.wide, g.instr, g.verify, g.arena};
}

// Makes `cg` hold a graph of what `launches` enqueues on stream s, unless it already holds one captured for `key`.  On
// failure the n_flight streams of `flight` (other sub-batches may be in flight) are synchronised.
template <typename Launches>
int capture_graph(cvo_ctx* ctx, CachedGraph& cg, const GraphKey& key, hipStream_t s, const LaunchGeom* flight, int n_flight,
                  const char* what, Launches&& launches) {
  if (cg.exec && cg.key == key) return CVO_OK;
  if (cg.exec) (void)hipGraphExecDestroy(cg.exec);
  cg.exec = nullptr;
  hipGraph_t gr = nullptr;
  HIP_TRY(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  launches();
  // (the capture is always ended, whatever the launches reported: a stream left in capture mode would poison
  // every later call on this context)
  const hipError_t e_launch = hipGetLastError();
  hipError_t e = hipStreamEndCapture(s, &gr);
  if (e == hipSuccess && e_launch != hipSuccess) e = e_launch;
  if (e == hipSuccess) e = hipGraphInstantiate(&cg.exec, gr, nullptr, nullptr, 0);
  if (gr) (void)hipGraphDestroy(gr);
  if (e != hipSuccess) {
    cg.exec = nullptr;
    for (int q = 0; q < n_flight; q++) (void)hipStreamSynchronize(flight[q].stream);
    return fail(ctx, CVO_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  cg.key = key;
  return CVO_OK;
}

}  // namespace
