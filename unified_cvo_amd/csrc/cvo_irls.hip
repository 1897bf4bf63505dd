// cvo_irls.hip -- multi-frame align: CvoGPU::align(frames, frames_to_hold_const, edges) (CvoGPU.cu:1637-1683), i.e.
// CvoBatchIRLS::solve (IRLS.cpp:77-215) with a Levenberg-Marquardt trust-region loop in place of ceres::Solve.
// Per outer iteration every frame is re-transformed in place, every edge re-evaluated (run_single_eval) and its kernel
// matrix gathered on the device into the edge's resident entry list (k_irls_gather); per trust-region step the device
// reduces the per-edge cost / gradient / Gauss-Newton blocks (k_irls_normal) or the cost (k_irls_cost), and the host
// assembles and solves the dense 6F' x 6F' system of the free frames (Cholesky, double).  That solve - the trust-region
// loop, its Ceres constants, the termination reasons - is cvo_irls_solve.h, which knows nothing of the device: here are
// the device workspace (IrlsDevice), the evaluations it calls back (irls_eval), the outer loop as tests/np_multiframe.py's
// multiframe_align states it (validate, refresh the edges, build the table and solve, or decay ell) and the kernels'
// debug hooks.  DESIGN.md section 4 lists the constants and the reproduced Jacobian quirk.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

// Device side of a solve, and its owner: ONE region holding the edges' entry lists, the active edges' table, the poses,
// the block partials and the per-edge sums.  A count of zero is laid out as one element: every pointer that reaches a
// kernel is a valid device address of its own (an edge table without entry slots, a launch of zero blocks).
struct IrlsDevice {
  DeviceRegion region;  // (fresh, of one call: every user synchronises before it goes)
  IrlsEntry* ent = nullptr;
  IrlsEdge* edges = nullptr;
  double *poses = nullptr, *part = nullptr, *out = nullptr;
  int n_edges = 0, n_blocks = 0;  // of the table load() put there

  int reserve(cvo_ctx* ctx, const char* who, size_t slots, size_t max_edges, size_t frames, size_t max_blocks) {
    return region.lay_out(ctx, who, [&](ScratchLayout& l) {
      l.take(ent, std::max<size_t>(slots, 1));
      l.take(edges, std::max<size_t>(max_edges, 1));
      l.take(poses, 12 * std::max<size_t>(frames, 1));
      l.take(part, IRLS_W * std::max<size_t>(max_blocks, 1));
      l.take(out, IRLS_W * std::max<size_t>(max_edges, 1));
    }, nullptr);
  }
  // the launch table `tab` of n_blocks blocks (irls_table_add), enqueued
  int load(cvo_ctx* ctx, const std::vector<IrlsEdge>& tab, int nb) {
    n_edges = (int)tab.size();
    n_blocks = nb;
    HIP_TRY(ctx, hipMemcpyAsync(edges, tab.data(), sizeof(IrlsEdge) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
    return CVO_OK;
  }
};

// One k_irls_normal (normal) or k_irls_cost launch at the poses X (12 per frame, n_frames), then the ordered pass;
// out = n_edges x (91 or 1) doubles.  One synchronisation.
int irls_eval(cvo_ctx* ctx, const IrlsDevice& dv, const std::vector<double>& X, bool normal, std::vector<double>& out) {
  const int W = normal ? IRLS_W : 1;
  out.assign((size_t)dv.n_edges * W, 0.0);
  if (dv.n_edges == 0) return CVO_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dv.poses, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice, ctx->stream));
  if (dv.n_blocks > 0) {
    const auto kernel = normal ? k_irls_eval<true> : k_irls_eval<false>;
    hipLaunchKernelGGL(kernel, dim3(dv.n_blocks), dim3(IRLS_THREADS), 0, ctx->stream, dv.edges, dv.n_edges, dv.poses, dv.part);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_irls_finish, dim3(dv.n_edges), dim3(128), 0, ctx->stream, dv.edges, dv.n_edges, dv.n_blocks, W, dv.part, dv.out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(out.data(), dv.out, sizeof(double) * out.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CVO_OK;
}

inline int irls_blocks(int n) { return (n + IRLS_BLOCK_ENTRIES - 1) / IRLS_BLOCK_ENTRIES; }

// Appends one edge to a launch table: its first block (blk0) follows the blocks of the edges before it.  Returns the
// table's block count so far (the launch's n_blocks once every edge is in).  The only place blk0 is assigned.
int irls_table_add(std::vector<IrlsEdge>& tab, int n_blocks, const cvo_cloud* c1, const cvo_cloud* c2, int f1, int f2,
                   const IrlsEntry* ent, int slots) {
  tab.push_back(IrlsEdge{/*x1*/ c1->x4, /*x2*/ c2->x4, ent, /*n*/ slots, /*n1*/ c1->n, /*n2*/ c2->n, f1, f2, /*blk0*/ n_blocks});
  return n_blocks + irls_blocks(slots);
}

// k_irls_gather of the matrix the last evaluation left in pair 0's workspace into `ent` ([N x K] slots)
int irls_gather(cvo_ctx* ctx, int N, int K, IrlsEntry* ent) {
  const size_t slots = (size_t)N * K;
  hipLaunchKernelGGL(k_irls_gather, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const PairDesc*)ctx->d_descs, K, ent);
  HIP_TRY(ctx, hipGetLastError());
  return CVO_OK;
}

// ---- the pieces of cvo_multiframe_align, cut where np_multiframe.multiframe_align is ----

// The whole call's checks, before anything is written
int multiframe_validate(cvo_ctx* ctx, const cvo_params_t* params, int n_frames, const cvo_cloud* const* clouds, const double* poses,
                        int n_edges, const int* edges, const cvo_multiframe_trace_t* trace, int trace_capacity) {
  if (!ctx || !params) return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: bad argument");
  if (ctx->queue_open) return fail(ctx, CVO_E_INVALID, "a batch queue is open on this context (cvo_batch_close it first)");
  if (n_frames < 0 || n_edges < 0 || (n_frames > 0 && (!clouds || !poses)) || (n_edges > 0 && !edges) ||
      (trace_capacity > 0 && !trace) || params->multiframe_num_neighbors <= 0)
    return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: bad argument");
  if (n_frames > CVO_MULTIFRAME_MAX_FRAMES || n_edges > CVO_MULTIFRAME_MAX_EDGES)
    return fail(ctx, CVO_E_UNSUPPORTED, "cvo_multiframe_align: at most 64 frames and 2048 edges (the dense host system "
                                        "of the free frames is kept at most 384 x 384)");
  for (int f = 0; f < n_frames; f++) {
    if (!clouds[f]) return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: null cloud");
    if (clouds[f]->ctx != ctx) return fail(ctx, CVO_E_INVALID, "cloud belongs to another context");
    for (int q = 0; q < 12; q++)  // a NaN pose would read as a small gradient (std::max drops it) and reach the kernels
      if (!std::isfinite(poses[12 * (size_t)f + q])) return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: non-finite pose");
  }
  for (int k = 0; k < n_edges; k++) {
    const int a = edges[2 * k], b = edges[2 * k + 1];
    if (a < 0 || a >= n_frames || b < 0 || b >= n_frames)
      return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: edge frame index out of range");
    if (a == b) return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: self-edge");
    if (clouds[a]->n == 0 || clouds[b]->n == 0) return fail(ctx, CVO_E_INVALID, "cvo_multiframe_align: empty cloud in an edge");
  }
  return CVO_OK;
}

// What the outer loop carries from one iteration to the next: the call's frames and edges, per used frame its
// transformed cloud (refilled in place), per edge BinaryStateGPU's neighbour budget, largest row count and lengthscale,
// where its entry list begins and whether its last evaluation made it active; the device workspace.
struct Multiframe {
  const cvo_params_t& P;
  const int F, E;
  const cvo_cloud* const* clouds;
  const int* edges;
  std::vector<cvo_cloud*> tf;
  std::vector<unsigned> Kn, lastmax;
  std::vector<float> ell_e;
  std::vector<size_t> ent_off;
  std::vector<char> active;
  IrlsDevice dv;
  Multiframe(const cvo_params_t& params, int n_frames, int n_edges, const cvo_cloud* const* frames, const int* pairs)
      : P(params), F(n_frames), E(n_edges), clouds(frames), edges(pairs), tf(F, nullptr), Kn(E, (unsigned)P.multiframe_num_neighbors),
        lastmax(E, 0u), ell_e(E, P.multiframe_ell_init), ent_off(E + 1, 0), active(E, 0) {}
  ~Multiframe() {
    for (cvo_cloud* c : tf) cvo_cloud_free(c);
  }
};

// The transformed clouds of the frames some edge uses, and the workspace: every edge's entry list at the full neighbour
// budget, a table and a record per edge, a partial per block of every edge
int multiframe_setup(cvo_ctx* ctx, Multiframe& S, const std::vector<double>& X) {
  std::vector<char> used(S.F, 0);
  for (int k = 0; k < S.E; k++) used[S.edges[2 * k]] = used[S.edges[2 * k + 1]] = 1;
  for (int f = 0; f < S.F; f++) {
    if (!used[f]) continue;
    float pf[12];
    for (int q = 0; q < 12; q++) pf[q] = (float)X[12 * (size_t)f + q];
    if (const int rc = cvo_cloud_transformed(ctx, S.clouds[f], pf, &S.tf[f]); rc != CVO_OK) return rc;
  }
  int max_blocks = 0;
  for (int k = 0; k < S.E; k++) {
    const size_t slots = (size_t)S.clouds[S.edges[2 * k]]->n * S.Kn[k];  // (Kn: still the full budget)
    if (slots > (size_t)INT32_MAX) return fail(ctx, CVO_E_UNSUPPORTED, "cvo_multiframe_align: edge too large");
    S.ent_off[k + 1] = S.ent_off[k] + slots;
    max_blocks += irls_blocks((int)slots);
  }
  return S.dv.reserve(ctx, "cvo_multiframe_align", S.ent_off[S.E], S.E, S.F, max_blocks);
}

// The edges at the poses X.  Every used frame is transformed in place (the pose cast to float,
// CvoFrameGPU::transform_pointcloud); then BinaryStateGPU::update_inner_product on every edge (IRLS_State_GPU.cu:43-79):
// neighbour budget, evaluation, the matrix gathered into the edge's entry list on the device, its nonzero counts to the
// host.  Two synchronisations per edge.  Fills the row's active edges and total nonzeros.
int multiframe_refresh(cvo_ctx* ctx, Multiframe& S, const std::vector<double>& X, cvo_multiframe_trace_t* row) {
  for (int f = 0; f < S.F; f++) {
    if (!S.tf[f]) continue;
    const cvo_cloud* c = S.clouds[f];
    Pose12 pz;
    for (int q = 0; q < 12; q++) pz.T[q] = (float)X[12 * (size_t)f + q];
    hipLaunchKernelGGL(k_transform_pose, dim3((c->n + 255) / 256), dim3(256), 0, ctx->stream, c->n, pz, c->x4, c->xs4,
                       S.tf[f]->x4, S.tf[f]->xs4);
    HIP_TRY(ctx, hipGetLastError());
    transformed_bounds(c, pz.T, S.tf[f]);
    S.tf[f]->tiles.release();  // tile spheres of the old coordinates
    S.tf[f]->tile4 = nullptr;
  }
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const unsigned K0 = (unsigned)S.P.multiframe_num_neighbors;
  std::vector<unsigned> h_nz;
  for (int k = 0; k < S.E; k++) {
    if (S.lastmax[k] > 0) S.Kn[k] = std::min(K0, (unsigned)(S.lastmax[k] * 1.1));
    cvo_params_t pe = S.P;
    pe.nearest_neighbors_max = (int)S.Kn[k];
    const cvo_cloud *c1 = S.tf[S.edges[2 * k]], *c2 = S.tf[S.edges[2 * k + 1]];
    BatchSetup bs;
    if (const int rc = run_single_eval(ctx, &pe, c1, c2, I16, S.ell_e[k], &bs); rc != CVO_OK) return rc;
    const int N = c1->n;
    if (const int rc = irls_gather(ctx, N, (int)S.Kn[k], S.dv.ent + S.ent_off[k]); rc != CVO_OK) return rc;
    h_nz.resize(N);
    HIP_TRY(ctx, hipMemcpyAsync(h_nz.data(), ctx->h_descs[0].nnz_row, sizeof(unsigned) * N, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned s = 0, mx = 0;
    for (int r = 0; r < N; r++) {
      const unsigned c = std::min(nnz_count(h_nz[r]), S.Kn[k]);
      s += c;
      mx = std::max(mx, c);
    }
    S.lastmax[k] = mx;
    row->total_nonzeros += s;
    S.active[k] = (long long)s > (long long)S.P.multiframe_min_nonzeros;
    row->n_active_edges += S.active[k];
  }
  return CVO_OK;
}

// The solve (ceres::Solve with IRLS.cpp:164-176's options) over the active edges: their launch table, then
// cvo_irls::solve on the device's reductions.  pb: the free-frame map; its edges are set here.  X: updated in place.
int multiframe_solve(cvo_ctx* ctx, Multiframe& S, cvo_irls::Problem& pb, std::vector<double>& X, cvo_irls::Result* res) {
  std::vector<IrlsEdge> tab;
  pb.edges.clear();
  int nb = 0;
  for (int k = 0; k < S.E; k++) {
    if (!S.active[k]) continue;
    const int a = S.edges[2 * k], b = S.edges[2 * k + 1];
    nb = irls_table_add(tab, nb, S.clouds[a], S.clouds[b], a, b, S.dv.ent + S.ent_off[k], S.clouds[a]->n * (int)S.Kn[k]);
    pb.edges.emplace_back(a, b);
  }
  if (const int rc = S.dv.load(ctx, tab, nb); rc != CVO_OK) return rc;
  auto normal = [&](const std::vector<double>& Y, std::vector<double>& out) { return irls_eval(ctx, S.dv, Y, true, out); };
  auto cost = [&](const std::vector<double>& Y, std::vector<double>& out) { return irls_eval(ctx, S.dv, Y, false, out); };
  return cvo_irls::solve(pb, X, S.P.multiframe_iterations_per_solve, normal, cost, res);
}

}  // namespace

extern "C" {

int cvo_multiframe_align(cvo_ctx* ctx, const cvo_params_t* params, int n_frames, const cvo_cloud* const* clouds,
                         double* poses, const int* hold_const, int n_edges, const int* edges,
                         cvo_multiframe_info_t* info, cvo_multiframe_trace_t* trace, int trace_capacity, int* n_trace) {
  const auto t_start = std::chrono::steady_clock::now();
  int rc = multiframe_validate(ctx, params, n_frames, clouds, poses, n_edges, edges, trace, trace_capacity);
  if (rc != CVO_OK) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const cvo_params_t& P = *params;
  std::vector<double> X(poses, poses + 12 * (size_t)n_frames);
  cvo_irls::Problem pb;  // frame -> index among the free frames
  for (int f = 0, nf = 0; f < n_frames; f++) pb.free_index.push_back(hold_const && hold_const[f] ? -1 : nf++);
  Multiframe S(P, n_frames, n_edges, clouds, edges);
  if ((rc = multiframe_setup(ctx, S, X)) != CVO_OK) return rc;

  cvo_multiframe_info_t inf{};
  std::vector<cvo_multiframe_trace_t> rows;
  int iter = 0;
  bool converged = false;
  double ell = P.multiframe_ell_init;
  unsigned last_nonzeros = 0;
  while (!converged) {
    cvo_multiframe_trace_t row{};
    row.iter = iter;
    row.ell = (float)ell;
    if ((rc = multiframe_refresh(ctx, S, X, &row)) != CVO_OK) return rc;
    inf.last_total_nonzeros = row.total_nonzeros;
    inf.outer_iterations++;
    if (row.n_active_edges == 0 || iter == P.multiframe_max_iters) {
      rows.push_back(row);
      break;
    }
    if (row.total_nonzeros > last_nonzeros || iter < P.multiframe_iterations_per_ell) {
      last_nonzeros = row.total_nonzeros;
      cvo_irls::Result r;
      if ((rc = multiframe_solve(ctx, S, pb, X, &r)) != CVO_OK) return rc;
      row.solved = 1;
      row.steps = r.steps;
      row.accepted = r.accepted;
      row.termination = r.termination;
      row.cost_initial = r.cost_initial;
      row.cost_final = r.cost_final;
      inf.solves++;
      inf.steps += r.steps;
      inf.accepted_steps += r.accepted;
    } else {
      if (ell >= P.multiframe_ell_min) {
        last_nonzeros = 0;
        ell = ell * P.multiframe_ell_decay_rate;
        for (int k = 0; k < n_edges; k++)  // BinaryStateGPU::update_ell
          if (S.ell_e[k] > P.multiframe_ell_min) S.ell_e[k] = S.ell_e[k] * P.multiframe_ell_decay_rate;
      } else {
        converged = true;
      }
      if (iter > P.multiframe_max_iters) converged = true;
    }
    rows.push_back(row);
    iter++;
  }
  // ---- outputs ----
  inf.final_ell = (float)ell;
  inf.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  if (n_frames > 0) std::memcpy(poses, X.data(), sizeof(double) * X.size());
  const int nt = std::min((int)rows.size(), std::max(trace_capacity, 0));
  for (int i = 0; i < nt; i++) trace[i] = rows[i];
  if (n_trace) *n_trace = nt;
  if (info) *info = inf;
  return CVO_OK;
}

int cvo_debug_irls_normal(cvo_ctx* ctx, const cvo_cloud* frame1, const cvo_cloud* frame2, const double pose1[12],
                          const double pose2[12], double* out) {
  if (!ctx || !frame1 || !frame2 || !pose1 || !pose2 || !out) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_normal: bad argument");
  if (ctx->last_pairs < 1 || !ctx->last_params.keep_columns)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_normal: no evaluation with column indices on this context");
  const PairDesc& D = ctx->h_descs[0];
  if (D.N != frame1->n || D.M != frame2->n || D.N <= 0)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_normal: the clouds are not those of the last evaluation");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int K = ctx->last_params.K_max;
  const size_t slots = (size_t)D.N * K;
  IrlsDevice dv;
  int rc = dv.reserve(ctx, "cvo_debug_irls_normal", slots, 1, 2, irls_blocks((int)slots));
  if (rc != CVO_OK || (rc = irls_gather(ctx, D.N, K, dv.ent)) != CVO_OK) return rc;
  std::vector<IrlsEdge> tab;
  const int nb = irls_table_add(tab, 0, frame1, frame2, 0, 1, dv.ent, (int)slots);
  if ((rc = dv.load(ctx, tab, nb)) != CVO_OK) return rc;
  std::vector<double> X(pose1, pose1 + 12), o;
  X.insert(X.end(), pose2, pose2 + 12);
  if ((rc = irls_eval(ctx, dv, X, true, o)) != CVO_OK) return rc;
  std::memcpy(out, o.data(), sizeof(double) * IRLS_W);
  return CVO_OK;
}

int cvo_debug_irls_eval(cvo_ctx* ctx, int n_frames, const cvo_cloud* const* clouds, const double* poses, int n_edges,
                        const int* edge_frames, const int* slot_off, const int* ent_r, const int* ent_c, const float* ent_w,
                        int normal, double* out) {
  // ---- validation on the host, before any launch: the kernel's own range guard is never what stops a bad index ----
  if (!ctx || n_frames < 0 || n_edges < 0 || (n_frames > 0 && (!clouds || !poses)) ||
      (n_edges > 0 && (!edge_frames || !slot_off || !out)))
    return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: bad argument");
  if (n_frames > CVO_MULTIFRAME_MAX_FRAMES || n_edges > CVO_MULTIFRAME_MAX_EDGES)
    return fail(ctx, CVO_E_UNSUPPORTED, "cvo_debug_irls_eval: at most 64 frames and 2048 edges");
  for (int f = 0; f < n_frames; f++) {
    if (!clouds[f]) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: null cloud");
    if (clouds[f]->ctx != ctx) return fail(ctx, CVO_E_INVALID, "cloud belongs to another context");
  }
  if (n_edges == 0) return CVO_OK;
  if (slot_off[0] < 0) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: negative slot offset");
  for (int k = 0; k < n_edges; k++) {
    const int a = edge_frames[2 * k], b = edge_frames[2 * k + 1];
    if (a < 0 || a >= n_frames || b < 0 || b >= n_frames)
      return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: edge frame index out of range");
    if (slot_off[k + 1] < slot_off[k]) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: slot offsets decrease");
  }
  const size_t first = (size_t)slot_off[0], total = (size_t)slot_off[n_edges];
  if (total > first && (!ent_r || !ent_c || !ent_w)) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: bad argument");
  std::vector<IrlsEntry> h_ent(total - first);
  for (int k = 0; k < n_edges; k++) {
    const int n1 = clouds[edge_frames[2 * k]]->n, n2 = clouds[edge_frames[2 * k + 1]]->n;
    for (size_t i = (size_t)slot_off[k]; i < (size_t)slot_off[k + 1]; i++) {
      if (ent_c[i] >= 0 && (ent_r[i] < 0 || ent_r[i] >= n1 || ent_c[i] >= n2))
        return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_eval: stored entry out of range");
      h_ent[i - first] = IrlsEntry{ent_r[i], ent_c[i], ent_w[i], 0.f};
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // ---- the workspace (an edge's blocks follow from its slot count alone), then the launch table by the driver's builder ----
  size_t blocks = 0;
  for (int k = 0; k < n_edges; k++) blocks += irls_blocks(slot_off[k + 1] - slot_off[k]);
  IrlsDevice dv;
  int rc = dv.reserve(ctx, "cvo_debug_irls_eval", h_ent.size(), n_edges, n_frames, blocks);
  if (rc != CVO_OK) return rc;
  std::vector<IrlsEdge> tab;
  int nb = 0;
  for (int k = 0; k < n_edges; k++) {
    const int a = edge_frames[2 * k], b = edge_frames[2 * k + 1];
    nb = irls_table_add(tab, nb, clouds[a], clouds[b], a, b, dv.ent + ((size_t)slot_off[k] - first), slot_off[k + 1] - slot_off[k]);
  }
  if (!h_ent.empty())
    HIP_TRY(ctx, hipMemcpyAsync(dv.ent, h_ent.data(), sizeof(IrlsEntry) * h_ent.size(), hipMemcpyHostToDevice, ctx->stream));
  if ((rc = dv.load(ctx, tab, nb)) != CVO_OK) return rc;
  std::vector<double> X(poses, poses + 12 * (size_t)n_frames), o;
  if ((rc = irls_eval(ctx, dv, X, normal != 0, o)) != CVO_OK) return rc;
  std::memcpy(out, o.data(), sizeof(double) * o.size());
  return CVO_OK;
}

int cvo_debug_irls_gather(cvo_ctx* ctx, int K, int* r, int* c, float* w) {
  if (!ctx || !r || !c || !w) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_gather: bad argument");
  if (ctx->last_pairs < 1 || !ctx->last_params.keep_columns)
    return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_gather: no evaluation with column indices on this context");
  if (K != ctx->last_params.K_max)  // the budget the rows were stored under: what the driver gathers at
    return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_gather: K is not the neighbour budget of the last evaluation");
  const int N = ctx->h_descs[0].N;
  if (N <= 0 || K <= 0 || (size_t)N * K > (size_t)INT32_MAX) return fail(ctx, CVO_E_INVALID, "cvo_debug_irls_gather: bad size");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t slots = (size_t)N * K;
  DeviceRegion d_ent;
  int rc = d_ent.reserve(ctx, sizeof(IrlsEntry) * slots, "cvo_debug_irls_gather", nullptr);
  if (rc != CVO_OK || (rc = irls_gather(ctx, N, K, (IrlsEntry*)d_ent.p)) != CVO_OK) return rc;
  std::vector<IrlsEntry> h(slots);
  HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_ent.p, sizeof(IrlsEntry) * slots, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < slots; i++) {
    r[i] = h[i].r;
    c[i] = h[i].c;
    w[i] = h[i].w;
  }
  return CVO_OK;
}

}  // extern "C"
