// cvo_irls.hip -- multi-frame align: CvoGPU::align(frames, frames_to_hold_const, edges) (CvoGPU.cu:1637-1683), i.e.
// CvoBatchIRLS::solve (IRLS.cpp:77-215) with a Levenberg-Marquardt trust-region loop in place of ceres::Solve.
// Per outer iteration every frame is re-transformed in place, every edge re-evaluated (run_single_eval) and its kernel
// matrix gathered on the device into the edge's resident entry list (k_irls_gather); per trust-region step the device
// reduces the per-edge cost / gradient / Gauss-Newton blocks (k_irls_normal) or the cost (k_irls_cost), and the host
// assembles and solves the dense 6F' x 6F' system of the free frames (Cholesky, double).  DESIGN.md section 4 lists the
// Ceres constants and the reproduced Jacobian quirk.
// A SECTION of the one translation unit cvo_hip.hip (which includes the sections in dependency order and says why it is one
// unit); not compiled on its own.  Shared declarations: cvo_internal.h.
namespace {

// Exp_SE3(delta, is_wu = false) (LieGroup.cpp:169-192): u = delta[0..2] (translation), w = delta[3..5] (rotation);
// Exp_SO3 / LeftJacobian_SO3 (LieGroup.cpp:28-55) with TOLERANCE = 1e-6f.  X: 3x4 row-major.
void irls_exp_se3(const double d[6], double X[12]) {
  const double w[3] = {d[3], d[4], d[5]};
  const double A[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double A2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A2[3 * i + j] = A[3 * i] * A[j] + A[3 * i + 1] * A[3 + j] + A[3 * i + 2] * A[6 + j];
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double R[9], V[9];
  for (int i = 0; i < 9; i++) R[i] = V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (!(th < (double)1e-6f)) {
    const double a = std::sin(th) / th, b = (1 - std::cos(th)) / (th * th), c = (th - std::sin(th)) / (th * th * th);
    for (int i = 0; i < 9; i++) {
      R[i] = R[i] + a * A[i] + b * A2[i];
      V[i] = V[i] + b * A[i] + c * A2[i];
    }
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) X[4 * r + c] = R[3 * r + c];
    X[4 * r + 3] = V[3 * r] * d[0] + V[3 * r + 1] * d[1] + V[3 * r + 2] * d[2];
  }
}

// LocalParameterizationSE3::Plus (local_parameterization_se3.hpp:22-41): T * Exp_SE3(delta)
void irls_plus(const double T[12], const double d[6], double out[12]) {
  double X[12];
  irls_exp_se3(d, X);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      double v = T[4 * r] * X[c] + T[4 * r + 1] * X[4 + c] + T[4 * r + 2] * X[8 + c];
      if (c == 3) v += T[4 * r + 3];
      out[4 * r + c] = v;
    }
}

// In-place Cholesky solve of the SPD system M x = b (n x n row-major); false when M is not positive definite.
bool irls_cholesky_solve(std::vector<double>& M, int n, std::vector<double>& b) {
  for (int j = 0; j < n; j++) {
    double d = M[(size_t)j * n + j];
    for (int k = 0; k < j; k++) d -= M[(size_t)j * n + k] * M[(size_t)j * n + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double l = std::sqrt(d);
    M[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; i++) {
      double v = M[(size_t)i * n + j];
      for (int k = 0; k < j; k++) v -= M[(size_t)i * n + k] * M[(size_t)j * n + k];
      M[(size_t)i * n + j] = v / l;
    }
  }
  for (int i = 0; i < n; i++) {
    double v = b[i];
    for (int k = 0; k < i; k++) v -= M[(size_t)i * n + k] * b[k];
    b[i] = v / M[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double v = b[i];
    for (int k = i + 1; k < n; k++) v -= M[(size_t)k * n + i] * b[k];
    b[i] = v / M[(size_t)i * n + i];
  }
  return true;
}

// Device side of one solve: the active edges' table, the poses, the block partials and the per-edge sums.
struct IrlsDevice {
  IrlsEdge* edges = nullptr;
  double* poses = nullptr;
  double* part = nullptr;
  double* out = nullptr;
  int n_edges = 0, n_blocks = 0;
};

// One k_irls_normal (normal) or k_irls_cost launch at the poses X (12 per frame, n_frames), then the ordered pass;
// out = n_edges x (91 or 1) doubles.  One synchronisation.
int irls_eval(cvo_ctx* ctx, const IrlsDevice& dv, const std::vector<double>& X, bool normal, std::vector<double>& out) {
  const int W = normal ? IRLS_W : 1;
  out.assign((size_t)dv.n_edges * W, 0.0);
  if (dv.n_edges == 0) return CVO_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dv.poses, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice, ctx->stream));
  if (dv.n_blocks > 0) {
    if (normal)
      hipLaunchKernelGGL(k_irls_eval<true>, dim3(dv.n_blocks), dim3(IRLS_THREADS), 0, ctx->stream, dv.edges, dv.n_edges,
                         dv.poses, dv.part);
    else
      hipLaunchKernelGGL(k_irls_eval<false>, dim3(dv.n_blocks), dim3(IRLS_THREADS), 0, ctx->stream, dv.edges, dv.n_edges,
                         dv.poses, dv.part);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_irls_finish, dim3(dv.n_edges), dim3(128), 0, ctx->stream, dv.edges, dv.n_edges, dv.n_blocks, W,
                     dv.part, dv.out);
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
  IrlsEdge ed;
  ed.x1 = c1->x4;
  ed.x2 = c2->x4;
  ed.ent = ent;
  ed.n = slots;
  ed.n1 = c1->n;
  ed.n2 = c2->n;
  ed.f1 = f1;
  ed.f2 = f2;
  ed.blk0 = n_blocks;
  tab.push_back(ed);
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

}  // namespace

extern "C" {

int cvo_multiframe_align(cvo_ctx* ctx, const cvo_params_t* params, int n_frames, const cvo_cloud* const* clouds,
                         double* poses, const int* hold_const, int n_edges, const int* edges,
                         cvo_multiframe_info_t* info, cvo_multiframe_trace_t* trace, int trace_capacity, int* n_trace) {
  const auto t_start = std::chrono::steady_clock::now();
  // ---- validation: the whole call, before anything is written ----
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
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const cvo_params_t& P = *params;
  const int F = n_frames, E = n_edges;
  std::vector<double> X(poses, poses + 12 * (size_t)F);
  std::vector<int> fi(F, -1);  // frame -> index among the free frames
  int nf = 0;
  for (int f = 0; f < F; f++)
    if (!(hold_const && hold_const[f])) fi[f] = nf++;
  const int m = 6 * nf;

  // ---- per-frame transformed clouds (refilled in place) and per-edge state and entry lists ----
  std::vector<cvo_cloud*> tf(F, nullptr);
  struct CloudsGuard {
    std::vector<cvo_cloud*>& v;
    ~CloudsGuard() {
      for (cvo_cloud* c : v) cvo_cloud_free(c);
    }
  } tf_guard{tf};
  std::vector<char> used(F, 0);
  for (int k = 0; k < E; k++) used[edges[2 * k]] = used[edges[2 * k + 1]] = 1;
  for (int f = 0; f < F; f++) {
    if (!used[f]) continue;
    float pf[12];
    for (int q = 0; q < 12; q++) pf[q] = (float)X[12 * (size_t)f + q];
    const int rc = cvo_cloud_transformed(ctx, clouds[f], pf, &tf[f]);
    if (rc != CVO_OK) return rc;
  }
  const unsigned K0 = (unsigned)P.multiframe_num_neighbors;
  std::vector<unsigned> Kn(E, K0), lastmax(E, 0u), nnz(E, 0u);
  std::vector<float> ell_e(E, P.multiframe_ell_init);
  std::vector<size_t> ent_off(E + 1, 0);
  int max_blocks = 0;
  for (int k = 0; k < E; k++) {
    const size_t slots = (size_t)clouds[edges[2 * k]]->n * K0;
    if (slots > (size_t)INT32_MAX) return fail(ctx, CVO_E_UNSUPPORTED, "cvo_multiframe_align: edge too large");
    ent_off[k + 1] = ent_off[k] + slots;
    max_blocks += irls_blocks((int)slots);
  }
  DeviceRegion d_ent, d_edges, d_poses, d_part, d_out;  // (of this call: they go with the scope)
  auto dmalloc = [&](DeviceRegion& a, size_t bytes) { return a.reserve(ctx, std::max<size_t>(bytes, 256), "cvo_multiframe_align", nullptr); };
  if (int rc; (rc = dmalloc(d_ent, sizeof(IrlsEntry) * ent_off[E])) != CVO_OK || (rc = dmalloc(d_edges, sizeof(IrlsEdge) * E)) != CVO_OK ||
      (rc = dmalloc(d_poses, sizeof(double) * 12 * F)) != CVO_OK ||
      (rc = dmalloc(d_part, sizeof(double) * IRLS_W * (size_t)max_blocks)) != CVO_OK ||
      (rc = dmalloc(d_out, sizeof(double) * IRLS_W * E)) != CVO_OK)
    return rc;
  IrlsEntry* ent = (IrlsEntry*)d_ent.p;
  IrlsDevice dv;
  dv.edges = (IrlsEdge*)d_edges.p;
  dv.poses = (double*)d_poses.p;
  dv.part = (double*)d_part.p;
  dv.out = (double*)d_out.p;

  cvo_multiframe_info_t inf{};
  std::vector<cvo_multiframe_trace_t> rows;
  const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<unsigned> h_nz;
  std::vector<double> out;
  int iter = 0;
  bool converged = false;
  double ell = P.multiframe_ell_init;
  unsigned last_nonzeros = 0;
  while (!converged) {
    // transform every frame (the pose cast to float, CvoFrameGPU::transform_pointcloud), in place
    for (int f = 0; f < F; f++) {
      if (!tf[f]) continue;
      Pose12 pz;
      for (int q = 0; q < 12; q++) pz.T[q] = (float)X[12 * (size_t)f + q];
      hipLaunchKernelGGL(k_transform_pose, dim3((clouds[f]->n + 255) / 256), dim3(256), 0, ctx->stream, clouds[f]->n, pz,
                         clouds[f]->x4, clouds[f]->xs4, tf[f]->x4, tf[f]->xs4);
      HIP_TRY(ctx, hipGetLastError());
      transformed_bounds(clouds[f], pz.T, tf[f]);
      tf[f]->tiles.release();  // tile spheres of the old coordinates
      tf[f]->tile4 = nullptr;
    }
    // BinaryStateGPU::update_inner_product on every edge (IRLS_State_GPU.cu:43-79): neighbour budget, evaluation,
    // the matrix gathered into the edge's entry list on the device, its nonzero counts to the host
    int counter = 0;
    unsigned total = 0;
    std::vector<char> active(E, 0);
    for (int k = 0; k < E; k++) {
      if (lastmax[k] > 0) Kn[k] = std::min(K0, (unsigned)(lastmax[k] * 1.1));
      cvo_params_t pe = P;
      pe.nearest_neighbors_max = (int)Kn[k];
      const cvo_cloud* c1 = tf[edges[2 * k]];
      const cvo_cloud* c2 = tf[edges[2 * k + 1]];
      BatchSetup S;
      int rc = run_single_eval(ctx, &pe, c1, c2, I16, ell_e[k], &S);
      if (rc != CVO_OK) return rc;
      const int N = c1->n;
      rc = irls_gather(ctx, N, (int)Kn[k], ent + ent_off[k]);
      if (rc != CVO_OK) return rc;
      h_nz.resize(N);
      HIP_TRY(ctx, hipMemcpyAsync(h_nz.data(), ctx->h_descs[0].nnz_row, sizeof(unsigned) * N, hipMemcpyDeviceToHost,
                                  ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      unsigned s = 0, mx = 0;
      for (int r = 0; r < N; r++) {
        const unsigned c = std::min(nnz_count(h_nz[r]), Kn[k]);
        s += c;
        mx = std::max(mx, c);
      }
      nnz[k] = s;
      lastmax[k] = mx;
      total += s;
      if ((long long)s > (long long)P.multiframe_min_nonzeros) {
        active[k] = 1;
        counter++;
      }
    }
    cvo_multiframe_trace_t row{};
    row.iter = iter;
    row.n_active_edges = counter;
    row.ell = (float)ell;
    row.total_nonzeros = total;
    inf.last_total_nonzeros = total;
    inf.outer_iterations++;
    if (counter == 0 || iter == P.multiframe_max_iters) {
      rows.push_back(row);
      break;
    }
    if (total > last_nonzeros || iter < P.multiframe_iterations_per_ell) {
      last_nonzeros = total;
      // ---- the solve (ceres::Solve with IRLS.cpp:164-176's options) ----
      std::vector<IrlsEdge> tab;
      int nb = 0;
      for (int k = 0; k < E; k++) {
        if (!active[k]) continue;
        const int a = edges[2 * k], b = edges[2 * k + 1];
        nb = irls_table_add(tab, nb, clouds[a], clouds[b], a, b, ent + ent_off[k], clouds[a]->n * (int)Kn[k]);
      }
      dv.n_edges = (int)tab.size();
      dv.n_blocks = nb;
      HIP_TRY(ctx, hipMemcpyAsync(dv.edges, tab.data(), sizeof(IrlsEdge) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
      // normal equations of the free frames at X
      std::vector<double> H, g;
      double cost = 0;
      auto assemble = [&](const std::vector<double>& o) {
        H.assign((size_t)m * m, 0.0);
        g.assign(m, 0.0);
        cost = 0;
        for (size_t t = 0; t < tab.size(); t++) {
          const double* v = &o[t * IRLS_W];
          cost += v[0];
          const int fr[2] = {fi[tab[t].f1], fi[tab[t].f2]};
          auto gi = [&](int q) { return fr[q / 6] < 0 ? -1 : 6 * fr[q / 6] + q % 6; };
          for (int q = 0; q < 12; q++)
            if (gi(q) >= 0) g[gi(q)] += v[1 + q];
          int h = 13;
          for (int q = 0; q < 12; q++)
            for (int s = q; s < 12; s++, h++) {
              const int i = gi(q), j = gi(s);
              if (i < 0 || j < 0) continue;
              H[(size_t)i * m + j] += v[h];
              if (s != q) H[(size_t)j * m + i] += v[h];
            }
        }
      };
      auto free_norm = [&](const std::vector<double>& Y) {
        double s = 0;
        for (int f = 0; f < F; f++)
          if (fi[f] >= 0)
            for (int q = 0; q < 12; q++) s += Y[12 * (size_t)f + q] * Y[12 * (size_t)f + q];
        return std::sqrt(s);
      };
      auto plus_all = [&](const std::vector<double>& Y, const std::vector<double>& d, double sign, std::vector<double>& Z) {
        Z = Y;
        for (int f = 0; f < F; f++) {
          if (fi[f] < 0) continue;
          double dd[6];
          for (int q = 0; q < 6; q++) dd[q] = sign * d[6 * fi[f] + q];
          irls_plus(&Y[12 * (size_t)f], dd, &Z[12 * (size_t)f]);
        }
      };
      auto gradient_small = [&]() {  // gradient_tolerance: |x - Plus(x, -g)|_inf <= 1e-5
        std::vector<double> Z;
        plus_all(X, g, -1.0, Z);
        double mx = 0;
        for (int f = 0; f < F; f++)
          if (fi[f] >= 0)
            for (int q = 0; q < 12; q++) mx = std::max(mx, std::fabs(X[12 * (size_t)f + q] - Z[12 * (size_t)f + q]));
        return mx <= 1e-5;
      };
      int rc = irls_eval(ctx, dv, X, true, out);
      if (rc != CVO_OK) return rc;
      assemble(out);
      row.solved = 1;
      row.cost_initial = row.cost_final = cost;
      std::vector<double> sc(m);  // Jacobi scaling from the first Jacobian: s_i = 1 / (1 + |J_i|)
      for (int i = 0; i < m; i++) sc[i] = 1.0 / (1.0 + std::sqrt(H[(size_t)i * m + i]));
      double mu = 1e4;             // initial_trust_region_radius
      const double mu_max = 1e16;  // max_trust_region_radius
      const double mu_min = 1e-32; // min_trust_region_radius
      double decrease = 2.0;       // LevenbergMarquardtStrategy's radius decrease factor, reset on success
      int invalid = 0, steps = 0, accepted = 0, term = 0;
      if (gradient_small()) term = 2;
      std::vector<double> Mx, dlt, Xc;
      while (!term) {
        if (steps >= P.multiframe_iterations_per_solve) {  // max_num_iterations
          term = 5;
          break;
        }
        steps++;
        Mx = H;
        for (int i = 0; i < m; i++) {  // (H + diag(D) / mu): D_ii = clamp(s_i^2 H_ii, min_lm_diagonal 1e-6, max_lm_diagonal 1e32) / s_i^2
          const double s2 = sc[i] * sc[i];
          const double Dii = std::min(std::max(s2 * H[(size_t)i * m + i], 1e-6), 1e32) / s2;
          Mx[(size_t)i * m + i] += Dii / mu;
        }
        dlt.assign(m, 0.0);
        for (int i = 0; i < m; i++) dlt[i] = -g[i];
        bool valid = irls_cholesky_solve(Mx, m, dlt);
        double model = 0, cost_new = NAN;
        if (valid) {  // model cost change -(g^T d + 1/2 d^T H d)
          double gd = 0, dHd = 0;
          for (int i = 0; i < m; i++) {
            gd += g[i] * dlt[i];
            double hd = 0;
            for (int j = 0; j < m; j++) hd += H[(size_t)i * m + j] * dlt[j];
            dHd += dlt[i] * hd;
          }
          model = -(gd + 0.5 * dHd);
          valid = std::isfinite(model) && model > 0;
        }
        if (valid) {
          double dn = 0;
          for (int i = 0; i < m; i++) dn += dlt[i] * dlt[i];
          if (std::sqrt(dn) <= 1e-5 * (free_norm(X) + 1e-5)) {  // parameter_tolerance
            term = 3;
            break;
          }
          plus_all(X, dlt, 1.0, Xc);
          rc = irls_eval(ctx, dv, Xc, false, out);
          if (rc != CVO_OK) return rc;
          cost_new = 0;
          for (size_t t = 0; t < tab.size(); t++) cost_new += out[t];
          valid = std::isfinite(cost_new);
        }
        if (!valid) {
          // max_num_consecutive_invalid_steps = 5: Ceres' TrustRegionMinimizer::HandleInvalidStep fails once
          // ++num_consecutive_invalid_steps_ >= max_num_consecutive_invalid_steps, i.e. on the 5th in a row
          if (++invalid >= 5) {
            term = 6;
            break;
          }
        } else {
          invalid = 0;
          const double rho = (cost - cost_new) / model;
          if (rho > 1e-3) {  // min_relative_decrease
            X = Xc;
            const double t = 2.0 * rho - 1.0;
            mu = std::min(mu_max, mu / std::max(1.0 / 3.0, 1.0 - t * t * t));
            decrease = 2.0;
            accepted++;
            const double cost_old = cost;
            rc = irls_eval(ctx, dv, X, true, out);
            if (rc != CVO_OK) return rc;
            assemble(out);
            row.cost_final = cost;
            if (std::fabs(cost_old - cost_new) / cost_old <= 1e-5) {  // function_tolerance
              term = 1;
              break;
            }
            if (gradient_small()) {  // gradient_tolerance
              term = 2;
              break;
            }
            continue;
          }
        }
        mu /= decrease;  // rejected (or invalid) step
        decrease *= 2.0;
        if (mu < mu_min) {
          term = 4;
          break;
        }
      }
      row.steps = steps;
      row.accepted = accepted;
      row.termination = term;
      inf.solves++;
      inf.steps += steps;
      inf.accepted_steps += accepted;
    } else {
      if (ell >= P.multiframe_ell_min) {
        last_nonzeros = 0;
        ell = ell * P.multiframe_ell_decay_rate;
        for (int k = 0; k < E; k++)  // BinaryStateGPU::update_ell
          if (ell_e[k] > P.multiframe_ell_min) ell_e[k] = ell_e[k] * P.multiframe_ell_decay_rate;
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
  if (F > 0) std::memcpy(poses, X.data(), sizeof(double) * X.size());
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
  DeviceRegion d_ent, d_edges, d_poses, d_part, d_out;
  const size_t slots = (size_t)D.N * K;
  const int nb = irls_blocks((int)slots);
  auto dmalloc = [&](DeviceRegion& a, size_t bytes) { return a.reserve(ctx, bytes, "cvo_debug_irls_normal", nullptr); };
  int rc;
  if ((rc = dmalloc(d_ent, sizeof(IrlsEntry) * slots)) != CVO_OK || (rc = dmalloc(d_edges, sizeof(IrlsEdge))) != CVO_OK ||
      (rc = dmalloc(d_poses, sizeof(double) * 24)) != CVO_OK ||
      (rc = dmalloc(d_part, sizeof(double) * IRLS_W * (size_t)std::max(nb, 1))) != CVO_OK ||
      (rc = dmalloc(d_out, sizeof(double) * IRLS_W)) != CVO_OK)
    return rc;
  rc = irls_gather(ctx, D.N, K, (IrlsEntry*)d_ent.p);
  if (rc != CVO_OK) return rc;
  std::vector<IrlsEdge> tab;
  (void)irls_table_add(tab, 0, frame1, frame2, 0, 1, (const IrlsEntry*)d_ent.p, (int)slots);
  HIP_TRY(ctx, hipMemcpyAsync(d_edges.p, tab.data(), sizeof(IrlsEdge), hipMemcpyHostToDevice, ctx->stream));
  IrlsDevice dv;
  dv.edges = (IrlsEdge*)d_edges.p;
  dv.poses = (double*)d_poses.p;
  dv.part = (double*)d_part.p;
  dv.out = (double*)d_out.p;
  dv.n_edges = 1;
  dv.n_blocks = nb;
  std::vector<double> X(pose1, pose1 + 12), o;
  X.insert(X.end(), pose2, pose2 + 12);
  rc = irls_eval(ctx, dv, X, true, o);
  if (rc != CVO_OK) return rc;
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
  // ---- the launch table, by the driver's builder ----
  DeviceRegion d_ent, d_edges, d_poses, d_part, d_out;
  auto dmalloc = [&](DeviceRegion& a, size_t bytes) { return a.reserve(ctx, bytes, "cvo_debug_irls_eval", nullptr); };
  int rc;
  if ((rc = dmalloc(d_ent, std::max<size_t>(sizeof(IrlsEntry) * h_ent.size(), 256))) != CVO_OK) return rc;
  std::vector<IrlsEdge> tab;
  int nb = 0;
  for (int k = 0; k < n_edges; k++) {
    const int a = edge_frames[2 * k], b = edge_frames[2 * k + 1];
    nb = irls_table_add(tab, nb, clouds[a], clouds[b], a, b, (const IrlsEntry*)d_ent.p + ((size_t)slot_off[k] - first),
                        slot_off[k + 1] - slot_off[k]);
  }
  if ((rc = dmalloc(d_edges, sizeof(IrlsEdge) * tab.size())) != CVO_OK ||
      (rc = dmalloc(d_poses, sizeof(double) * 12 * (size_t)n_frames)) != CVO_OK ||
      (rc = dmalloc(d_part, sizeof(double) * IRLS_W * (size_t)std::max(nb, 1))) != CVO_OK ||
      (rc = dmalloc(d_out, sizeof(double) * IRLS_W * tab.size())) != CVO_OK)
    return rc;
  if (!h_ent.empty())
    HIP_TRY(ctx, hipMemcpyAsync(d_ent.p, h_ent.data(), sizeof(IrlsEntry) * h_ent.size(), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(d_edges.p, tab.data(), sizeof(IrlsEdge) * tab.size(), hipMemcpyHostToDevice, ctx->stream));
  IrlsDevice dv;
  dv.edges = (IrlsEdge*)d_edges.p;
  dv.poses = (double*)d_poses.p;
  dv.part = (double*)d_part.p;
  dv.out = (double*)d_out.p;
  dv.n_edges = n_edges;
  dv.n_blocks = nb;
  std::vector<double> X(poses, poses + 12 * (size_t)n_frames), o;
  rc = irls_eval(ctx, dv, X, normal != 0, o);
  if (rc != CVO_OK) return rc;
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
  if (rc != CVO_OK) return rc;
  rc = irls_gather(ctx, N, K, (IrlsEntry*)d_ent.p);
  if (rc != CVO_OK) return rc;
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
