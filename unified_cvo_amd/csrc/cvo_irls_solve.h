// cvo_irls_solve.h -- the trust-region solve of multi-frame align, without a device: the Levenberg-Marquardt loop that
// stands in for ceres::Solve under IRLS.cpp:164-176's options, on the dense normal equations of the free frames.  The
// per-edge records (cost | g[12] | upper(H)[78]) come from two callbacks, so the same loop runs over the device
// reductions (cvo_irls.hip) and over plain host loops (host/cvo_irls_solve_check.cpp, tests/test_irls_solve_cpu.py);
// tests/np_multiframe.py's solve() is its float64 restatement, name for name.  DESIGN.md section 4 lists the constants.
// Plain C++17, standard headers only.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <utility>
#include <vector>

namespace cvo_irls {

// Per edge: cost, g[12], the upper triangle of the 12 x 12 H row by row [78].  THE definition: k_irls_eval /
// k_irls_finish (cvo_k_irls.h) write this record, assemble() reads it.
constexpr int IRLS_W = 91;

// Ceres Solver::Options defaults upstream does not override (IRLS.cpp:164-176 sets only the tolerances and the cap)
constexpr double INITIAL_TRUST_REGION_RADIUS = 1e4;  // initial_trust_region_radius
constexpr double MAX_TRUST_REGION_RADIUS = 1e16;     // max_trust_region_radius
constexpr double MIN_TRUST_REGION_RADIUS = 1e-32;    // min_trust_region_radius
constexpr double MIN_RELATIVE_DECREASE = 1e-3;       // min_relative_decrease
constexpr double MIN_LM_DIAGONAL = 1e-6;             // min_lm_diagonal
constexpr double MAX_LM_DIAGONAL = 1e32;             // max_lm_diagonal
// max_num_consecutive_invalid_steps: Ceres' TrustRegionMinimizer::HandleInvalidStep fails once
// ++num_consecutive_invalid_steps_ >= max_num_consecutive_invalid_steps, i.e. on the 5th in a row
constexpr int MAX_CONSECUTIVE_INVALID_STEPS = 5;
// set by upstream (IRLS.cpp:164-166)
constexpr double FUNCTION_TOLERANCE = 1e-5;   // function_tolerance
constexpr double GRADIENT_TOLERANCE = 1e-5;   // gradient_tolerance
constexpr double PARAMETER_TOLERANCE = 1e-5;  // parameter_tolerance
constexpr double SO3_TOLERANCE = (double)1e-6f;  // LieGroup.cpp:9, a float compared with a double

// Why a solve ended: the values of cvo_multiframe_trace_t::termination (include/cvo_hip.h), 0 to 6 as np_multiframe.TERM_*
// numbers them.  0 = no solve (ell decayed or the loop ended), 1 = function tolerance, 2 = gradient tolerance, 3 = parameter
// tolerance, 4 = trust-region radius below its minimum, 5 = iteration cap, 6 = too many invalid steps in a row.
enum Termination : int { TERM_NONE, TERM_FUNCTION, TERM_GRADIENT, TERM_PARAMETER, TERM_RADIUS, TERM_ITERATIONS, TERM_INVALID };
static_assert(TERM_NONE == 0 && TERM_INVALID == 6, "cvo_multiframe_trace_t::termination");

// Exp_SE3(delta, is_wu = false) (LieGroup.cpp:169-192): u = delta[0..2] (translation), w = delta[3..5] (rotation);
// Exp_SO3 / LeftJacobian_SO3 (LieGroup.cpp:28-55) with TOLERANCE = 1e-6f.  X: 3x4 row-major.
inline void irls_exp_se3(const double d[6], double X[12]) {
  const double w[3] = {d[3], d[4], d[5]};
  const double A[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double A2[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) A2[3 * i + j] = A[3 * i] * A[j] + A[3 * i + 1] * A[3 + j] + A[3 * i + 2] * A[6 + j];
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double R[9], V[9];
  for (int i = 0; i < 9; i++) R[i] = V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  if (!(th < SO3_TOLERANCE)) {
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
inline void irls_plus(const double T[12], const double d[6], double out[12]) {
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
inline bool irls_cholesky_solve(std::vector<double>& M, int n, std::vector<double>& b) {
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

// One solve's problem: the frame -> index-among-the-free-frames map (-1: held) and the active edges' frame pairs, in the
// order of the records the callbacks fill
struct Problem {
  std::vector<int> free_index;
  std::vector<std::pair<int, int>> edges;
  int frames() const { return (int)free_index.size(); }
  int unknowns() const { return 6 * (int)std::count_if(free_index.begin(), free_index.end(), [](int i) { return i >= 0; }); }
};

// The normal equations of the free frames at one set of poses: cost, g (m) and H (m x m row-major)
struct Normal {
  double cost = 0;
  std::vector<double> g, H;
};

// ... from the edges' records `o` (IRLS_W doubles each), edges in table order
inline void assemble(const Problem& pb, const std::vector<double>& o, Normal& nq) {
  const int m = pb.unknowns();
  nq.H.assign((size_t)m * m, 0.0);
  nq.g.assign(m, 0.0);
  nq.cost = 0;
  for (size_t t = 0; t < pb.edges.size(); t++) {
    const double* v = &o[t * IRLS_W];
    nq.cost += v[0];
    const int fr[2] = {pb.free_index[pb.edges[t].first], pb.free_index[pb.edges[t].second]};
    auto gi = [&](int q) { return fr[q / 6] < 0 ? -1 : 6 * fr[q / 6] + q % 6; };
    for (int q = 0; q < 12; q++)
      if (gi(q) >= 0) nq.g[gi(q)] += v[1 + q];
    int h = 13;
    for (int q = 0; q < 12; q++)
      for (int s = q; s < 12; s++, h++) {
        const int i = gi(q), j = gi(s);
        if (i < 0 || j < 0) continue;
        nq.H[(size_t)i * m + j] += v[h];
        if (s != q) nq.H[(size_t)j * m + i] += v[h];
      }
  }
}

// |Y| over the free frames' poses
inline double free_norm(const Problem& pb, const std::vector<double>& Y) {
  double s = 0;
  for (int f = 0; f < pb.frames(); f++)
    if (pb.free_index[f] >= 0)
      for (int q = 0; q < 12; q++) s += Y[12 * (size_t)f + q] * Y[12 * (size_t)f + q];
  return std::sqrt(s);
}

// Z = Y with every free frame moved by Plus(Y_f, sign * d_f)
inline void plus_all(const Problem& pb, const std::vector<double>& Y, const std::vector<double>& d, double sign, std::vector<double>& Z) {
  Z = Y;
  for (int f = 0; f < pb.frames(); f++) {
    if (pb.free_index[f] < 0) continue;
    double dd[6];
    for (int q = 0; q < 6; q++) dd[q] = sign * d[6 * pb.free_index[f] + q];
    irls_plus(&Y[12 * (size_t)f], dd, &Z[12 * (size_t)f]);
  }
}

// gradient_tolerance: |x - Plus(x, -g)|_inf <= 1e-5
inline bool gradient_small(const Problem& pb, const std::vector<double>& X, const std::vector<double>& g) {
  std::vector<double> Z;
  plus_all(pb, X, g, -1.0, Z);
  double mx = 0;
  for (int f = 0; f < pb.frames(); f++)
    if (pb.free_index[f] >= 0)
      for (int q = 0; q < 12; q++) mx = std::max(mx, std::fabs(X[12 * (size_t)f + q] - Z[12 * (size_t)f + q]));
  return mx <= GRADIENT_TOLERANCE;
}

// One Levenberg-Marquardt step at radius mu: (H + diag(D) / mu) dlt = -g with D_ii = clamp(s_i^2 H_ii, min_lm_diagonal,
// max_lm_diagonal) / s_i^2 (s: the Jacobi scaling), and the model cost change -(g^T d + 1/2 d^T H d).  False: the step is
// invalid (the system is not positive definite, or the model does not decrease).
inline bool lm_step(const std::vector<double>& H, const std::vector<double>& g, const std::vector<double>& sc, double mu,
                    std::vector<double>& dlt, double* model) {
  const int m = (int)g.size();
  std::vector<double> Mx = H;
  for (int i = 0; i < m; i++) {
    const double s2 = sc[i] * sc[i];
    const double Dii = std::min(std::max(s2 * H[(size_t)i * m + i], MIN_LM_DIAGONAL), MAX_LM_DIAGONAL) / s2;
    Mx[(size_t)i * m + i] += Dii / mu;
  }
  dlt.assign(m, 0.0);
  for (int i = 0; i < m; i++) dlt[i] = -g[i];
  if (!irls_cholesky_solve(Mx, m, dlt)) return false;
  double gd = 0, dHd = 0;
  for (int i = 0; i < m; i++) {
    gd += g[i] * dlt[i];
    double hd = 0;
    for (int j = 0; j < m; j++) hd += H[(size_t)i * m + j] * dlt[j];
    dHd += dlt[i] * hd;
  }
  *model = -(gd + 0.5 * dHd);
  return std::isfinite(*model) && *model > 0;
}

// Fills the edges' records at the poses X (12 doubles per frame): IRLS_W doubles per edge (normal) or one, the cost.
// Returns the project's status; anything but 0 (CVO_OK) ends the solve.
using Eval = std::function<int(const std::vector<double>& X, std::vector<double>& out)>;

struct Result {
  int steps = 0, accepted = 0;
  Termination termination = TERM_NONE;
  double cost_initial = 0, cost_final = 0;
};

// One trust-region solve from the poses X, at most max_iterations steps (max_num_iterations: every step counts).  X ends
// as the last accepted step's poses; when a callback fails its status is returned and X and *res stay as they were.
inline int solve(const Problem& pb, std::vector<double>& X, int max_iterations, const Eval& normal, const Eval& cost, Result* res) {
  const int m = pb.unknowns();
  std::vector<double> Y = X, Yc, out, dlt;
  Normal nq;
  Result r;
  auto done = [&](Termination why) {
    r.termination = why;
    X = Y;
    *res = r;
    return 0;
  };
  if (const int rc = normal(Y, out)) return rc;
  assemble(pb, out, nq);
  r.cost_initial = r.cost_final = nq.cost;
  std::vector<double> sc(m);  // Jacobi scaling from the first Jacobian: s_i = 1 / (1 + |J_i|)
  for (int i = 0; i < m; i++) sc[i] = 1.0 / (1.0 + std::sqrt(nq.H[(size_t)i * m + i]));
  double mu = INITIAL_TRUST_REGION_RADIUS;
  double decrease = 2.0;  // LevenbergMarquardtStrategy's radius decrease factor, reset on success
  int invalid = 0;
  if (gradient_small(pb, Y, nq.g)) return done(TERM_GRADIENT);
  for (;;) {
    if (r.steps >= max_iterations) return done(TERM_ITERATIONS);
    r.steps++;
    double model = 0, cost_new = NAN;
    bool valid = lm_step(nq.H, nq.g, sc, mu, dlt, &model);
    if (valid) {
      double dn = 0;
      for (int i = 0; i < m; i++) dn += dlt[i] * dlt[i];
      if (std::sqrt(dn) <= PARAMETER_TOLERANCE * (free_norm(pb, Y) + PARAMETER_TOLERANCE)) return done(TERM_PARAMETER);
      plus_all(pb, Y, dlt, 1.0, Yc);
      if (const int rc = cost(Yc, out)) return rc;
      cost_new = 0;
      for (size_t t = 0; t < pb.edges.size(); t++) cost_new += out[t];
      valid = std::isfinite(cost_new);
    }
    if (!valid) {
      if (++invalid >= MAX_CONSECUTIVE_INVALID_STEPS) return done(TERM_INVALID);
    } else {
      invalid = 0;
      const double rho = (nq.cost - cost_new) / model;
      if (rho > MIN_RELATIVE_DECREASE) {
        Y = Yc;
        const double t = 2.0 * rho - 1.0;
        mu = std::min(MAX_TRUST_REGION_RADIUS, mu / std::max(1.0 / 3.0, 1.0 - t * t * t));
        decrease = 2.0;
        r.accepted++;
        const double cost_old = nq.cost;
        if (const int rc = normal(Y, out)) return rc;
        assemble(pb, out, nq);
        r.cost_final = nq.cost;
        if (std::fabs(cost_old - cost_new) / cost_old <= FUNCTION_TOLERANCE) return done(TERM_FUNCTION);
        if (gradient_small(pb, Y, nq.g)) return done(TERM_GRADIENT);
        continue;
      }
    }
    mu /= decrease;  // rejected (or invalid) step
    decrease *= 2.0;
    if (mu < MIN_TRUST_REGION_RADIUS) return done(TERM_RADIUS);
  }
}

}  // namespace cvo_irls
