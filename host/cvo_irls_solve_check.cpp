// The multi-frame trust-region solve (unified_cvo_amd/csrc/cvo_irls_solve.h) without a device: host compiler only.
//   cvo_irls_solve_check problem.txt [--nan-cost] [--double-cost] [--synthetic-normal] [--fail-normal] [--fail-cost]
// problem.txt (numbers as strtod reads them, hex floats included):
//   frames F            then F lines   held t0 .. t11            (held: 1 = constant; the pose, 3x4 row-major)
//   cap N                              the step cap (max_num_iterations)
//   edges E             then per edge  f1 f2 n  and n lines  p1x p1y p1z p2x p2y p2z w
// Per edge the program evaluates (cost | g[12] | upper(H)[78]) with plain double loops in the arithmetic of
// cvo_k_irls.h's comment block (upstream's Jacobian, without the factor 2 w), the terms in file order, runs
// cvo_irls::solve and prints status, steps, accepted, termination, both costs and the poses, doubles as %a
// (tests/test_irls_solve_cpu.py compares them with tests/np_multiframe.py's solve).  The switches inject what no finite
// cloud reaches: a step cost that is NaN; a step cost that is always twice the current cost; a normal callback that
// returns cost = 1, every component of g = 1e24 and H = 0 per edge; a callback that fails with status 7.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cvo_irls_solve.h"

struct Term {
  double p1[3], p2[3], w;
};
struct Edge {
  int f1, f2;
  std::vector<Term> terms;
};

// One edge's record (normal: IRLS_W doubles, else the cost alone) at the poses T1, T2
static void edge_eval(const Edge& E, const double* T1, const double* T2, bool normal, double* acc) {
  for (int q = 0; q < (normal ? cvo_irls::IRLS_W : 1); q++) acc[q] = 0.0;
  for (const Term& t : E.terms) {
    double e[3];
    for (int r = 0; r < 3; r++) {
      const double q1 = T1[4 * r] * t.p1[0] + T1[4 * r + 1] * t.p1[1] + T1[4 * r + 2] * t.p1[2] + T1[4 * r + 3];
      const double q2 = T2[4 * r] * t.p2[0] + T2[4 * r + 1] * t.p2[1] + T2[4 * r + 2] * t.p2[2] + T2[4 * r + 3];
      e[r] = q1 - q2;
    }
    const double res = t.w * (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    acc[0] += 0.5 * (res * res);
    if (!normal) continue;
    double J[12];
    for (int c = 0; c < 3; c++) {
      J[c] = T1[c] * e[0] + T1[4 + c] * e[1] + T1[8 + c] * e[2];            // a = R1^T e
      J[6 + c] = -(T2[c] * e[0] + T2[4 + c] * e[1] + T2[8 + c] * e[2]);     // -b, b = R2^T e
    }
    J[3] = t.p1[1] * J[2] - t.p1[2] * J[1];  // p1 x a
    J[4] = t.p1[2] * J[0] - t.p1[0] * J[2];
    J[5] = t.p1[0] * J[1] - t.p1[1] * J[0];
    J[9] = t.p2[1] * J[8] - t.p2[2] * J[7];  // p2 x (-b)
    J[10] = t.p2[2] * J[6] - t.p2[0] * J[8];
    J[11] = t.p2[0] * J[7] - t.p2[1] * J[6];
    for (int q = 0; q < 12; q++) acc[1 + q] += J[q] * res;
    int h = 13;
    for (int q = 0; q < 12; q++)
      for (int s = q; s < 12; s++, h++) acc[h] += J[q] * J[s];
  }
}

int main(int argc, char* argv[]) {
  bool nan_cost = false, double_cost = false, synthetic = false, fail_normal = false, fail_cost = false;
  for (int i = 2; i < argc; i++) {
    const struct { const char* name; bool* flag; } sw[] = {{"--nan-cost", &nan_cost}, {"--double-cost", &double_cost},
        {"--synthetic-normal", &synthetic}, {"--fail-normal", &fail_normal}, {"--fail-cost", &fail_cost}};
    bool known = false;
    for (const auto& s : sw)
      if (!std::strcmp(argv[i], s.name)) *s.flag = known = true;
    if (!known) argc = 1;  // (the usage line)
  }
  std::FILE* f = argc >= 2 ? std::fopen(argv[1], "r") : nullptr;
  if (!f) {
    std::fprintf(stderr, "usage: %s problem.txt [--nan-cost] [--double-cost] [--synthetic-normal] [--fail-normal] [--fail-cost]\n", argv[0]);
    return 2;
  }
  int F = 0, E = 0, cap = 0;
  bool ok = std::fscanf(f, " frames %d", &F) == 1 && F >= 0 && F <= 64;
  cvo_irls::Problem pb;
  std::vector<double> X((size_t)(ok ? F : 0) * 12);
  for (int k = 0, nf = 0; ok && k < F; k++) {
    int held = 0;
    ok = std::fscanf(f, "%d", &held) == 1;
    for (int q = 0; ok && q < 12; q++) ok = std::fscanf(f, "%lf", &X[12 * (size_t)k + q]) == 1;
    pb.free_index.push_back(held ? -1 : nf++);
  }
  ok = ok && std::fscanf(f, " cap %d edges %d", &cap, &E) == 2 && E >= 0 && E <= 2048;
  std::vector<Edge> edges(ok ? E : 0);
  for (Edge& e : edges) {
    int n = 0;
    ok = ok && std::fscanf(f, "%d %d %d", &e.f1, &e.f2, &n) == 3 && e.f1 >= 0 && e.f1 < F && e.f2 >= 0 && e.f2 < F && n >= 0;
    for (int i = 0; ok && i < n; i++) {
      Term t;
      ok = std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf", &t.p1[0], &t.p1[1], &t.p1[2], &t.p2[0], &t.p2[1], &t.p2[2], &t.w) == 7;
      e.terms.push_back(t);
    }
    pb.edges.emplace_back(e.f1, e.f2);
  }
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "%s: malformed problem\n", argv[1]);
    return 2;
  }

  std::vector<double> current(edges.size(), 0.0);  // per edge, the cost the last normal evaluation returned
  auto normal = [&](const std::vector<double>& Y, std::vector<double>& out) {
    if (fail_normal) return 7;
    out.assign(edges.size() * cvo_irls::IRLS_W, 0.0);
    for (size_t k = 0; k < edges.size(); k++) {
      double* v = &out[k * cvo_irls::IRLS_W];
      if (synthetic) {
        v[0] = 1.0;
        for (int q = 0; q < 12; q++) v[1 + q] = 1e24;
      } else {
        edge_eval(edges[k], &Y[12 * (size_t)edges[k].f1], &Y[12 * (size_t)edges[k].f2], true, v);
      }
      current[k] = v[0];
    }
    return 0;
  };
  auto cost = [&](const std::vector<double>& Y, std::vector<double>& out) {
    if (fail_cost) return 7;
    out.assign(edges.size(), 0.0);
    for (size_t k = 0; k < edges.size(); k++) {
      if (nan_cost) out[k] = NAN;
      else if (double_cost) out[k] = 2.0 * current[k];
      else edge_eval(edges[k], &Y[12 * (size_t)edges[k].f1], &Y[12 * (size_t)edges[k].f2], false, &out[k]);
    }
    return 0;
  };
  cvo_irls::Result r;
  const int status = cvo_irls::solve(pb, X, cap, normal, cost, &r);
  std::printf("status %d\nsteps %d\naccepted %d\ntermination %d\ncost_initial %a\ncost_final %a\n", status, r.steps,
              r.accepted, (int)r.termination, r.cost_initial, r.cost_final);
  for (int k = 0; k < F; k++) {
    std::printf("pose %d", k);
    for (int q = 0; q < 12; q++) std::printf(" %a", X[12 * (size_t)k + q]);
    std::printf("\n");
  }
  return 0;
}
