// The host form of the bounded L-BFGS (csrc/lbfgs_host.h, unmodified) on analytic objectives, as a program of its own:
// the history wrap (more than 10 pairs), a pair that fails the curvature guard, a line search that fails, and four
// problems in lock step against each alone.  Built with -fsanitize=address,undefined by tests/test_lbfgs_cpu.py, so an
// index past a vector in the history shift or a read of a finished problem's stale state ends the run; exits 0 when
// every check holds.  The bit-level comparison with the restatement is in tests/test_lbfgs_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lbfgs_host.h"

using namespace lc;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

using Objective = double (*)(int D, const double *x, double *g);

static double rosenbrock(int D, const double *x, double *g) {
  double f = 0;
  for (int i = 0; i < D; ++i) g[i] = 0;
  for (int i = 0; i + 1 < D; ++i) {
    const double u = x[i + 1] - x[i] * x[i], v = 1.0 - x[i];
    f += 100.0 * u * u + v * v;
    g[i] += -400.0 * x[i] * u - 2.0 * v;
    g[i + 1] += 200.0 * u;
  }
  return f;
}

// concave around the origin: a step taken there has s . y < 0
static double double_well(int D, const double *x, double *g) {
  double f = 0;
  for (int i = 0; i < D; ++i) {
    f += 0.25 * x[i] * x[i] * x[i] * x[i] - 0.5 * x[i] * x[i];
    g[i] = x[i] * x[i] * x[i] - x[i];
  }
  for (int i = 0; i + 1 < D; ++i) {
    f += 0.1 * x[i] * x[i + 1];
    g[i] += 0.1 * x[i + 1];
    g[i + 1] += 0.1 * x[i];
  }
  return f;
}

// sum_i (i + 1) x_i^2 whose gradient has the wrong sign once the loss is at most 1
static double lying_bowl(int D, const double *x, double *g) {
  double f = 0;
  for (int i = 0; i < D; ++i) f += (i + 1) * x[i] * x[i];
  for (int i = 0; i < D; ++i) g[i] = (f > 1.0 ? 2.0 : -2.0) * (i + 1) * x[i];
  return f;
}

struct Run {
  std::vector<double> x;
  LbfgsResult res;
  int rc = 0, negative_sy = 0;
};

static Run run(Objective fn, int nb, int D, std::vector<double> x, const std::vector<double> &lo, const std::vector<double> &hi,
               int maxiter) {
  Run r;
  std::vector<double> px, pg;  // previous evaluation, to see the pairs the optimiser sees
  BatchEval eval = [&](const std::vector<double> &X, std::vector<double> &F, std::vector<double> &G) -> int {
    if ((int)X.size() != nb * D || (int)F.size() != nb || (int)G.size() != nb * D) return 99;
    for (int b = 0; b < nb; ++b) F[b] = fn(D, &X[(size_t)b * D], &G[(size_t)b * D]);
    if (!px.empty())
      for (int b = 0; b < nb; ++b) {
        double sy = 0;
        for (int i = 0; i < D; ++i) sy += (X[b * D + i] - px[b * D + i]) * (G[b * D + i] - pg[b * D + i]);
        if (sy < 0) ++r.negative_sy;
      }
    px = X;
    pg = G;
    return 0;
  };
  r.rc = batched_lbfgs(nb, D, x, lo, hi, maxiter, eval, r.res);
  r.x = x;
  return r;
}

static void rosen_problems(int D, std::vector<double> &x, std::vector<double> &lo, std::vector<double> &hi) {
  const double inf = std::numeric_limits<double>::infinity();
  x.assign(4 * D, 0.0);
  lo.assign(4 * D, -inf);
  hi.assign(4 * D, inf);
  for (int b = 0; b < 4; ++b)
    for (int i = 0; i < D; ++i) x[b * D + i] = -1.2 + 2.4 * std::fmod(0.37 * (b * D + i) + 0.11, 1.0);
  hi[0] = 0.5;  // the optimum has x_0 = 1: ends active
  x[0] = 0.2;
  lo[1 * D + D - 1] = 1.5;  // the optimum has x_{D-1} = 1: ends active
  x[1 * D + D - 1] = 2.0;
  for (int i = 0; i < D; ++i) {
    lo[3 * D + i] = -2.0;
    hi[3 * D + i] = 2.0;
  }
  x[3 * D] = 3.5;  // a start outside the box
  x[3 * D + D - 1] = -4.0;
}

static void test_wrap_and_bounds() {
  for (int D : {2, 7, 40}) {
    std::vector<double> x, lo, hi;
    rosen_problems(D, x, lo, hi);
    for (int maxiter : {0, 1, 2, 13, 300}) {
      Run r = run(rosenbrock, 4, D, x, lo, hi, maxiter);
      CHECK(r.rc == 0);
      for (int b = 0; b < 4; ++b) {
        CHECK(r.res.iters[b] <= maxiter);
        for (int i = 0; i < D; ++i) CHECK(r.x[b * D + i] >= lo[b * D + i] && r.x[b * D + i] <= hi[b * D + i]);
        std::vector<double> g(D);
        CHECK(rosenbrock(D, &r.x[(size_t)b * D], g.data()) == r.res.f[b]);  // the loss returned is that of the point returned
      }
      if (maxiter == 0) CHECK(r.res.evaluations == 1);
      if (maxiter == 13 && D > 2) CHECK(r.res.iters[0] == 13 || r.res.iters[2] == 13);  // more than 10 pairs stored
      if (maxiter == 300) {
        CHECK(r.x[0] == 0.5 && r.x[1 * D + D - 1] == 1.5);
        for (int i = 0; i < D; ++i) CHECK(std::fabs(r.x[2 * D + i] - 1.0) < 1e-4);
        for (int b = 0; b < 4; ++b) CHECK(r.res.iters[b] > 10 || D == 2);
      }
    }
  }
}

static void test_rejected_pair() {
  const int D = 6;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> x(D), lo(D, -inf), hi(D, inf);
  for (int i = 0; i < D; ++i) x[i] = 0.1 * (1 + 0.1 * i);
  Run r = run(double_well, 1, D, x, lo, hi, 60);
  CHECK(r.rc == 0 && r.negative_sy > 0);
  std::vector<double> g(D);
  CHECK(double_well(D, r.x.data(), g.data()) == r.res.f[0] && r.res.f[0] < -0.1 * D);
  for (int i = 0; i < D; ++i) CHECK(std::fabs(g[i]) < 1e-5);
}

static void test_failed_line_search() {
  const int D = 5;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> x(D), lo(D, -inf), hi(D, inf);
  for (int i = 0; i < D; ++i) x[i] = 1.5 + 1.5 * i / (D - 1);
  Run r = run(lying_bowl, 1, D, x, lo, hi, 60);
  std::vector<double> g(D);
  CHECK(r.rc == 0 && r.res.iters[0] >= 1 && r.res.iters[0] < 60);
  CHECK(lying_bowl(D, r.x.data(), g.data()) == r.res.f[0]);  // the last accepted point, not the last trial
  CHECK(r.res.f[0] <= 1.0 && r.res.f[0] > 0.0);
  CHECK(r.res.evaluations >= 1 + r.res.iters[0] + 25);
}

static void test_lock_step() {
  const int D = 7;
  std::vector<double> x, lo, hi;
  rosen_problems(D, x, lo, hi);
  for (int maxiter : {13, 300}) {
    Run all = run(rosenbrock, 4, D, x, lo, hi, maxiter);
    int worst = 0;
    for (int b = 0; b < 4; ++b) {
      std::vector<double> x1(x.begin() + b * D, x.begin() + (b + 1) * D), l1(lo.begin() + b * D, lo.begin() + (b + 1) * D),
          h1(hi.begin() + b * D, hi.begin() + (b + 1) * D);
      Run one = run(rosenbrock, 1, D, x1, l1, h1, maxiter);
      CHECK(one.rc == 0 && one.res.iters[0] == all.res.iters[b]);
      CHECK(std::memcmp(one.x.data(), &all.x[(size_t)b * D], D * sizeof(double)) == 0);
      CHECK(std::memcmp(&one.res.f[0], &all.res.f[b], sizeof(double)) == 0);
      worst = std::max(worst, one.res.evaluations);
    }
    CHECK(all.res.evaluations == worst);
  }
  // an infinite start beside healthy problems, and a callback that fails
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> xi = x;
  int calls = 0;
  BatchEval eval = [&](const std::vector<double> &X, std::vector<double> &F, std::vector<double> &G) -> int {
    if (++calls == 4) return 41;
    for (int b = 0; b < 4; ++b) F[b] = rosenbrock(D, &X[(size_t)b * D], &G[(size_t)b * D]);
    F[2] = inf;
    return 0;
  };
  LbfgsResult res;
  CHECK(batched_lbfgs(4, D, xi, lo, hi, 300, eval, res) == 41 && calls == 4);
}

int main() {
  test_wrap_and_bounds();
  test_rejected_pair();
  test_failed_line_search();
  test_lock_step();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
