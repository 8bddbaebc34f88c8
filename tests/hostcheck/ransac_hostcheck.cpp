// ransac_hostcheck.cpp -- glimpse_amd/csrc/glh_lm.h, what lane 0 of a team runs in glh_calib.hip's one fit (team_fit),
// driven on the CPU.  The pieces -- the p x p solve, the damped system, the clamp into the bounds, the damping rule and
// the forward-difference step -- against a plain Gaussian elimination with partial pivoting; the whole loop (lm_begin,
// lm_first, lm_propose, lm_judge, lm_finish) to its end on small linear residuals whose sums a CPU function fills: to the
// minimiser by elimination for 1, 3 and 18 parameters, and into every status.  A stand-alone program:
// tests/test_ransac_host.py builds it with -fsanitize=address,undefined and runs it; it prints one line per check and
// exits 1 on the first failure.  Test-only: the product never runs this code on the CPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../glimpse_amd/csrc/glh_lm.h"

using namespace glh;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {  // xorshift64*: the same numbers on every machine
  g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

#define REQUIRE(cond, ...)                  \
  do {                                      \
    if (!(cond)) {                          \
      std::printf("FAILED %s: ", #cond);    \
      std::printf(__VA_ARGS__);             \
      std::printf("\n");                    \
      std::exit(1);                         \
    }                                       \
  } while (0)

// M y = b by Gaussian elimination with partial pivoting; false when a pivot is 0
static bool gauss(int p, std::vector<double> M, std::vector<double> b, std::vector<double>& y) {
  for (int c = 0; c < p; ++c) {
    int piv = c;
    for (int r = c + 1; r < p; ++r)
      if (std::fabs(M[r * p + c]) > std::fabs(M[piv * p + c])) piv = r;
    if (M[piv * p + c] == 0.0) return false;
    for (int k = 0; k < p; ++k) std::swap(M[c * p + k], M[piv * p + k]);
    std::swap(b[c], b[piv]);
    for (int r = c + 1; r < p; ++r) {
      const double f = M[r * p + c] / M[c * p + c];
      for (int k = c; k < p; ++k) M[r * p + k] -= f * M[c * p + k];
      b[r] -= f * b[c];
    }
  }
  y.assign(p, 0.0);
  for (int r = p - 1; r >= 0; --r) {
    double s = b[r];
    for (int k = r + 1; k < p; ++k) s -= M[r * p + k] * y[k];
    y[r] = s / M[r * p + r];
  }
  return true;
}

// J^T J (packed) and J^T r of a random m x p Jacobian
static void normal_equations(int p, int m, std::vector<double>& tri, std::vector<double>& g) {
  std::vector<double> J((size_t)m * p), r(m);
  for (double& v : J) v = 2.0 * uniform() - 1.0;
  for (double& v : r) v = 2.0 * uniform() - 1.0;
  tri.assign((size_t)p * (p + 1) / 2, 0.0);
  g.assign(p, 0.0);
  for (int i = 0; i < p; ++i) {
    for (int j = i; j < p; ++j)
      for (int k = 0; k < m; ++k) tri[lm_tri(p, i, j)] += J[(size_t)k * p + i] * J[(size_t)k * p + j];
    for (int k = 0; k < m; ++k) g[i] += J[(size_t)k * p + i] * r[k];
  }
}

// A small residual for the whole loop: r = A x - b, m residuals taken two to a row as the device takes them, in the box
// [lb, ub] with the scales `scale`.
struct Linear {
  int p, m;
  std::vector<double> A, b, lb, ub, scale;
  Linear(int p_, int m_) : p(p_), m(m_), A((size_t)m_ * p_), b(m_), lb(p_, -INFINITY), ub(p_, INFINITY), scale(p_, 1.0) {
    for (double& v : A) v = 2.0 * uniform() - 1.0;
    for (double& v : b) v = 2.0 * uniform() - 1.0;
  }
  double residual(const double* x, int k) const {
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += A[(size_t)k * p + j] * x[j];
    return s - b[k];
  }
  // the minimiser without bounds: A^T A x = A^T b by Gaussian elimination
  std::vector<double> minimiser() const {
    std::vector<double> M((size_t)p * p, 0.0), c(p, 0.0), x;
    for (int i = 0; i < p; ++i) {
      for (int j = 0; j < p; ++j)
        for (int k = 0; k < m; ++k) M[i * p + j] += A[(size_t)k * p + i] * A[(size_t)k * p + j];
      for (int k = 0; k < m; ++k) c[i] += A[(size_t)k * p + i] * b[k];
    }
    REQUIRE(gauss(p, M, c, x), "normal equations of size %d", p);
    return x;
  }
};

// What team_evaluate leaves in LDS, on the CPU: the evaluation (glh_lm.h: the packed sums) of q at xe, J in scaled
// variables by forward differences, the steps kept in s.dx.
template <int MAXP>
static void evaluate(const Linear& q, const double* xe, LmState<MAXP>& s, double* sums) {
  const int p = q.p, m = q.m, nT = p * (p + 1) / 2;
  std::vector<double> r(m), J((size_t)m * p), xs(xe, xe + p);
  for (int k = 0; k < m; ++k) r[k] = q.residual(xe, k);
  for (int j = 0; j < p; ++j) {
    xs[j] = xe[j] + lm_fd_step(xe[j], q.lb[j], q.ub[j]);
    s.dx[j] = xs[j] - xe[j];
    for (int k = 0; k < m; ++k) J[(size_t)k * p + j] = (q.residual(xs.data(), k) - r[k]) / s.dx[j] * q.scale[j];
    xs[j] = xe[j];
  }
  for (int e = 0; e < lm_sums(p); ++e) sums[e] = 0.0;
  for (int k = 0; k < m; ++k) {
    for (int i = 0; i < p; ++i) {
      for (int j = i; j < p; ++j) sums[lm_tri(p, i, j)] += J[(size_t)k * p + i] * J[(size_t)k * p + j];
      sums[nT + i] += J[(size_t)k * p + i] * r[k];
    }
    sums[nT + p] += r[k] * r[k];
  }
  for (int k = 0; k + 1 < m; k += 2) sums[nT + p + 2] += std::hypot(r[k], r[k + 1]);
  sums[nT + p + 1] = sums[nT + p + 3] = m / 2;  // every row counts and is a member
}

// team_fit on the CPU: glh_lm.h decides, `evaluate` stands for the team.
template <int MAXP>
static int32_t fit(const Linear& q, const std::vector<double>& x0, int max_nfev, std::vector<double>& x, double* mean_error) {
  const double tol = 1e-8;
  const int p = q.p;
  LmState<MAXP> s;
  std::vector<double> sums(lm_sums(p));
  lm_begin(s, p, x0.data());
  evaluate(q, s.x, s, sums.data());
  lm_first(s, p, sums.data());
  for (int it = 0; it < max_nfev; ++it) {
    if (s.state != LM_RUNNING) break;
    lm_propose(s, p, q.lb.data(), q.ub.data(), q.scale.data(), tol);
    if (s.state != LM_RUNNING) break;
    evaluate(q, s.xt, s, sums.data());
    lm_judge(s, p, q.scale.data(), sums.data(), tol, tol);
  }
  x.assign(s.x, s.x + p);
  return lm_finish(s, mean_error);
}

// The largest deviation of the fits of the linear problems from their minimisers by elimination, over the size of the
// minimiser, that whole_loop() allows: ten times what this Gauss-Newton leaves with ftol = xtol = gtol = 1e-8 on these
// inputs (measured, x86-64, g++ -O1: 4.1e-10, 6.95e-09 and 9.21e-09 for p = 1, 3 and 18), as 1e-7.  That is the size
// to expect: a difference quotient over a step of sqrt(eps) carries the residuals' rounding, eps / sqrt(eps) = 1.5e-8
// of their size, and the fit ends at the minimiser under that Jacobian.
static const double LINEAR_TOLERANCE = 1e-7;

static void whole_loop() {
  double worst = 0.0, mean;
  std::vector<double> x;
  for (int p : {1, 3, 18}) {
    const Linear q(p, 2 * p);
    const std::vector<double> want = q.minimiser(), zero(p, 0.0);
    const int32_t status = p <= 3 ? fit<3>(q, zero, 100 * p, x, &mean) : fit<LM_MAX_P>(q, zero, 100 * p, x, &mean);
    REQUIRE(status > 0 && mean == mean, "linear problem of size %d: status %d, mean error %g", p, status, mean);
    double size = 0.0, off = 0.0;
    for (int i = 0; i < p; ++i) size = std::fmax(size, std::fabs(want[i])), off = std::fmax(off, std::fabs(x[i] - want[i]));
    std::printf("lm loop: r = A x - b, p %d, %d rows: status %d, |x - elimination| / |x| = %.3g\n", p, 2 * p, status, off / size);
    worst = std::fmax(worst, off / size);
    // the size of the state's arrays does not enter the arithmetic
    if (p == 3) {
      std::vector<double> y;
      REQUIRE(fit<LM_MAX_P>(q, zero, 100 * p, y, nullptr) == status && y == x, "LmState<3> and LmState<%d> differ", LM_MAX_P);
    }
    // a start at the minimiser has no gradient left (b = A x: the residuals there are rounding, and so is their share
    // in the difference quotients)
    Linear exact = q;
    for (int k = 0; k < q.m; ++k) exact.b[k] = q.residual(want.data(), k) + q.b[k];
    REQUIRE(fit<LM_MAX_P>(exact, want, 100 * p, x, &mean) == LM_GTOL && x == want, "a start at the minimiser, p %d", p);
    // one trial step is not enough; the values are those of the step taken, no mean error without convergence
    REQUIRE(fit<LM_MAX_P>(q, zero, 1, x, &mean) == LM_CAP && x != zero && mean != mean, "max_nfev = 1, p %d", p);
  }
  std::printf("lm loop: largest deviation %.3g\n", worst);
  REQUIRE(worst < LINEAR_TOLERANCE, "against the minimiser by elimination: %g", worst);
  {
    Linear q(3, 6);  // a parameter no residual depends on
    for (int k = 0; k < 6; ++k) q.A[(size_t)k * 3 + 1] = 0.0;
    REQUIRE(fit<3>(q, {0.0, 0.0, 0.0}, 300, x, &mean) == LM_SINGULAR && mean != mean, "a dead parameter was fitted");
    const Linear few(3, 2);  // one row, two residuals, three parameters
    REQUIRE(fit<3>(few, {0.0, 0.0, 0.0}, 300, x, &mean) == LM_FEW_ROWS, "fewer residuals than parameters");
    Linear nan(3, 6);
    nan.b[4] = NAN;
    REQUIRE(fit<3>(nan, {0.0, 0.0, 0.0}, 300, x, &mean) == LM_NOT_FINITE, "a cost that is not a number");
    // a step the bounds cut to nothing: the minimiser -1 lies below the bound 0, the start 1e-170 above it, so the step
    // taken is -1e-170, whose square is 0
    Linear cut(1, 2);
    cut.A = {1.0, 1.0}, cut.b = {-1.0, -1.0}, cut.lb = {0.0};
    REQUIRE(fit<3>(cut, {1e-170}, 100, x, &mean) == LM_XTOL && x[0] == 1e-170, "a step cut to nothing");
    // and from the bound itself the variable is frozen: nothing is left to move
    REQUIRE(fit<3>(cut, {0.0}, 100, x, &mean) == LM_GTOL && x[0] == 0.0, "a start on the bound");
  }
  std::printf("lm loop: gtol, cap, singular, few rows, not finite, xtol\n");
}

int main() {
  whole_loop();
  // the packed triangle is row by row without gaps
  for (int p = 1; p <= LM_MAX_P; ++p) {
    int e = 0;
    for (int i = 0; i < p; ++i)
      for (int j = i; j < p; ++j, ++e) REQUIRE(lm_tri(p, i, j) == e, "p %d (%d, %d)", p, i, j);
    REQUIRE(e == p * (p + 1) / 2, "p %d", p);
  }
  std::printf("lm_tri: sizes 1 .. %d\n", LM_MAX_P);

  // the damped system and its solve against Gaussian elimination, sizes 1 .. 18, with and without frozen variables
  double worst = 0.0;
  for (int p = 1; p <= LM_MAX_P; ++p)
    for (int trial = 0; trial < 20; ++trial) {
      std::vector<double> tri, g, M((size_t)p * p), b(p), y;
      normal_equations(p, 2 * p + 3, tri, g);
      const double lambda = trial % 4 == 0 ? 0.0 : std::pow(10.0, -6.0 + trial % 7);
      const uint32_t frozen = trial % 3 == 2 ? (1u << (trial % p)) | (1u << ((trial * 7) % p)) : 0u;
      lm_system(p, tri.data(), g.data(), lambda, frozen, M.data(), b.data());
      for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) {
          const bool fi = (frozen >> i) & 1u, fj = (frozen >> j) & 1u;
          const double a = tri[lm_tri(p, i < j ? i : j, i < j ? j : i)];
          const double want = i == j ? (fi ? 1.0 : a + lambda * a) : ((fi || fj) ? 0.0 : a);
          REQUIRE(M[i * p + j] == want, "system p %d (%d, %d)", p, i, j);
        }
      std::vector<double> M0 = M, b0 = b;
      REQUIRE(gauss(p, M0, b0, y), "gauss p %d", p);
      REQUIRE(lm_solve(p, M.data(), b.data()), "solve p %d trial %d", p, trial);
      double scale = 0.0;
      for (int i = 0; i < p; ++i) scale = std::fmax(scale, std::fabs(y[i]));
      for (int i = 0; i < p; ++i) {
        if ((frozen >> i) & 1u) REQUIRE(b[i] == 0.0, "frozen variable %d moves by %g", i, b[i]);
        worst = std::fmax(worst, std::fabs(b[i] - y[i]) / scale);
      }
      // the residual of the system, which does not depend on its condition
      for (int i = 0; i < p; ++i) {
        double s = -b0[i], size = std::fabs(b0[i]);
        for (int j = 0; j < p; ++j) s += M0[i * p + j] * b[j], size += std::fabs(M0[i * p + j] * b[j]);
        REQUIRE(std::fabs(s) <= 1e-12 * size, "residual p %d row %d: %g of %g", p, i, s, size);
      }
    }
  REQUIRE(worst < 1e-6, "against Gaussian elimination: %g", worst);
  std::printf("lm_solve: sizes 1 .. %d against Gaussian elimination, largest relative difference %.3g\n", LM_MAX_P, worst);

  // singular: a parameter no residual depends on (a zero row and column), with any damping; a NaN; an indefinite matrix
  for (int p = 1; p <= LM_MAX_P; ++p) {
    std::vector<double> tri, g, M((size_t)p * p), b(p);
    normal_equations(p, 2 * p + 3, tri, g);
    const int dead = p / 2;
    for (int i = 0; i < p; ++i) tri[lm_tri(p, i < dead ? i : dead, i < dead ? dead : i)] = 0.0;
    g[dead] = 0.0;
    lm_system(p, tri.data(), g.data(), 1e-3, 0u, M.data(), b.data());
    REQUIRE(!lm_solve(p, M.data(), b.data()), "a dead parameter solved, p %d", p);
    normal_equations(p, 2 * p + 3, tri, g);
    tri[0] = NAN;
    lm_system(p, tri.data(), g.data(), 1e-3, 0u, M.data(), b.data());
    REQUIRE(!lm_solve(p, M.data(), b.data()), "a NaN solved, p %d", p);
  }
  {
    double M[4] = {1.0, 2.0, 2.0, 1.0}, b[2] = {1.0, 1.0};  // eigenvalues 3 and -1
    REQUIRE(!lm_solve(2, M, b), "an indefinite matrix solved");
    double Z[4] = {1.0, 1.0, 1.0, 1.0}, c[2] = {1.0, 1.0};  // rank 1, no damping
    REQUIRE(!lm_solve(2, Z, c), "a singular matrix solved");
  }
  std::printf("lm_solve: singular, NaN and indefinite systems are refused\n");

  // a step that hits a bound: cut to the bound, y rewritten to the step taken; one the bounds leave nothing of
  {
    const double x[3] = {1.0, -2.0, 5.0}, scale[3] = {0.5, 2.0, 1.0}, lb[3] = {0.0, -3.0, 5.0}, ub[3] = {1.25, INFINITY, 6.0};
    double y[3] = {2.0, -4.0, -1.0}, xt[3];
    const double len2 = lm_clamp(3, x, scale, lb, ub, y, xt);
    REQUIRE(xt[0] == 1.25 && xt[1] == -3.0 && xt[2] == 5.0, "clamped to %g %g %g", xt[0], xt[1], xt[2]);
    REQUIRE(y[0] == 0.5 && y[1] == -0.5 && y[2] == 0.0 && len2 == 0.5, "steps %g %g %g, %g", y[0], y[1], y[2], len2);
    double inside[3] = {0.25, 0.5, 0.5};
    REQUIRE(lm_clamp(3, x, scale, lb, ub, inside, xt) == 0.25 * 0.25 + 0.5 * 0.5 + 0.5 * 0.5, "an inner step was changed");
    REQUIRE(xt[0] == 1.125 && xt[1] == -1.0 && xt[2] == 5.5 && inside[0] == 0.25, "inner step");
    double out[3] = {0.0, 0.0, -3.0};
    REQUIRE(lm_clamp(3, x, scale, lb, ub, out, xt) == 0.0 && xt[2] == 5.0, "a step out of the box was kept");
    REQUIRE(lm_frozen(5.0, 5.0, 6.0, 1.0) && !lm_frozen(5.0, 5.0, 6.0, -1.0) && lm_frozen(6.0, 5.0, 6.0, -1.0) &&
                !lm_frozen(5.5, 5.0, 6.0, 1.0),
            "active bounds");
  }
  std::printf("lm_clamp, lm_frozen: steps into, onto and out of the bounds\n");

  // the damping rule stays inside its range and moves by tens
  {
    double lambda = LM_LAMBDA_START;
    REQUIRE(lm_damping(1e-3, true) == 1e-3 * 0.1 && lm_damping(1e-3, false) == 1e-2, "the rule");
    for (int k = 0; k < 40; ++k) lambda = lm_damping(lambda, true);
    REQUIRE(lambda == LM_LAMBDA_MIN, "floor %g", lambda);
    for (int k = 0; k < 40; ++k) lambda = lm_damping(lambda, false);
    REQUIRE(lambda == LM_LAMBDA_MAX, "ceiling %g", lambda);
  }
  // scipy's forward-difference step: sign, size, turned round at a bound, shortened in a narrow box
  {
    const double h = 1.4901161193847656e-08;
    REQUIRE(lm_fd_step(0.0, -INFINITY, INFINITY) == h && lm_fd_step(-0.5, -INFINITY, INFINITY) == -h, "sign");
    REQUIRE(lm_fd_step(100.0, -INFINITY, INFINITY) == 100.0 * h, "size");
    REQUIRE(lm_fd_step(1.0, 0.0, 1.0) == -h && lm_fd_step(-1.0, -1.0, 0.0) == h, "turned round");
    REQUIRE(lm_fd_step(0.0, -1e-9, 2e-9) == 2e-9 && lm_fd_step(0.0, -2e-9, 1e-9) == -2e-9, "shortened");
  }
  std::printf("lm_damping, lm_fd_step\nok\n");
  return 0;
}
