// glh_lm.h -- the damped Gauss-Newton (Levenberg-Marquardt) fit that glh_calib.hip runs once per row set (team_fit, behind
// glh_calib_fit_sets and glh_calib_ransac_groups), without the sums over the rows: its small dense pieces -- the
// forward-difference step, the active bounds, the damped normal equations and their p x p solve, the clamp of a step
// into the bounds, the damping rule -- and the state machine that decides with them what to try, what to accept and when
// to stop (LmState; lm_begin, lm_first, lm_propose, lm_judge, lm_finish).  Everything is `__host__ __device__` and free of device
// intrinsics, so that tests/hostcheck/ransac_hostcheck.cpp drives the very same code on the CPU, the pieces against a
// plain Gaussian elimination and the whole loop on small residuals of its own.  On the device lane 0 of the team runs
// these (p <= 18: a few thousand operations); the team evaluates the sums in between.
//
// The fit works in scaled variables y = x / scale (scipy.optimize.least_squares' x_scale): J holds d r / d y, A = J^T J
// is kept as its upper triangle, row by row (lm_tri), g = J^T r.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GLH_LM_HD __host__ __device__ inline
#else
#define GLH_LM_HD inline
#endif

namespace glh {

constexpr int LM_MAX_P = 18;                     // the camera vector's 20 entries without imgsz
constexpr int LM_MAX_TRI = LM_MAX_P * (LM_MAX_P + 1) / 2;
constexpr int LM_MAX_REJECT = 16;                // rejected steps in a row before the fit gives up (status LM_CAP)
constexpr double LM_LAMBDA_START = 1e-3;         // Marquardt's start
constexpr double LM_LAMBDA_MIN = 1e-12, LM_LAMBDA_MAX = 1e12;

// status of a fitted set: > 0 converged, by scipy.optimize.least_squares' numbering; <= 0 failed
enum : int32_t {
  LM_RUNNING = 100,  // (the state of a fit that has not ended: never a status)
  LM_GTOL = 1,       // max |g| of the free variables below gtol
  LM_FTOL = 2,       // an accepted step reduced the cost by less than ftol * cost
  LM_XTOL = 3,       // a step shorter than xtol * (xtol + |y|), or one that the bounds cut to nothing
  LM_CAP = 0,        // the evaluation cap or LM_MAX_REJECT was reached first
  LM_FEW_ROWS = -1,  // fewer residuals (two per row whose prediction is a number) than parameters
  LM_NOT_FINITE = -2,
  LM_SINGULAR = -3   // a parameter that no residual depends on, or a pivot that is not a positive number
};

// index of A[i][j], i <= j < p, in the packed upper triangle
GLH_LM_HD int lm_tri(int p, int i, int j) { return i * p - (i * (i - 1)) / 2 + (j - i); }

// scipy.optimize's 2-point step at x inside [lb, ub] (approx_derivative, relative step sqrt(eps)): sqrt(eps) *
// (+1 if x >= 0 else -1) * max(1, |x|), turned round where x + h leaves the bounds and x - h does not, shortened to the
// wider side where neither fits.
GLH_LM_HD double lm_fd_step(double x, double lb, double ub) {
  double h = 1.4901161193847656e-08 * (x >= 0.0 ? 1.0 : -1.0) * fmax(1.0, fabs(x));
  const double lower = x - lb, upper = ub - x;
  if (x + h < lb || x + h > ub) {
    if (fabs(h) <= fmax(lower, upper))
      h = -h;
    else
      h = upper >= lower ? upper : -lower;
  }
  return h;
}

// A variable on a bound whose descent direction (-g) points out of the box takes no part in the step.
GLH_LM_HD bool lm_frozen(double x, double lb, double ub, double g) { return (x <= lb && g > 0.0) || (x >= ub && g < 0.0); }

// M = A + lambda diag(A) (row-major p x p, both triangles), b = -g; a frozen variable's row and column are the
// identity's and its b is 0, so its step is exactly 0.
GLH_LM_HD void lm_system(int p, const double* tri, const double* g, double lambda, uint32_t frozen, double* M, double* b) {
  for (int i = 0; i < p; ++i) {
    const bool fi = (frozen >> i) & 1u;
    for (int j = i; j < p; ++j) {
      const bool fj = (frozen >> j) & 1u;
      double v = tri[lm_tri(p, i, j)];
      if (i == j) v = fi ? 1.0 : v + lambda * v;
      else if (fi || fj) v = 0.0;
      M[i * p + j] = M[j * p + i] = v;
    }
    b[i] = fi ? 0.0 : -g[i];
  }
}

// Solves M y = b for a symmetric positive definite M by Cholesky (M = L L^T, L left in the lower triangle), y left in b.
// false: a pivot is not a positive finite number (M is singular or indefinite to rounding, or holds a NaN).
GLH_LM_HD bool lm_solve(int p, double* M, double* b) {
  for (int j = 0; j < p; ++j) {
    double d = M[j * p + j];
    for (int k = 0; k < j; ++k) d -= M[j * p + k] * M[j * p + k];
    if (!(d > 0.0) || !(d < INFINITY)) return false;
    d = sqrt(d);
    M[j * p + j] = d;
    for (int i = j + 1; i < p; ++i) {
      double s = M[i * p + j];
      for (int k = 0; k < j; ++k) s -= M[i * p + k] * M[j * p + k];
      M[i * p + j] = s / d;
    }
  }
  for (int i = 0; i < p; ++i) {  // L z = b
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= M[i * p + k] * b[k];
    b[i] = s / M[i * p + i];
  }
  for (int i = p - 1; i >= 0; --i) {  // L^T y = z
    double s = b[i];
    for (int k = i + 1; k < p; ++k) s -= M[k * p + i] * b[k];
    b[i] = s / M[i * p + i];
  }
  for (int i = 0; i < p; ++i)
    if (!(fabs(b[i]) < INFINITY)) return false;
  return true;
}

// xt = x + scale * y cut into [lb, ub]; y is overwritten with the scaled step actually taken, (xt - x) / scale.
// Returns the squared length of that step (0: the bounds left nothing of it).
GLH_LM_HD double lm_clamp(int p, const double* x, const double* scale, const double* lb, const double* ub, double* y,
                          double* xt) {
  double len2 = 0.0;
  for (int i = 0; i < p; ++i) {
    double t = x[i] + scale[i] * y[i];
    if (t < lb[i]) t = lb[i];
    if (t > ub[i]) t = ub[i];
    if (t != x[i] + scale[i] * y[i]) y[i] = (t - x[i]) / scale[i];
    xt[i] = t;
    len2 += y[i] * y[i];
  }
  return len2;
}

// The damping rule: a step that lowered the cost divides lambda by 10, one that did not multiplies it by 10, inside
// [LM_LAMBDA_MIN, LM_LAMBDA_MAX].
GLH_LM_HD double lm_damping(double lambda, bool accepted) {
  lambda = accepted ? lambda * 0.1 : lambda * 10.0;
  return lambda < LM_LAMBDA_MIN ? LM_LAMBDA_MIN : (lambda > LM_LAMBDA_MAX ? LM_LAMBDA_MAX : lambda);
}

// The fit of one row set between two evaluations.  An EVALUATION at a point is the packed sums over the set's rows, in
// this order: A's triangle (lm_tri), g, sum r r, the rows that count (whose prediction is a number), sum |r| over them,
// and the set's members.
template <int MAXP>
struct LmState {
  double tri[MAXP * (MAXP + 1) / 2], g[MAXP];  // A and g at x
  double x[MAXP], xt[MAXP], dx[MAXP], y[MAXP];  // the point, the trial point, the evaluation's steps, the scaled step
  double M[MAXP * MAXP], b[MAXP];
  double cost, lambda, err_sum, count, members, len2;
  int32_t state, rejects;  // LM_RUNNING or the status; rejected steps in a row
};

GLH_LM_HD int lm_sums(int p) { return p * (p + 1) / 2 + p + 4; }

// The evaluation `sums` becomes the state at x.
template <int MAXP>
GLH_LM_HD void lm_keep(LmState<MAXP>& s, int p, const double* sums) {
  const int nT = p * (p + 1) / 2;
  for (int e = 0; e < nT; ++e) s.tri[e] = sums[e];
  for (int i = 0; i < p; ++i) s.g[i] = sums[nT + i];
  s.cost = 0.5 * sums[nT + p];
  s.count = sums[nT + p + 1];
  s.err_sum = sums[nT + p + 2];
  s.members = sums[nT + p + 3];
}

// The fit starts at x0: s.x, to be evaluated next.
template <int MAXP>
GLH_LM_HD void lm_begin(LmState<MAXP>& s, int p, const double* x0) {
  for (int i = 0; i < p; ++i) s.x[i] = x0[i];
  s.lambda = LM_LAMBDA_START;
  s.state = LM_RUNNING;
  s.rejects = 0;
}

// `sums`, the evaluation at the start; the fit ends there when the set has fewer residuals than parameters or a cost that
// is not finite.
template <int MAXP>
GLH_LM_HD void lm_first(LmState<MAXP>& s, int p, const double* sums) {
  lm_keep(s, p, sums);
  if (2.0 * s.count < (double)p)
    s.state = LM_FEW_ROWS;
  else if (!(s.cost < INFINITY))
    s.state = LM_NOT_FINITE;
}

// One trial step from x: s.xt, to be evaluated next while the state is still LM_RUNNING.
template <int MAXP>
GLH_LM_HD void lm_propose(LmState<MAXP>& s, int p, const double* lb, const double* ub, const double* scale, double gtol) {
  uint32_t frozen = 0;
  double gmax = 0.0;
  for (int i = 0; i < p; ++i) {
    if (lm_frozen(s.x[i], lb[i], ub[i], s.g[i]))
      frozen |= 1u << i;
    else
      gmax = fmax(gmax, fabs(s.g[i]));
  }
  if (!(gmax >= gtol)) {
    s.state = gmax == gmax ? LM_GTOL : LM_NOT_FINITE;
  } else {
    lm_system(p, s.tri, s.g, s.lambda, frozen, s.M, s.b);
    if (!lm_solve(p, s.M, s.b)) {
      s.state = LM_SINGULAR;
    } else {
      for (int i = 0; i < p; ++i) s.y[i] = s.b[i];
      s.len2 = lm_clamp(p, s.x, scale, lb, ub, s.y, s.xt);
      if (s.len2 == 0.0) s.state = LM_XTOL;
    }
  }
}

// `sums`, the evaluation at s.xt, is accepted or rejected; the fit ends on ftol, xtol or LM_MAX_REJECT.
template <int MAXP>
GLH_LM_HD void lm_judge(LmState<MAXP>& s, int p, const double* scale, const double* sums, double ftol, double xtol) {
  const int nT = p * (p + 1) / 2;
  const double count = sums[nT + p + 1], cost = 0.5 * sums[nT + p];
  double norm2 = 0.0;
  for (int i = 0; i < p; ++i) norm2 += (s.x[i] / scale[i]) * (s.x[i] / scale[i]);
  const bool is_short = sqrt(s.len2) < xtol * (xtol + sqrt(norm2));
  // (a step that lowers the cost by losing rows -- points it pushes behind the camera -- is no improvement)
  const bool accepted = count >= s.count && cost < s.cost;
  s.lambda = lm_damping(s.lambda, accepted);
  if (accepted) {
    const double before = s.cost;
    for (int i = 0; i < p; ++i) s.x[i] = s.xt[i];
    lm_keep(s, p, sums);
    s.rejects = 0;
    if (before - s.cost < ftol * before)
      s.state = LM_FTOL;
    else if (is_short)
      s.state = LM_XTOL;
  } else if (is_short) {
    s.state = LM_XTOL;
  } else if (++s.rejects >= LM_MAX_REJECT) {
    s.state = LM_CAP;
  }
}

// The status of the fit that ended at s.x (one still running met the evaluation cap) and, where asked for, np.mean of |r|
// over the set's own rows: NaN as soon as one of them has no prediction, or when the fit failed.
template <int MAXP>
GLH_LM_HD int32_t lm_finish(const LmState<MAXP>& s, double* mean_error) {
  const int32_t status = s.state == LM_RUNNING ? (int32_t)LM_CAP : s.state;
  if (mean_error) *mean_error = (status > 0 && s.count == s.members) ? s.err_sum / s.count : NAN;
  return status;
}

}  // namespace glh
