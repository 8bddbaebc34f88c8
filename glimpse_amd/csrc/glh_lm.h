// glh_lm.h -- the small dense pieces of the damped Gauss-Newton (Levenberg-Marquardt) fit that glh_calib.hip runs once
// per row set (k_calib_fit): the forward-difference step, the active bounds, the damped normal equations and their
// p x p solve, the clamp of a step into the bounds and the damping rule.  Everything is `__host__ __device__` and free of
// device intrinsics, so that tests/hostcheck/ransac_hostcheck.cpp drives the very same code on the CPU against a plain
// Gaussian elimination.  One thread of the workgroup runs these (p <= 18: a few thousand operations).
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

}  // namespace glh
