// glh_regrid_host.h -- the per-axis host arithmetic of glh_regrid.hip (declared in glh_regrid.h): FITPACK's interpolating
// knots, de Boor's recurrence, and the banded collocation matrix with its LU factors.  Plain C++ with no HIP in it, so that
// tests/hostcheck/regrid_hostcheck.cpp can compile the very same lines for the CPU and tests/test_regrid.py can compare
// them with tests/regrid_restatement.py bit for bit.  Build with -ffp-contract=off (every expression rounds as written).
#pragma once
#include <cmath>
#include <vector>

#include "glh_regrid.h"

namespace glh {

inline void regrid_knots(const double* x, int n, double lo, double hi, int k, std::vector<double>& t) {
  t.assign((size_t)n + k + 1, 0.0);
  for (int i = 0; i <= k; ++i) t[i] = lo, t[n + i] = hi;
  const int interior = n - k - 1;
  if (k % 2)
    for (int m = 0; m < interior; ++m) t[k + 1 + m] = x[(k + 1) / 2 + m];
  else
    for (int m = 0; m < interior; ++m) t[k + 1 + m] = (x[k / 2 + m] + x[k / 2 + m + 1]) / 2;
}

inline int regrid_basis(const double* t, int n, int k, double x, double* h) {
  const double lo = t[k], hi = t[n];
  if (x < lo) x = lo;
  if (x > hi) x = hi;
  // l = k + the number of interior knots t[k + 1 .. n - 1] that are <= x
  int a = k + 1, b = n;
  while (a < b) {
    const int mid = a + (b - a) / 2;
    if (t[mid] <= x)
      a = mid + 1;
    else
      b = mid;
  }
  const int l = a - 1;
  double hh[RG_MAX_K];
  h[0] = 1.0;
  for (int j = 1; j <= k; ++j) {
    for (int i = 0; i < j; ++i) hh[i] = h[i];
    h[0] = 0.0;
    for (int i = 0; i < j; ++i) {
      const int li = l + i + 1, lj = li - j;
      const double f = hh[i] / (t[li] - t[lj]);
      h[i] = h[i] + f * (t[li] - x);
      h[i + 1] = f * (x - t[lj]);
    }
  }
  return l;
}

inline bool regrid_factor(const double* x, int n, const double* t, int k, std::vector<double>& lu) {
  const int w = 2 * k + 1;
  lu.assign((size_t)n * w, 0.0);
  double h[RG_H];
  for (int i = 0; i < n; ++i) {
    const int l = regrid_basis(t, n, k, x[i], h);
    for (int a = 0; a <= k; ++a) {
      const int d = l - k + a - i + k;
      if (d < 0 || d >= w) {
        if (h[a] != 0.0) return false;
        continue;
      }
      lu[(size_t)i * w + d] = h[a];
    }
  }
  for (int p = 0; p < n; ++p) {
    const double pivot = lu[(size_t)p * w + k];
    if (!(pivot != 0.0) || !std::isfinite(pivot)) return false;
    const int last = p + k < n - 1 ? p + k : n - 1;
    for (int i = p + 1; i <= last; ++i) {
      double* row = &lu[(size_t)i * w];
      const double m = row[p - i + k] / pivot;
      row[p - i + k] = m;
      for (int j = p + 1; j <= last; ++j) row[j - i + k] = row[j - i + k] - m * lu[(size_t)p * w + (j - p + k)];
    }
  }
  return true;
}

}  // namespace glh
