// The per-axis host arithmetic of glimpse_amd/csrc/glh_regrid.hip (glh_regrid_host.h), compiled for the CPU so that
// tests/test_regrid.py can compare it with tests/regrid_restatement.py bit for bit.  Test-only.
#include "../../glimpse_amd/csrc/glh_regrid_host.h"

extern "C" {

// t [n + k + 1]
void rg_knots(const double* x, int n, double lo, double hi, int k, double* t) {
  std::vector<double> v;
  glh::regrid_knots(x, n, lo, hi, k, v);
  for (size_t i = 0; i < v.size(); ++i) t[i] = v[i];
}

// the knot interval; h [6]
int rg_basis(const double* t, int n, int k, double x, double* h) { return glh::regrid_basis(t, n, k, x, h); }

// lu [n][2 k + 1]; 1 when factored
int rg_factor(const double* x, int n, const double* t, int k, double* lu) {
  std::vector<double> v;
  if (!glh::regrid_factor(x, n, t, k, v)) return 0;
  for (size_t i = 0; i < v.size(); ++i) lu[i] = v[i];
  return 1;
}
}
