// glh_regrid.h -- what glimpse_hip.hip (the C ABI: glh_stage_raster_regrid, glh_stage_zoom_linear,
// glh_stage_raster_interpolate) hands to glh_regrid.hip (the host factoring, the kernels and the launches of
// Raster.sample(grid=True), Raster.resize and RasterInterpolant, raster.py:1042-1070, :1178-1187, :1673-1700), and the
// per-axis host arithmetic itself, which is plain C++ and is also what tests/regrid_restatement.py restates.
// Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace glh {

constexpr int RG_TIMES = 4;     // entries of times_ms (include/glimpse_hip.h)
constexpr int RG_MAX_K = 5;     // spline orders 1 .. 5
constexpr int RG_H = RG_MAX_K + 1;  // basis values kept per output coordinate (the first k + 1 are used)

// One raster to be evaluated as a spline on a grid of coordinates.
struct RegridSource {
  const double* z;      // [ny][nx], rows and columns in ascending coordinate order, finite (0 where nan_mask is set)
  const uint8_t* nan;   // [ny][nx] 1 where the cell is NaN, or null; only with kx == ky == 1
  int nx, ny;
  const double* gx;     // [nx] ascending cell centres
  const double* gy;     // [ny]
  double xmin, xmax, ymin, ymax;  // the box: the knots' ends
  int kx, ky;
  int use_zmin;         // samples below zmin become NaN (raster.py:1068)
  double zmin;
  int flip_x, flip_y;   // output column j holds xo[mx - 1 - j] / row i holds yo[my - 1 - i]
};

struct RegridJob {
  int device;
  RegridSource src;
  const double* xo;  // [mx] ascending (non-decreasing)
  const double* yo;  // [my]
  int mx, my;
  double* out;       // [my][mx]
  double* times_ms;  // [RG_TIMES] or null: upload, solve, evaluate, download
};

struct ZoomJob {
  int device;
  const double* a;  // [ny][nx]
  int nx, ny, mx, my;
  double* out;      // [my][mx]
  double* times_ms;
};

struct InterpolateJob {
  int device;
  int nx, ny;               // the first rasters' grid, and the outputs'
  const double* m0;         // [ny][nx]
  const double* m1;         // [ny][nx], or null when m1_src is regridded onto (xo, yo)
  const RegridSource* m1_src;
  const double* s0;         // null: no sigma output
  const double* s1;
  const RegridSource* s1_src;
  const double* xo;         // [nx], [ny] ascending: needed with a source
  const double* yo;
  double scale, scale2, third, ratio;
  double* z;                // [ny][nx]
  double* sigma;            // [ny][nx] or null
  double* times_ms;         // upload, regrid, blend, download
};

// ---- per-axis host arithmetic (exposed for the stand-alone host check) ------------------------------------------------
// FITPACK's interpolating knots of order k on the sites x[n] within [lo, hi]: t [n + k + 1].
void regrid_knots(const double* x, int n, double lo, double hi, int k, std::vector<double>& t);
// The knot interval l (k <= l <= n - 1, t[l] <= x < t[l + 1], the last one closed) of x clamped to the box, and the k + 1
// B-spline values h[0 .. k] of B_{l-k} .. B_l there (de Boor's recurrence as fpbspl runs it).
int regrid_basis(const double* t, int n, int k, double x, double* h);
// The collocation matrix of the sites in band storage lu [n][2 k + 1] (entry (i, j) at [i][j - i + k]), factored in place
// by LU without pivoting: L's multipliers below the diagonal, U on and above.  False if an entry falls outside the band or
// a pivot is 0 (neither happens for sites inside the box).
bool regrid_factor(const double* x, int n, const double* t, int k, std::vector<double>& lu);

// Run the jobs; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int regrid_run(const RegridJob& job);
int zoom_run(const ZoomJob& job);
int interpolate_run(const InterpolateJob& job);

}  // namespace glh
