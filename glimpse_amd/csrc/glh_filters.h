// glh_filters.h -- what glimpse_hip.hip (the C ABI: glh_stage_max_filter, glh_stage_gaussian_filter,
// glh_stage_fill_crevasses) hands to glh_filters.hip (the kernels and launches of helpers.maximum_filter,
// helpers.gaussian_filter and Raster.fill_crevasses, helpers.py:347-430, raster.py:1266-1291).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

// A maximum window's tile and halo live in LDS: each side of the window is at most this many cells.
constexpr int FL_MAX_WINDOW = 31;
// A Gaussian pass keeps the half of its weight table it reads (radius + 1 float64) in LDS.
constexpr int FL_MAX_RADIUS = 4096;
constexpr int FL_TIMES = 5;  // entries of times_ms (include/glimpse_hip.h)

struct FiltersJob {
  int device;
  const void* a;  // [ny][nx] float64, or float32 when f32
  int f32;
  int nx, ny;
  const uint8_t* mask;  // [ny][nx], 0 = excluded; null: every cell is included
  int fill;
  int do_max;          // the maximum stage runs (window size_y rows x size_x columns, each >= 1)
  int size_y, size_x;
  int max_mode;        // GLH_HP_* boundary mode of the maximum
  int do_gauss;        // the Gaussian stage runs
  const double* w0;    // [2 * r0 + 1] weights along axis 0 (rows), null: the axis is skipped
  int r0;
  const double* w1;    // [2 * r1 + 1] along axis 1 (columns), null: skipped
  int r1;
  int gauss_mode;
  void* out;         // [ny][nx] of a's dtype
  double* times_ms;  // [FL_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int filters_run(const FiltersJob& job);

}  // namespace glh
