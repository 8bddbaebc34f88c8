// glh_horizon.h -- what glimpse_hip.hip (the C ABI: glh_stage_horizon) hands to glh_horizon.hip (the kernel and the launch
// of Raster.horizon, raster.py:1391-1463).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

constexpr int HZ_TIMES = 3;  // entries of times_ms (include/glimpse_hip.h)

struct HorizonJob {
  int device;
  const void* z;  // [ny][nx] float64, or float32 when f32
  int f32;
  int nx, ny;
  double xlim0, ylim0, d0, d1;
  const double* origins;  // [m][3]
  const int32_t* starts;  // [m][2] (col, row)
  const int32_t* ends;    // [m][n][2] (col, row)
  int m, n;
  int correction;
  double radius, refraction;
  int32_t* cell;     // [m][n][2] (row, col), -1 -1 without a horizon point
  double* dz;        // [m][n]
  double* times_ms;  // [HZ_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int horizon_run(const HorizonJob& job);

}  // namespace glh
