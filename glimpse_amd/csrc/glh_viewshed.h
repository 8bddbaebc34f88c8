// glh_viewshed.h -- what glimpse_hip.hip (the C ABI: glh_stage_viewshed) hands to glh_viewshed.hip (the kernels, the sort
// and the launches of Raster.viewshed, raster.py:1293-1389).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

// Ring numbers (distance from the origin in cells) are histogram bins on the device: an origin further than this many
// cells from the DEM's farthest corner is refused.
constexpr int VS_MAX_RINGS = 1 << 24;
constexpr int VS_TIMES = 8;  // entries of times_ms (include/glimpse_hip.h)

struct ViewshedJob {
  int device;
  const void* z;  // [ny][nx] float64, or float32 when f32
  int f32;
  int nx, ny;
  const double* x;  // [nx]
  const double* y;  // [ny]
  double inv_d;
  const double* origins;  // [m][3]
  int m;
  int correction;
  double radius, refraction;
  uint8_t* visible;  // [m][ny][nx]
  double* times_ms;  // [VS_TIMES] or null
};

// Distance (in cells, + 0.5: the ring number before truncation) of the DEM's farthest corner from an origin.
double viewshed_farthest_cells(const ViewshedJob& job, const double* origin);
// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int viewshed_run(const ViewshedJob& job);

}  // namespace glh
