// glh_terrain.h -- what glimpse_hip.hip (the C ABI: glh_stage_gradient, glh_stage_hillshade, glh_stage_polygon_mask) hands
// to glh_terrain.hip (the kernels and launches of Raster.gradient, Raster.hillshade and helpers.polygons_to_mask,
// raster.py:1465-1474, :1249-1264, helpers.py:1701-1768).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

constexpr int TR_TIMES = 5;  // entries of times_ms (include/glimpse_hip.h)

struct GradientJob {
  int device;
  const void* z;  // [ny][nx] float64, or float32 when f32
  int f32;
  int nx, ny;      // each >= 2
  double d0, d1;   // signed cell sizes along x (columns) and y (rows)
  void* dzdx;      // [ny][nx] of z's dtype
  void* dzdy;
  double* times_ms;  // [TR_TIMES] or null
};

struct HillshadeJob {
  int device;
  const void* z;
  int f32;
  int nx, ny;
  double d0, d1;        // the spacings handed to the gradient along x and y (the caller has negated dy)
  double vert_exag;
  double direction[3];  // the unit vector towards the light
  double fraction;
  double* out;  // [ny][nx] float64
  double* times_ms;
};

struct PolygonMaskJob {
  int device;
  const double* xy;         // [n_vertices][2] continuous cell coordinates (column, row)
  const int32_t* ring_off;  // [n_polygons + n_holes + 1] ascending, ring_off[0] = 0
  int n_polygons, n_holes;  // the polygon rings come first
  int nx, ny;
  uint8_t* out;  // [ny][nx]
  double* times_ms;
};

// Each runs its job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int gradient_run(const GradientJob& job);
int hillshade_run(const HillshadeJob& job);
int polygon_mask_run(const PolygonMaskJob& job);

}  // namespace glh
