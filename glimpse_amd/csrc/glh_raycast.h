// glh_raycast.h -- what glimpse_hip.hip (the C ABI: glh_stage_raycast) hands to glh_raycast.hip (the kernels and the
// launches of Raster.intersect_rays, Camera.uv_to_dem and Camera.xyz_map: rays cast onto a DEM).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

struct CamDev;

constexpr int RC_TIMES = 4;  // entries of times_ms (include/glimpse_hip.h)

struct RaycastJob {
  int device;
  const void* z;  // [ny][nx] float64, or float32 when z_f32
  int z_f32;
  int nx, ny;
  double x0, y0, d0, d1;  // the centre of cell (0, 0) and the signed cell sizes
  int mode;               // GLH_RAYCAST_DIRECTIONS, _UV, _GRID
  const CamDev* cam;      // _UV, _GRID: the camera the rays leave
  const double* origins;  // _DIRECTIONS: [n_origins][3], n_origins 1 (every ray's) or n
  int n_origins;
  const double* rays;  // _DIRECTIONS: [n][3] directions; _UV: [n][2] image coordinates; _GRID: null
  int n;               // rays (_GRID: cols * rows)
  int step, cols, rows;  // _GRID: pixel centres step / 2 + k step, cols x rows of them
  int correction;
  double radius, refraction;
  int block;         // 0, or the power of two of patches a side whose maximum lets a ray skip them
  double* t;         // [n]
  double* xyz;       // [n][3]
  int32_t* patch;    // [n] row * (nx - 1) + column of the hit patch, -1 without a hit
  uint8_t* status;   // [n] GLH_RAYCAST_HIT ...
  double* times_ms;  // [RC_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int raycast_run(const RaycastJob& job);

}  // namespace glh
