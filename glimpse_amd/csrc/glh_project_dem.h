// glh_project_dem.h -- what glimpse_hip.hip (the C ABI: glh_stage_project_dem, glh_stage_rasterize) hands to
// glh_project_dem.hip (the kernels, the sort and the launches of Camera.project_dem, camera.py:967-1129, and
// Camera.rasterize, camera.py:858-883).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

struct CamDev;

constexpr int PD_TIMES = 8;  // entries of times_ms (include/glimpse_hip.h)

// One axis of the tiling (Grid.tile_indices, raster.py:581-610): tile k covers cells [start[k], end[k]) and brings
// end[k] - start[k] coordinates of its own, one tile after another in `coords`.
struct PdAxis {
  int n;
  const int32_t* start;
  const int32_t* end;
  const double* coords;
};

struct ProjectDemJob {
  int device;
  const CamDev* cam;
  int width, height;    // imgsz
  const void* z;        // [ny][nx] float64, or float32 when z_f32
  int z_f32;
  int nx, ny;
  const uint8_t* mask;  // [ny][nx], or null: every cell
  const void* values;   // [ny][nx][layers] of v_dtype, or null when layers == 0
  int v_dtype, layers;
  PdAxis tx, ty;
  int return_depth;
  double* out;          // [height][width][layers + return_depth]
  double* times_ms;     // [PD_TIMES] or null
};

struct RasterizeJob {
  int device;
  const int32_t* keys;   // [n] pixel of every point, each in [0, n_pixels)
  int n;
  const double* values;  // [n][layers]
  int layers;
  int n_pixels;
  double* out;           // [n_pixels][layers]
  double* times_ms;      // [PD_TIMES] or null
};

// Cells of every tile together (a cell counts once per tile it belongs to); what the device indexes with 32 bits.
int64_t project_dem_memberships(const ProjectDemJob& job);
// Each runs its job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int project_dem_run(const ProjectDemJob& job);
int rasterize_run(const RasterizeJob& job);

}  // namespace glh
