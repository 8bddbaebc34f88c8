// glh_orient.h -- what glimpse_hip.hip (the C ABI: glh_orient_create / _eval / _destroy, glh_stage_uv_to_xy) hands to
// glh_orient.hip (the objective and gradient of optimize.ObserverCameras.fit, optimize.py:2047-2072, and
// Camera._uv_to_xy, camera.py:1510-1519).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct glh_orient;  // the C ABI's handle: the uploaded matches of one sequence (glh_orient.hip)

namespace glh {

constexpr int OR_TIMES = 4;     // entries of times_ms (include/glimpse_hip.h)
constexpr int OR_CHUNK = 4096;  // matches per workgroup of the map kernel: part of the summation order

// The arguments have been checked (glimpse_hip.hip).  A GLH_* status, with the message left for glh_last_error() on
// failure (glh_stage.h: fail).
int orient_create(int device, int n_images, int n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                  const int64_t* pair_offset, const double* xy_i, const double* xy_j, glh_orient** out);
int orient_eval(glh_orient* h, const double* R, const double* Rprime, double* objective, double* gradient,
                double* times_ms);
void orient_destroy(glh_orient* h);

struct CamDev;
int uv_to_xy_run(int device, const CamDev& cam, const double* uv, int n, double* xy);

}  // namespace glh
