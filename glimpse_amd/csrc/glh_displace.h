// glh_displace.h -- what glimpse_hip.hip (the C ABI: glh_stage_displacements) hands to glh_displace.hip (the kernels and
// the launch of glimpse_amd.displacements: dense template matching between frames).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

constexpr int DP_TIMES = 3;       // entries of times_ms (include/glimpse_hip.h)
constexpr int DP_MIN_SIDE = 3;    // template sides
constexpr int DP_MAX_SIDE = 63;
constexpr int DP_MAX_REACH = 32;  // offsets -reach .. reach per axis

struct DisplaceJob {
  int device;
  const void* frames;  // [n_frames][height][width] uint8, or float32 when is_float
  int is_float;
  int width, height, n_frames;
  const int32_t* pairs;  // [n_pairs][2]: the frame of the templates, the frame searched
  int n_pairs;
  const int32_t* corners;  // [n][2]: (l, t) of each template box in the first frame of a pair
  const uint8_t* valid;    // [n]: 0 = "template outside"
  int n;
  const int32_t* guess;  // null (0), [n][2], or [n_pairs][n][2] when guess_per_pair
  int guess_per_pair;
  int w, h, rx, ry;
  int subpixel;
  double* duv;       // [n_pairs][n][2]
  double* score;     // [n_pairs][n]
  uint8_t* status;   // [n_pairs][n] GLH_DISPLACE_MATCHED ...
  double* surface;   // null, or [n_pairs][n][2 ry + 1][2 rx + 1]
  double* times_ms;  // [DP_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int displacements_run(const DisplaceJob& job);

}  // namespace glh
