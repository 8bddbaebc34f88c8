// glh_ortho.h -- what glimpse_hip.hip (the C ABI: glh_stage_orthorectify) hands to glh_ortho.hip (the kernel and the
// launches of Image.orthorectify: an oblique frame resampled onto the DEM's grid).  Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

struct CamDev;

struct OrthoJob {
  int device;
  const void* frames;      // [n_frames][height][width][channels]
  int depth_bits, is_float;  // 8 / 0, 16 / 0, 32 / 1, 64 / 1
  int width, height, channels, n_frames;
  const CamDev* cams;      // [n_frames] each frame's own camera
  const void* z;           // [ny][nx] float64, or float32 when z_f32
  int z_f32;
  int nx, ny;
  const double* x;         // [nx] cell-centre x of every column
  const double* y;         // [ny] cell-centre y of every row
  const uint8_t* seen;     // [n_seen][ny][nx] non-zero: the cell may be seen; or null: every cell
  int n_seen;
  const int32_t* seen_of;  // [n_frames] which of the n_seen masks a frame takes; null: the first
  int method;              // RPJ_LINEAR, RPJ_NEAREST
  void* out;               // [n_frames][ny][nx][channels] float32 for float32 frames, else float64
  double* kernel_ms;       // or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int orthorectify_run(const OrthoJob& job);

}  // namespace glh
