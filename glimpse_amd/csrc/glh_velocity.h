// glh_velocity.h -- what glimpse_hip.hip (the C ABI: glh_stage_velocity_field) hands to glh_velocity.hip (the kernels and
// the launch of glimpse_amd.velocity_field: displacements tested against their neighbours and stacked over the pairs).
// Host-only declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

constexpr int VF_TIMES = 4;            // entries of times_ms (include/glimpse_hip.h)
constexpr int VF_MAX_RADIUS = 2;       // the neighbourhood is (2 radius + 1)^2 nodes
constexpr int VF_MAX_NODES = 1 << 24;  // of one call: the launch limit

struct VelocityJob {
  int device;
  const double* duv;      // [n_pairs][n][2]
  const double* score;    // [n_pairs][n]
  const uint8_t* status;  // [n_pairs][n]
  int n_pairs, rows, cols;  // n = rows * cols, row-major
  const double* dt;       // [n_pairs]
  double scale[2];
  double min_score;
  int max_status;  // candidates have status <= max_status
  int radius, min_neighbors;
  double threshold, epsilon;
  int min_count;
  double* v;         // [n][2]
  double* sigma;     // [n][2]
  int32_t* count;    // [n]
  uint8_t* kept;     // [n_pairs][n]
  double* times_ms;  // [VF_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int velocity_field_run(const VelocityJob& job);

}  // namespace glh
