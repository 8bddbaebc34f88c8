// glh_sift.h -- what glimpse_hip.hip (the C ABI: glh_sift_create / _detect / _read / _counts / _layer / _destroy) hands to
// glh_sift.hip (SIFT detection and description, optimize.SIFT; the rule is INPUTS.md's "SIFT: the rule").  Host-only
// declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct glh_sift;  // the C ABI's handle: the pyramid and the lists of one device (glh_sift.hip)

namespace glh {

constexpr int SF_TIMES = 7;         // entries of times_ms (include/glimpse_hip.h)
constexpr int SF_MAX_LAYERS = 8;    // nOctaveLayers
constexpr int SF_MAX_OCTAVES = 32;  // (a doubled side below 2^24 has at most 21)
constexpr int SF_MAX_RADIUS = 4096; // of a weight table: its half fits the blur pass's LDS
constexpr int SF_MAX_SIDE = 1 << 23;  // of the image: a doubled row or column index fits 24 bits of a sort key
constexpr double SF_MAX_SIGMA = 16.0;
constexpr int SF_REFINED_COLS = 12;  // status, octave, layer, row, column, xc, xr, xi, contrast, size, pt x, pt y
constexpr int SF_KEYPOINT_COLS = 6;  // pt x, pt y, size, angle, response, octave (packed)
constexpr int SF_CELL_COLS = 5;      // octave, layer, row, column, orientation bin

struct SiftParams {
  int S;  // nOctaveLayers
  double contrast, edge, sigma;
  int radius[SF_MAX_LAYERS + 3];           // [0] the base's blur, [i] layer i - 1 -> layer i
  const double* table[SF_MAX_LAYERS + 3];  // [2 r + 1] each, host
};

// The arguments have been checked (glimpse_hip.hip).  A GLH_* status, with the message left for glh_last_error() on
// failure (glh_stage.h: fail).
int sift_create(int device, glh_sift** out);
int sift_detect(glh_sift* h, const uint8_t* image, int w, int h_px, const SiftParams& p, int* n, double* times_ms);
void sift_counts(const glh_sift* h, int32_t* out);  // octaves, candidates, keypoints, S, doubled width, doubled height
int sift_read(const glh_sift* h, double* keypoints, uint8_t* descriptors);
int sift_layer(glh_sift* h, int kind, int octave, int index, void* out);
void sift_destroy(glh_sift* h);

}  // namespace glh
