// glh_clahe.h -- what glimpse_hip.hip (the C ABI: glh_stage_clahe) hands to glh_clahe.hip (the kernels and launches of
// optimize.CLAHE), and the host arithmetic of the rule's steps 1 and 2 (INPUTS.md, "CLAHE: the rule").  Host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace glh {

constexpr int CL_TIMES = 5;  // entries of times_ms (include/glimpse_hip.h)
constexpr int CL_BINS = 256;

// Steps 1 and 2 of the rule: the extended size, the tile and the clip limit.
struct ClaheGeometry {
  int64_t ext_w, ext_h;
  int64_t tw, th;  // a tile's columns and rows
  int64_t area;    // tw * th
  int64_t lim;     // 0: no clipping
};

// w, h >= 1, 1 <= tiles_x <= w, 1 <= tiles_y <= h, clip_limit finite.
inline ClaheGeometry clahe_geometry(int w, int h, double clip_limit, int tiles_x, int tiles_y) {
  ClaheGeometry g;
  const bool fits = w % tiles_x == 0 && h % tiles_y == 0;
  g.ext_w = fits ? w : (int64_t)w + (tiles_x - w % tiles_x);
  g.ext_h = fits ? h : (int64_t)h + (tiles_y - h % tiles_y);
  g.tw = g.ext_w / tiles_x;
  g.th = g.ext_h / tiles_y;
  g.area = g.tw * g.th;
  g.lim = 0;
  if (clip_limit > 0.0) {
    // max(int(clipLimit * area / 256), 1); no bin holds more than `area`, so any limit from there on clips nothing and
    // the truncation stays inside int64 whatever clipLimit is
    const double v = clip_limit * (double)g.area / 256.0;
    g.lim = v >= (double)g.area ? g.area : (int64_t)v;
    if (g.lim < 1) g.lim = 1;
  }
  return g;
}

struct ClaheJob {
  int device;
  const uint8_t* src;  // [h][w][channels]
  int w, h, channels;
  int tiles_x, tiles_y;
  ClaheGeometry geo;
  uint8_t* dst;      // [h][w]
  uint8_t* luts;     // [tiles_y][tiles_x][256] or null
  double* times_ms;  // [CL_TIMES] or null
};

// Runs the job; a GLH_* status, with the message left for glh_last_error() on failure (glh_stage.h: fail).
int clahe_run(const ClaheJob& job);

}  // namespace glh
