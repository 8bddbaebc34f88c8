// The host arithmetic of glimpse_amd/csrc/glh_clahe.hip (glh_clahe.h: the extended size, the tile and the clip limit),
// compiled for the CPU so that tests/test_clahe.py can compare it with tests/clahe_restated.py.  Test-only.
#include "../../glimpse_amd/csrc/glh_clahe.h"

extern "C" {

// out [6]: ext_w, ext_h, tw, th, area, lim
void cl_geometry(int w, int h, double clip_limit, int tiles_x, int tiles_y, int64_t* out) {
  const glh::ClaheGeometry g = glh::clahe_geometry(w, h, clip_limit, tiles_x, tiles_y);
  out[0] = g.ext_w, out[1] = g.ext_h, out[2] = g.tw, out[3] = g.th, out[4] = g.area, out[5] = g.lim;
}
}
