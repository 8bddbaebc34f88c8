// plan_sweep.h -- TEST-ONLY: the fused step's host plan (glimpse_amd/csrc/glh_point_plan.h: pt_plan) over every particle
// count 1 .. n_max, one to four observers, rasters off and on, with the pairwise-sum counts of glh_host.h: pairwise_plan.
// Shared by hostcheck.cpp (tests/test_hostcheck.py) and sanitize_main.cpp (the same sweep under ASan + UBSan).
#pragma once
#include "../../glimpse_amd/csrc/glh_host.h"

namespace glh {

inline PtSetup hc_setup(int N, int O, int tw, int th, int max_search_dim, int interp_k, const int* bits,
                        const int* channels, bool rasters, bool small_lds) {
  PtSetup s{};
  s.N = N, s.O = O, s.tw = tw, s.th = th, s.max_search_dim = max_search_dim, s.interp_k = interp_k;
  for (int o = 0; o < O && o < PT_MAX_OBS; ++o) s.bits[o] = bits[o], s.channels[o] = channels[o];
  s.rasters = rasters, s.small_lds = small_lds;
  PairwisePlan pl;
  pairwise_plan(N, pl);
  s.nleaves = (int)pl.leaf_off.size(), s.nnodes = pl.nnodes;
  s.nlevels = (int)pl.level_off.size() - 1, s.nroots = (int)pl.roots.size();
  return s;
}

// 21 x 21 templates of one-channel 8-bit frames.  Conditions read from the code: an accepted plan's dynamic LDS lies
// between what phase F parks its sums in and the workgroup's share less the raster windows, its shape is pt_shape's, and
// the cell table converts at most two rows per thread (cell_cap <= tb / 2); a refused plan is all zeros.
// Returns the number of violations; accepted[0] the number of accepted plans.
inline long pt_plan_sweep(int n_max, long* accepted) {
  const int bits[PT_MAX_OBS] = {8, 8, 8, 8}, channels[PT_MAX_OBS] = {1, 1, 1, 1};
  long bad = 0;
  *accepted = 0;
  for (int N = 1; N <= n_max; ++N) {
    PtSetup s = hc_setup(N, PT_MAX_OBS, 21, 21, 255, 3, bits, channels, false, false);  // (pairwise_plan once per count)
    for (int rast = 0; rast < 2; ++rast)
      for (int O = 1; O <= PT_MAX_OBS; ++O) {
        s.O = O, s.rasters = rast != 0;
        const PtPlan p = pt_plan(s);
        if (!p.accepted) {
          bad += p.tb || p.ppt || p.r2_bytes || p.cell_cap || p.lds_bytes;
          continue;
        }
        ++*accepted;
        int tb, ppt;
        pt_shape(N, O, &tb, &ppt);
        bad += p.tb != tb || p.ppt != ppt;
        bad += p.lds_bytes > PT_LDS_MAX - (rast ? PT_PATCH_LDS : 0);
        bad += p.lds_bytes < pt_park_bytes();
        bad += p.cell_cap > p.tb / 2 || p.cell_cap < 0;
        bad += p.r2_bytes <= 0 || p.r2_bytes > p.lds_bytes;
      }
  }
  return bad;
}

}  // namespace glh
