// glh_point_plan.h -- the fused frame step's LDS layout (shared with the kernel, glh_point.h) and the three decisions the
// host takes before every launch of it: the LDS plan (is the step taken at all, how large is region 2, one or two workgroups
// per CU), the cell cap of fast arithmetic, and the instantiation (launch shape and code) of glh_point_variants.h.
// Plain C++ under GLH_HD, like glh_math.h: tests/hostcheck compiles it with g++ and sweeps it without a GPU.
#pragma once
#include <algorithm>

#include "glh_math.h"

namespace glh {

constexpr int PT_MAX_TILE = 63;  // largest template side the fused kernel handles (rows padded to 64 floats)
constexpr int PT_MAX_OBS = 4;    // observers per point in the fused kernel (= MAX_OBS of the library)

constexpr int PT_BLK = 512;    // threads per workgroup (TB) for N <= 5120: two workgroups share a CU
constexpr int PT_BLK_BIG = 1024;  // TB for larger N: c[N] alone is > half the LDS, one 16-wave workgroup per CU

// LDS plan of the fused kernel (glh_point.h): c[N] + region 2
constexpr int PT_LDS_MAX = 152 * 1024;   // dynamic LDS of one workgroup (static <= 5 KB on top, 160 KB per CU)
constexpr int PT_LDS_HALF = 75 * 1024;   // dynamic LDS that still lets two workgroups share a CU
constexpr int PT_PATCH_LDS = 3328;       // static LDS of the raster windows (code 2: glh_point.h, PtPatches), taken off both
static_assert(PT_PATCH_LDS >= 2 * (int)sizeof(RasterPatch), "the raster windows fit their share");

// row stride (floats) of the zero-padded template tile, of the staged SSD kernel (glh_kernels.h) and of the fused step
GLH_HD int ssd_twp(int tw) { return (tw + 7) & ~7; }

GLH_HD int pt_align16(int x) { return (x + 15) & ~15; }
// LDS row stride (floats) of the search tile: >= ws + 11 readable columns and == 8 (mod 32), so the
// row-split lanes of a strip (rows g = 0..7) start in distinct 16-byte bank slots
GLH_HD int pt_search_ld(int ws) { return ((ws + 3 + 31) / 32) * 32 + 8; }
// histogram | LUT of nb bins (round 4: the cumulative counts are not written out any more -- the thread that owns a bin
// makes its LUT entry behind the scan, from registers)
GLH_HD int pt_hcl_bytes(int nb) { return pt_align16(nb * 4) + pt_align16(nb * 8); }
// bytes of the arrays that always live in LDS: template tile + histogram / cumulative counts / LUT
GLH_HD int pt_small_bytes(int tw, int th, int nb) { return pt_align16(th * ssd_twp(tw) * 4) + pt_hcl_bytes(nb); }

// The raw-key tile of a w x h crop is stored with its 'reflect' border already in place (2 rows above and below,
// 2 columns left, 3 right), row stride even: every 5x5 window of a PAIR of pixels is then three aligned 32-bit
// words per row, without index arithmetic.
GLH_HD int pt_keys_stride(int w) { return (w + 6 + 1) & ~1; }
GLH_HD int pt_keys_count(int w, int h) { return (h + 4) * pt_keys_stride(w); }

// dynamic LDS the moment sums of phase F are parked in: [13][512] doubles + their 13 totals
GLH_HD int pt_park_bytes() { return (13 * 512 + 16) * 8; }

// ints of the NumPy pairwise-sum plan staged in LDS: leaf_off | leaf_len | ops | level_off | roots
GLH_HD int pt_plan_ints(int nleaves, int nnodes, int nlevels, int nroots) {
  return 2 * nleaves + 3 * (nnodes - nleaves) + (nlevels + 1) + nroots;
}

// The launch shape of the fused step (glh_point.h) for N particles and O observers: threads per workgroup (tb) and PPT;
// glh_point_variants.h carries every shape this returns.
// N <= 5120: 512 threads, two workgroups per CU; larger N: 1024 threads, one per CU.  u of observer 0 in registers
// (PPT per thread) and its v in c[] up to 10240 particles, both parked in LDS / the uv scratch beyond that and with
// three or four observers.  Two observers keep observer 0 in registers as well (round 4: the first observer's pass is
// peeled off the observer loop, so the registers are dead during the second observer's tile pipeline).
GLH_HD void pt_shape(int N, int O, int* tb, int* ppt) {
  const bool big = N > 10 * PT_BLK;
  *tb = big ? PT_BLK_BIG : PT_BLK;
  int p = N <= 4 * *tb ? 4 : (N <= 10 * *tb ? 10 : 0);
  if ((big || O == 2) && p == 4) p = 10;  // (the library carries no PPT 4 of 1024 threads or of two observers)
  if ((big && p != 10) || O >= 3) p = 0;
  *ppt = p;
}

// What the plan reads of a context: fixed once the sequence, the observers' frame types and the rasters are set.
struct PtSetup {
  int N, O, tw, th;                     // particles, observers, template size
  int max_search_dim, interp_k;         // largest search-tile side of the context; order of the surface sampling (0: general)
  int bits[PT_MAX_OBS], channels[PT_MAX_OBS];  // of every observer's frames
  bool rasters;                         // the context holds a gridded dem / dem_sigma / viewshed
  int nleaves, nnodes, nlevels, nroots;  // the pairwise-sum plan of N items (glh_host.h: pairwise_plan)
  bool small_lds;                       // test hook (glh_set_fused(2)): region 2 at its minimum, typical tiles go to HBM
};

struct PtPlan {
  bool accepted;  // the fused kernel can take the sequence (otherwise every other field is 0: the staged kernels run)
  int tb, ppt;    // pt_shape
  int r2_bytes;   // LDS behind c[N]
  int cell_cap;   // fast arithmetic: surfaces of up to this many cells are sampled in per-cell form
  int lds_bytes;  // dynamic LDS of the launch
};

// LDS plan of the fused kernel (glh_point.h): c[N] + region 2.  Two workgroups per CU when the
// state and a typical tile fit in half the LDS, otherwise one.
GLH_HD PtPlan pt_plan(const PtSetup& s) {
  const PtPlan refused{};
  if (s.O > PT_MAX_OBS || s.tw > PT_MAX_TILE || s.th > PT_MAX_TILE) return refused;
  // (other median windows and bilinear sampling run on the general instantiations: pt_code)
  if (s.interp_k == 0) return refused;  // orders other than (3, 3) / (1, 1): staged kernels

  int nb = 256;
  for (int o = 0; o < s.O; ++o) {
    if (s.channels[o] != 1 && s.channels[o] != 3) return refused;
    // 16-bit and float frames: ranked in LDS / by linear buckets (glh_point.h: pt_tile_prep_wide, the float branch of
    // the observer pass) while a tile's pixel count fits a 16-bit key; wider workspaces: staged kernels
    if (s.bits[o] >= 16 && s.max_search_dim > 255) return refused;
    if (s.channels[o] == 3 || s.bits[o] >= 16) nb = 766;  // (16-bit / float: the bucket table is no larger)
  }
  // c[N] and, behind region 2, the pairwise-sum plan
  const int cN = pt_align16(s.N * 8) + pt_align16(4 * pt_plan_ints(s.nleaves, s.nnodes, s.nlevels, s.nroots));
  // phase D/E: tree nodes | clast, then (over them) three rank tables of N uint16
  const int plan = std::max(pt_align16(s.nnodes * 8) + PT_BLK_BIG * 8, 3 * pt_align16(s.N * 2));
  // (the big-tile path parks the scratch surface of a dense spline fit behind the template tile)
  // (... and the scratch of a dense spline fit of the largest surface fitted that way, when that surface itself stays in its
  // HBM workspace: glh_point.h, the last branch of the observer pass)
  const int r2_min = std::max(plan, std::max(pt_small_bytes(s.tw, s.th, nb) + GLH_SPL_DENSE_NINV / 2 * 8,
                                             pt_align16(GLH_SPL_DENSE_MAX * GLH_SPL_DENSE_MAX * 8)));
  // a 48 x 48 search tile of this template in LDS (what a ~2 px cloud needs)
  // (the template CDF lies over the search tile while the LUT is made: no bytes of its own)
  const int typical = pt_small_bytes(s.tw, s.th, nb) + 48 * pt_search_ld(48) * 4 + pt_keys_count(48, 48) * 2;
  // (a context with rasters runs the instantiations that keep windows of them in static LDS)
  const int patch = s.rasters ? PT_PATCH_LDS : 0;
  const int lds_half = PT_LDS_HALF - patch, lds_max = PT_LDS_MAX - patch;
  int r2;
  if (cN + std::max(r2_min, typical) <= lds_half)
    r2 = lds_half - cN;
  else
    r2 = std::min(lds_max - cN, 72 * 1024);
  if (s.small_lds) r2 = r2_min;  // test hook: typical tiles no longer fit -> HBM workspaces
  if (r2 < r2_min || cN + r2 > lds_max) return refused;  // (N beyond ~10 900: the staged kernels take the step)
  PtPlan p{};
  p.accepted = true;
  pt_shape(s.N, s.O, &p.tb, &p.ppt);
  p.r2_bytes = r2;
  // Fast arithmetic samples small fitted surfaces in per-cell power form (glh_math.h: spline_cell_row).  The fused
  // kernel holds the cell table in region 2 and converts at most two rows per thread; the staged kernels apply the
  // same bound (whether or not the fused kernel takes the step: 0 only where the plan refuses), so that a given surface is
  // evaluated by the same formula on either path (bit-identical results).
  p.cell_cap = std::min(r2 / (GLH_CELL_LD * 8), 2 * p.tb / 4);
  // (at least what phase F parks its partial sums in: every plan but the small-LDS test hook has more)
  p.lds_bytes = std::max(cN + r2, pt_park_bytes());
  return p;
}

// What varies from launch to launch of one context.
struct PtLaunch {
  bool fast, philox, compact, masked;  // fast arithmetic; device Philox draws; run-length compact input; an observer mask is set
  bool all_cartesian;                  // every point on CartesianMotion
  int hp_rx, hp_ry, interp_k;          // half sizes of the median window; order of the surface sampling
  bool on[PT_MAX_OBS];                 // the observer has an image on this frame
  uint32_t cam_flags[PT_MAX_OBS];      // cam_flags of that image's camera
  int bits[PT_MAX_OBS];                // of the observer's frames
};

struct PtCode {
  int surf;        // SURF of glh_point_variants.h: 0 plain, 1 general, 2 general with the raster samples
  bool fast, con;  // FAST, CON
  int flags;       // Context.last_variant()[3]: fast | general << 1 | contract << 2 | rasters << 3
};

// The code of the instantiation (glh_point_variants.h) a launch runs, for O observers of a context with or without rasters.
GLH_HD PtCode pt_code(const PtLaunch& l, int O, bool rast) {
  // the general instantiation: gridded surfaces and / or motion models other than CartesianMotion
  const bool fast = l.fast;
  // ... and, in fast arithmetic, everything the common instantiation is not compiled for (glh_point.h: COMMON): it
  // takes device Philox draws, compact input records, every observer on and unmasked, and cameras within
  // perspective + radial numerator (project_simple_fast)
  bool common = fast && l.philox && l.compact && !l.masked;
  for (int o = 0; o < O; ++o) common &= l.on[o] && !(l.cam_flags[o] & CAM_F_NOT_SIMPLE);
  // (the contract is independent of the surfaces and motion models: the general code has its instantiation too)
  bool plain = l.hp_rx == 2 && l.hp_ry == 2 && l.interp_k == 3;  // the 5 x 5 median, bicubic sampling ...
  for (int o = 0; o < O; ++o) plain &= l.bits[o] == 8;            // ... of 8-bit frames
  // (rast: the instantiations with the raster samples)
  const bool surf = rast || !l.all_cartesian || (fast && !common) || !plain;
  // codes the library carries (glh_point_variants.h): exact / exact general / fast common / fast general / fast
  // general under the contract
  return PtCode{rast ? 2 : (surf ? 1 : 0), fast, surf ? common : fast,
                (fast ? 1 : 0) | (surf ? 2 : 0) | (common ? 4 : 0) | (rast ? 8 : 0)};
}

}  // namespace glh
