// glh_ransac_plan.h -- the host plan of glh_calib_ransac_groups (optimize.ransac_pairs): what is checked before a device is
// touched, where a hypothesis's consensus mask lies, and how a list of groups is cut into chunks whose masks stay below a
// budget.  Plain C++ without a HIP header, so that tests/hostcheck/ransac_pairs_hostcheck.cpp compiles the very same code
// for the CPU under the sanitizers.
//
// A GROUP is one match control of the handle with one of its two cameras fitted; it owns hypotheses hyp_offset[g] ..
// hyp_offset[g + 1], each a sample of n of the group's rows.  Hypothesis h of group g keeps one byte per row of the group
// at mask_offset[g] + (h - hyp_offset[g]) * rows(g): the masks of all hypotheses are rg_mask_bytes() in all.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

namespace glh {

constexpr int RANSAC_TIMES = 6;                          // entries of glh_calib_ransac_groups' times_ms
constexpr int RANSAC_DRAWN_TIMES = RANSAC_TIMES + 1;     // of glh_calib_ransac_groups_drawn's: the draw, appended
constexpr int64_t RANSAC_MASK_LIMIT = (int64_t)1 << 31;  // mask bytes of one call: fewer than this
constexpr int RANSAC_KIND_MATCHES = 2;                   // GLH_CALIB_MATCHES: the first of the three match kinds
constexpr int RANSAC_NOT_REFITTED = -100;                // refit_status of a hypothesis that was not accepted

struct RgCall {
  // the handle's controls
  int n_cams, n_controls;
  const int32_t *kind, *cam_a, *cam_b;  // [n_controls]
  const int64_t* row_offset;            // [n_controls + 1]
  // the call
  int n_groups;
  const int32_t *group_control, *group_cam;  // [G]
  int p;
  const int32_t* slots;                   // [p]
  const double *x0, *lb, *ub, *x_scale;   // [G][p]
  const int64_t* hyp_offset;              // [G + 1]
  int n;
  const int64_t* samples;                 // [hyp_offset[G]][n], global row numbers
  int max_nfev;
  double ftol, xtol, gtol, max_error;
  bool outputs;                           // every output pointer is there
  // glh_calib_ransac_groups_drawn (`draws`): the samples of a group with drawn[g] == 1 are drawn on the device as those of
  // pair group_id[g] (glh_ransac_draw.h) and its entries of `samples` are not read
  bool draws = false;
  const int32_t* group_id = nullptr;      // [G]
  const uint8_t* drawn = nullptr;         // [G]
};

inline bool rg_drawn(const RgCall& c, int g) { return c.draws && c.drawn[g] != 0; }

inline int64_t rg_rows(const RgCall& c, int g) {
  return c.row_offset[c.group_control[g] + 1] - c.row_offset[c.group_control[g]];
}

// rows * hypotheses, RANSAC_MASK_LIMIT where that is reached (no overflow for any pair of non-negative int64)
inline int64_t rg_mask_bytes(int64_t rows, int64_t hyps) {
  if (rows <= 0 || hyps <= 0) return 0;
  if (rows >= RANSAC_MASK_LIMIT || hyps >= RANSAC_MASK_LIMIT || rows > (RANSAC_MASK_LIMIT - 1) / hyps) return RANSAC_MASK_LIMIT;
  return rows * hyps;
}

// mask_offset[g] for g = 0 .. n_groups (the last is the total), capped at RANSAC_MASK_LIMIT.  Returns the total.
inline int64_t rg_mask_offsets(int n_groups, const int64_t* rows, const int64_t* hyps, int64_t* mask_offset) {
  int64_t at = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (mask_offset) mask_offset[g] = at;
    const int64_t b = rg_mask_bytes(rows[g], hyps[g]);
    at = at >= RANSAC_MASK_LIMIT - b ? RANSAC_MASK_LIMIT : at + b;
  }
  if (mask_offset) mask_offset[n_groups] = at;
  return at;
}

// chunk_of[g]: consecutive groups share a chunk while the chunk's mask bytes stay at or below `budget`; a group whose own
// masks exceed it is a chunk of its own.  Returns the number of chunks.
inline int rg_chunks(int n_groups, const int64_t* rows, const int64_t* hyps, int64_t budget, int32_t* chunk_of) {
  int chunk = -1;
  int64_t used = 0;
  for (int g = 0; g < n_groups; ++g) {
    const int64_t b = rg_mask_bytes(rows[g], hyps[g]);
    if (chunk < 0 || b > budget - used || used > budget) {  // (b > budget - used: used + b > budget without overflow)
      ++chunk;
      used = 0;
    }
    used += b;
    chunk_of[g] = chunk;
  }
  return chunk + 1;
}

#define RANSAC_FAIL(...)                    \
  do {                                  \
    snprintf(msg, cap, __VA_ARGS__);    \
    return false;                       \
  } while (0)

// true: the call can be served.  false: `msg` says why not (GLH_E_INVALID).  Nothing here touches a device.
inline bool rg_check(const RgCall& c, char* msg, size_t cap) {
  if (!c.row_offset || (c.n_controls && (!c.kind || !c.cam_a || !c.cam_b))) RANSAC_FAIL("ransac groups: a handle without controls");
  if (c.n_groups < 0 || c.n_groups >= (1 << 24)) RANSAC_FAIL("ransac groups: %d groups: fewer than 2^24 are served", c.n_groups);
  if (!c.slots || !c.x0 || !c.lb || !c.ub || !c.x_scale || !c.hyp_offset || !c.outputs ||
      (c.n_groups && (!c.group_control || !c.group_cam)))
    RANSAC_FAIL("ransac groups: null argument");
  if (c.draws && c.n_groups && (!c.group_id || !c.drawn)) RANSAC_FAIL("ransac groups: null argument: the groups' ids and drawn flags");
  if (c.p < 1 || c.p > 18) RANSAC_FAIL("ransac groups: %d parameters: 1 .. 18 are served", c.p);
  uint32_t seen = 0;
  for (int i = 0; i < c.p; ++i) {
    const int s = c.slots[i];
    if (s < 0 || s >= 20 || s == 6 || s == 7 || ((seen >> s) & 1u))
      RANSAC_FAIL("ransac groups: parameter %d is entry %d of the camera vector: distinct ones of 0 .. 5, 8 .. 19", i, s);
    seen |= 1u << s;
  }
  if (c.n < 1) RANSAC_FAIL("ransac groups: samples of %d rows", c.n);
  if (c.max_nfev < 1 || !(c.ftol >= 0.0 && c.ftol < 1.0) || !(c.xtol >= 0.0 && c.xtol < 1.0) ||
      !(c.gtol >= 0.0 && c.gtol < INFINITY))
    RANSAC_FAIL("ransac groups: %d evaluations, ftol %g, xtol %g, gtol %g", c.max_nfev, c.ftol, c.xtol, c.gtol);
  if (!(c.max_error == c.max_error)) RANSAC_FAIL("ransac groups: max_error is NaN");
  if (c.hyp_offset[0] != 0) RANSAC_FAIL("ransac groups: hyp_offset[0] is %lld, not 0", (long long)c.hyp_offset[0]);
  int64_t covered = 0, mask = 0;
  for (int g = 0; g < c.n_groups; ++g) {
    const int ctl = c.group_control[g];
    if (ctl < 0 || ctl >= c.n_controls) RANSAC_FAIL("ransac groups: group %d is control %d of %d", g, ctl, c.n_controls);
    if (c.kind[ctl] < RANSAC_KIND_MATCHES)
      RANSAC_FAIL("ransac groups: group %d is control %d, a POINTS or LINES control: the match kinds are served", g, ctl);
    if (g > 0 && ctl <= c.group_control[g - 1])
      RANSAC_FAIL("ransac groups: group %d is control %d after control %d: the groups name distinct controls in ascending order", g,
              ctl, c.group_control[g - 1]);
    const int cam = c.group_cam[g];
    if (cam < 0 || cam >= c.n_cams) RANSAC_FAIL("ransac groups: group %d fits camera %d of %d", g, cam, c.n_cams);
    if (cam != c.cam_a[ctl] && cam != c.cam_b[ctl])
      RANSAC_FAIL("ransac groups: group %d fits camera %d, which is neither camera (%d, %d) of its control", g, cam, c.cam_a[ctl],
              c.cam_b[ctl]);
    if (c.hyp_offset[g + 1] < c.hyp_offset[g] || c.hyp_offset[g + 1] >= RANSAC_MASK_LIMIT)
      RANSAC_FAIL("ransac groups: group %d ends at hypothesis %lld after %lld: not decreasing, fewer than 2^31 in all", g,
              (long long)c.hyp_offset[g + 1], (long long)c.hyp_offset[g]);
    const int64_t rows = rg_rows(c, g), hyps = c.hyp_offset[g + 1] - c.hyp_offset[g];
    if (c.draws) {
      if (c.group_id[g] < 0) RANSAC_FAIL("ransac groups: group %d has the id %d: ids are not negative", g, c.group_id[g]);
      if (c.drawn[g] > 1) RANSAC_FAIL("ransac groups: group %d has the drawn flag %d: 0 or 1", g, c.drawn[g]);
      if (c.drawn[g] && hyps > 0 && rows <= c.n)
        RANSAC_FAIL("ransac groups: group %d draws samples of %d of its %lld rows: a drawn group has more rows than that", g, c.n,
                    (long long)rows);
    }
    covered += rows;
    const int64_t b = rg_mask_bytes(rows, hyps);
    mask = mask >= RANSAC_MASK_LIMIT - b ? RANSAC_MASK_LIMIT : mask + b;
    for (int i = 0; i < c.p; ++i) {
      const size_t k = (size_t)g * c.p + i;
      if (!(c.lb[k] <= c.x0[k] && c.x0[k] <= c.ub[k]) || !(fabs(c.x0[k]) < INFINITY))
        RANSAC_FAIL("ransac groups: group %d, parameter %d starts at %g outside its bounds %g .. %g", g, i, c.x0[k], c.lb[k], c.ub[k]);
      if (!(c.lb[k] < c.ub[k]))
        RANSAC_FAIL("ransac groups: group %d, parameter %d has the bounds %g .. %g: the lower one must be below the upper one", g, i,
                c.lb[k], c.ub[k]);
      if (!(c.x_scale[k] > 0.0 && c.x_scale[k] < INFINITY))
        RANSAC_FAIL("ransac groups: group %d, parameter %d has scale %g", g, i, c.x_scale[k]);
    }
  }
  // every row of the handle gets its final byte from its group
  if (covered != c.row_offset[c.n_controls])
    RANSAC_FAIL("ransac groups: the groups hold %lld of the handle's %lld rows: every row belongs to exactly one group", (long long)covered,
            (long long)c.row_offset[c.n_controls]);
  if (mask >= RANSAC_MASK_LIMIT) RANSAC_FAIL("ransac groups: the consensus masks take 2^31 bytes or more: fewer are served in one call");
  const int64_t H = c.n_groups ? c.hyp_offset[c.n_groups] : 0;
  bool given = false;  // a group whose hypotheses come from `samples`
  for (int g = 0; g < c.n_groups; ++g) given = given || (!rg_drawn(c, g) && c.hyp_offset[g + 1] > c.hyp_offset[g]);
  if (given && !c.samples) RANSAC_FAIL("ransac groups: null samples");
  if (H > 0 && H > (RANSAC_MASK_LIMIT - 1) / c.n) RANSAC_FAIL("ransac groups: %lld samples of %d rows: fewer than 2^31 rows in all", (long long)H, c.n);
  for (int g = 0; g < c.n_groups; ++g) {
    if (rg_drawn(c, g)) continue;
    const int64_t first = c.row_offset[c.group_control[g]], last = c.row_offset[c.group_control[g] + 1];
    for (int64_t k = c.hyp_offset[g] * c.n; k < c.hyp_offset[g + 1] * c.n; ++k)
      if (c.samples[k] < first || c.samples[k] >= last)
        RANSAC_FAIL("ransac groups: hypothesis %lld of group %d samples row %lld outside its control's rows %lld .. %lld", (long long)(k / c.n),
                g, (long long)c.samples[k], (long long)first, (long long)last);
  }
  return true;
}
#undef RANSAC_FAIL

}  // namespace glh
