// glh_ransac_plan.h -- the host plan of glh_calib_ransac_groups (optimize.ransac_pairs): what is checked before a device is
// touched, where a hypothesis's consensus mask lies, and how a list of groups is cut into chunks whose masks stay below a
// budget; and what glh_calib_fit_sets checks (fs_check), with the checks the two share (par_*_ok).  Both read the handle's
// CalibTable and the struct the call is served from (glh_calib.h).  Plain C++ without a HIP header, so that tests/hostcheck/
// (ransac_pairs_hostcheck.cpp, fit_sets_hostcheck.cpp) compiles the very same code for the CPU under the sanitizers.
//
// A GROUP is one match control of the handle with one of its two cameras fitted; it owns hypotheses hyp_offset[g] ..
// hyp_offset[g + 1], each a sample of n of the group's rows.  Hypothesis h of group g keeps one byte per row of the group
// at mask_offset[g] + (h - hyp_offset[g]) * rows(g): the masks of all hypotheses are rg_mask_bytes() in all.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/glimpse_hip.h"
#include "glh_calib.h"

namespace glh {

constexpr int RANSAC_TIMES = 6;                          // entries of glh_calib_ransac_groups' times_ms
constexpr int RANSAC_DRAWN_TIMES = RANSAC_TIMES + 1;     // of glh_calib_ransac_groups_drawn's: the draw, appended
constexpr int64_t RANSAC_MASK_LIMIT = (int64_t)1 << 31;  // mask bytes of one call: fewer than this
constexpr int RANSAC_NOT_REFITTED = -100;                // refit_status of a hypothesis that was not accepted

inline bool rg_drawn(const CalibRansac& c, int g) { return c.draws && c.drawn[g] != 0; }

inline int64_t table_rows(const CalibTable& t, int control) { return t.row_offset[control + 1] - t.row_offset[control]; }

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

// What fs_check ("calib fit") and rg_check ("ransac groups") both check; `who` begins the message.  1 .. 18 parameters,
// distinct entries of the camera vector (imgsz, entries 6 and 7, is no parameter: optimize.Cameras' masks never hold it).
inline bool par_slots_ok(const char* who, const CalibPar& c, char* msg, size_t cap) {
  if (c.p < 1 || c.p > 18) RANSAC_FAIL("%s: %d parameters: 1 .. 18 are served", who, c.p);
  uint32_t seen = 0;
  for (int i = 0; i < c.p; ++i) {
    const int s = c.slots[i];
    if (s < 0 || s >= 20 || s == 6 || s == 7 || ((seen >> s) & 1u))
      RANSAC_FAIL("%s: parameter %d is entry %d of the camera vector: distinct ones of 0 .. 5, 8 .. 19", who, i, s);
    seen |= 1u << s;
  }
  return true;
}

inline bool par_options_ok(const char* who, const CalibPar& c, char* msg, size_t cap) {
  if (c.max_nfev < 1 || !(c.ftol >= 0.0 && c.ftol < 1.0) || !(c.xtol >= 0.0 && c.xtol < 1.0) ||
      !(c.gtol >= 0.0 && c.gtol < INFINITY))
    RANSAC_FAIL("%s: %d evaluations, ftol %g, xtol %g, gtol %g", who, c.max_nfev, c.ftol, c.xtol, c.gtol);
  return true;
}

// Block `block` of p starts, bounds and scales; `group` names it in the message (negative: the call's only block).
inline bool par_block_ok(const char* who, int group, size_t block, const CalibPar& c, char* msg, size_t cap) {
  for (int i = 0; i < c.p; ++i) {
    const size_t k = block * c.p + i;
    const bool outside = !(c.lb[k] <= c.x0[k] && c.x0[k] <= c.ub[k]) || !(fabs(c.x0[k]) < INFINITY), empty = !(c.lb[k] < c.ub[k]);
    if (!outside && !empty && c.scale[k] > 0.0 && c.scale[k] < INFINITY) continue;
    char where[32] = "";
    if (group >= 0) snprintf(where, sizeof(where), "group %d, ", group);
    if (outside) RANSAC_FAIL("%s: %sparameter %d starts at %g outside its bounds %g .. %g", who, where, i, c.x0[k], c.lb[k], c.ub[k]);
    if (empty)  // (as scipy.optimize.least_squares: no room for a difference step)
      RANSAC_FAIL("%s: %sparameter %d has the bounds %g .. %g: the lower one must be below the upper one", who, where, i, c.lb[k],
                  c.ub[k]);
    RANSAC_FAIL("%s: %sparameter %d has scale %g", who, where, i, c.scale[k]);
  }
  return true;
}

// glh_calib_fit_sets, as rg_check below: true, or false and why not in `msg`.
inline bool fs_check(const CalibTable& t, const CalibFit& f, char* msg, size_t cap) {
  const int64_t N = t.row_offset[t.n_controls];
  if (!f.vectors || !f.slots || !f.x0 || !f.lb || !f.ub || !f.scale || !f.set_offset || !f.x || !f.status || !f.mean_error)
    RANSAC_FAIL("calib fit: null argument");
  if (f.fit_cam < 0 || f.fit_cam >= t.n_cams) RANSAC_FAIL("calib fit: camera %d of %d", f.fit_cam, t.n_cams);
  if (!par_slots_ok("calib fit", f, msg, cap) || !par_block_ok("calib fit", -1, 0, f, msg, cap)) return false;
  if (f.n_sets < 0 || f.n_sets >= (1 << 24)) RANSAC_FAIL("calib fit: %d sets: fewer than 2^24 are served", f.n_sets);
  if (!par_options_ok("calib fit", f, msg, cap)) return false;
  if (f.set_offset[0] != 0) RANSAC_FAIL("calib fit: set_offset[0] is %lld, not 0", (long long)f.set_offset[0]);
  for (int q = 0; q < f.n_sets; ++q)
    if (f.set_offset[q + 1] < f.set_offset[q] || f.set_offset[q + 1] >= ((int64_t)1 << 31))
      RANSAC_FAIL("calib fit: set %d ends at row %lld after %lld: not decreasing, fewer than 2^31 rows in all", q,
                  (long long)f.set_offset[q + 1], (long long)f.set_offset[q]);
  const int64_t total = f.set_offset[f.n_sets];
  if (total > 0 && !f.set_rows) RANSAC_FAIL("calib fit: null set rows");
  bool any_lines = false;
  for (int c = 0; c < t.n_controls; ++c) {
    if (t.kind[c] == GLH_CALIB_ROTATION && table_rows(t, c) > 0 && !f.observed)
      RANSAC_FAIL("calib fit: control %d is a ROTATION control, whose obs are camera coordinates: pass observed", c);
    any_lines = any_lines || (t.kind[c] == GLH_CALIB_LINES && table_rows(t, c) > 0);
  }
  for (int64_t k = 0; k < total; ++k) {
    const int64_t r = f.set_rows[k];
    if (r < 0 || r >= N) RANSAC_FAIL("calib fit: row %lld of %lld", (long long)r, (long long)N);
    if (any_lines) {
      const int c = (int)(std::upper_bound(t.row_offset, t.row_offset + t.n_controls + 1, r) - t.row_offset) - 1;
      if (t.kind[c] == GLH_CALIB_LINES) RANSAC_FAIL("calib fit: row %lld belongs to control %d, a Lines control", (long long)r, c);
    }
  }
  if (f.score) {
    if (!f.inlier) RANSAC_FAIL("calib fit: null inlier output");
    if (!(f.max_error == f.max_error)) RANSAC_FAIL("calib fit: max_error is NaN");
    if (any_lines) RANSAC_FAIL("calib fit: scoring covers every row, and the handle holds a Lines control");
    if ((int64_t)f.n_sets * N >= ((int64_t)1 << 31))
      RANSAC_FAIL("calib fit: %d sets of %lld rows to score: fewer than 2^31 in all are served", f.n_sets, (long long)N);
  }
  return true;
}

// true: the call can be served, once its cameras are expanded.  false: `msg` says why not (GLH_E_INVALID).  No device is touched.
inline bool rg_check(const CalibTable& t, const CalibRansac& c, char* msg, size_t cap) {
  if (!t.row_offset || (t.n_controls && (!t.kind || !t.cam_a || !t.cam_b))) RANSAC_FAIL("ransac groups: a handle without controls");
  if (c.n_groups < 0 || c.n_groups >= (1 << 24)) RANSAC_FAIL("ransac groups: %d groups: fewer than 2^24 are served", c.n_groups);
  const bool outputs = c.x && c.status && c.consensus && c.refit_x && c.refit_status && c.mean_error && c.winner && c.inlier;
  if (!c.slots || !c.x0 || !c.lb || !c.ub || !c.scale || !c.hyp_offset || !outputs ||
      (c.n_groups && (!c.group_control || !c.group_cam)))
    RANSAC_FAIL("ransac groups: null argument");
  if (c.draws && c.n_groups && (!c.group_id || !c.drawn)) RANSAC_FAIL("ransac groups: null argument: the groups' ids and drawn flags");
  if (!par_slots_ok("ransac groups", c, msg, cap)) return false;
  if (c.n < 1) RANSAC_FAIL("ransac groups: samples of %d rows", c.n);
  if (!par_options_ok("ransac groups", c, msg, cap)) return false;
  if (!(c.max_error == c.max_error)) RANSAC_FAIL("ransac groups: max_error is NaN");
  if (c.hyp_offset[0] != 0) RANSAC_FAIL("ransac groups: hyp_offset[0] is %lld, not 0", (long long)c.hyp_offset[0]);
  int64_t covered = 0, mask = 0;
  for (int g = 0; g < c.n_groups; ++g) {
    const int ctl = c.group_control[g];
    if (ctl < 0 || ctl >= t.n_controls) RANSAC_FAIL("ransac groups: group %d is control %d of %d", g, ctl, t.n_controls);
    if (t.kind[ctl] < GLH_CALIB_MATCHES)  // (the first of the three match kinds)
      RANSAC_FAIL("ransac groups: group %d is control %d, a POINTS or LINES control: the match kinds are served", g, ctl);
    if (g > 0 && ctl <= c.group_control[g - 1])
      RANSAC_FAIL("ransac groups: group %d is control %d after control %d: the groups name distinct controls in ascending order", g,
              ctl, c.group_control[g - 1]);
    const int cam = c.group_cam[g];
    if (cam < 0 || cam >= t.n_cams) RANSAC_FAIL("ransac groups: group %d fits camera %d of %d", g, cam, t.n_cams);
    if (cam != t.cam_a[ctl] && cam != t.cam_b[ctl])
      RANSAC_FAIL("ransac groups: group %d fits camera %d, which is neither camera (%d, %d) of its control", g, cam, t.cam_a[ctl],
              t.cam_b[ctl]);
    if (c.hyp_offset[g + 1] < c.hyp_offset[g] || c.hyp_offset[g + 1] >= RANSAC_MASK_LIMIT)
      RANSAC_FAIL("ransac groups: group %d ends at hypothesis %lld after %lld: not decreasing, fewer than 2^31 in all", g,
              (long long)c.hyp_offset[g + 1], (long long)c.hyp_offset[g]);
    const int64_t rows = table_rows(t, ctl), hyps = c.hyp_offset[g + 1] - c.hyp_offset[g];
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
    if (!par_block_ok("ransac groups", g, (size_t)g, c, msg, cap)) return false;
  }
  // every row of the handle gets its final byte from its group
  if (covered != t.row_offset[t.n_controls])
    RANSAC_FAIL("ransac groups: the groups hold %lld of the handle's %lld rows: every row belongs to exactly one group", (long long)covered,
            (long long)t.row_offset[t.n_controls]);
  if (mask >= RANSAC_MASK_LIMIT) RANSAC_FAIL("ransac groups: the consensus masks take 2^31 bytes or more: fewer are served in one call");
  const int64_t H = c.n_groups ? c.hyp_offset[c.n_groups] : 0;
  bool given = false;  // a group whose hypotheses come from `samples`
  for (int g = 0; g < c.n_groups; ++g) given = given || (!rg_drawn(c, g) && c.hyp_offset[g + 1] > c.hyp_offset[g]);
  if (given && !c.samples) RANSAC_FAIL("ransac groups: null samples");
  if (H > 0 && H > (RANSAC_MASK_LIMIT - 1) / c.n) RANSAC_FAIL("ransac groups: %lld samples of %d rows: fewer than 2^31 rows in all", (long long)H, c.n);
  for (int g = 0; g < c.n_groups; ++g) {
    if (rg_drawn(c, g)) continue;
    const int64_t first = t.row_offset[c.group_control[g]], last = t.row_offset[c.group_control[g] + 1];
    for (int64_t k = c.hyp_offset[g] * c.n; k < c.hyp_offset[g + 1] * c.n; ++k)
      if (c.samples[k] < first || c.samples[k] >= last)
        RANSAC_FAIL("ransac groups: hypothesis %lld of group %d samples row %lld outside its control's rows %lld .. %lld", (long long)(k / c.n),
                g, (long long)c.samples[k], (long long)first, (long long)last);
  }
  for (int g = 0; g < c.n_groups; ++g)
    if (t.kind[c.group_control[g]] == GLH_CALIB_ROTATION && !c.observed && table_rows(t, c.group_control[g]) > 0)
      RANSAC_FAIL("ransac groups: control %d is a ROTATION control, whose obs are camera coordinates: pass observed", c.group_control[g]);
  return true;
}
#undef RANSAC_FAIL

}  // namespace glh
