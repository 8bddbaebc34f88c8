// glh_calib.h -- what glimpse_hip.hip (the C ABI: glh_calib_create / _eval / _fit_sets / _ransac_groups / _destroy) hands to glh_calib.hip (the
// predictions of the controls of optimize.Cameras -- Points, Lines and the match classes -- under many sets of camera
// vectors at once): one struct per call, filled once from the ABI's arguments, checked on the host (glh_ransac_plan.h:
// fs_check for CalibFit, rg_check for CalibRansac; CalibPar is what the two have in common) and served from.  Host-only
// declarations without a HIP header, so that the checks compile for the CPU too.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct glh_calib;  // the C ABI's handle: the uploaded controls (glh_calib.hip)

namespace glh {

constexpr int CAL_TIMES = 5;   // entries of times_ms (include/glimpse_hip.h)
constexpr int CAL_TB = 256;    // threads of a workgroup, all three kernels
constexpr int CAL_TILE = 256;  // projected points of a Lines job held in LDS at a time (tests/calib_restated.py: TILE)
constexpr int CAL_FIT_TIMES = 4;  // entries of glh_calib_fit_sets' times_ms
constexpr int CAL_FIT_TB = 128;   // threads of k_fit_sets' workgroup: the rows of a set it takes at a time

struct CamDev;

struct CalibControls {
  int n_cams, n_controls;
  const int32_t *kind, *cam_a, *cam_b, *directions;  // [n_controls]
  const int64_t* row_offset;            // [n_controls + 1]
  const double* obs;                    // [N][2]
  const double* src;                    // [N][3]
};

struct CalibTable {  // what a handle keeps of its controls: an evaluation's jobs are checked against it
  int n_cams, n_controls;
  const int32_t* kind;        // [n_controls]
  const int64_t* row_offset;  // [n_controls + 1]
  const int32_t *cam_a, *cam_b;  // [n_controls]
};

struct CalibEval {
  int n_sets;
  const CamDev* cams;  // [n_sets][n_cams], expanded by the caller
  const double* rot;   // [n_sets][n_cams][9]
  int n_jobs;
  const int32_t *job_control, *job_set, *job_side;  // [n_jobs]
  const int64_t* job_seg;                           // [n_jobs + 1]
  const int64_t* seg_vertex;                        // [n_segments + 1]
  const int64_t* seg_count;                         // [n_segments]
  const double* seg_par;                            // [n_segments][5]
  const double* vertex;                             // [n_vertices][3]
  double* predicted;
  double* times_ms;
};

struct CalibPar {  // what a fit is started from and stopped by: one block of p values for glh_calib_fit_sets, one per group for the groups
  int p;
  const int32_t* slots;                // [p]
  const double *x0, *lb, *ub, *scale;  // [p] or [G][p]
  int max_nfev;
  double ftol, xtol, gtol;
};

struct CalibFit : CalibPar {  // glh_calib_fit_sets' arguments (include/glimpse_hip.h), checked by glh_ransac_plan.h's fs_check
  const CamDev* cams;     // [n_cams], expanded once the call is checked (glimpse_hip.hip)
  const double* vectors;  // [n_cams][GLH_CAM_LEN]
  int fit_cam;
  const double* weights;                 // [N][2] or null
  const double* observed;                // [N][2] or null: the handle's obs
  int n_sets;
  const int64_t *set_offset, *set_rows;  // [n_sets + 1], [set_offset[n_sets]]
  int score;
  double max_error;
  double* x;           // [n_sets][p]
  int32_t* status;     // [n_sets]
  double* mean_error;  // [n_sets]
  uint8_t* inlier;     // [n_sets][N] when score
  double* times_ms;
};

struct CalibRansac : CalibPar {  // glh_calib_ransac_groups' arguments (include/glimpse_hip.h), checked by glh_ransac_plan.h's rg_check
  const CamDev* cams;    // [n_cams], expanded once the call is checked (glimpse_hip.hip)
  const double* vectors; // [n_cams][GLH_CAM_LEN]
  int n_groups;
  const int32_t *group_control, *group_cam;  // [G]
  const double *weights, *observed;          // [N][2] or null
  const int64_t* hyp_offset;                 // [G + 1]
  int n;
  const int64_t* samples;                    // [H][n]
  double max_error;
  int64_t min_inliers;
  double* x;               // [H][p]
  int32_t* status;         // [H]
  int32_t* consensus;      // [H]
  double* refit_x;         // [H][p]
  int32_t* refit_status;   // [H]
  double* mean_error;      // [H]
  int32_t* winner;         // [G]
  uint8_t* inlier;         // [N]
  double* times_ms;
  // glh_calib_ransac_groups_drawn (`draws`; once checked: `drawn` is not null): a group with drawn[g] == 1 gets its samples
  // from k_rg_draw as pair group_id[g]'s (glh_ransac_draw.h), not from `samples`; times_ms then has RANSAC_DRAWN_TIMES entries
  bool draws = false;
  const int32_t* group_id = nullptr;   // [G]
  const uint8_t* drawn = nullptr;      // [G]
  uint32_t seed0 = 0, seed1 = 0;
  int64_t* samples_out = nullptr;      // [H][n] global rows of every hypothesis, or null
};

struct RansacDraw {  // glh_stage_ransac_samples' arguments (include/glimpse_hip.h), checked by the caller
  int device, n_groups;
  const int64_t* rows;        // [G]
  const int32_t* group_id;    // [G]
  const int64_t* hyp_offset;  // [G + 1]
  int n;
  uint32_t seed0, seed1;
  int64_t* samples;           // [H][n] rows within the group
  double* times_ms;           // [3] or null: upload, draw, download
};

// The arguments have been checked (glimpse_hip.hip).  A GLH_* status, with the message left for glh_last_error() on
// failure (glh_stage.h: fail).
int calib_create(int device, const CalibControls& c, glh_calib** out);
CalibTable calib_table(const glh_calib* h);
int calib_eval(glh_calib* h, const CalibEval& e);
int calib_fit_sets(glh_calib* h, const CalibFit& f);
int calib_ransac_groups(glh_calib* h, const CalibRansac& r);
int ransac_draw_samples(const RansacDraw& r);
void calib_destroy(glh_calib* h);

}  // namespace glh
