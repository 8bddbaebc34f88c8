// glh_calib.hip -- the residual function of optimize.Cameras (optimize.py:1721-1764) on the device: the work behind
// glh_calib_create / _eval / _destroy (include/glimpse_hip.h; glimpse_hip.hip validates the arguments).
//
// The reference loops over the controls in Python, once per residual evaluation, and the optimiser evaluates the residuals
// once per Jacobian column.  Here the controls are uploaded once and one call evaluates a list of JOBS: one control under
// one SET of camera vectors (the base set, or the set with one parameter perturbed).  The output is `predicted` of every
// job, concatenated in job order.
//
//   k_calib_rows, one thread per row of a Points or match job; a workgroup belongs to one job, so its cameras and their
//   flags are uniform.  Points: project_f (Camera.xyz_to_uv).  Matches: unproject of the other camera (Camera.uv_to_xyz,
//   ray directions), then project_f with CAM_F_DIRECTIONS: the two kernels Matches.predicted runs, back to back.
//   RotationMatches: the rays come from the uploaded camera coordinates by Camera._xy_to_xyz, term by term, with the
//   rotation matrix the caller made (NumPy's, as the host method uses); RotationMatchesXY stops at camera coordinates
//   (Camera._xyz_to_xy, again with the caller's matrix).
//
//   k_calib_line_points, one thread per projected point of a Lines job (Lines._xyzs_to_uvs, optimize.py:320-353).  The
//   caller has projected, split and clipped the world polylines (vertices, not pixels) and counted the points of each
//   clipped segment; the thread finds its segment by binary search over the job's point offsets, its distance by
//   np.linspace's rule, its vertex interval by np.interp's search and interpolates both camera coordinates by np.interp's
//   rule (glh_math.h), then applies Camera._distort and _xy_to_uv in the host method's operation order.
//
//   k_calib_nearest, one thread per observed point of a Lines job: the projected point of smallest dx dx + dy dy, the
//   first of equal ones, index 0 when no distance is smaller than +inf (np.argmin over cdist(..., "sqeuclidean")).  The
//   job's projected points stream through LDS in tiles of CAL_TILE; every thread scans all of them in index order, so no
//   reduction across lanes is needed and the answer does not depend on the launch shape.
//
// float64, no contraction (-ffp-contract=off), no atomics: two evaluations give the same bytes, and
// tests/calib_restated.py restates the Lines path in NumPy bit for bit.
//
// Both batched entry points fit one camera's parameters to a set of rows with ONE fit, team_fit: a damped Gauss-Newton
// run by a team of one or two waves, whose residuals and forward-difference columns come from calib_row, the device
// function k_calib_rows runs, under cameras rebuilt on the device from the stepped vector (team_evaluate); J^T J and
// J^T r are summed within each wave, then over the waves and the tiles in a fixed order; what to try, what to accept and
// when to stop is glh_lm.h's state machine, run by lane 0 and driven on the CPU by tests/hostcheck/ransac_hostcheck.cpp.
// Every loop is bounded.
//
// glh_calib_fit_sets (optimize.ransac(batched=True)) fits many sets of rows in one call:
//
//   k_fit_sets, one team of two waves per set, whose rows may span controls;
//
//   k_calib_score, one thread per (set, row) over all rows of the handle: |weighted residual| < max_error under the set's
//   fitted values; k_calib_members then marks the set's own rows.
//
// These are not NumPy's bits (the rotation matrix is the device's) and need not be: the values optimize.ransac returns
// come from the host's fit on the set the device picked.
//
// glh_calib_ransac_groups (optimize.ransac_pairs) runs the whole RANSAC of many one-camera models -- the groups of a
// handle -- in one pass: k_rg_fit, k_rg_score, k_rg_winner and k_rg_final, described where they stand below.
// glh_calib_ransac_groups_drawn puts k_rg_draw in front: the samples of the groups it names are drawn on the device
// (glh_ransac_draw.h), into the buffer the others read.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_calib.h"
#include "glh_lm.h"
#include "glh_ransac_draw.h"
#include "glh_ransac_plan.h"
#include "glh_stage.h"

namespace glh {
namespace {

struct CalJob {
  int64_t row0;  // the control's first row in the uploaded arrays
  int64_t out0;  // the job's first row in `predicted`
  int64_t puv0;  // (Lines) the job's first projected point
  int32_t kind, directions;
  int32_t cam_t, cam_o;  // target and other camera of the job's set, as indices into the expanded cameras
  int32_t side;          // (matches) 0: predict in the first camera from the second's points; 1: the reverse
  int32_t n_rows;
  int32_t seg0, n_segs;  // (Lines) the job's clipped segments
  int32_t n_puv, pad_;
};

struct CalSeg {
  double start, stop, step, delta, div;  // np.linspace's numbers (optimize.py: segment_table)
  int32_t v0, nv;                        // the segment's vertices
  int32_t p0, count;                     // its points, from p0 within the job
};

struct CalBlock {
  int32_t job, first;
};

// `predicted` of one row of a Points or match control: what k_calib_rows stores and what the fits and the scores take
// their residuals from (team_residual).  ct, co: the camera that predicts and the other one of a match; Rt, Ro: their
// rotation matrices as the ROTATION kinds multiply by them.
__device__ __forceinline__ void calib_row(int kind, int directions, int side, const CamDev& ct, const CamDev& co, const double* Rt,
                                          const double* Ro, const double2* __restrict__ obs, const double* __restrict__ src,
                                          size_t row, double& u, double& v) {
  const uint32_t ft = cam_flags(ct);
  if (kind == GLH_CALIB_POINTS) {
    project_f(ct, ft | (directions ? CAM_F_DIRECTIONS : 0u), src[3 * row], src[3 * row + 1], src[3 * row + 2], u, v);
  } else {
    // the other camera's points: the second side's are kept in src[.][0:2], the first side's are the observed ones
    const double x = side == 0 ? src[3 * row] : obs[row].x, y = side == 0 ? src[3 * row + 1] : obs[row].y;
    double d[3];
    if (kind == GLH_CALIB_MATCHES) {
      unproject(co, cam_flags(co), x, y, 1.0, 1, d);
    } else {
      for (int k = 0; k < 3; ++k) d[k] = (Ro[k] * x + Ro[3 + k] * y) + Ro[6 + k];  // Camera._xy_to_xyz (camera.py:1486-1492)
    }
    if (kind == GLH_CALIB_ROTATION_XY) {
      double c[3];  // Camera._xyz_to_xy (camera.py:1435-1470), directions
      for (int k = 0; k < 3; ++k) c[k] = Rt[3 * k] * d[0] + Rt[3 * k + 1] * d[1] + Rt[3 * k + 2] * d[2];
      u = c[0] / c[2];
      v = c[1] / c[2];
      if (c[2] <= 0.0) u = v = NAN;
    } else {
      project_f(ct, ft | CAM_F_DIRECTIONS, d[0], d[1], d[2], u, v);
    }
  }
}

__global__ void __launch_bounds__(CAL_TB) k_calib_rows(const CalBlock* __restrict__ blocks, const CalJob* __restrict__ jobs,
                                                       const CamDev* __restrict__ cams, const double* __restrict__ rot,
                                                       const double2* __restrict__ obs, const double* __restrict__ src,
                                                       double2* __restrict__ out) {
  const CalBlock b = blocks[blockIdx.x];
  const CalJob j = jobs[b.job];
  const int r = b.first + (int)threadIdx.x;
  if (r >= j.n_rows) return;
  double u, v;
  calib_row(j.kind, j.directions, j.side, cams[j.cam_t], cams[j.cam_o], rot + 9 * (size_t)j.cam_t, rot + 9 * (size_t)j.cam_o, obs,
            src, (size_t)j.row0 + r, u, v);
  out[(size_t)j.out0 + r] = make_double2(u, v);
}

__global__ void __launch_bounds__(CAL_TB) k_calib_line_points(const CalBlock* __restrict__ blocks, const CalJob* __restrict__ jobs,
                                                              const CamDev* __restrict__ cams, const CalSeg* __restrict__ segs,
                                                              const double* __restrict__ vx, const double* __restrict__ vy,
                                                              const double* __restrict__ vd, double2* __restrict__ puv) {
  const CalBlock b = blocks[blockIdx.x];
  const CalJob j = jobs[b.job];
  const int p = b.first + (int)threadIdx.x;
  if (p >= j.n_puv) return;
  // the last segment that starts at or before p (every segment holds at least one point)
  int lo = 0, hi = j.n_segs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (segs[j.seg0 + mid].p0 <= p)
      lo = mid;
    else
      hi = mid;
  }
  const CalSeg s = segs[j.seg0 + lo];
  const int i = p - s.p0;
  // np.linspace(start, stop, count): arange * step + start, the last value set to stop; a single point is start
  double t;
  if (s.count > 1 && i == s.count - 1) {
    t = s.stop;
  } else {
    const double a = (double)i;
    t = s.count == 1 ? a * s.delta : (s.step != 0.0 ? a * s.step : (a / s.div) * s.delta);
    t = t + s.start;
  }
  const int q = np_interp_find(t, vd + s.v0, s.nv);
  const double x = np_interp_at(q, t, vd + s.v0, vx + s.v0, s.nv), y = np_interp_at(q, t, vd + s.v0, vy + s.v0, s.nv);
  // Camera._distort (camera.py:1180-1196) and _xy_to_uv (:1499-1508)
  const CamDev& c = cams[j.cam_t];
  const uint32_t f = cam_flags(c);
  double qx = x, qy = y;
  if (f & (CAM_F_ANYK | CAM_F_ANYP)) {
    const double r2 = x * x + y * y;
    if (f & CAM_F_ANYK) {
      const double dr = radial_factor(c, f, r2);
      qx = x * dr;
      qy = y * dr;
    }
    if (f & CAM_F_ANYP) {
      double dtx, dty;
      tangential_terms(c, x, y, r2, dtx, dty);
      qx = qx + dtx;
      qy = qy + dty;
    }
  }
  puv[(size_t)j.puv0 + p] = make_double2(qx * c.f[0] + c.off[0], qy * c.f[1] + c.off[1]);
}

__global__ void __launch_bounds__(CAL_TB) k_calib_nearest(const CalBlock* __restrict__ blocks, const CalJob* __restrict__ jobs,
                                                          const double2* __restrict__ obs, const double2* __restrict__ puv,
                                                          double2* __restrict__ out) {
  static_assert(CAL_TILE == CAL_TB, "one projected point per thread and tile");
  __shared__ double2 s_p[CAL_TILE];
  const CalBlock b = blocks[blockIdx.x];
  const CalJob j = jobs[b.job];
  const int r = b.first + (int)threadIdx.x;
  const bool live = r < j.n_rows;
  const double2 o = live ? obs[(size_t)j.row0 + r] : make_double2(0.0, 0.0);
  const double2* __restrict__ pj = puv + (size_t)j.puv0;
  double best = INFINITY;
  int index = 0;
  for (int base = 0; base < j.n_puv; base += CAL_TILE) {
    const int n = j.n_puv - base < CAL_TILE ? j.n_puv - base : CAL_TILE;
    __syncthreads();
    if ((int)threadIdx.x < n) s_p[threadIdx.x] = pj[base + threadIdx.x];
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const double dx = o.x - s_p[k].x, dy = o.y - s_p[k].y;
      const double d = dx * dx + dy * dy;
      if (d < best) {
        best = d;
        index = base + k;
      }
    }
  }
  if (live) out[(size_t)j.out0 + r] = pj[index];
}

// ---- the team fit: a team of one or two waves fits the fitted camera's parameters to one set of rows -------------------
struct CalCtl {
  int32_t kind, directions, cam_a, cam_b;
};

// What every fit and every score is given, whichever entry point it serves.  The fits hold one wave per SIMD and reload
// kernel arguments in the tile loop, where nothing hides a scalar load: the order keeps src .. weights, and RArgs' x0 ..
// scale behind this struct, each within one 64-byte line and the first on a 16-byte boundary (measured on the refits of
// tools/ransac_pairs_probe.py: 0.7 % of their time).
struct FitBase {
  const CamDev* cams;        // [n_cams] the cameras at their own vectors
  const CalCtl* ctl;         // [n_controls]
  int32_t p, max_nfev;
  const double2* obs;
  const double* src;
  const double2* observed;   // [N] what the predictions are compared with: obs, or the caller's
  const double2* weights;    // [N], or null
  double ftol, xtol, gtol;
  int32_t slot[LM_MAX_P];
};

// What a team works on: the fitted camera and its parameters, its set of rows -- a list, or the rows row0 + k, k < n,
// whose mask byte is not 0 -- and the rows' control: one for all of them (c, kept in registers), or the one row_ctl names
// for each (a set that spans controls).
struct Team {
  const double *x0, *lb, *ub, *scale;  // [p]
  const double* base;                  // [GLH_CAM_LEN] the fitted camera's vector
  const int32_t* rows;
  const uint8_t* mask;
  const int32_t* row_ctl;              // [N], or null
  int64_t row0;
  CalCtl c;
  int32_t fit_cam, n;
};

// A team's LDS.  MAXP: the instantiation's largest p; TW: the team's waves.
template <int MAXP, int TW>
struct FitShared {
  static constexpr int E = MAXP * (MAXP + 1) / 2 + MAXP + 4;  // lm_sums(MAXP)
  CamDev cam[MAXP + 1];               // the fitted camera at the point and with each parameter stepped
  double vec[MAXP + 1][GLH_CAM_LEN];
  double J[2][MAXP + 1][TW * 64];     // [u, v][column, the last is r][lane]: a lane reads its own entries only
  double part[TW][E];                 // the waves' sums of one tile
  double acc[E];                      // the sums of the last evaluation
  LmState<MAXP> lm;
};
static_assert(sizeof(FitShared<LM_MAX_P, 2>) <= 64 * 1024, "the largest team's LDS");

// glh_host.h's expand_camera (camera.py:239-280) on the device, for a camera that is not a raster grid: the rotation
// matrix comes from the device's own cos and sin, so it is not NumPy's to the bit (the values that leave optimize.ransac
// come from the host's fit).
__device__ void camera_from_vector(const double* v, CamDev* c) {
  const double d2r = M_PI / 180.0;
  double C[3], S[3];
  for (int i = 0; i < 3; ++i) {
    const double r = v[3 + i] * d2r;
    C[i] = cos(r);
    S[i] = sin(r);
    c->xyz[i] = v[i];
  }
  c->R[0] = C[0] * C[2] + S[0] * S[1] * S[2];
  c->R[1] = C[0] * S[1] * S[2] - C[2] * S[0];
  c->R[2] = -C[1] * S[2];
  c->R[3] = C[2] * S[0] * S[1] - C[0] * S[2];
  c->R[4] = S[0] * S[2] + C[0] * C[2] * S[1];
  c->R[5] = -C[1] * C[2];
  c->R[6] = C[1] * S[0];
  c->R[7] = C[0] * C[1];
  c->R[8] = S[1];
  for (int i = 0; i < 2; ++i) {
    c->imgsz[i] = v[6 + i];
    c->f[i] = v[8 + i];
    c->off[i] = v[6 + i] / 2 + v[10 + i];
    c->p[i] = v[18 + i];
  }
  c->any_k = c->any_kden = 0;
  for (int i = 0; i < 6; ++i) {
    c->k[i] = v[12 + i];
    if (v[12 + i] != 0.0) {
      c->any_k = 1;
      if (i >= 3) c->any_kden = 1;
    }
  }
  c->any_p = (c->p[0] != 0.0 || c->p[1] != 0.0) ? 1 : 0;
  c->has_corr = v[20] != 0.0;
  c->radius = v[21];
  c->refraction = v[22];
  c->is_grid = 0;
  c->pad_ = 0;
}

// Between the lanes of a team: a wave's LDS accesses execute in order, so one wave needs the compiler's fence alone.
template <int TW>
__device__ __forceinline__ void team_sync() {
  if (TW == 1) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// The weighted residual of global row `row` with `fitted` in the fitted camera's place.
__device__ __forceinline__ void team_residual(const FitBase& a, const Team& w, const CamDev& fitted, size_t row, double& ru,
                                              double& rv) {
  CalCtl c = w.c;
  if (w.row_ctl) c = a.ctl[w.row_ctl[row]];
  const CamDev& ct = c.cam_a == w.fit_cam ? fitted : a.cams[c.cam_a];
  const CamDev& co = c.cam_b == w.fit_cam ? fitted : a.cams[c.cam_b];
  double u, v;
  calib_row(c.kind, c.directions, 0, ct, co, ct.R, co.R, a.obs, a.src, row, u, v);
  const double2 o = a.observed[row];
  ru = u - o.x;
  rv = v - o.y;
  if (a.weights) {
    const double2 wt = a.weights[row];
    ru = ru * wt.x;
    rv = rv * wt.y;
  }
}

// The sum over the wave, in the order of the butterfly: every lane ends with the same bits.
__device__ __forceinline__ double wave_sum(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// s.acc = the evaluation (glh_lm.h) of the team's set at the point xe: A = J^T J (packed), g = J^T r, sum r r, the rows
// that count, sum |r| and the members, J in scaled variables by forward differences.  A row whose prediction is NaN at the
// point or at a stepped point adds nothing.  Each sum is taken within the wave, then over the waves and the tiles in
// order.  t: the lane within the team.  Every lane of the team calls this.
template <int MAXP, int TW>
__device__ void team_evaluate(const FitBase& a, const Team& w, FitShared<MAXP, TW>& s, const double* xe, int t) {
  constexpr int TT = TW * 64, E = FitShared<MAXP, TW>::E, Q = (E + TT - 1) / TT;
  const int p = a.p;
  const int nE = lm_sums(p);
  team_sync<TW>();  // (xe is written, the last evaluation's sums are read)
  if (t <= p) {
    double* v = s.vec[t];
    for (int k = 0; k < GLH_CAM_LEN; ++k) v[k] = w.base[k];
    for (int i = 0; i < p; ++i) v[a.slot[i]] = xe[i];
    if (t > 0) {
      const int i = t - 1;
      const double stepped = xe[i] + lm_fd_step(xe[i], w.lb[i], w.ub[i]);
      v[a.slot[i]] = stepped;
      s.lm.dx[i] = stepped - xe[i];
    }
    camera_from_vector(v, &s.cam[t]);
  }
  team_sync<TW>();
  double sum[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) sum[q] = 0.0;
  const int wave = t >> 6, lane = t & 63;
  for (int first = 0; first < w.n; first += TT) {
    const int k = first + t;
    bool member = k < w.n;
    size_t row = 0;
    if (member) {
      if (w.rows) {
        row = (size_t)w.rows[k];
      } else {
        row = (size_t)w.row0 + k;
        member = w.mask[k] != 0;
      }
    }
    bool ok = member;
    double ru = 0.0, rv = 0.0;
    if (ok) {
      team_residual(a, w, s.cam[0], row, ru, rv);
      ok = !(isnan(ru) || isnan(rv));
      for (int j = 0; j < p; ++j) {
        double su, sv;
        team_residual(a, w, s.cam[j + 1], row, su, sv);
        const double ju = (su - ru) / s.lm.dx[j] * w.scale[j], jv = (sv - rv) / s.lm.dx[j] * w.scale[j];
        ok = ok && !(isnan(ju) || isnan(jv));
        s.J[0][j][t] = ju;
        s.J[1][j][t] = jv;
      }
    }
    if (!ok) {
      ru = rv = 0.0;
      for (int j = 0; j < p; ++j) s.J[0][j][t] = s.J[1][j][t] = 0.0;
    }
    s.J[0][p][t] = ru;
    s.J[1][p][t] = rv;
    int e = 0;
    for (int i = 0; i < p; ++i)  // A's upper triangle row by row (lm_tri), then g: column p is r
      for (int j = i; j < p; ++j, ++e) {
        const double v = wave_sum(s.J[0][i][t] * s.J[0][j][t] + s.J[1][i][t] * s.J[1][j][t]);
        if (lane == 0) s.part[wave][e] = v;
      }
    for (int i = 0; i <= p; ++i, ++e) {  // (the last of these is sum r r)
      const double v = wave_sum(s.J[0][i][t] * ru + s.J[1][i][t] * rv);
      if (lane == 0) s.part[wave][e] = v;
    }
    {
      const double c = wave_sum(ok ? 1.0 : 0.0), h = wave_sum(ok ? hypot(ru, rv) : 0.0), m = wave_sum(member ? 1.0 : 0.0);
      if (lane == 0) s.part[wave][e] = c, s.part[wave][e + 1] = h, s.part[wave][e + 2] = m;
    }
    team_sync<TW>();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int i = t + q * TT;
      if (i < nE) {
        double v = s.part[0][i];
        for (int k2 = 1; k2 < TW; ++k2) v += s.part[k2][i];
        sum[q] += v;
      }
    }
    team_sync<TW>();
  }
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (t + q * TT < nE) s.acc[t + q * TT] = sum[q];
  team_sync<TW>();
}

// The fit's state as every lane of the team sees it between two writes of lane 0.
template <int MAXP, int TW>
__device__ __forceinline__ int team_state(FitShared<MAXP, TW>& s) {
  team_sync<TW>();
  const int v = s.lm.state;
  team_sync<TW>();
  return v;
}

// The damped Gauss-Newton of one team on its set: the team evaluates, lane 0 decides (glh_lm.h) and leaves the values, the
// status and, where asked for, the mean error over the set's rows.
template <int MAXP, int TW>
__device__ void team_fit(const FitBase& a, const Team& w, FitShared<MAXP, TW>& s, int t, double* x, int32_t* status,
                         double* mean_error) {
  const int p = a.p;
  if (t == 0) lm_begin(s.lm, p, w.x0);
  team_evaluate<MAXP, TW>(a, w, s, s.lm.x, t);
  if (t == 0) lm_first(s.lm, p, s.acc);
  for (int it = 0; it < a.max_nfev; ++it) {  // one trial step per round: bounded, whatever the residuals do
    if (team_state<MAXP, TW>(s) != LM_RUNNING) break;
    if (t == 0) lm_propose(s.lm, p, w.lb, w.ub, w.scale, a.gtol);
    if (team_state<MAXP, TW>(s) != LM_RUNNING) break;
    team_evaluate<MAXP, TW>(a, w, s, s.lm.xt, t);
    if (t == 0) lm_judge(s.lm, p, w.scale, s.acc, a.ftol, a.xtol);
  }
  team_sync<TW>();
  if (t == 0) {
    for (int i = 0; i < p; ++i) x[i] = s.lm.x[i];
    *status = lm_finish(s.lm, mean_error);
  }
}

// The fitted camera at the values x, by thread 0 into LDS (the caller synchronises).
__device__ __forceinline__ void fitted_camera(const FitBase& a, const double* base, const double* x, double* vec, CamDev* cam) {
  for (int k = 0; k < GLH_CAM_LEN; ++k) vec[k] = base[k];
  for (int i = 0; i < a.p; ++i) vec[a.slot[i]] = x[i];
  camera_from_vector(vec, cam);
}

// The instantiation's largest p: 3 (a view direction) or everything.
constexpr int FIT_SMALL_P = 3;

// ---- glh_calib_fit_sets: one team of two waves per set; a set may span controls ---------------------------------------
struct SetArgs : FitBase {
  const int32_t* row_ctl;      // [N] the control of every row
  const int64_t* set_offset;   // [S + 1]
  const int32_t* set_rows;
  const double* par;           // x0, lb, ub, scale [p] each, then the fitted camera's vector
  double* x;                   // [S][p]
  int32_t* status;             // [S]
  double* mean_error;          // [S]
  int32_t fit_cam, n_rows;
};

// The team of every set of the call, its rows apart.
__device__ __forceinline__ Team set_team(const SetArgs& a) {
  Team w{};
  w.x0 = a.par, w.lb = a.par + a.p, w.ub = a.par + 2 * a.p, w.scale = a.par + 3 * a.p, w.base = a.par + 4 * a.p;
  w.row_ctl = a.row_ctl;
  w.fit_cam = a.fit_cam;
  return w;
}

// The tile is 128 rows for every p: the tile width fixes the order of the sums, and so the bytes.
template <int MAXP>
__global__ void __launch_bounds__(CAL_FIT_TB) k_fit_sets(const SetArgs a) {
  static_assert(CAL_FIT_TB == 2 * 64, "a team of two waves");
  __shared__ FitShared<MAXP, 2> s;
  const int set = (int)blockIdx.x;
  Team w = set_team(a);
  w.rows = a.set_rows + a.set_offset[set];
  w.n = (int)(a.set_offset[set + 1] - a.set_offset[set]);
  team_fit<MAXP, 2>(a, w, s, (int)threadIdx.x, a.x + (size_t)set * a.p, a.status + set, a.mean_error + set);
}

// inlier[set][row] = |weighted residual| < max_error under the set's fitted values, for every row of the handle: one
// thread per (set, row), a workgroup within one set.  NaN is no inlier; a set whose fit failed has none.
__global__ void __launch_bounds__(CAL_TB) k_calib_score(const SetArgs a, int blocks_per_set, double max_error,
                                                        uint8_t* __restrict__ inlier) {
  __shared__ CamDev cam;
  __shared__ double vec[GLH_CAM_LEN];
  const int set = (int)(blockIdx.x / (unsigned)blocks_per_set);
  const int row = (int)(blockIdx.x % (unsigned)blocks_per_set) * CAL_TB + (int)threadIdx.x;
  const Team w = set_team(a);
  if (threadIdx.x == 0) fitted_camera(a, w.base, a.x + (size_t)set * a.p, vec, &cam);
  __syncthreads();
  if (row >= a.n_rows) return;
  uint8_t in = 0;
  if (a.status[set] > 0) {
    double ru, rv;
    team_residual(a, w, cam, (size_t)row, ru, rv);
    in = hypot(ru, rv) < max_error ? 1 : 0;
  }
  inlier[(size_t)set * a.n_rows + row] = in;
}

// The set's own rows are its members (2), whatever their error: after k_calib_score on the same stream.
__global__ void __launch_bounds__(CAL_TB) k_calib_members(const SetArgs a, uint8_t* __restrict__ inlier) {
  const int set = (int)blockIdx.x;
  const int64_t first = a.set_offset[set], last = a.set_offset[set + 1];
  for (int64_t k = first + threadIdx.x; k < last; k += CAL_TB) inlier[(size_t)set * a.n_rows + a.set_rows[k]] = 2;
}

// ---- glh_calib_ransac_groups: RANSAC over many groups in one pass --------------------------------------------------------
// A group is one match control with one of its cameras fitted (glh_ransac_plan.h).  Four steps on one stream, nothing read
// back in between:
//
//   k_rg_draw (glh_calib_ransac_groups_drawn alone), one thread per hypothesis of a drawn group: its sample, written into
//   the buffer of samples before anything reads it (described where it stands, after the others);
//   k_rg_fit (hypotheses), one TEAM per sample of n rows: a team is one wave when n <= 64 -- several teams to a workgroup,
//   the wave's butterfly is then the whole reduction and no workgroup barrier is used -- and a workgroup of two waves
//   beyond.  The fit is team_fit, the one k_fit_sets runs; camera, start, bounds and scales are the group's, and the
//   control is the group's for every row.
//   k_rg_score, one workgroup per hypothesis over the rows of ITS group: the mask byte (1: error < max_error, 2: a row of
//   the sample) stays on the device, the count of 1s is the consensus.
//   k_rg_fit (refits), one workgroup per hypothesis with status > 0 and consensus > min_inliers: it walks its group's rows
//   in order and skips those whose mask byte is 0, so equal sets give equal bytes.
//   k_rg_winner, one thread per group: the valid refit of smallest mean error, the earlier one of equal ones;
//   k_rg_final, one workgroup per group: error <= max_error of every row under the winner's refitted values.
struct RGroup {
  int64_t row0;   // the group's first row in the handle
  int64_t mask0;  // the first mask byte of its first hypothesis
  int32_t n_rows, ctl, fit_cam, hyp0, n_hyp, pad_;
};

struct RArgs : FitBase {
  const double *x0, *lb, *ub, *scale;  // [G][p]
  const double* vectors;     // [n_cams][GLH_CAM_LEN]
  const RGroup* groups;      // [G]
  const int32_t* hyp_group;  // [H]
  const int32_t* samples;    // [H][n] global rows
  uint8_t* mask;
  double* x;                 // [H][p]
  double* refit_x;           // [H][p]
  double* mean_error;        // [H]
  int32_t *status, *consensus, *refit_status;  // [H]
  int32_t* winner;           // [G]
  uint8_t* inlier;           // [N]
  int32_t n, n_hyp, n_groups, min_inliers;
  double max_error;
};

// The team of group gi, its set of rows apart.
__device__ __forceinline__ Team group_team(const RArgs& a, int gi, const RGroup& g) {
  Team w{};
  w.x0 = a.x0 + (size_t)gi * a.p, w.lb = a.lb + (size_t)gi * a.p, w.ub = a.ub + (size_t)gi * a.p;
  w.scale = a.scale + (size_t)gi * a.p;
  w.base = a.vectors + (size_t)g.fit_cam * GLH_CAM_LEN;
  w.row0 = g.row0;
  w.c = a.ctl[g.ctl];
  w.fit_cam = g.fit_cam;
  return w;
}

// refit == 0: hypothesis h is fitted to its sample; refit != 0: to sample and consensus, if it was accepted.
template <int MAXP, int TW, int TEAMS>
__global__ void __launch_bounds__(TW * 64 * TEAMS) k_rg_fit(const RArgs a, int refit) {
  static_assert(TW == 1 || TEAMS == 1, "teams that share a workgroup must not meet at a workgroup barrier");
  __shared__ FitShared<MAXP, TW> sh[TEAMS];
  const int team = (int)threadIdx.x / (TW * 64), t = (int)threadIdx.x % (TW * 64);
  const int h = (int)blockIdx.x * TEAMS + team;
  if (h >= a.n_hyp) return;
  const int gi = a.hyp_group[h];
  const RGroup g = a.groups[gi];
  Team w = group_team(a, gi, g);
  if (!refit) {
    w.rows = a.samples + (size_t)h * a.n, w.n = a.n;
    team_fit<MAXP, TW>(a, w, sh[team], t, a.x + (size_t)h * a.p, a.status + h, nullptr);
    return;
  }
  if (!(a.status[h] > 0 && a.consensus[h] > a.min_inliers)) {
    if (t == 0) {
      for (int i = 0; i < a.p; ++i) a.refit_x[(size_t)h * a.p + i] = NAN;
      a.refit_status[h] = RANSAC_NOT_REFITTED;
      a.mean_error[h] = NAN;
    }
    return;
  }
  w.mask = a.mask + g.mask0 + (size_t)(h - g.hyp0) * g.n_rows, w.n = g.n_rows;
  team_fit<MAXP, TW>(a, w, sh[team], t, a.refit_x + (size_t)h * a.p, a.refit_status + h, a.mean_error + h);
}

__global__ void __launch_bounds__(CAL_TB) k_rg_score(const RArgs a) {
  __shared__ CamDev cam;
  __shared__ double vec[GLH_CAM_LEN];
  __shared__ int32_t count;
  const int h = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int gi = a.hyp_group[h];
  const RGroup g = a.groups[gi];
  const Team w = group_team(a, gi, g);
  uint8_t* __restrict__ m = a.mask + g.mask0 + (size_t)(h - g.hyp0) * g.n_rows;
  const bool fitted = a.status[h] > 0;  // (a hypothesis whose fit failed has no consensus)
  if (tid == 0) {
    count = 0;
    fitted_camera(a, w.base, a.x + (size_t)h * a.p, vec, &cam);
  }
  __syncthreads();
  for (int k = tid; k < g.n_rows; k += CAL_TB) {
    uint8_t in = 0;
    if (fitted) {
      double ru, rv;
      team_residual(a, w, cam, (size_t)g.row0 + k, ru, rv);
      in = hypot(ru, rv) < a.max_error ? 1 : 0;
    }
    m[k] = in;
  }
  __syncthreads();
  if (fitted)
    for (int k = tid; k < a.n; k += CAL_TB) m[(int64_t)a.samples[(size_t)h * a.n + k] - g.row0] = 2;
  __syncthreads();
  int local = 0;
  for (int k = tid; k < g.n_rows; k += CAL_TB) local += m[k] == 1 ? 1 : 0;
  for (int s = 32; s >= 1; s >>= 1) local += __shfl_xor(local, s);
  if ((tid & 63) == 0) atomicAdd(&count, local);
  __syncthreads();
  if (tid == 0) a.consensus[h] = count;
}

__global__ void __launch_bounds__(CAL_TB) k_rg_winner(const RArgs a) {
  const int gi = (int)(blockIdx.x * CAL_TB + threadIdx.x);
  if (gi >= a.n_groups) return;
  const RGroup g = a.groups[gi];
  int best = -1;
  double least = 0.0;
  for (int k = 0; k < g.n_hyp; ++k) {
    const double mean = a.mean_error[g.hyp0 + k];
    if (a.refit_status[g.hyp0 + k] > 0 && mean == mean && (best < 0 || mean < least)) best = k, least = mean;
  }
  a.winner[gi] = best;
}

__global__ void __launch_bounds__(CAL_TB) k_rg_final(const RArgs a) {
  __shared__ CamDev cam;
  __shared__ double vec[GLH_CAM_LEN];
  const int gi = (int)blockIdx.x, tid = (int)threadIdx.x;
  const RGroup g = a.groups[gi];
  const Team w = group_team(a, gi, g);
  const int win = a.winner[gi];
  if (tid == 0 && win >= 0) fitted_camera(a, w.base, a.refit_x + (size_t)(g.hyp0 + win) * a.p, vec, &cam);
  __syncthreads();
  for (int k = tid; k < g.n_rows; k += CAL_TB) {
    uint8_t in = 0;
    if (win >= 0) {
      double ru, rv;
      team_residual(a, w, cam, (size_t)g.row0 + k, ru, rv);
      in = hypot(ru, rv) <= a.max_error ? 1 : 0;
    }
    a.inlier[(size_t)g.row0 + k] = in;
  }
}

// One thread per hypothesis of a drawn group (`drawn` null: every group): it builds its sample in its own row of
// `samples` by glh_ransac_draw.h's rd_draw, as hypothesis h - hyp0 of pair group_id[g] with the group's row count, in
// global row numbers.  No thread reads what another writes; hypotheses of groups that are not drawn are left as uploaded.
struct DrawArgs {
  const RGroup* groups;      // [G]
  const int32_t* hyp_group;  // [H]
  const int32_t* group_id;   // [G]
  const uint8_t* drawn;      // [G] or null
  int32_t* samples;          // [H][n]
  int32_t n, n_hyp;
  uint32_t seed0, seed1;
};

__global__ void __launch_bounds__(CAL_TB) k_rg_draw(const DrawArgs a) {
  const int64_t h = (int64_t)blockIdx.x * CAL_TB + threadIdx.x;
  if (h >= a.n_hyp) return;
  const int gi = a.hyp_group[h];
  if (a.drawn && !a.drawn[gi]) return;
  const RGroup g = a.groups[gi];
  rd_draw(a.seed0, a.seed1, (uint32_t)a.group_id[gi], (uint32_t)((int32_t)h - g.hyp0), (uint32_t)g.n_rows, a.n, (int32_t)g.row0,
          a.samples + (size_t)h * a.n);
}

}  // namespace
}  // namespace glh

struct glh_calib : glh::DeviceObject {
  int n_cams = 0, n_controls = 0;
  std::vector<int32_t> kind, cam_a, cam_b, directions;
  std::vector<int64_t> row_offset;
  glh::DevBuf obs, src;
  glh::GrowBuf in, puv, out;  // (they only grow: the evaluations of a fit are all of one size)
  glh::StageEvents<glh::CAL_TIMES + 1> ev;
  std::vector<char> stage;
  // the batched fit (calib_fit_sets): the control of every row and the controls' table, uploaded with the controls
  glh::DevBuf ctl, row_ctl;
  glh::GrowBuf fit_in, fit_out;
  glh::StageEvents<glh::CAL_FIT_TIMES + 1> fit_ev;
  // RANSAC over groups (calib_ransac_groups): its buffers, the masks apart, and its events, made by the first call
  glh::GrowBuf rg_in, rg_out, rg_mask;
  glh::StageEvents<glh::RANSAC_DRAWN_TIMES + 1> rg_ev;  // (the last one: after the draw)
  bool rg_ready = false;
};

namespace glh {

static int calib_fill(glh_calib* h, const CalibControls& c) {
  h->n_cams = c.n_cams, h->n_controls = c.n_controls;
  h->kind.assign(c.kind, c.kind + c.n_controls);
  h->cam_a.assign(c.cam_a, c.cam_a + c.n_controls);
  h->cam_b.assign(c.cam_b, c.cam_b + c.n_controls);
  h->directions.assign(c.directions, c.directions + c.n_controls);
  h->row_offset.assign(c.row_offset, c.row_offset + c.n_controls + 1);
  const size_t N = (size_t)c.row_offset[c.n_controls];
  CHK(h->ev.create());
  const double none[3] = {0.0, 0.0, 0.0};
  CHK(h->obs.up(N ? c.obs : none, (N ? N : 1) * 16));
  CHK(h->src.up(N ? c.src : none, (N ? N : 1) * 24));
  CHK(h->fit_ev.create());
  std::vector<CalCtl> ctl((size_t)c.n_controls + 1);  // (one more: an empty table still has an address)
  std::vector<int32_t> row_ctl(N ? N : 1, 0);
  for (int k = 0; k < c.n_controls; ++k) {
    ctl[k] = CalCtl{c.kind[k], c.directions[k], c.cam_a[k], c.cam_b[k]};
    for (int64_t r = c.row_offset[k]; r < c.row_offset[k + 1]; ++r) row_ctl[(size_t)r] = k;
  }
  CHK(h->ctl.up(ctl.data(), ctl.size() * sizeof(CalCtl)));
  CHK(h->row_ctl.up(row_ctl.data(), row_ctl.size() * sizeof(int32_t)));
  return GLH_OK;
}

int calib_create(int device, const CalibControls& c, glh_calib** out) {
  return create_object("calib", device, out, [&](glh_calib* h) { return calib_fill(h, c); });
}

CalibTable calib_table(const glh_calib* h) {
  return CalibTable{h->n_cams, h->n_controls, h->kind.data(), h->row_offset.data(), h->cam_a.data(), h->cam_b.data()};
}

int calib_eval(glh_calib* h, const CalibEval& e) {
  CHK(h->use());
  hipStream_t s = h->stream;
  const size_t n_cam_sets = (size_t)e.n_sets * h->n_cams;
  const size_t S = (size_t)e.job_seg[e.n_jobs], V = (size_t)e.seg_vertex[S];
  // the jobs, the workgroups of the three kernels and the segment table, in one staging buffer
  std::vector<CalJob> jobs((size_t)e.n_jobs);
  std::vector<CalSeg> segs(S);
  std::vector<CalBlock> rows_b, points_b, nearest_b;
  int64_t out_rows = 0, puv_total = 0;
  for (int q = 0; q < e.n_jobs; ++q) {
    const int c = e.job_control[q];
    CalJob& j = jobs[q];
    j.row0 = h->row_offset[c];
    j.out0 = out_rows;
    j.puv0 = puv_total;
    j.kind = h->kind[c];
    j.directions = h->directions[c];
    j.side = e.job_side[q];
    const int base = e.job_set[q] * h->n_cams;
    j.cam_t = base + (j.side == 0 ? h->cam_a[c] : h->cam_b[c]);
    j.cam_o = base + (j.side == 0 ? h->cam_b[c] : h->cam_a[c]);
    j.n_rows = (int32_t)(h->row_offset[c + 1] - h->row_offset[c]);
    j.seg0 = (int32_t)e.job_seg[q];
    j.n_segs = (int32_t)(e.job_seg[q + 1] - e.job_seg[q]);
    j.pad_ = 0;
    int32_t n_puv = 0;
    for (int64_t k = e.job_seg[q]; k < e.job_seg[q + 1]; ++k) {
      CalSeg& g = segs[(size_t)k];
      const double* par = e.seg_par + 5 * k;
      g.start = par[0], g.stop = par[1], g.step = par[2], g.delta = par[3], g.div = par[4];
      g.v0 = (int32_t)e.seg_vertex[k];
      g.nv = (int32_t)(e.seg_vertex[k + 1] - e.seg_vertex[k]);
      g.p0 = n_puv;
      g.count = (int32_t)e.seg_count[k];
      n_puv += g.count;
    }
    j.n_puv = n_puv;
    for (int first = 0; first < j.n_rows; first += CAL_TB)
      (j.kind == GLH_CALIB_LINES ? nearest_b : rows_b).push_back(CalBlock{q, first});
    for (int first = 0; first < n_puv; first += CAL_TB) points_b.push_back(CalBlock{q, first});
    out_rows += j.n_rows;
    puv_total += n_puv;
  }
  Stage in(h->stage);
  const auto i_cams = in.put<const CamDev>(e.cams, n_cam_sets);
  const auto i_rot = in.put<const double>(e.rot, n_cam_sets * 9);
  const auto i_jobs = in.put<const CalJob>(jobs.data(), jobs.size());
  const auto i_segs = in.put<const CalSeg>(segs.data(), segs.size());
  const auto i_rows = in.put<const CalBlock>(rows_b.data(), rows_b.size()), i_points = in.put<const CalBlock>(points_b.data(), points_b.size()),
             i_nearest = in.put<const CalBlock>(nearest_b.data(), nearest_b.size());
  const auto i_vx = in.room<double>(V), i_vy = in.room<double>(V), i_vd = in.room<double>(V);
  double *vx = in.host(i_vx), *vy = in.host(i_vy), *vd = in.host(i_vd);
  for (size_t k = 0; k < V; ++k) vx[k] = e.vertex[3 * k], vy[k] = e.vertex[3 * k + 1], vd[k] = e.vertex[3 * k + 2];

  CHK(h->in.reserve(in.bytes()));
  CHK(h->puv.reserve((size_t)(puv_total ? puv_total : 1) * 16));
  CHK(h->out.reserve((size_t)(out_rows ? out_rows : 1) * 16));
  CHK(h->ev.record(0, s));
  HIPCHK(hipMemcpy(h->in.p, in.hold(), in.bytes(), hipMemcpyHostToDevice));
  CHK(h->ev.record(1, s));
  void* d = h->in.p;
  if (!rows_b.empty()) {
    hipLaunchKernelGGL(k_calib_rows, dim3((unsigned)rows_b.size()), dim3(CAL_TB), 0, s, in.on(d, i_rows), in.on(d, i_jobs),
                       in.on(d, i_cams), in.on(d, i_rot), h->obs.as<double2>(), h->src.as<double>(), h->out.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(2, s));
  if (!points_b.empty()) {
    hipLaunchKernelGGL(k_calib_line_points, dim3((unsigned)points_b.size()), dim3(CAL_TB), 0, s, in.on(d, i_points),
                       in.on(d, i_jobs), in.on(d, i_cams), in.on(d, i_segs), in.on(d, i_vx), in.on(d, i_vy), in.on(d, i_vd),
                       h->puv.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(3, s));
  if (!nearest_b.empty()) {
    hipLaunchKernelGGL(k_calib_nearest, dim3((unsigned)nearest_b.size()), dim3(CAL_TB), 0, s, in.on(d, i_nearest),
                       in.on(d, i_jobs), h->obs.as<double2>(), h->puv.as<double2>(), h->out.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(4, s));
  if (out_rows) CHK(h->out.down(e.predicted, (size_t)out_rows * 16));
  CHK(h->ev.record(5, s));
  HIPCHK(hipEventSynchronize(h->ev.e[5]));
  h->ev.report(e.times_ms, CAL_TIMES, CAL_TIMES);
  return GLH_OK;
}

int calib_fit_sets(glh_calib* h, const CalibFit& f) {
  CHK(h->use());
  hipStream_t s = h->stream;
  const size_t N = (size_t)h->row_offset[h->n_controls], S = (size_t)f.n_sets, T = (size_t)f.set_offset[f.n_sets];
  const size_t p = (size_t)f.p;
  // in: the cameras, the weights, the sets, the fitted camera's parameters and vector; out: x, mean_error, status, inlier
  Stage in(h->stage);
  StagePlan out;  // (downloaded one by one into the caller's arrays)
  const auto i_cams = in.put<const CamDev>(f.cams, (size_t)h->n_cams);
  const auto i_weights = in.put<const double2>(f.weights, f.weights ? N : 0), i_observed = in.put<const double2>(f.observed, f.observed ? N : 0);
  const auto i_offset = in.put<const int64_t>(f.set_offset, S + 1);
  const auto i_rows = in.room<int32_t>(T);
  int32_t* rows = in.host(i_rows);
  for (size_t k = 0; k < T; ++k) rows[k] = (int32_t)f.set_rows[k];
  const auto i_par = in.room<double>(4 * p + GLH_CAM_LEN);
  double* par = in.host(i_par);  // (set_team's order)
  for (size_t i = 0; i < p; ++i) par[i] = f.x0[i], par[p + i] = f.lb[i], par[2 * p + i] = f.ub[i], par[3 * p + i] = f.scale[i];
  std::memcpy(par + 4 * p, f.vectors + (size_t)f.fit_cam * GLH_CAM_LEN, GLH_CAM_LEN * 8);
  const auto o_x = out.place<double>(S * p), o_mean = out.place<double>(S);
  const auto o_status = out.place<int32_t>(S);
  const auto o_inlier = out.place<uint8_t>(f.score ? S * N : 0);
  CHK(h->fit_in.reserve(in.bytes()));
  CHK(h->fit_out.reserve(out.bytes(0)));
  CHK(h->fit_ev.record(0, s));
  HIPCHK(hipMemcpy(h->fit_in.p, in.hold(), in.bytes(), hipMemcpyHostToDevice));
  CHK(h->fit_ev.record(1, s));
  void *d = h->fit_in.p, *o = h->fit_out.p;
  SetArgs a{};
  a.cams = in.on(d, i_cams);
  a.ctl = h->ctl.as<CalCtl>();
  a.row_ctl = h->row_ctl.as<int32_t>();
  a.obs = h->obs.as<double2>();
  a.src = h->src.as<double>();
  a.weights = f.weights ? in.on(d, i_weights) : nullptr;
  a.observed = f.observed ? in.on(d, i_observed) : h->obs.as<double2>();
  a.set_offset = in.on(d, i_offset);
  a.set_rows = in.on(d, i_rows);
  a.par = in.on(d, i_par);
  a.x = out.on(o, o_x);
  a.status = out.on(o, o_status);
  a.mean_error = out.on(o, o_mean);
  for (size_t i = 0; i < p; ++i) a.slot[i] = f.slots[i];
  a.fit_cam = f.fit_cam, a.p = f.p, a.max_nfev = f.max_nfev, a.n_rows = (int32_t)N;
  a.ftol = f.ftol, a.xtol = f.xtol, a.gtol = f.gtol;
  if (S) {
    if (f.p <= FIT_SMALL_P)
      hipLaunchKernelGGL(k_fit_sets<FIT_SMALL_P>, dim3((unsigned)S), dim3(CAL_FIT_TB), 0, s, a);
    else
      hipLaunchKernelGGL(k_fit_sets<LM_MAX_P>, dim3((unsigned)S), dim3(CAL_FIT_TB), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  CHK(h->fit_ev.record(2, s));
  if (S && N && f.score) {
    const int blocks_per_set = (int)((N + CAL_TB - 1) / CAL_TB);
    uint8_t* inlier = out.on(o, o_inlier);
    hipLaunchKernelGGL(k_calib_score, dim3((unsigned)(S * (size_t)blocks_per_set)), dim3(CAL_TB), 0, s, a, blocks_per_set,
                       f.max_error, inlier);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_calib_members, dim3((unsigned)S), dim3(CAL_TB), 0, s, a, inlier);
    HIPCHK(hipGetLastError());
  }
  CHK(h->fit_ev.record(3, s));
  if (S) {
    HIPCHK(hipMemcpy(f.x, a.x, o_x.bytes(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(f.mean_error, a.mean_error, o_mean.bytes(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(f.status, a.status, o_status.bytes(), hipMemcpyDeviceToHost));
    if (N && f.score) HIPCHK(hipMemcpy(f.inlier, out.on(o, o_inlier), o_inlier.bytes(), hipMemcpyDeviceToHost));
  }
  CHK(h->fit_ev.record(4, s));
  HIPCHK(hipEventSynchronize(h->fit_ev.e[4]));
  h->fit_ev.report(f.times_ms, CAL_FIT_TIMES, CAL_FIT_TIMES);
  return GLH_OK;
}

template <int MAXP, int TW, int TEAMS>
static void rg_launch(const RArgs& a, int refit, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.n_hyp + TEAMS - 1) / TEAMS);
  hipLaunchKernelGGL((k_rg_fit<MAXP, TW, TEAMS>), dim3(blocks), dim3(TW * 64 * TEAMS), 0, s, a, refit);
}

int calib_ransac_groups(glh_calib* h, const CalibRansac& r) {
  CHK(h->use());
  hipStream_t s = h->stream;
  if (!h->rg_ready) {
    CHK(h->rg_ev.create());
    h->rg_ready = true;
  }
  const size_t N = (size_t)h->row_offset[h->n_controls], G = (size_t)r.n_groups, H = G ? (size_t)r.hyp_offset[G] : 0;
  const size_t p = (size_t)r.p, n = (size_t)r.n, C = (size_t)h->n_cams;
  // the groups, and where their masks lie (glh_ransac_plan.h)
  std::vector<RGroup> groups(G);
  std::vector<int64_t> rows(G), hyps(G), mask_offset(G + 1);
  for (size_t g = 0; g < G; ++g) {
    const int c = r.group_control[g];
    rows[g] = h->row_offset[c + 1] - h->row_offset[c];
    hyps[g] = r.hyp_offset[g + 1] - r.hyp_offset[g];
  }
  const size_t mask_bytes = (size_t)rg_mask_offsets((int)G, rows.data(), hyps.data(), mask_offset.data());
  for (size_t g = 0; g < G; ++g)
    groups[g] = RGroup{h->row_offset[r.group_control[g]], mask_offset[g], (int32_t)rows[g], r.group_control[g], r.group_cam[g],
                       (int32_t)r.hyp_offset[g], (int32_t)hyps[g], 0};
  Stage in(h->stage), out(h->stage);  // (one host buffer: the upload has left it when the download fills it)
  const auto i_cams = in.put<const CamDev>(r.cams, C);
  const auto i_vec = in.put<const double>(r.vectors, C * GLH_CAM_LEN);
  const auto i_weights = in.put<const double2>(r.weights, r.weights ? N : 0), i_observed = in.put<const double2>(r.observed, r.observed ? N : 0);
  const auto i_groups = in.put<const RGroup>(groups.data(), G);
  const auto i_hg = in.room<int32_t>(H);
  int32_t* hg = in.host(i_hg);
  for (size_t g = 0; g < G; ++g)
    for (int64_t k = r.hyp_offset[g]; k < r.hyp_offset[g + 1]; ++k) hg[k] = (int32_t)g;
  const auto i_samples = in.room<int32_t>(H * n);
  int32_t* samples = in.host(i_samples);
  for (size_t g = 0; g < G; ++g) {
    const size_t first = (size_t)r.hyp_offset[g] * n, last = (size_t)r.hyp_offset[g + 1] * n;
    if (r.drawn && r.drawn[g])
      std::memset(samples + first, 0, (last - first) * 4);  // (k_rg_draw's to fill)
    else
      for (size_t k = first; k < last; ++k) samples[k] = (int32_t)r.samples[k];
  }
  const auto i_id = in.put<const int32_t>(r.group_id, r.drawn ? G : 0);
  const auto i_drawn = in.put<const uint8_t>(r.drawn, r.drawn ? G : 0);
  const auto i_x0 = in.put<const double>(r.x0, G * p), i_lb = in.put<const double>(r.lb, G * p);
  const auto i_ub = in.put<const double>(r.ub, G * p), i_scale = in.put<const double>(r.scale, G * p);
  // out, in the order of the download: the doubles, the int32s, the bytes
  const auto o_x = out.place<double>(H * p), o_refit = out.place<double>(H * p), o_mean = out.place<double>(H);
  const auto o_status = out.place<int32_t>(H), o_consensus = out.place<int32_t>(H), o_rstatus = out.place<int32_t>(H), o_winner = out.place<int32_t>(G);
  const auto o_inlier = out.place<uint8_t>(N);
  CHK(h->rg_in.reserve(in.bytes()));
  CHK(h->rg_out.reserve(out.bytes()));
  CHK(h->rg_mask.reserve(mask_bytes));
  CHK(h->rg_ev.record(0, s));
  HIPCHK(hipMemcpy(h->rg_in.p, in.hold(), in.bytes(), hipMemcpyHostToDevice));
  CHK(h->rg_ev.record(1, s));
  void *d = h->rg_in.p, *o = h->rg_out.p;
  RArgs a{};
  a.cams = in.on(d, i_cams);
  a.vectors = in.on(d, i_vec);
  a.ctl = h->ctl.as<CalCtl>();
  a.obs = h->obs.as<double2>();
  a.src = h->src.as<double>();
  a.observed = r.observed ? in.on(d, i_observed) : h->obs.as<double2>();
  a.weights = r.weights ? in.on(d, i_weights) : nullptr;
  a.groups = in.on(d, i_groups);
  a.hyp_group = in.on(d, i_hg);
  a.samples = in.on(d, i_samples);
  a.x0 = in.on(d, i_x0), a.lb = in.on(d, i_lb), a.ub = in.on(d, i_ub), a.scale = in.on(d, i_scale);
  a.mask = h->rg_mask.as<uint8_t>();
  a.x = out.on(o, o_x), a.refit_x = out.on(o, o_refit), a.mean_error = out.on(o, o_mean);
  a.status = out.on(o, o_status), a.consensus = out.on(o, o_consensus), a.refit_status = out.on(o, o_rstatus);
  a.winner = out.on(o, o_winner), a.inlier = out.on(o, o_inlier);
  for (size_t i = 0; i < p; ++i) a.slot[i] = r.slots[i];
  a.p = r.p, a.n = r.n, a.max_nfev = r.max_nfev, a.n_hyp = (int32_t)H, a.n_groups = (int32_t)G;
  // (a consensus is at most 2^31 - 1 rows, at least 0)
  a.min_inliers = (int32_t)(r.min_inliers > INT32_MAX ? INT32_MAX : (r.min_inliers < -1 ? -1 : r.min_inliers));
  a.ftol = r.ftol, a.xtol = r.xtol, a.gtol = r.gtol, a.max_error = r.max_error;
  const int drawn_at = RANSAC_DRAWN_TIMES;  // the event after the draw
  if (r.drawn) {
    if (H) {
      // (the staging buffer is the device's to write once it is uploaded: the draw fills the rows the host left empty)
      const DrawArgs da{a.groups, a.hyp_group, in.on(d, i_id), in.on(d, i_drawn), in.on(d, i_samples), a.n, a.n_hyp, r.seed0, r.seed1};
      hipLaunchKernelGGL(k_rg_draw, dim3((unsigned)((H + CAL_TB - 1) / CAL_TB)), dim3(CAL_TB), 0, s, da);
      HIPCHK(hipGetLastError());
    }
    CHK(h->rg_ev.record(drawn_at, s));
  }
  const bool small = r.p <= FIT_SMALL_P;
  if (H) {
    if (r.n <= 64)
      small ? rg_launch<FIT_SMALL_P, 1, 4>(a, 0, s) : rg_launch<LM_MAX_P, 1, 1>(a, 0, s);
    else
      small ? rg_launch<FIT_SMALL_P, 2, 1>(a, 0, s) : rg_launch<LM_MAX_P, 2, 1>(a, 0, s);
    HIPCHK(hipGetLastError());
  }
  CHK(h->rg_ev.record(2, s));
  if (H) {
    hipLaunchKernelGGL(k_rg_score, dim3((unsigned)H), dim3(CAL_TB), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  CHK(h->rg_ev.record(3, s));
  if (H) {
    small ? rg_launch<FIT_SMALL_P, 2, 1>(a, 1, s) : rg_launch<LM_MAX_P, 2, 1>(a, 1, s);
    HIPCHK(hipGetLastError());
  }
  CHK(h->rg_ev.record(4, s));
  if (G) {
    hipLaunchKernelGGL(k_rg_winner, dim3((unsigned)((G + CAL_TB - 1) / CAL_TB)), dim3(CAL_TB), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rg_final, dim3((unsigned)G), dim3(CAL_TB), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  CHK(h->rg_ev.record(5, s));
  if (r.samples_out && H) {
    std::vector<int32_t> rows(H * n);
    HIPCHK(hipMemcpy(rows.data(), in.on(d, i_samples), i_samples.bytes(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < H * n; ++k) r.samples_out[k] = rows[k];
  }
  HIPCHK(hipMemcpy(out.hold(), o, out.bytes(), hipMemcpyDeviceToHost));
  CHK(h->rg_ev.record(6, s));
  HIPCHK(hipEventSynchronize(h->rg_ev.e[6]));
  out.take(r.x, o_x), out.take(r.refit_x, o_refit), out.take(r.mean_error, o_mean);
  out.take(r.status, o_status), out.take(r.consensus, o_consensus), out.take(r.refit_status, o_rstatus);
  out.take(r.winner, o_winner), out.take(r.inlier, o_inlier);
  h->rg_ev.report(r.times_ms, RANSAC_TIMES, RANSAC_TIMES);
  if (r.drawn && r.times_ms) {  // the fit began after the draw
    r.times_ms[RANSAC_TIMES] = h->rg_ev.ms(1, drawn_at);
    r.times_ms[1] = h->rg_ev.ms(drawn_at, 2);
  }
  return GLH_OK;
}

// glh_stage_ransac_samples: the draw alone, every group drawn, rows counted within the group.
int ransac_draw_samples(const RansacDraw& r) {
  HIPCHK(hipSetDevice(r.device));
  const size_t G = (size_t)r.n_groups, H = G ? (size_t)r.hyp_offset[G] : 0, n = (size_t)r.n;
  std::vector<RGroup> groups(G);
  std::vector<int32_t> hyp_group(H);
  for (size_t g = 0; g < G; ++g) {
    groups[g] = RGroup{0, 0, (int32_t)r.rows[g], 0, 0, (int32_t)r.hyp_offset[g], (int32_t)(r.hyp_offset[g + 1] - r.hyp_offset[g]), 0};
    for (int64_t k = r.hyp_offset[g]; k < r.hyp_offset[g + 1]; ++k) hyp_group[(size_t)k] = (int32_t)g;
  }
  StageEvents<4> ev;
  CHK(ev.create());
  DevBuf d_groups, d_hg, d_id, d_samples;
  CHK(ev.record(0, nullptr));
  CHK(d_groups.up(groups.data(), G * sizeof(RGroup)));
  CHK(d_hg.up(hyp_group.data(), H * 4));
  CHK(d_id.up(r.group_id, G * 4));
  CHK(d_samples.alloc(H * n * 4));
  CHK(ev.record(1, nullptr));
  if (H) {
    const DrawArgs da{d_groups.as<RGroup>(), d_hg.as<int32_t>(), d_id.as<int32_t>(), nullptr, d_samples.as<int32_t>(), (int32_t)n,
                      (int32_t)H, r.seed0, r.seed1};
    hipLaunchKernelGGL(k_rg_draw, dim3((unsigned)((H + CAL_TB - 1) / CAL_TB)), dim3(CAL_TB), 0, nullptr, da);
    HIPCHK(hipGetLastError());
  }
  CHK(ev.record(2, nullptr));
  std::vector<int32_t> rows(H * n);
  if (H) CHK(d_samples.down(rows.data(), H * n * 4));
  CHK(ev.record(3, nullptr));
  HIPCHK(hipEventSynchronize(ev.e[3]));
  for (size_t k = 0; k < H * n; ++k) r.samples[k] = rows[k];
  ev.report(r.times_ms, 3, 3);
  return GLH_OK;
}

void calib_destroy(glh_calib* h) { destroy_object(h); }

}  // namespace glh
