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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_calib.h"
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

__global__ void __launch_bounds__(CAL_TB) k_calib_rows(const CalBlock* __restrict__ blocks, const CalJob* __restrict__ jobs,
                                                       const CamDev* __restrict__ cams, const double* __restrict__ rot,
                                                       const double2* __restrict__ obs, const double* __restrict__ src,
                                                       double2* __restrict__ out) {
  const CalBlock b = blocks[blockIdx.x];
  const CalJob j = jobs[b.job];
  const int r = b.first + (int)threadIdx.x;
  if (r >= j.n_rows) return;
  const CamDev& ct = cams[j.cam_t];
  const uint32_t ft = cam_flags(ct);
  const size_t row = (size_t)j.row0 + r;
  double u, v;
  if (j.kind == GLH_CALIB_POINTS) {
    project_f(ct, ft | (j.directions ? CAM_F_DIRECTIONS : 0u), src[3 * row], src[3 * row + 1], src[3 * row + 2], u, v);
  } else {
    // the other camera's points: the second side's are kept in src[.][0:2], the first side's are the observed ones
    const double x = j.side == 0 ? src[3 * row] : obs[row].x, y = j.side == 0 ? src[3 * row + 1] : obs[row].y;
    double d[3];
    if (j.kind == GLH_CALIB_MATCHES) {
      const CamDev& co = cams[j.cam_o];
      unproject(co, cam_flags(co), x, y, 1.0, 1, d);
    } else {
      const double* __restrict__ Ro = rot + 9 * (size_t)j.cam_o;  // Camera._xy_to_xyz (camera.py:1486-1492)
      for (int k = 0; k < 3; ++k) d[k] = (Ro[k] * x + Ro[3 + k] * y) + Ro[6 + k];
    }
    if (j.kind == GLH_CALIB_ROTATION_XY) {
      const double* __restrict__ Rt = rot + 9 * (size_t)j.cam_t;  // Camera._xyz_to_xy (camera.py:1435-1470), directions
      double c[3];
      for (int k = 0; k < 3; ++k) c[k] = Rt[3 * k] * d[0] + Rt[3 * k + 1] * d[1] + Rt[3 * k + 2] * d[2];
      u = c[0] / c[2];
      v = c[1] / c[2];
      if (c[2] <= 0.0) u = v = NAN;
    } else {
      project_f(ct, ft | CAM_F_DIRECTIONS, d[0], d[1], d[2], u, v);
    }
  }
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

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

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
  return GLH_OK;
}

int calib_create(int device, const CalibControls& c, glh_calib** out) {
  return create_object("calib", device, out, [&](glh_calib* h) { return calib_fill(h, c); });
}

CalibTable calib_table(const glh_calib* h) { return CalibTable{h->n_cams, h->n_controls, h->kind.data(), h->row_offset.data()}; }

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
  size_t at = 0;
  const size_t o_cams = at;
  at = align16(at + n_cam_sets * sizeof(CamDev));
  const size_t o_rot = at;
  at = align16(at + n_cam_sets * 72);
  const size_t o_jobs = at;
  at = align16(at + jobs.size() * sizeof(CalJob));
  const size_t o_segs = at;
  at = align16(at + segs.size() * sizeof(CalSeg));
  const size_t o_rows = at;
  at = align16(at + rows_b.size() * sizeof(CalBlock));
  const size_t o_points = at;
  at = align16(at + points_b.size() * sizeof(CalBlock));
  const size_t o_nearest = at;
  at = align16(at + nearest_b.size() * sizeof(CalBlock));
  const size_t o_vx = at;
  at = align16(at + V * 8);
  const size_t o_vy = at;
  at = align16(at + V * 8);
  const size_t o_vd = at;
  at = align16(at + V * 8);
  h->stage.resize(at ? at : 16);
  char* st = h->stage.data();
  std::memcpy(st + o_cams, e.cams, n_cam_sets * sizeof(CamDev));
  std::memcpy(st + o_rot, e.rot, n_cam_sets * 72);
  if (!jobs.empty()) std::memcpy(st + o_jobs, jobs.data(), jobs.size() * sizeof(CalJob));
  if (!segs.empty()) std::memcpy(st + o_segs, segs.data(), segs.size() * sizeof(CalSeg));
  if (!rows_b.empty()) std::memcpy(st + o_rows, rows_b.data(), rows_b.size() * sizeof(CalBlock));
  if (!points_b.empty()) std::memcpy(st + o_points, points_b.data(), points_b.size() * sizeof(CalBlock));
  if (!nearest_b.empty()) std::memcpy(st + o_nearest, nearest_b.data(), nearest_b.size() * sizeof(CalBlock));
  double *vx = reinterpret_cast<double*>(st + o_vx), *vy = reinterpret_cast<double*>(st + o_vy),
         *vd = reinterpret_cast<double*>(st + o_vd);
  for (size_t k = 0; k < V; ++k) vx[k] = e.vertex[3 * k], vy[k] = e.vertex[3 * k + 1], vd[k] = e.vertex[3 * k + 2];

  CHK(h->in.reserve(h->stage.size()));
  CHK(h->puv.reserve((size_t)(puv_total ? puv_total : 1) * 16));
  CHK(h->out.reserve((size_t)(out_rows ? out_rows : 1) * 16));
  CHK(h->ev.record(0, s));
  HIPCHK(hipMemcpy(h->in.p, st, h->stage.size(), hipMemcpyHostToDevice));
  CHK(h->ev.record(1, s));
  const char* d = h->in.as<char>();
  const CalJob* d_jobs = reinterpret_cast<const CalJob*>(d + o_jobs);
  const CamDev* d_cams = reinterpret_cast<const CamDev*>(d + o_cams);
  if (!rows_b.empty()) {
    hipLaunchKernelGGL(k_calib_rows, dim3((unsigned)rows_b.size()), dim3(CAL_TB), 0, s,
                       reinterpret_cast<const CalBlock*>(d + o_rows), d_jobs, d_cams,
                       reinterpret_cast<const double*>(d + o_rot), h->obs.as<double2>(), h->src.as<double>(),
                       h->out.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(2, s));
  if (!points_b.empty()) {
    hipLaunchKernelGGL(k_calib_line_points, dim3((unsigned)points_b.size()), dim3(CAL_TB), 0, s,
                       reinterpret_cast<const CalBlock*>(d + o_points), d_jobs, d_cams,
                       reinterpret_cast<const CalSeg*>(d + o_segs), reinterpret_cast<const double*>(d + o_vx),
                       reinterpret_cast<const double*>(d + o_vy), reinterpret_cast<const double*>(d + o_vd),
                       h->puv.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(3, s));
  if (!nearest_b.empty()) {
    hipLaunchKernelGGL(k_calib_nearest, dim3((unsigned)nearest_b.size()), dim3(CAL_TB), 0, s,
                       reinterpret_cast<const CalBlock*>(d + o_nearest), d_jobs, h->obs.as<double2>(),
                       h->puv.as<double2>(), h->out.as<double2>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(4, s));
  if (out_rows) CHK(h->out.down(e.predicted, (size_t)out_rows * 16));
  CHK(h->ev.record(5, s));
  HIPCHK(hipEventSynchronize(h->ev.e[5]));
  h->ev.report(e.times_ms, CAL_TIMES, CAL_TIMES);
  return GLH_OK;
}

void calib_destroy(glh_calib* h) { destroy_object(h); }

}  // namespace glh
