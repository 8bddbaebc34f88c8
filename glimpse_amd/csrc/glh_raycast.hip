// glh_raycast.hip -- rays cast onto a DEM on the device: the work behind glh_stage_raycast (include/glimpse_hip.h;
// glimpse_hip.hip validates the arguments and calls raycast_run).  Raster.intersect_rays, Camera.uv_to_dem and
// Camera.xyz_map go from the image to the world: where Camera.project_dem and Image.orthorectify start at a DEM cell and
// ask where it lands in the frame, this starts at a pixel and asks which point of the terrain it sees.  The reference has
// the parts (helpers.intersect_rays_box, intersect_rays_plane, bresenham_line) and no ray cast, so the rule is the
// contract: INPUTS.md, "Ray casting: the rule", restated in NumPy in tests/raycast_rule.py, whose names the device
// functions below keep.  In short:
//
//   surface    the bilinear patches between the cell centres; in grid coordinates p = (x - x[0]) / d0, q = (y - y[0]) / d1
//              patch (i, j) is [i, i + 1] x [j, j + 1], the domain [0, nx - 1] x [0, ny - 1]: no half-cell rim.
//   traversal  the 2-D slab test gives the entry (clamped to t >= 0) and the exit; patches are visited in the order of the
//              crossing times (line - p0) / dp of the integer lines, each computed afresh from its index, the p line
//              first on a tie.  Inside a patch g(t) = ray height - apparent surface = (A t + B) t + C.
//   hit        the first patch with g <= 0 at its exit; t is the root in (t0, t1] by the cancellation-free form.
//   skip       with `block` = B a ray tests each block of B x B patches it enters against the block's highest cell
//              (k_rc_block_max) and jumps to the block's exit when it clears it; the patch it lands in is the one the
//              plain march would be in, found by comparing the same crossing times (rc_column_at), so the result does
//              not depend on B.
//
// One thread per ray; the three ray sources (explicit directions, a camera's uv, a camera's pixel grid made on the device)
// share the march.  No atomics, no LDS (nothing is shared: a ray reads the four corners of the patches it crosses, and
// the rays of a wave -- an 8 x 8 block of pixels in grid mode -- cross neighbouring patches, which the caches serve).
// Every loop is bounded by the grid's size and invalid rays are sorted out before the first one, so no input makes a
// thread spin.  Lanes of a wave diverge where one skips a block while its neighbour steps a patch, and when their rays end
// at different depths; the 8 x 8 pixel blocks keep both short.
//
// float64 throughout, operation by operation as NumPy rounds (-ffp-contract=off); sqrt and / are the correctly rounded
// ones, not glh_math.h's sqrt_nr / rcp_nr.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_raycast.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int RC_TB = 256;          // threads of a workgroup: four waves
constexpr int RC_TILE = 16;         // grid mode: a workgroup is a 16 x 16 tile of pixels, a wave an 8 x 8 quarter of it
constexpr double RC_SKIP_MARGIN = 9.313225746154785e-10;  // 2^-30 (tests/raycast_rule.py: SKIP_MARGIN)

struct RcArgs {
  CamDev cam;      // by value: the kernel reads it from scalar registers
  uint32_t flags;  // cam_flags(cam)
  const void* z;
  int z_f32, nx, ny;
  double x0, y0, d0, d1;
  int mode;
  const double* origins;
  int origin_stride;  // 0: one origin for every ray; 3: one each
  const double* rays;
  int n, step, cols, rows;
  int correction;
  double knum, kden;  // refraction - 1, 2 radius
  int block, shift, nbx;
  const double* zmax;  // [nby][nbx] k_rc_block_max's, or null
  double* t;
  double* xyz;
  int32_t* patch;
  uint8_t* status;
};

__device__ __forceinline__ double rc_z(const RcArgs& a, int row, int col) {
  const size_t i = (size_t)row * a.nx + col;
  return a.z_f32 ? (double)static_cast<const float*>(a.z)[i] : static_cast<const double*>(a.z)[i];
}

__device__ __forceinline__ double rc_lower(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double rc_upper(double a, double b) { return b > a ? b : a; }

// crossing(): the time at which a ray crosses an integer line of an axis
__device__ __forceinline__ double rc_crossing(double line, double p0, double dp) { return __ddiv_rn(line - p0, dp); }

__device__ __forceinline__ int rc_clamp_column(double c, int last) {
  return c > 0.0 ? (c < (double)last ? (int)c : last) : 0;
}

// column_at(): the column a ray is in once every line crossing with a time <= T (< T when strict) has been made.  The
// guess is off by a rounding at most for any ray that is near the grid; the loops are bounded by the axis for the others.
__device__ int rc_column_at(double T, double p0, double dp, int n, bool strict) {
  const int last = n - 2;
  if (dp == 0.0) return rc_clamp_column(floor(p0), last);
  const bool up = dp > 0.0;
  const int s = up ? 1 : -1;
  int c = rc_clamp_column(floor(p0 + T * dp), last);
  auto reached = [&](int col) {
    const double e = rc_crossing((double)(up ? col : col + 1), p0, dp);
    return strict ? e < T : e <= T;
  };
  for (int k = 0; k < n; ++k) {
    const int next = c + s;
    if (next < 0 || next > last || !reached(next)) break;
    c = next;
  }
  for (int k = 0; k < n; ++k) {
    const int prev = c - s;
    if (prev < 0 || prev > last || reached(c)) break;
    c = prev;
  }
  return c;
}

struct RcRay {
  double p0, q0, dp, dq, oz, dz, K;
};

// _patch(): g(t) = (A t + B) t + C in patch (i, j); false when a corner is NaN
struct RcPatch {
  double A, B, C;
  bool whole;
};
__device__ __forceinline__ RcPatch rc_patch(const RcArgs& a, const RcRay& r, int i, int j) {
  const double z00 = rc_z(a, j, i), z10 = rc_z(a, j, i + 1), z01 = rc_z(a, j + 1, i), z11 = rc_z(a, j + 1, i + 1);
  const double e1 = z10 - z00;
  const double e2 = z01 - z00;
  const double e3 = (z11 - z01) - e1;
  const double u0 = r.p0 - (double)i;
  const double v0 = r.q0 - (double)j;
  RcPatch p;
  p.C = (r.oz - z00) - ((u0 * e1 + v0 * e2) + (u0 * v0) * e3);
  p.B = r.dz - ((r.dp * e1 + r.dq * e2) + (u0 * r.dq + v0 * r.dp) * e3);
  p.A = -((r.dp * r.dq) * e3) - r.K;
  p.whole = !(isnan(z00) || isnan(z10) || isnan(z01) || isnan(z11));
  return p;
}

__device__ __forceinline__ double rc_g(const RcPatch& p, double t) { return (p.A * t + p.B) * t + p.C; }

__device__ __forceinline__ double rc_outside(double r, double t0, double t1) {
  return r < t0 ? t0 - r : (r > t1 ? r - t1 : 0.0);
}

// _root(): the root of the patch's quadratic nearest [t0, t1], clamped into it
__device__ double rc_root(const RcPatch& p, double t0, double t1) {
  double t;
  if (p.A == 0.0) {
    t = __ddiv_rn(-p.C, p.B);
  } else {
    double disc = p.B * p.B - (4.0 * p.A) * p.C;
    disc = disc > 0.0 ? disc : 0.0;
    const double qq = (p.B + copysign(__dsqrt_rn(disc), p.B)) * -0.5;
    const double ra = __ddiv_rn(qq, p.A);
    const double rb = qq != 0.0 ? __ddiv_rn(p.C, qq) : ra;
    const double lo = rb < ra ? rb : ra;
    const double hi = rb < ra ? ra : rb;
    t = rc_outside(hi, t0, t1) < rc_outside(lo, t0, t1) ? hi : lo;
  }
  t = t >= t0 ? t : t0;
  return t > t1 ? t1 : t;
}

struct RcResult {
  double t;
  int patch, status;
};

// cast(): one ray
__device__ RcResult rc_cast(const RcArgs& a, const double* o, const double* d) {
  const RcResult none[5] = {{NAN, -1, GLH_RAYCAST_HIT},
                            {NAN, -1, GLH_RAYCAST_MISS},
                            {NAN, -1, GLH_RAYCAST_BELOW},
                            {NAN, -1, GLH_RAYCAST_LEAVES},
                            {NAN, -1, GLH_RAYCAST_INVALID}};
  const int nx = a.nx, ny = a.ny;
  RcRay r;
  r.p0 = __ddiv_rn(o[0] - a.x0, a.d0);
  r.q0 = __ddiv_rn(o[1] - a.y0, a.d1);
  r.dp = __ddiv_rn(d[0], a.d0);
  r.dq = __ddiv_rn(d[1], a.d1);
  r.oz = o[2];
  r.dz = d[2];
  r.K = a.correction ? __ddiv_rn(a.knum * (d[0] * d[0] + d[1] * d[1]), a.kden) : 0.0;
  bool valid = isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) &&
               (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
  valid = valid && isfinite(r.p0) && isfinite(r.q0) && isfinite(r.dp) && isfinite(r.dq) && isfinite(r.K);
  if (!valid) return none[GLH_RAYCAST_INVALID];

  // the domain: the 2-D slab test, the entry clamped to t >= 0
  double near_p = -INFINITY, far_p = INFINITY, near_q = -INFINITY, far_q = INFINITY;
  bool in_p = true, in_q = true;
  if (r.dp != 0.0) {
    const double ta = rc_crossing(0.0, r.p0, r.dp), tb = rc_crossing((double)(nx - 1), r.p0, r.dp);
    near_p = rc_lower(ta, tb), far_p = rc_upper(ta, tb);
  } else {
    in_p = r.p0 >= 0.0 && r.p0 <= (double)(nx - 1);
  }
  if (r.dq != 0.0) {
    const double ta = rc_crossing(0.0, r.q0, r.dq), tb = rc_crossing((double)(ny - 1), r.q0, r.dq);
    near_q = rc_lower(ta, tb), far_q = rc_upper(ta, tb);
  } else {
    in_q = r.q0 >= 0.0 && r.q0 <= (double)(ny - 1);
  }
  double t_in = rc_upper(near_p, near_q);
  t_in = t_in > 0.0 ? t_in : 0.0;
  const double t_out = rc_lower(far_p, far_q);
  if (!(in_p && in_q && t_in <= t_out)) return none[GLH_RAYCAST_MISS];

  // where the ray enters: every crossing with a time <= t_in has been made
  int i = rc_column_at(t_in, r.p0, r.dp, nx, false);
  int j = rc_column_at(t_in, r.q0, r.dq, ny, false);
  RcPatch p = rc_patch(a, r, i, j);
  if (rc_g(p, t_in) <= 0.0) return none[GLH_RAYCAST_BELOW];
  if (r.dp == 0.0 && r.dq == 0.0) {  // a vertical ray: one patch, g linear
    if (!(p.whole && p.B < 0.0)) return none[GLH_RAYCAST_LEAVES];
    const double tv = __ddiv_rn(-p.C, p.B);
    return RcResult{tv >= t_in ? tv : t_in, j * (nx - 1) + i, GLH_RAYCAST_HIT};
  }

  double t0 = t_in;
  const int sp = r.dp > 0.0 ? 1 : -1, sq = r.dq > 0.0 ? 1 : -1;
  int tested = -1;
  const int cap = 2 * (nx + ny) + 8;  // a ray crosses at most nx + ny lines, and skips fewer blocks than that
  for (int it = 0; it < cap; ++it) {
    if (a.block) {
      const int bi = i >> a.shift, bj = j >> a.shift;
      const int blk = bj * a.nbx + bi;
      if (blk != tested) {
        tested = blk;
        int lp = r.dp > 0.0 ? (bi + 1) * a.block : bi * a.block, lq = r.dq > 0.0 ? (bj + 1) * a.block : bj * a.block;
        lp = lp < nx - 1 ? lp : nx - 1;
        lq = lq < ny - 1 ? lq : ny - 1;
        const double tlp = r.dp != 0.0 ? rc_crossing((double)lp, r.p0, r.dp) : INFINITY;
        const double tlq = r.dq != 0.0 ? rc_crossing((double)lq, r.q0, r.dq) : INFINITY;
        const double te = rc_lower(rc_lower(tlp, tlq), t_out);
        const double h0 = r.oz + t0 * r.dz, h1 = r.oz + te * r.dz;
        const double hmin = rc_lower(h0, h1);
        const double cmax = rc_upper(r.K * (t0 * t0), r.K * (te * te));
        const double zm = a.zmax[blk];
        const double margin =
            RC_SKIP_MARGIN * ((((fabs(r.oz) + fabs(t0 * r.dz)) + fabs(te * r.dz)) + fabs(zm)) + fabs(cmax));
        if (zm == -INFINITY || hmin - (zm + cmax) > margin) {
          if (te >= t_out) return none[GLH_RAYCAST_LEAVES];
          int i_new, j_new;
          if (tlp <= tlq) {  // the block is left through a p line: the q crossings before it have been made
            i_new = r.dp > 0.0 ? lp : lp - 1;
            j_new = rc_column_at(tlp, r.q0, r.dq, ny, true);
          } else {  // through a q line: on a tie the p line goes first, so the p crossings up to it have been made
            i_new = rc_column_at(tlq, r.p0, r.dp, nx, false);
            j_new = r.dq > 0.0 ? lq : lq - 1;
          }
          i = i_new < 0 ? 0 : (i_new > nx - 2 ? nx - 2 : i_new);
          j = j_new < 0 ? 0 : (j_new > ny - 2 ? ny - 2 : j_new);
          t0 = te;
          continue;
        }
      }
    }
    // one patch
    const double tnp = r.dp != 0.0 ? rc_crossing((double)(i + (r.dp > 0.0 ? 1 : 0)), r.p0, r.dp) : INFINITY;
    const double tnq = r.dq != 0.0 ? rc_crossing((double)(j + (r.dq > 0.0 ? 1 : 0)), r.q0, r.dq) : INFINITY;
    const double t1 = rc_lower(rc_lower(tnp, tnq), t_out);
    p = rc_patch(a, r, i, j);
    if (p.whole && rc_g(p, t1) <= 0.0)
      return RcResult{rc_g(p, t0) <= 0.0 ? t0 : rc_root(p, t0, t1), j * (nx - 1) + i, GLH_RAYCAST_HIT};
    if (t1 >= t_out) break;
    if (tnp <= tnq)  // (on a tie the p line is taken first)
      i += sp;
    else
      j += sq;
    if (i < 0 || i > nx - 2 || j < 0 || j > ny - 2) break;
    t0 = t1;
  }
  return none[GLH_RAYCAST_LEAVES];
}

// The NaN-ignoring maximum over the cells of every block of B x B patches (one more cell than patches each way; -inf for a
// block without a value): one wave per block, its lanes striding over the cells, a butterfly of maxima at the end (a
// maximum does not depend on the order it is formed in).
__global__ __launch_bounds__(RC_TB) void k_rc_block_max(const void* z, int z_f32, int nx, int ny, int block, int nbx,
                                                        int nblocks, double* out) {
  const int64_t wave = (int64_t)blockIdx.x * (RC_TB / 64) + threadIdx.x / 64;
  if (wave >= nblocks) return;
  const int lane = threadIdx.x & 63;
  const int bj = (int)(wave / nbx), bi = (int)(wave % nbx);
  const int c0 = bi * block, r0 = bj * block;
  const int c1 = c0 + block < nx - 1 ? c0 + block : nx - 1, r1 = r0 + block < ny - 1 ? r0 + block : ny - 1;
  const int w = c1 - c0 + 1, count = w * (r1 - r0 + 1);
  double m = -INFINITY;
  for (int k = lane; k < count; k += 64) {
    const size_t i = (size_t)(r0 + k / w) * nx + (c0 + k % w);
    const double v = z_f32 ? (double)static_cast<const float*>(z)[i] : static_cast<const double*>(z)[i];
    if (v > m) m = v;  // (false for NaN)
  }
  for (int off = 32; off; off >>= 1) {
    const double other = __shfl_xor(m, off);
    if (other > m) m = other;
  }
  if (lane == 0) out[wave] = m;
}

__global__ __launch_bounds__(RC_TB) void k_raycast(const RcArgs a) {
  int idx;
  double o[3], d[3];
  if (a.mode == GLH_RAYCAST_GRID) {
    // a wave is an 8 x 8 block of pixels: its rays fan out over neighbouring patches
    const int wave = threadIdx.x / 64, lane = threadIdx.x & 63;
    const int col = blockIdx.x * RC_TILE + (wave & 1) * 8 + (lane & 7);
    const int row = blockIdx.y * RC_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (col >= a.cols || row >= a.rows) return;
    idx = row * a.cols + col;
    const double u = 0.5 * (double)a.step + (double)col * (double)a.step;
    const double v = 0.5 * (double)a.step + (double)row * (double)a.step;
    unproject(a.cam, a.flags, u, v, 1.0, 1, d);
    o[0] = a.cam.xyz[0], o[1] = a.cam.xyz[1], o[2] = a.cam.xyz[2];
  } else {
    const int64_t k = (int64_t)blockIdx.x * RC_TB + threadIdx.x;
    if (k >= a.n) return;
    idx = (int)k;
    if (a.mode == GLH_RAYCAST_UV) {
      const double u = a.rays[2 * (size_t)idx], v = a.rays[2 * (size_t)idx + 1];
      if (isfinite(u) && isfinite(v))
        unproject(a.cam, a.flags, u, v, 1.0, 1, d);
      else
        d[0] = d[1] = d[2] = NAN;
      o[0] = a.cam.xyz[0], o[1] = a.cam.xyz[1], o[2] = a.cam.xyz[2];
    } else {
      for (int c = 0; c < 3; ++c) {
        o[c] = a.origins[(size_t)idx * a.origin_stride + c];
        d[c] = a.rays[3 * (size_t)idx + c];
      }
    }
  }
  const RcResult h = rc_cast(a, o, d);
  a.t[idx] = h.t;
  for (int c = 0; c < 3; ++c) a.xyz[3 * (size_t)idx + c] = o[c] + h.t * d[c];
  a.patch[idx] = h.patch;
  a.status[idx] = (uint8_t)h.status;
}

}  // namespace

int raycast_run(const RaycastJob& j) {
  const size_t cells = (size_t)j.nx * j.ny, n = (size_t)j.n;
  const size_t zbytes = cells * (j.z_f32 ? 4 : 8);
  const size_t ray_doubles = j.mode == GLH_RAYCAST_DIRECTIONS ? 3 : (j.mode == GLH_RAYCAST_UV ? 2 : 0);
  int shift = 0;
  while (j.block && (1 << shift) < j.block) ++shift;
  const int nbx = j.block ? (j.nx - 1 + j.block - 1) / j.block : 0, nby = j.block ? (j.ny - 1 + j.block - 1) / j.block : 0;
  const int nblocks = nbx * nby;
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<RC_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dz, dorg, drays, dzmax, dt, dxyz, dpatch, dstatus;
  CHK(dz.alloc(zbytes));
  CHK(dorg.alloc((size_t)j.n_origins * 24));
  CHK(drays.alloc(n * ray_doubles * 8));
  CHK(dzmax.alloc((size_t)nblocks * 8));
  CHK(dt.alloc(n * 8));
  CHK(dxyz.alloc(n * 24));
  CHK(dpatch.alloc(n * 4));
  CHK(dstatus.alloc(n));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dz.p, j.z, zbytes, hipMemcpyHostToDevice));
  if (j.mode == GLH_RAYCAST_DIRECTIONS)
    HIPCHK(hipMemcpy(dorg.p, j.origins, (size_t)j.n_origins * 24, hipMemcpyHostToDevice));
  if (ray_doubles) HIPCHK(hipMemcpy(drays.p, j.rays, n * ray_doubles * 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  if (j.block) {
    hipLaunchKernelGGL(k_rc_block_max, dim3((unsigned)((nblocks + RC_TB / 64 - 1) / (RC_TB / 64))), dim3(RC_TB), 0, s, dz.p,
                       j.z_f32, j.nx, j.ny, j.block, nbx, nblocks, dzmax.as<double>());
    HIPCHK(hipGetLastError());
  }
  CHK(ev.record(2, s));
  RcArgs a{};
  if (j.cam) {
    a.cam = *j.cam;
    a.flags = cam_flags(a.cam);
  }
  a.z = dz.p, a.z_f32 = j.z_f32, a.nx = j.nx, a.ny = j.ny;
  a.x0 = j.x0, a.y0 = j.y0, a.d0 = j.d0, a.d1 = j.d1;
  a.mode = j.mode;
  a.origins = dorg.as<double>(), a.origin_stride = j.n_origins == 1 ? 0 : 3;
  a.rays = drays.as<double>();
  a.n = j.n, a.step = j.step, a.cols = j.cols, a.rows = j.rows;
  a.correction = j.correction, a.knum = j.refraction - 1.0, a.kden = 2.0 * j.radius;
  a.block = j.block, a.shift = shift, a.nbx = nbx;
  a.zmax = j.block ? dzmax.as<double>() : nullptr;
  a.t = dt.as<double>(), a.xyz = dxyz.as<double>(), a.patch = dpatch.as<int32_t>(), a.status = dstatus.as<uint8_t>();
  if (j.mode == GLH_RAYCAST_GRID)
    hipLaunchKernelGGL(k_raycast, dim3((j.cols + RC_TILE - 1) / RC_TILE, (j.rows + RC_TILE - 1) / RC_TILE), dim3(RC_TB), 0, s, a);
  else
    hipLaunchKernelGGL(k_raycast, dim3((unsigned)((n + RC_TB - 1) / RC_TB)), dim3(RC_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  CHK(dt.down(j.t, n * 8));
  CHK(dxyz.down(j.xyz, n * 24));
  CHK(dpatch.down(j.patch, n * 4));
  CHK(dstatus.down(j.status, n));
  CHK(ev.record(4, s));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  ev.report(j.times_ms, RC_TIMES, RC_TIMES);
  return GLH_OK;
}

}  // namespace glh
