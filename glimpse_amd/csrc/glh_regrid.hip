// glh_regrid.hip -- Raster.sample(grid=True) / Raster.resample (raster.py:1042-1083), Raster.resize (:1178-1187) and
// RasterInterpolant._interpolate (:1673-1700) on the device: the work behind glh_stage_raster_regrid,
// glh_stage_zoom_linear and glh_stage_raster_interpolate (include/glimpse_hip.h; glimpse_hip.hip validates the arguments).
//
// The reference fits scipy.interpolate.RectBivariateSpline(bbox = the raster's outer limits, s = 0) and evaluates it on a
// grid.  With s = 0 FITPACK's regrid interpolates: the spline is the tensor product whose coefficients C solve
// Ay C Ax^T = Z, with Ax / Ay the collocation matrices of the cell centres in the B-spline bases of FITPACK's knots.  Here:
//
//   host.     Per axis the knots, the banded collocation matrix (k diagonals on either side) and its LU factors without
//             pivoting (the matrices are totally positive); per output coordinate the knot interval and the k + 1 basis
//             values (de Boor's recurrence, as fpbspl runs it).  O(n k^2) and O(m k^2) flops: not worth a launch.
//   columns.  k_solve_cols: one thread per column marches down the rows, forward then backward substitution, the last k
//             values in registers; neighbouring threads touch neighbouring addresses, the factors are wave-uniform loads.
//   rows.     k_solve_rows: a workgroup owns 64 rows and walks them in tiles of 64 columns, left to right and back.  A tile
//             is loaded by rows (coalesced), kept in LDS with a leading dimension of 65 doubles, and lane r substitutes
//             along row r of it (stride 65 doubles: no two lanes of a half wave on one bank), then it is stored by rows.
//   order 1.  Every interior coefficient is the cell's value; only the first and the last coefficient of a line differ
//             (the end knots sit half a cell beyond the outer centres): k_ends_cols / k_ends_rows apply the closed form and
//             the solve kernels are not launched.  (An axis of two cells has no interior knot: it takes the general solve.)
//   evaluate. k_eval: one thread per output cell sums (ky + 1)(kx + 1) terms c * (hy * hx), rows outer, columns inner.
//   NaN.      Order 1 only: the cells' NaN mask travels beside the values (which hold 0 there); a sample is NaN when a
//             coefficient of nonzero weight has a NaN cell in its support: its own cell, and for the first / last
//             coefficient of a line the neighbour it is extrapolated from.
//
// Everything on the device is float64, operation by operation with the explicit round-to-nearest intrinsics (the library
// is built with -ffp-contract=off besides), every sum in a fixed order, no atomics: two calls give the same bytes, and
// tests/regrid_restatement.py, which does the same operations in NumPy, gives them too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/glimpse_hip.h"
#include "glh_regrid.h"
#include "glh_stage.h"
#include "glh_regrid_host.h"

namespace glh {

namespace {

constexpr int RG_WAVE = 64;
constexpr int RG_TILE = 64;        // rows per workgroup and columns per tile of k_solve_rows
constexpr int RG_LD = RG_TILE + 1;  // leading dimension of the LDS tile, in doubles
constexpr int RG_ROWS_TB = 256;

// ---- kernels -----------------------------------------------------------------------------------------------------------
// Forward then backward substitution down every column of w [ny][nx] with the factors lu [ny][2 K + 1].
template <int K>
__global__ void __launch_bounds__(RG_WAVE) k_solve_cols(double* __restrict__ w, int nx, int ny, const double* __restrict__ lu) {
  const int col = blockIdx.x * RG_WAVE + threadIdx.x;
  if (col >= nx) return;
  constexpr int W = 2 * K + 1;
  double p[K];  // p[d] = y[i - K + d]
#pragma unroll
  for (int d = 0; d < K; ++d) p[d] = 0.0;
  for (int i = 0; i < ny; ++i) {
    double acc = w[(size_t)i * nx + col];
#pragma unroll
    for (int d = 0; d < K; ++d)
      if (i - K + d >= 0) acc = __dsub_rn(acc, __dmul_rn(lu[(size_t)i * W + d], p[d]));
    w[(size_t)i * nx + col] = acc;
#pragma unroll
    for (int d = 0; d + 1 < K; ++d) p[d] = p[d + 1];
    p[K - 1] = acc;
  }
#pragma unroll
  for (int d = 0; d < K; ++d) p[d] = 0.0;  // p[d] = c[i + 1 + d]
  for (int i = ny - 1; i >= 0; --i) {
    double acc = w[(size_t)i * nx + col];
#pragma unroll
    for (int d = 0; d < K; ++d)
      if (i + 1 + d < ny) acc = __dsub_rn(acc, __dmul_rn(lu[(size_t)i * W + K + 1 + d], p[d]));
    acc = __ddiv_rn(acc, lu[(size_t)i * W + K]);
    w[(size_t)i * nx + col] = acc;
#pragma unroll
    for (int d = K - 1; d > 0; --d) p[d] = p[d - 1];
    p[0] = acc;
  }
}

__device__ __forceinline__ void rg_tile_load(double (*tile)[RG_LD], const double* w, int nx, int ny, int row0, int col0) {
  const int lane = threadIdx.x & (RG_WAVE - 1);
  for (int r = threadIdx.x / RG_WAVE; r < RG_TILE; r += RG_ROWS_TB / RG_WAVE)
    if (row0 + r < ny && col0 + lane < nx) tile[r][lane] = w[(size_t)(row0 + r) * nx + col0 + lane];
}

__device__ __forceinline__ void rg_tile_store(double (*tile)[RG_LD], double* w, int nx, int ny, int row0, int col0) {
  const int lane = threadIdx.x & (RG_WAVE - 1);
  for (int r = threadIdx.x / RG_WAVE; r < RG_TILE; r += RG_ROWS_TB / RG_WAVE)
    if (row0 + r < ny && col0 + lane < nx) w[(size_t)(row0 + r) * nx + col0 + lane] = tile[r][lane];
}

// The same substitutions along every row of w [ny][nx] with the factors lu [nx][2 K + 1].
template <int K>
__global__ void __launch_bounds__(RG_ROWS_TB) k_solve_rows(double* __restrict__ w, int nx, int ny, const double* __restrict__ lu) {
  __shared__ double tile[RG_TILE][RG_LD];
  constexpr int W = 2 * K + 1;
  const int row0 = blockIdx.x * RG_TILE;
  const int r = threadIdx.x;
  const bool solver = r < RG_TILE && row0 + r < ny;
  const int tiles = (nx + RG_TILE - 1) / RG_TILE;
  double p[K];
#pragma unroll
  for (int d = 0; d < K; ++d) p[d] = 0.0;
  for (int tl = 0; tl < tiles; ++tl) {
    const int col0 = tl * RG_TILE;
    rg_tile_load(tile, w, nx, ny, row0, col0);
    __syncthreads();
    if (solver) {
      const int cols = nx - col0 < RG_TILE ? nx - col0 : RG_TILE;
      for (int c = 0; c < cols; ++c) {
        const int i = col0 + c;
        double acc = tile[r][c];
#pragma unroll
        for (int d = 0; d < K; ++d)
          if (i - K + d >= 0) acc = __dsub_rn(acc, __dmul_rn(lu[(size_t)i * W + d], p[d]));
        tile[r][c] = acc;
#pragma unroll
        for (int d = 0; d + 1 < K; ++d) p[d] = p[d + 1];
        p[K - 1] = acc;
      }
    }
    __syncthreads();
    rg_tile_store(tile, w, nx, ny, row0, col0);
    __syncthreads();
  }
#pragma unroll
  for (int d = 0; d < K; ++d) p[d] = 0.0;
  for (int tl = tiles - 1; tl >= 0; --tl) {
    const int col0 = tl * RG_TILE;
    rg_tile_load(tile, w, nx, ny, row0, col0);
    __syncthreads();
    if (solver) {
      const int cols = nx - col0 < RG_TILE ? nx - col0 : RG_TILE;
      for (int c = cols - 1; c >= 0; --c) {
        const int i = col0 + c;
        double acc = tile[r][c];
#pragma unroll
        for (int d = 0; d < K; ++d)
          if (i + 1 + d < nx) acc = __dsub_rn(acc, __dmul_rn(lu[(size_t)i * W + K + 1 + d], p[d]));
        acc = __ddiv_rn(acc, lu[(size_t)i * W + K]);
        tile[r][c] = acc;
#pragma unroll
        for (int d = K - 1; d > 0; --d) p[d] = p[d - 1];
        p[0] = acc;
      }
    }
    __syncthreads();
    rg_tile_store(tile, w, nx, ny, row0, col0);
    __syncthreads();
  }
}

// Order 1, three or more cells on the axis: c[0] = (z[0] - a01 z[1]) / a00, c[n - 1] = (z[n - 1] - b0 z[n - 2]) / b1.
struct RgEnds {
  double a00, a01, b0, b1;
};

__global__ void __launch_bounds__(RG_WAVE) k_ends_cols(double* __restrict__ w, int nx, int ny, RgEnds e) {
  const int col = blockIdx.x * RG_WAVE + threadIdx.x;
  if (col >= nx) return;
  const double z0 = w[col], z1 = w[(size_t)nx + col];
  const double zl = w[(size_t)(ny - 1) * nx + col], zk = w[(size_t)(ny - 2) * nx + col];
  w[col] = __ddiv_rn(__dsub_rn(z0, __dmul_rn(e.a01, z1)), e.a00);
  w[(size_t)(ny - 1) * nx + col] = __ddiv_rn(__dsub_rn(zl, __dmul_rn(e.b0, zk)), e.b1);
}

__global__ void __launch_bounds__(RG_WAVE) k_ends_rows(double* __restrict__ w, int nx, int ny, RgEnds e) {
  const int row = blockIdx.x * RG_WAVE + threadIdx.x;
  if (row >= ny) return;
  double* line = w + (size_t)row * nx;
  const double z0 = line[0], z1 = line[1], zl = line[nx - 1], zk = line[nx - 2];
  line[0] = __ddiv_rn(__dsub_rn(z0, __dmul_rn(e.a01, z1)), e.a00);
  line[nx - 1] = __ddiv_rn(__dsub_rn(zl, __dmul_rn(e.b0, zk)), e.b1);
}

struct RgEval {
  const double* c;     // [ny][nx] coefficients
  const uint8_t* nan;  // [ny][nx] or null
  int nx, ny, kx, ky;
  const int32_t* lx;   // [mx] knot interval per output column
  const double* hx;    // [mx][RG_H]
  const int32_t* ly;   // [my]
  const double* hy;    // [my][RG_H]
  int mx, my;
  int use_zmin;
  double zmin;
  int flip_x, flip_y;
  double* out;         // [my][mx]
};

// the other cell the coefficient i of an order-1 line of n cells depends on (itself in the interior)
__device__ __forceinline__ int rg_partner(int i, int n) { return i == 0 ? 1 : (i == n - 1 ? n - 2 : i); }

__global__ void __launch_bounds__(256) k_eval(RgEval a) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)a.mx * a.my) return;
  const int i = (int)(idx / a.mx), j = (int)(idx % a.mx);
  const int row0 = a.ly[i] - a.ky, col0 = a.lx[j] - a.kx;
  const double* hy = a.hy + (size_t)i * RG_H;
  const double* hx = a.hx + (size_t)j * RG_H;
  double acc = 0.0;
  bool blank = false;
  for (int p = 0; p <= a.ky; ++p)
    for (int q = 0; q <= a.kx; ++q) {
      const int r = row0 + p, c = col0 + q;
      acc = __dadd_rn(acc, __dmul_rn(a.c[(size_t)r * a.nx + c], __dmul_rn(hy[p], hx[q])));
      if (a.nan && hy[p] != 0.0 && hx[q] != 0.0) {
        const int r2 = rg_partner(r, a.ny), c2 = rg_partner(c, a.nx);
        blank = blank || a.nan[(size_t)r * a.nx + c] || a.nan[(size_t)r * a.nx + c2] || a.nan[(size_t)r2 * a.nx + c] ||
                a.nan[(size_t)r2 * a.nx + c2];
      }
    }
  if (blank || (a.use_zmin && acc < a.zmin)) acc = NAN;
  const int oi = a.flip_y ? a.my - 1 - i : i, oj = a.flip_x ? a.mx - 1 - j : j;
  a.out[(size_t)oi * a.mx + oj] = acc;
}

// scipy.ndimage.zoom(a, zoom, order=1): output index i samples input coordinate i (n_in - 1) / (n_out - 1).
__global__ void __launch_bounds__(256) k_zoom_linear(const double* __restrict__ a, int nx, int ny, int mx, int my,
                                                     double sx, double sy, double* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)mx * my) return;
  const int i = (int)(idx / mx), j = (int)(idx % mx);
  const double cy = __dmul_rn((double)i, sy), cx = __dmul_rn((double)j, sx);
  int i0 = (int)floor(cy), j0 = (int)floor(cx);
  i0 = i0 > ny - 1 ? ny - 1 : i0;
  j0 = j0 > nx - 1 ? nx - 1 : j0;
  const int i1 = i0 + 1 < ny ? i0 + 1 : ny - 1, j1 = j0 + 1 < nx ? j0 + 1 : nx - 1;
  const double ty = __dsub_rn(cy, (double)i0), tx = __dsub_rn(cx, (double)j0);
  const double uy = __dsub_rn(1.0, ty), ux = __dsub_rn(1.0, tx);
  double acc = __dmul_rn(a[(size_t)i0 * nx + j0], __dmul_rn(uy, ux));
  acc = __dadd_rn(acc, __dmul_rn(a[(size_t)i0 * nx + j1], __dmul_rn(uy, tx)));
  acc = __dadd_rn(acc, __dmul_rn(a[(size_t)i1 * nx + j0], __dmul_rn(ty, ux)));
  acc = __dadd_rn(acc, __dmul_rn(a[(size_t)i1 * nx + j1], __dmul_rn(ty, tx)));
  out[idx] = acc;
}

// RasterInterpolant._interpolate (raster.py:1681-1698), cell by cell in its operation order.
__global__ void __launch_bounds__(256) k_blend(const double* __restrict__ m0, const double* __restrict__ m1,
                                               const double* __restrict__ s0, const double* __restrict__ s1, size_t n,
                                               double scale, double scale2, double third, double ratio,
                                               double* __restrict__ z, double* __restrict__ sigma) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const double a = m0[idx];
  const double dz = __dsub_rn(m1[idx], a);
  z[idx] = __dadd_rn(a, __dmul_rn(dz, scale));
  if (!sigma) return;
  const double v0 = __dmul_rn(s0[idx], s0[idx]), v1 = __dmul_rn(s1[idx], s1[idx]);
  const double z_var = __dadd_rn(v0, __dmul_rn(scale2, __dadd_rn(v0, v1)));
  const double zi = __dmul_rn(__dmul_rn(third, dz), ratio);
  sigma[idx] = __dsqrt_rn(__dadd_rn(z_var, __dmul_rn(zi, zi)));
}

// ---- host --------------------------------------------------------------------------------------------------------------
// What the host prepares for one axis.
struct AxisPlan {
  int n = 0, k = 0, m = 0;
  bool closed = false;  // order 1 with three or more cells: the closed form of the first and last coefficient
  RgEnds ends{};
  std::vector<double> t, lu, h;  // knots; factors [n][2 k + 1] (general solve only); basis values [m][RG_H]
  std::vector<int32_t> l;        // [m]
};

bool plan_axis(const double* x, int n, double lo, double hi, int k, const double* xo, int m, AxisPlan& p) {
  p.n = n, p.k = k, p.m = m;
  regrid_knots(x, n, lo, hi, k, p.t);
  p.closed = k == 1 && n >= 3;
  if (p.closed) {
    p.ends.a00 = (x[1] - x[0]) / (x[1] - lo);
    p.ends.a01 = (x[0] - lo) / (x[1] - lo);
    p.ends.b0 = (hi - x[n - 1]) / (hi - x[n - 2]);
    p.ends.b1 = (x[n - 1] - x[n - 2]) / (hi - x[n - 2]);
  } else if (!regrid_factor(x, n, p.t.data(), k, p.lu)) {
    return false;
  }
  p.l.resize(m);
  p.h.assign((size_t)m * RG_H, 0.0);
  for (int i = 0; i < m; ++i) p.l[i] = regrid_basis(p.t.data(), n, k, xo[i], &p.h[(size_t)i * RG_H]);
  return true;
}

template <int K>
void launch_cols(double* w, int nx, int ny, const double* lu, hipStream_t s) {
  hipLaunchKernelGGL(k_solve_cols<K>, dim3((unsigned)((nx + RG_WAVE - 1) / RG_WAVE)), dim3(RG_WAVE), 0, s, w, nx, ny, lu);
}

template <int K>
void launch_rows(double* w, int nx, int ny, const double* lu, hipStream_t s) {
  hipLaunchKernelGGL(k_solve_rows<K>, dim3((unsigned)((ny + RG_TILE - 1) / RG_TILE)), dim3(RG_ROWS_TB), 0, s, w, nx, ny, lu);
}

// Uploads `src`, solves for the coefficients and evaluates them on (xo, yo) into the device array d_out [my][mx].  The
// null stream; e_solve / e_eval are recorded before the solve and before the evaluation when given.  The device buffers
// live until this returns (hipFree waits for the kernels).
int regrid_on_device(const RegridSource& src, const double* xo, int mx, const double* yo, int my, double* d_out,
                     hipEvent_t e_solve, hipEvent_t e_eval) {
  hipStream_t s = nullptr;
  AxisPlan px, py;
  if (!plan_axis(src.gx, src.nx, src.xmin, src.xmax, src.kx, xo, mx, px) ||
      !plan_axis(src.gy, src.ny, src.ymin, src.ymax, src.ky, yo, my, py))
    return fail(GLH_E_INVALID, "regrid: the collocation matrix of the cell centres could not be factored within its band "
                               "(are the centres inside the box, half a cell from its limits?)");
  const size_t cells = (size_t)src.nx * src.ny;
  DevBuf dc, dnan, dlux, dluy, dlx, dly, dhx, dhy;
  CHK(dc.up(src.z, cells * 8));
  if (src.nan) CHK(dnan.up(src.nan, cells));
  if (!px.closed) CHK(dlux.up(px.lu.data(), px.lu.size() * 8));
  if (!py.closed) CHK(dluy.up(py.lu.data(), py.lu.size() * 8));
  CHK(dlx.up(px.l.data(), (size_t)mx * 4));
  CHK(dly.up(py.l.data(), (size_t)my * 4));
  CHK(dhx.up(px.h.data(), px.h.size() * 8));
  CHK(dhy.up(py.h.data(), py.h.size() * 8));
  if (e_solve) HIPCHK(hipEventRecord(e_solve, s));
  double* w = dc.as<double>();
  if (py.closed) {
    hipLaunchKernelGGL(k_ends_cols, dim3((unsigned)((src.nx + RG_WAVE - 1) / RG_WAVE)), dim3(RG_WAVE), 0, s, w, src.nx, src.ny,
                       py.ends);
  } else {
    const double* lu = dluy.as<double>();
    switch (src.ky) {
      case 1: launch_cols<1>(w, src.nx, src.ny, lu, s); break;
      case 2: launch_cols<2>(w, src.nx, src.ny, lu, s); break;
      case 3: launch_cols<3>(w, src.nx, src.ny, lu, s); break;
      case 4: launch_cols<4>(w, src.nx, src.ny, lu, s); break;
      default: launch_cols<5>(w, src.nx, src.ny, lu, s); break;
    }
  }
  HIPCHK(hipGetLastError());
  if (px.closed) {
    hipLaunchKernelGGL(k_ends_rows, dim3((unsigned)((src.ny + RG_WAVE - 1) / RG_WAVE)), dim3(RG_WAVE), 0, s, w, src.nx, src.ny,
                       px.ends);
  } else {
    const double* lu = dlux.as<double>();
    switch (src.kx) {
      case 1: launch_rows<1>(w, src.nx, src.ny, lu, s); break;
      case 2: launch_rows<2>(w, src.nx, src.ny, lu, s); break;
      case 3: launch_rows<3>(w, src.nx, src.ny, lu, s); break;
      case 4: launch_rows<4>(w, src.nx, src.ny, lu, s); break;
      default: launch_rows<5>(w, src.nx, src.ny, lu, s); break;
    }
  }
  HIPCHK(hipGetLastError());
  if (e_eval) HIPCHK(hipEventRecord(e_eval, s));
  const RgEval a{w,  dnan.as<uint8_t>(), src.nx, src.ny, src.kx, src.ky, dlx.as<int32_t>(), dhx.as<double>(),
                 dly.as<int32_t>(), dhy.as<double>(), mx, my, src.use_zmin, src.zmin, src.flip_x, src.flip_y, d_out};
  const size_t outs = (size_t)mx * my;
  hipLaunchKernelGGL(k_eval, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  return GLH_OK;
}

}  // namespace

int regrid_run(const RegridJob& j) {
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<RG_TIMES + 1> ev;
  CHK(ev.create());
  const size_t outs = (size_t)j.mx * j.my;
  DevBuf dout;
  CHK(dout.alloc(outs * 8));
  CHK(ev.record(0, s));
  CHK(regrid_on_device(j.src, j.xo, j.mx, j.yo, j.my, dout.as<double>(), ev.e[1], ev.e[2]));
  CHK(ev.record(3, s));
  CHK(dout.down(j.out, outs * 8));
  CHK(ev.record(4, s));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  ev.report(j.times_ms, RG_TIMES, RG_TIMES);
  return GLH_OK;
}

int zoom_run(const ZoomJob& j) {
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<RG_TIMES + 1> ev;
  CHK(ev.create());
  const size_t cells = (size_t)j.nx * j.ny, outs = (size_t)j.mx * j.my;
  DevBuf da, dout;
  CHK(dout.alloc(outs * 8));
  CHK(ev.record(0, s));
  CHK(da.up(j.a, cells * 8));
  CHK(ev.record(1, s));
  CHK(ev.record(2, s));  // (no solve)
  const double sx = j.mx > 1 ? (double)(j.nx - 1) / (double)(j.mx - 1) : 0.0;
  const double sy = j.my > 1 ? (double)(j.ny - 1) / (double)(j.my - 1) : 0.0;
  hipLaunchKernelGGL(k_zoom_linear, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, da.as<double>(), j.nx, j.ny, j.mx,
                     j.my, sx, sy, dout.as<double>());
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  CHK(dout.down(j.out, outs * 8));
  CHK(ev.record(4, s));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  ev.report(j.times_ms, RG_TIMES, RG_TIMES);
  return GLH_OK;
}

int interpolate_run(const InterpolateJob& j) {
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<RG_TIMES + 1> ev;
  CHK(ev.create());
  const size_t cells = (size_t)j.nx * j.ny;
  DevBuf dm0, dm1, ds0, ds1, dz, dsig;
  CHK(dz.alloc(cells * 8));
  if (j.sigma) CHK(dsig.alloc(cells * 8));
  CHK(ev.record(0, s));
  CHK(dm0.up(j.m0, cells * 8));
  if (j.m1_src)
    CHK(dm1.alloc(cells * 8));
  else
    CHK(dm1.up(j.m1, cells * 8));
  if (j.sigma) {
    CHK(ds0.up(j.s0, cells * 8));
    if (j.s1_src)
      CHK(ds1.alloc(cells * 8));
    else
      CHK(ds1.up(j.s1, cells * 8));
  }
  CHK(ev.record(1, s));  // (the sources of the regridding are uploaded within the next span)
  if (j.m1_src) CHK(regrid_on_device(*j.m1_src, j.xo, j.nx, j.yo, j.ny, dm1.as<double>(), nullptr, nullptr));
  if (j.sigma && j.s1_src) CHK(regrid_on_device(*j.s1_src, j.xo, j.nx, j.yo, j.ny, ds1.as<double>(), nullptr, nullptr));
  CHK(ev.record(2, s));
  hipLaunchKernelGGL(k_blend, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, dm0.as<double>(), dm1.as<double>(),
                     ds0.as<double>(), ds1.as<double>(), cells, j.scale, j.scale2, j.third, j.ratio, dz.as<double>(),
                     j.sigma ? dsig.as<double>() : nullptr);
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  CHK(dz.down(j.z, cells * 8));
  if (j.sigma) CHK(dsig.down(j.sigma, cells * 8));
  CHK(ev.record(4, s));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  ev.report(j.times_ms, RG_TIMES, RG_TIMES);
  return GLH_OK;
}

}  // namespace glh
