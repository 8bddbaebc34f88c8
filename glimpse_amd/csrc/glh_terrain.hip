// glh_terrain.hip -- Raster.gradient (raster.py:1465-1474), Raster.hillshade (raster.py:1249-1264) and
// helpers.polygons_to_mask (helpers.py:1701-1768) on the device: the work behind glh_stage_gradient, glh_stage_hillshade
// and glh_stage_polygon_mask (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls the *_run here).
//
// What the reference computes, and so what is computed here, operation by operation:
//   gradient   np.gradient(array, d[1], d[0]): along a line of n >= 2 cells with spacing h, (f[i+1] - f[i-1]) / (2 h) inside
//              and (f[1] - f[0]) / h, (f[n-1] - f[n-2]) / h at the ends.  The difference is formed in the array's dtype, the
//              quotient in float64 against the float64 spacing and rounded to the array's dtype (for float64 arrays that is
//              one correctly rounded division: NumPy's bits).
//   hillshade  matplotlib's LightSource.hillshade: the gradients e_dx, e_dy of vert_exag * array (the product in the array's
//              dtype), the normal (-e_dx, -e_dy, 1) over sqrt((n0^2 + n1^2) + n2^2), the intensity n0 l0 + n1 l1 + n2 l2
//              summed left to right against the light direction; imin, imax over all cells (NaN if any cell is NaN);
//              I *= fraction; if imax - imin > 1e-6: I = (I - imin) / (imax - imin); clip to [0, 1].
//   polygons   per ring the even-odd rule on cell centres (c + 0.5, r + 0.5): an edge with y1 != y2 crosses row r when
//              min(y1, y2) <= r + 0.5 < max(y1, y2), at x = x1 + (cy - y1) * (x2 - x1) / (y2 - y1), and toggles every cell of
//              the row with c + 0.5 > x.  Polygon rings set the cells of odd parity, hole rings then clear them.
// Every operation is correctly rounded (the library is built with -ffp-contract=off and the divisions and the square root are
// the round-to-nearest intrinsics), so the results equal the NumPy restatement of tests/terrain_restatement.py in every bit.
// A NaN result is written as the one quiet positive NaN (np.nan's bits): which NaN an operation returns differs between
// processors, and NumPy propagates the positive NaN a DEM holds.
//
// Kernels: k_tr_gradient and k_tr_intensity are one stencil over tiles of 64 x 16 cells, a thread per column and four rows
// of the tile; the four neighbours are read straight from memory -- lanes are neighbouring columns, so every read is a
// coalesced row segment, and a row is read again by the rows above and below it out of the caches.  k_tr_intensity also
// reduces its tile's minimum, maximum and saw-NaN flag (wave shuffles, then LDS) into one partial per workgroup;
// k_tr_reduce folds the partials in a fixed order (min and max are exact, so any fixed order gives the same value);
// k_tr_normalise scales, normalises and clips the stored intensity in place.  No floating-point atomics.
// k_pm_cross is a thread per (row, edge) pair of one ring inside the ring's bounding rows: a crossing toggles the bit of
// the first toggled column with atomicXor on a 32-bit word (XOR commutes: the bits do not depend on scheduling).  k_pm_fill
// is a wave per row: the prefix XOR of the row's toggle bits (in the word by shifts, across the wave by a ballot) is the
// parity of every cell; cells of odd parity are written -- 1 for a polygon, 0 for a hole -- 64 neighbouring columns per
// store, and the toggle words are put back to zero for the next ring.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_terrain.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int TR_TB = 256;
constexpr int TR_TW = 64, TR_TH = 16;  // cells of one stencil tile (columns, rows)
constexpr int TR_ROWS_PER_PASS = TR_TB / TR_TW;

// ---- the stencil -------------------------------------------------------------------------------------------------------
// np.gradient along one line: `lo`, `hi` the two cells read, `den` h at the ends and 2 h inside
template <typename T>
__device__ __forceinline__ T tr_quotient(T hi, T lo, double den) {
  const T diff = hi - lo;
  return (T)__ddiv_rn((double)diff, den);
}

struct TrStencilArgs {
  const void* z;  // [ny][nx]
  int nx, ny;
  int tiles_x;
  double hx, hy;  // spacing along the columns (x) and along the rows (y)
  // gradient
  void* dzdx;
  void* dzdy;
  // hillshade
  double ve;          // vert_exag
  double l0, l1, l2;  // light direction
  double* raw;        // [ny][nx] the intensity before the contrast stretch
  double* part;       // [3][tiles] minimum, maximum, saw-NaN per workgroup
  int tiles;
};

// the two gradients of z (SCALED: of scale * z, the product in T) at (r, c)
template <typename T, bool SCALED>
__device__ __forceinline__ void tr_gradients(const TrStencilArgs& p, int r, int c, T scale, T& gx, T& gy) {
  const T* z = static_cast<const T*>(p.z);
  const int cl = c > 0 ? c - 1 : 0, ch = c < p.nx - 1 ? c + 1 : p.nx - 1;
  const int rl = r > 0 ? r - 1 : 0, rh = r < p.ny - 1 ? r + 1 : p.ny - 1;
  const size_t row = (size_t)r * p.nx;
  T xl = z[row + cl], xh = z[row + ch], yl = z[(size_t)rl * p.nx + c], yh = z[(size_t)rh * p.nx + c];
  if (SCALED) {
    xl = scale * xl;
    xh = scale * xh;
    yl = scale * yl;
    yh = scale * yh;
  }
  gx = tr_quotient<T>(xh, xl, ch - cl == 2 ? 2.0 * p.hx : p.hx);
  gy = tr_quotient<T>(yh, yl, rh - rl == 2 ? 2.0 * p.hy : p.hy);
}

template <typename T>
__global__ void __launch_bounds__(TR_TB) k_tr_gradient(TrStencilArgs p) {
  const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
  const int c = tx * TR_TW + (threadIdx.x & (TR_TW - 1));
  const int r0 = ty * TR_TH + (threadIdx.x / TR_TW);
  if (c >= p.nx) return;
  T* dzdx = static_cast<T*>(p.dzdx);
  T* dzdy = static_cast<T*>(p.dzdy);
  for (int k = 0; k < TR_TH; k += TR_ROWS_PER_PASS) {
    const int r = r0 + k;
    if (r >= p.ny) break;
    T gx, gy;
    tr_gradients<T, false>(p, r, c, (T)1, gx, gy);
    const size_t g = (size_t)r * p.nx + c;
    dzdx[g] = gx != gx ? (T)NAN : gx;  // (one NaN, the quiet positive one: which NaN an operation returns is the hardware's)
    dzdy[g] = gy != gy ? (T)NAN : gy;
  }
}

struct TrStats {
  double lo, hi;
  int nan;
};

__device__ __forceinline__ void tr_fold(TrStats& a, double lo, double hi, int nan) {
  a.lo = lo < a.lo ? lo : a.lo;
  a.hi = hi > a.hi ? hi : a.hi;
  a.nan |= nan;
}

// every thread of the workgroup calls this; thread 0 returns the workgroup's statistics
__device__ __forceinline__ TrStats tr_block_reduce(TrStats s) {
  __shared__ double s_lo[TR_TB / 64], s_hi[TR_TB / 64];
  __shared__ int s_nan[TR_TB / 64];
  for (int off = 32; off > 0; off >>= 1) tr_fold(s, __shfl_xor(s.lo, off), __shfl_xor(s.hi, off), __shfl_xor(s.nan, off));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_lo[wave] = s.lo;
    s_hi[wave] = s.hi;
    s_nan[wave] = s.nan;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < TR_TB / 64; ++w) tr_fold(s, s_lo[w], s_hi[w], s_nan[w]);
  return s;
}

// the intensity of the cell (r, c) before the contrast stretch
template <typename T>
__device__ __forceinline__ double tr_raw_intensity(const TrStencilArgs& p, int r, int c) {
  T gx, gy;
  tr_gradients<T, true>(p, r, c, (T)p.ve, gx, gy);
  const double n0 = -(double)gx, n1 = -(double)gy;
  const double mag = __dsqrt_rn((n0 * n0 + n1 * n1) + 1.0);
  const double u0 = __ddiv_rn(n0, mag), u1 = __ddiv_rn(n1, mag), u2 = __ddiv_rn(1.0, mag);
  return (u0 * p.l0 + u1 * p.l1) + u2 * p.l2;
}

template <typename T>
__global__ void __launch_bounds__(TR_TB) k_tr_intensity(TrStencilArgs p) {
  const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
  const int c = tx * TR_TW + (threadIdx.x & (TR_TW - 1));
  const int r0 = ty * TR_TH + (threadIdx.x / TR_TW);
  TrStats s{INFINITY, -INFINITY, 0};
  if (c < p.nx) {
    for (int k = 0; k < TR_TH; k += TR_ROWS_PER_PASS) {
      const int r = r0 + k;
      if (r >= p.ny) break;
      const double v = tr_raw_intensity<T>(p, r, c);
      p.raw[(size_t)r * p.nx + c] = v;
      if (v != v)
        s.nan = 1;
      else
        tr_fold(s, v, v, 0);
    }
  }
  s = tr_block_reduce(s);
  if (threadIdx.x == 0) {
    p.part[blockIdx.x] = s.lo;
    p.part[p.tiles + blockIdx.x] = s.hi;
    p.part[2 * (size_t)p.tiles + blockIdx.x] = (double)s.nan;
  }
}

// one workgroup: stats[0] = imin, stats[1] = imax (both NaN when a cell is NaN, as NumPy's min and max are)
__global__ void __launch_bounds__(TR_TB) k_tr_reduce(const double* part, int tiles, double* stats) {
  TrStats s{INFINITY, -INFINITY, 0};
  for (int i = threadIdx.x; i < tiles; i += TR_TB) tr_fold(s, part[i], part[tiles + i], part[2 * (size_t)tiles + i] != 0.0);
  s = tr_block_reduce(s);
  if (threadIdx.x == 0) {
    stats[0] = s.nan ? NAN : s.lo;
    stats[1] = s.nan ? NAN : s.hi;
  }
}

// I *= fraction; the stretch when the range allows it; np.clip(I, 0, 1)
__device__ __forceinline__ double tr_stretch(double x, const double* stats, double fraction) {
  const double imin = stats[0], range = stats[1] - stats[0];
  x = x * fraction;
  if (range > 1e-6) {  // (false when the range is NaN)
    x = x - imin;
    x = __ddiv_rn(x, range);
  }
  if (x != x) return NAN;  // (the quiet positive one, as in k_tr_gradient)
  x = x > 0.0 ? x : 0.0;   // (-0.0 becomes 0.0)
  return x < 1.0 ? x : 1.0;
}

__global__ void __launch_bounds__(TR_TB) k_tr_normalise(double* v, size_t n, const double* stats, double fraction) {
  const size_t i = (size_t)blockIdx.x * TR_TB + threadIdx.x;
  if (i < n) v[i] = tr_stretch(v[i], stats, fraction);
}

// ---- polygons ----------------------------------------------------------------------------------------------------------
struct PmRingArgs {
  const double* xy;  // [n][2] all the rings' vertices
  int v0, nv;        // this ring's first vertex and its number of vertices
  int rb0, nrows;    // the ring's bounding rows rb0 .. rb0 + nrows - 1, inside the grid
  int cb0, cb1;      // its bounding columns, inside the grid
  int wpr;           // 32-bit toggle words per row
  int nx;
  uint32_t* bits;  // [ny][wpr]
  uint8_t* out;    // [ny][nx]
  int hole;
};

__global__ void __launch_bounds__(TR_TB) k_pm_cross(PmRingArgs p) {
  const size_t i = (size_t)blockIdx.x * TR_TB + threadIdx.x;
  if (i >= (size_t)p.nrows * p.nv) return;
  const int row = p.rb0 + (int)(i / p.nv), e = (int)(i % p.nv);
  const int e2 = e + 1 == p.nv ? 0 : e + 1;  // the ring is closed implicitly
  const double x1 = p.xy[2 * (size_t)(p.v0 + e)], y1 = p.xy[2 * (size_t)(p.v0 + e) + 1];
  const double x2 = p.xy[2 * (size_t)(p.v0 + e2)], y2 = p.xy[2 * (size_t)(p.v0 + e2) + 1];
  if (y1 == y2) return;  // horizontal edges do not count
  const double cy = row + 0.5;
  const double lo = y1 < y2 ? y1 : y2, hi = y1 < y2 ? y2 : y1;
  if (!(lo <= cy && cy < hi)) return;
  const double x = __dadd_rn(x1, __ddiv_rn(__dmul_rn(cy - y1, x2 - x1), y2 - y1));
  // the first column with c + 0.5 > x, within the ring's columns: none for a NaN, none at or beyond cb1 + 0.5
  if (!(x < p.cb1 + 0.5)) return;
  int c0 = p.cb0;
  if (x >= (double)p.cb0) {
    c0 = (int)floor(x);
    if (!(c0 + 0.5 > x)) ++c0;
  }
  atomicXor(&p.bits[(size_t)row * p.wpr + (c0 >> 5)], 1u << (c0 & 31));
}

__global__ void __launch_bounds__(TR_TB) k_pm_fill(PmRingArgs p) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * (TR_TB / 64) + (threadIdx.x >> 6);
  if (k >= p.nrows) return;  // (the whole wave)
  const int row = p.rb0 + k;
  const int w_first = p.cb0 >> 5, w_last = p.cb1 >> 5;
  uint32_t* bits = p.bits + (size_t)row * p.wpr;
  uint8_t* out = p.out + (size_t)row * p.nx;
  const uint8_t value = p.hole ? 0 : 1;
  unsigned carry = 0;  // the parity that enters this group of 64 words
  for (int wbase = w_first; wbase <= w_last; wbase += 64) {
    const int w = wbase + lane;
    uint32_t v = 0;
    if (w <= w_last) {
      v = bits[w];
      if (v) bits[w] = 0;
    }
    if (__ballot(v != 0) == 0 && carry == 0) continue;
    v ^= v << 1;  // bit b: the parity of bits 0 .. b
    v ^= v << 2;
    v ^= v << 4;
    v ^= v << 8;
    v ^= v << 16;
    const unsigned long long odd = __ballot(v >> 31);
    if ((carry ^ (unsigned)__popcll(odd & ((1ull << lane) - 1ull))) & 1u) v = ~v;
    carry ^= (unsigned)__popcll(odd) & 1u;
    for (int j = 0; j < 32; ++j) {  // 64 neighbouring columns per store
      const int src = 2 * j + (lane >> 5);
      const uint32_t wv = (uint32_t)__shfl((int)v, src);
      const int col = (wbase + src) * 32 + (lane & 31);
      if (((wv >> (lane & 31)) & 1u) && col >= p.cb0 && col <= p.cb1) out[col] = value;
    }
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
}  // namespace

int gradient_run(const GradientJob& j) {
  const size_t n = (size_t)j.nx * j.ny, bytes = n * (j.f32 ? 4 : 8);
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<TR_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dz, dx, dy;
  CHK(dz.alloc(bytes));
  CHK(dx.alloc(bytes));
  CHK(dy.alloc(bytes));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dz.p, j.z, bytes, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  TrStencilArgs a{};
  a.z = dz.p;
  a.nx = j.nx;
  a.ny = j.ny;
  a.tiles_x = (j.nx + TR_TW - 1) / TR_TW;
  a.hx = j.d0;
  a.hy = j.d1;
  a.dzdx = dx.p;
  a.dzdy = dy.p;
  const dim3 grid((unsigned)((size_t)a.tiles_x * ((j.ny + TR_TH - 1) / TR_TH)));
  if (j.f32)
    hipLaunchKernelGGL(k_tr_gradient<float>, grid, dim3(TR_TB), 0, s, a);
  else
    hipLaunchKernelGGL(k_tr_gradient<double>, grid, dim3(TR_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  CHK(dx.down(j.dzdx, bytes));
  CHK(dy.down(j.dzdy, bytes));
  CHK(ev.record(3, s));
  HIPCHK(hipEventSynchronize(ev.e[3]));
  ev.report(j.times_ms, 3, TR_TIMES);
  return GLH_OK;
}

int hillshade_run(const HillshadeJob& j) {
  const size_t n = (size_t)j.nx * j.ny, bytes = n * (j.f32 ? 4 : 8);
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<TR_TIMES + 1> ev;
  CHK(ev.create());
  TrStencilArgs a{};
  a.nx = j.nx;
  a.ny = j.ny;
  a.tiles_x = (j.nx + TR_TW - 1) / TR_TW;
  a.tiles = a.tiles_x * ((j.ny + TR_TH - 1) / TR_TH);
  DevBuf dz, draw, dpart, dstats;
  CHK(dz.alloc(bytes));
  CHK(draw.alloc(n * 8));
  CHK(dpart.alloc((size_t)a.tiles * 3 * 8));
  CHK(dstats.alloc(2 * 8));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dz.p, j.z, bytes, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  a.z = dz.p;
  a.hx = j.d0;
  a.hy = j.d1;
  a.ve = j.vert_exag;
  a.l0 = j.direction[0];
  a.l1 = j.direction[1];
  a.l2 = j.direction[2];
  a.raw = draw.as<double>();
  a.part = dpart.as<double>();
  if (j.f32)
    hipLaunchKernelGGL(k_tr_intensity<float>, dim3((unsigned)a.tiles), dim3(TR_TB), 0, s, a);
  else
    hipLaunchKernelGGL(k_tr_intensity<double>, dim3((unsigned)a.tiles), dim3(TR_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  hipLaunchKernelGGL(k_tr_reduce, dim3(1), dim3(TR_TB), 0, s, a.part, a.tiles, dstats.as<double>());
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  hipLaunchKernelGGL(k_tr_normalise, dim3((unsigned)((n + TR_TB - 1) / TR_TB)), dim3(TR_TB), 0, s, a.raw, n,
                     dstats.as<const double>(), j.fraction);
  HIPCHK(hipGetLastError());
  CHK(ev.record(4, s));
  CHK(draw.down(j.out, n * 8));
  CHK(ev.record(5, s));
  HIPCHK(hipEventSynchronize(ev.e[5]));
  ev.report(j.times_ms, 5, TR_TIMES);
  return GLH_OK;
}

int polygon_mask_run(const PolygonMaskJob& j) {
  const size_t n = (size_t)j.nx * j.ny;
  const int rings = j.n_polygons + j.n_holes, wpr = (j.nx + 31) / 32;
  const size_t n_vertices = (size_t)j.ring_off[rings];
  // per ring its bounding rows and columns inside the grid, a cell wider than the vertices on every side (the rule is
  // tested per crossing on the device; the bounds only have to hold every cell it can touch)
  struct Ring {
    int v0, nv, rb0, rb1, cb0, cb1;
  };
  std::vector<Ring> ring((size_t)rings);
  int n_live = 0;
  for (int k = 0; k < rings; ++k) {
    const int v0 = j.ring_off[k], nv = j.ring_off[k + 1] - v0;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int v = v0; v < v0 + nv; ++v) {
      const double x = j.xy[2 * (size_t)v], y = j.xy[2 * (size_t)v + 1];
      xmin = x < xmin ? x : xmin;
      xmax = x > xmax ? x : xmax;
      ymin = y < ymin ? y : ymin;
      ymax = y > ymax ? y : ymax;
    }
    Ring r{v0, nv, 0, -1, 0, -1};
    if (xmax >= 0.0 && xmin < (double)j.nx && ymax >= 0.0 && ymin < (double)j.ny) {
      const double c0 = std::floor(xmin) - 1.0, c1 = std::floor(xmax) + 1.0;
      const double r0 = std::floor(ymin) - 1.0, r1 = std::floor(ymax) + 1.0;
      r.cb0 = c0 > 0.0 ? (int)c0 : 0;
      r.cb1 = c1 < (double)(j.nx - 1) ? (int)c1 : j.nx - 1;
      r.rb0 = r0 > 0.0 ? (int)r0 : 0;
      r.rb1 = r1 < (double)(j.ny - 1) ? (int)r1 : j.ny - 1;
      if (((size_t)(r.rb1 - r.rb0 + 1) * nv + TR_TB - 1) / TR_TB > 0x7fffffffull)
        return fail(GLH_E_UNSUPPORTED, "polygon_mask: ring %d: %d rows x %d edges is more than one launch holds", k,
                    r.rb1 - r.rb0 + 1, nv);
      ++n_live;
    }
    ring[k] = r;
  }
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<TR_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dxy, dbits, dout;
  CHK(dxy.alloc(n_vertices * 16));
  CHK(dbits.alloc((size_t)j.ny * wpr * 4));
  CHK(dout.alloc(n));
  CHK(ev.record(0, s));
  if (n_live) HIPCHK(hipMemcpy(dxy.p, j.xy, n_vertices * 16, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(dbits.p, 0, (size_t)j.ny * wpr * 4, s));
  HIPCHK(hipMemsetAsync(dout.p, 0, n, s));
  CHK(ev.record(1, s));
  for (int k = 0; k < rings; ++k) {
    const Ring& r = ring[k];
    if (r.rb1 < r.rb0 || r.cb1 < r.cb0) continue;
    const int nrows = r.rb1 - r.rb0 + 1;
    const PmRingArgs a{dxy.as<const double>(), r.v0, r.nv, r.rb0, nrows, r.cb0, r.cb1, wpr, j.nx,
                       dbits.as<uint32_t>(), dout.as<uint8_t>(), k >= j.n_polygons};
    hipLaunchKernelGGL(k_pm_cross, dim3((unsigned)(((size_t)nrows * r.nv + TR_TB - 1) / TR_TB)), dim3(TR_TB), 0, s, a);
    hipLaunchKernelGGL(k_pm_fill, dim3((unsigned)((nrows + TR_TB / 64 - 1) / (TR_TB / 64))), dim3(TR_TB), 0, s, a);
  }
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  CHK(dout.down(j.out, n));
  CHK(ev.record(3, s));
  HIPCHK(hipEventSynchronize(ev.e[3]));
  ev.report(j.times_ms, 3, TR_TIMES);
  return GLH_OK;
}

}  // namespace glh
