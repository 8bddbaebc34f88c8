// glh_horizon.hip -- Raster.horizon (raster.py:1391-1463) on the device: the work behind glh_stage_horizon
// (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls horizon_run).
//
// The reference walks one helpers.bresenham_line (helpers.py:1139-1180) per heading from the origin's cell to the cell
// where the ray leaves the raster, and keeps the cell of greatest elevation ratio dz / distance unless it is the line's
// last cell with a value.  Here a workgroup takes one (origin, heading) and its lanes stride along the line; nobody walks:
//
//   cell k of a line.  After the reference's swaps (steep: the axes; x1 > x2: the endpoints, and the list is reversed at
//   the end) the loop visits x = x1 + j, j = 0 .. dx, and keeps 0 <= error < dx after every step: it starts at e0 = dx / 2,
//   loses ady <= dx per step and gains dx back when it falls below 0.  After j steps error = e0 - j ady + s dx with s the
//   y steps taken so far, so s is the smallest count that keeps the sum >= 0:  s = max(0, ceil((j ady - e0) / dx)),
//   y = y1 + ystep s.  The reversed list maps k -> dx - k.  k = 0 is the origin's cell, which the reference skips.
//
//   per line.  np.nanargmax: the cell with a value of greatest ratio, the lowest k among equals; the heading has a
//   horizon point only if a cell with a value lies beyond it (raster.py:1456).  (ratio, k) and the last k with a value are
//   reduced across a wave by shuffles and across the waves through LDS, in a fixed order: no atomics, the same bytes on
//   every run.
//
// Every float64 expression is evaluated operation by operation as NumPy does, with the explicit round-to-nearest
// intrinsics (the library is built with -ffp-contract=off besides); sqrt and / are the correctly rounded ones, not
// glh_math.h's sqrt_nr / rcp_nr, which are within an ulp and belong to its fast arithmetic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/glimpse_hip.h"
#include "glh_horizon.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int HZ_WAVE = 64;
constexpr int HZ_SHORT = 256;  // a job whose longest line has at most this many cells: one wave per line; else four

struct HzArgs {
  const void* z;  // [ny][nx] float64, or float32 when `f32`
  int nx, ny;
  int f32;   // the reference's dz is float32 (a float32 DEM and an origin NumPy does not promote with)
  int corr;  // helpers.elevation_corrections (helpers.py:1790) added to dz
  int n;     // headings per origin
  double xlim0, ylim0, d0, d1;
  double cnum, cden;      // refraction - 1, 2 * radius
  const double* origins;  // [m][3]
  const int32_t* starts;  // [m][2] (col, row)
  const int32_t* ends;    // [m][n][2] (col, row)
  int32_t* cell;          // [m][n][2] (row, col)
  double* dz;             // [m][n]
};

struct HzLine {
  int x1, y1, dx, ady, e0, ystep;
  bool steep, swapped;
};

__device__ __forceinline__ HzLine hz_line(int sx, int sy, int ex, int ey) {
  HzLine l;
  int x1 = sx, y1 = sy, x2 = ex, y2 = ey;
  l.steep = abs(y2 - y1) > abs(x2 - x1);
  if (l.steep) {
    x1 = sy, y1 = sx, x2 = ey, y2 = ex;
  }
  l.swapped = x1 > x2;
  if (l.swapped) {
    int t = x1;
    x1 = x2, x2 = t;
    t = y1;
    y1 = y2, y2 = t;
  }
  l.x1 = x1, l.y1 = y1;
  l.dx = x2 - x1;
  l.ady = abs(y2 - y1);
  l.e0 = l.dx / 2;
  l.ystep = y1 < y2 ? 1 : -1;
  return l;
}

// Cell k = 1 .. dx of the line (so dx >= 1).  j ady is formed in 64 bits; dx and ady run along different axes of the grid,
// so j ady <= dx ady < nx ny < 2^31 and the rounded-up numerator stays below 2^32: the division is an unsigned 32-bit one.
__device__ __forceinline__ void hz_cell(const HzLine& l, int k, int& col, int& row) {
  const int j = l.swapped ? l.dx - k : k;
  const long long num = (long long)j * l.ady - l.e0;
  const int s = num > 0 ? (int)((uint32_t)(num + l.dx - 1) / (uint32_t)l.dx) : 0;
  const int x = l.x1 + j, y = l.y1 + l.ystep * s;
  col = l.steep ? y : x;
  row = l.steep ? x : y;
}

__device__ __forceinline__ double hz_dz(const HzArgs& a, int row, int col, double oz) {
  const size_t i = (size_t)row * a.nx + col;
  if (a.f32) return (double)__fsub_rn(static_cast<const float*>(a.z)[i], (float)oz);  // float32, widened afterwards
  return __dsub_rn(static_cast<const double*>(a.z)[i], oz);
}

// candidate a beats b: the greater ratio, the lowest k among equals.  k < 0: no candidate.
__device__ __forceinline__ bool hz_better(double ra, int ka, double rb, int kb) {
  return ka >= 0 && (kb < 0 || ra > rb || (ra == rb && ka < kb));
}

template <int TB>
__global__ void __launch_bounds__(TB) k_horizon(HzArgs a) {
  const int line = blockIdx.x;  // origin * n + heading
  const int o = line / a.n;
  const double ox = a.origins[3 * o], oy = a.origins[3 * o + 1], oz = a.origins[3 * o + 2];
  const HzLine l = hz_line(a.starts[2 * o], a.starts[2 * o + 1], a.ends[2 * (size_t)line], a.ends[2 * (size_t)line + 1]);
  double br = 0.0;
  int bk = -1, last = -1;
  for (long long kk = 1 + (long long)threadIdx.x; kk <= l.dx; kk += TB) {
    const int k = (int)kk;
    int col, row;
    hz_cell(l, k, col, row);
    const double dz = hz_dz(a, row, col, oz);
    if (isnan(dz)) continue;
    // rowcol_to_xy (raster.py:475-476), dxy = sum((xy - origin) ** 2) (:1449)
    const double x = __dadd_rn(__dmul_rn(__dadd_rn((double)col, 0.5), a.d0), a.xlim0);
    const double y = __dadd_rn(__dmul_rn(__dadd_rn((double)row, 0.5), a.d1), a.ylim0);
    const double ex = __dsub_rn(x, ox), ey = __dsub_rn(y, oy);
    const double dxy = __dadd_rn(__dmul_rn(ex, ex), __dmul_rn(ey, ey));
    const double num = a.corr ? __dadd_rn(dz, __ddiv_rn(__dmul_rn(a.cnum, dxy), a.cden)) : dz;
    const double r = __ddiv_rn(num, __dsqrt_rn(dxy));
    if (hz_better(r, k, br, bk)) br = r, bk = k;
    last = k;
  }
  // the wave: a butterfly; (ratio, k) pairs are totally ordered (no two share a k), so every lane ends with the same one
  for (int off = HZ_WAVE / 2; off; off >>= 1) {
    const double r2 = __shfl_xor(br, off);
    const int k2 = __shfl_xor(bk, off), l2 = __shfl_xor(last, off);
    if (hz_better(r2, k2, br, bk)) br = r2, bk = k2;
    last = last > l2 ? last : l2;
  }
  if constexpr (TB > HZ_WAVE) {
    __shared__ double s_r[TB / HZ_WAVE];
    __shared__ int s_k[TB / HZ_WAVE], s_l[TB / HZ_WAVE];
    if ((threadIdx.x & (HZ_WAVE - 1)) == 0) {
      const int w = threadIdx.x / HZ_WAVE;
      s_r[w] = br, s_k[w] = bk, s_l[w] = last;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int w = 1; w < TB / HZ_WAVE; ++w) {
        if (hz_better(s_r[w], s_k[w], br, bk)) br = s_r[w], bk = s_k[w];
        last = last > s_l[w] ? last : s_l[w];
      }
  }
  if (threadIdx.x != 0) return;
  int col = -1, row = -1;
  double dz = NAN;
  if (bk >= 0 && last > bk) {  // "Save point if not last non-nan value" (raster.py:1456)
    hz_cell(l, bk, col, row);
    dz = hz_dz(a, row, col, oz);
  }
  a.cell[2 * (size_t)line] = row;
  a.cell[2 * (size_t)line + 1] = col;
  a.dz[line] = dz;
}

// ---- host --------------------------------------------------------------------------------------------------------------
}  // namespace

int horizon_run(const HorizonJob& j) {
  const size_t cells = (size_t)j.nx * j.ny, lines = (size_t)j.m * j.n;
  // the longest line of the job chooses the workgroup: a line has max(|dx|, |dy|) cells after its start
  int longest = 0;
  for (int o = 0; o < j.m; ++o)
    for (int h = 0; h < j.n; ++h) {
      const int32_t* e = j.ends + 2 * ((size_t)o * j.n + h);
      const int ax = abs(e[0] - j.starts[2 * o]), ay = abs(e[1] - j.starts[2 * o + 1]);
      const int len = ax > ay ? ax : ay;
      if (len > longest) longest = len;
    }
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernel)
  StageEvents<HZ_TIMES + 1> ev;
  CHK(ev.create());
  const size_t zbytes = cells * (j.f32 ? 4 : 8);
  DevBuf dz, dorg, dstart, dend, dcell, dout;
  CHK(dz.alloc(zbytes));
  CHK(dorg.alloc((size_t)j.m * 24));
  CHK(dstart.alloc((size_t)j.m * 8));
  CHK(dend.alloc(lines * 8));
  CHK(dcell.alloc(lines * 8));
  CHK(dout.alloc(lines * 8));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dz.p, j.z, zbytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dorg.p, j.origins, (size_t)j.m * 24, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dstart.p, j.starts, (size_t)j.m * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dend.p, j.ends, lines * 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  const HzArgs a{dz.p, j.nx, j.ny, j.f32, j.correction, j.n, j.xlim0, j.ylim0, j.d0, j.d1, j.refraction - 1.0, 2.0 * j.radius,
                 dorg.as<double>(), dstart.as<int32_t>(), dend.as<int32_t>(), dcell.as<int32_t>(), dout.as<double>()};
  if (longest <= HZ_SHORT)
    hipLaunchKernelGGL(k_horizon<HZ_WAVE>, dim3((unsigned)lines), dim3(HZ_WAVE), 0, s, a);
  else
    hipLaunchKernelGGL(k_horizon<4 * HZ_WAVE>, dim3((unsigned)lines), dim3(4 * HZ_WAVE), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  CHK(dcell.down(j.cell, lines * 8));
  CHK(dout.down(j.dz, lines * 8));
  CHK(ev.record(3, s));
  HIPCHK(hipEventSynchronize(ev.e[3]));
  ev.report(j.times_ms, HZ_TIMES, HZ_TIMES);
  return GLH_OK;
}

}  // namespace glh
