// glh_viewshed.hip -- Raster.viewshed (raster.py:1293-1389) on the device: the work behind glh_stage_viewshed
// (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls viewshed_run).  A translation unit of its own:
// it is the only one that includes rocPRIM (the device radix sort), which takes a while to compile.
//
// The reference's algorithm, stage by stage (its answers are pinned by tests/golden/g28_viewshed.npz, quirks included):
//   1. per cell: offsets from the origin, ring number (distance in cells, rounded), heading, elevation ratio dz / dxy;
//   2. the cells ordered as np.lexsort((heading, ring)): a stable radix sort on the order-preserving 64-bit image of the
//      heading, then a stable radix sort on the ring number;
//   3. ring after ring (the non-empty ones, ascending; ring 0 is never processed when other rings exist): the previous
//      ring's running maximum interpolated to each cell's heading as np.interp(..., period=2 pi) does, visible = elevation
//      > maximum, and the new running maximum.  One launch per ring; nothing waits on another workgroup.
// Every float64 expression is evaluated operation by operation as NumPy does (the library is built with -ffp-contract=off,
// and the expressions whose contraction would move a cell to another ring use the explicit round-to-nearest intrinsics).
#include <hip/hip_runtime.h>

#include <cstring>  // (before rocPRIM: its headers call the host memset)

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_viewshed.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int VS_TB = 256;

// ---- stage 1 ---------------------------------------------------------------------------------------------------------
// the order-preserving image of a double: a < b  <=>  image(a) < image(b) as unsigned integers (-0.0 before +0.0)
__device__ __forceinline__ uint64_t heading_image(double h) {
  const uint64_t b = (uint64_t)__double_as_longlong(h);
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double heading_of(uint64_t k) {
  const uint64_t b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
  return __longlong_as_double((long long)b);
}

struct VsCellArgs {
  const void* z;      // [ny][nx] float64, or float32 when `f32`
  const double* x;    // [nx] Grid.x as NumPy made it
  const double* y;    // [ny]
  int nx, ny;
  int f32;            // the reference's dz is float32 (a float32 DEM and an origin NumPy does not promote with)
  int corr;           // helpers.elevation_corrections (helpers.py:1790) added to dz
  double inv_d;       // 1 / abs(d[0])
  double ox, oy, oz;
  double cnum, cden;  // refraction - 1, 2 * radius
  uint64_t* hkey;     // [n] heading_image(heading)
  double* elev;       // [n]
  uint32_t* ring;     // [n]
  uint32_t* idx;      // [n] 0 .. n - 1
  uint32_t* hist;     // [nbins] cells per ring number
  int nbins;
  int* err;           // set when a ring number does not fit the histogram (the host sized it from the corners)
};

__global__ void __launch_bounds__(VS_TB) k_vs_cells(VsCellArgs a) {
  const int col = blockIdx.x * VS_TB + threadIdx.x, row = blockIdx.y;
  if (col >= a.nx) return;
  const size_t i = (size_t)row * a.nx + col;
  const double dx = __dsub_rn(a.x[col], a.ox), dy = __dsub_rn(a.y[row], a.oy);
  const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));  // dx ** 2 + dy ** 2 (raster.py:1321)
  const double c = a.corr ? __ddiv_rn(__dmul_rn(a.cnum, d2), a.cden) : 0.0;
  double dz;
  if (a.f32) {
    // dz = array.ravel() - origin[2] in float32; `dz += corrections` adds in float64 and rounds the sum back to float32
    float dzf = __fsub_rn(static_cast<const float*>(a.z)[i], (float)a.oz);
    if (a.corr) dzf = (float)__dadd_rn((double)dzf, c);
    dz = (double)dzf;
  } else {
    dz = __dsub_rn(static_cast<const double*>(a.z)[i], a.oz);
    if (a.corr) dz = __dadd_rn(dz, c);
  }
  const double dxy = __dsqrt_rn(d2);
  const double cells = __dadd_rn(__dmul_rn(dxy, a.inv_d), 0.5);
  uint32_t ring = (uint32_t)(long long)cells;  // .astype(int) truncates; cells >= 0.5
  if (!(cells < (double)a.nbins)) {
    *a.err = 1;
    ring = (uint32_t)(a.nbins - 1);
  }
  a.hkey[i] = heading_image(atan2(dy, dx));
  a.elev[i] = __ddiv_rn(dz, dxy);  // (dxy == 0 only in ring 0, which is never swept: raster.py:1333-1350)
  a.ring[i] = ring;
  a.idx[i] = (uint32_t)i;
  atomicAdd(a.hist + ring, 1u);
}

// ---- stage 2 helpers ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VS_TB) k_vs_gather_ring(const uint32_t* ring, const uint32_t* idx, uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * VS_TB + threadIdx.x;
  if (i < n) out[i] = ring[idx[i]];
}
__global__ void __launch_bounds__(VS_TB) k_vs_gather_sorted(const uint64_t* hkey, const double* elev, const uint32_t* idx,
                                                           double* hs, double* es, size_t n) {
  const size_t i = (size_t)blockIdx.x * VS_TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = idx[i];
  hs[i] = heading_of(hkey[c]);
  es[i] = elev[c];
}

// ---- stage 3 -----------------------------------------------------------------------------------------------------------
constexpr double VS_PERIOD = 6.283185307179586;  // 2 * np.pi

// NumPy's float remainder x % period for |x| <= pi: fmod(x, period) is x itself, `+ period` when the signs differ (one
// rounding; a tiny negative x gives `period` itself), a zero result takes the sign of the period.
__device__ __forceinline__ double np_mod_period(double h) {
  if (h < 0.0) return __dadd_rn(h, VS_PERIOD);
  return h == 0.0 ? 0.0 : h;
}

// The previous ring as np.interp(period=...) sees it: its n headings h[0 .. n) ascending in (-pi, pi] and its running
// maxima m[]; `r` = how many headings are negative.  np.interp takes xp % period, sorts it -- a rotation of the heading
// order: the non-negative headings first, then the negative ones + period -- and adds one wrapped knot at either end:
// knot 0 = last - period, knots 1 .. n, knot n + 1 = first + period.
struct VsPrev {
  const double* h;
  const double* m;
  int n, r;
  __device__ __forceinline__ int source(int q) const {  // the cell of the previous ring behind knot q
    int t = q == 0 ? n - 1 : (q == n + 1 ? 0 : q - 1);
    return t < n - r ? r + t : t - (n - r);
  }
  __device__ __forceinline__ double xp(int q) const {
    const double v = np_mod_period(h[source(q)]);
    return q == 0 ? __dsub_rn(v, VS_PERIOD) : (q == n + 1 ? __dadd_rn(v, VS_PERIOD) : v);
  }
  __device__ __forceinline__ double fp(int q) const { return m[source(q)]; }
};

// np.interp for one x in [0, period] (numpy/_core/src/multiarray/compiled_base.c: arr_interp): the last knot j with
// xp[j] <= x, the value at a knot hit, else slope * (x - xp[j]) + fp[j] with NumPy's NaN fallbacks.  x is never left of
// knot 0 (<= 0) nor right of knot n + 1 (>= period).
__device__ double vs_interp(const VsPrev& p, double x) {
  const int last = p.n + 1;
  if (x >= p.xp(last)) return p.fp(last);
  int lo = 0, hi = last;  // xp[lo] <= x < xp[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (x >= p.xp(mid))
      lo = mid;
    else
      hi = mid;
  }
  const double xa = p.xp(lo), fa = p.fp(lo);
  if (xa == x) return fa;
  const double xb = p.xp(lo + 1), fb = p.fp(lo + 1);
  const double slope = __ddiv_rn(__dsub_rn(fb, fa), __dsub_rn(xb, xa));
  double res = __dadd_rn(__dmul_rn(slope, __dsub_rn(x, xa)), fa);
  if (isnan(res)) {
    res = __dadd_rn(__dmul_rn(slope, __dsub_rn(x, xb)), fb);
    if (isnan(res) && fa == fb) res = fa;
  }
  return res;
}

struct VsSweepArgs {
  const double* hs;     // [n] headings in sorted order
  const double* es;     // [n] elevation ratios in sorted order
  double* ms;           // [n] running maximum per sorted cell (written for the next ring)
  const uint32_t* idx;  // [n] sorted position -> cell
  uint8_t* vis;         // [n] per cell
  int* rot;             // [rings] negative headings of each processed ring
  int* has_nan;         // [rings] the reference's max_elevations_has_nan as ring k sees it
  uint32_t* n_nan;      // [rings] cells of ring k whose interpolated maximum is NaN (ring 0 of the sweep: NaN elevations)
  uint32_t* n_new;      // [rings] ... of which the cell's own elevation is not NaN
};

// One processed ring: k = its number among the processed rings, cells [start, end) of the sorted order, the previous
// processed ring at [prev, start).
__global__ void __launch_bounds__(VS_TB) k_vs_ring(VsSweepArgs a, int k, size_t prev, size_t start, size_t end) {
  const size_t i = start + (size_t)blockIdx.x * VS_TB + threadIdx.x;
  if (i >= end) return;
  const double h = a.hs[i], e = a.es[i];
  // this ring's rotation point, for the next ring: the first non-negative heading (all negative: the host preset n)
  if (h >= 0.0 && (i == start || a.hs[i - 1] < 0.0)) a.rot[k] = (int)(i - start);
  bool visible;
  double running;
  if (k == 0) {  // "First ring is always visible (if not NaN)" (raster.py:1383-1386)
    visible = !isnan(e);
    running = e;
    if (!visible) atomicAdd(a.n_nan, 1u);
  } else {
    // max_elevations_has_nan (raster.py:1373-1380): set by NaN elevations in the first ring, cleared by the first ring in
    // which every NaN maximum met a cell with an elevation.  Every thread derives it from the previous launch's counts.
    const bool flag = k == 1 ? a.n_nan[0] > 0 : (a.has_nan[k - 1] && a.n_nan[k - 1] != a.n_new[k - 1]);
    if (i == start) a.has_nan[k] = flag;
    VsPrev p{a.hs + prev, a.ms + prev, (int)(start - prev), a.rot[k - 1]};
    running = vs_interp(p, np_mod_period(h));
    visible = e > running;
    if (flag && isnan(running)) {
      atomicAdd(a.n_nan + k, 1u);
      if (!isnan(e)) {
        atomicAdd(a.n_new + k, 1u);
        visible = true;
      }
    }
    if (visible) running = e;
  }
  a.ms[i] = running;
  a.vis[a.idx[i]] = visible ? 1 : 0;
}

// ---- host --------------------------------------------------------------------------------------------------------------
}  // namespace

double viewshed_farthest_cells(const ViewshedJob& j, const double* origin) {
  // the farthest cell from the origin is a corner: its distance in cells (+ 0.5) bounds every ring number
  double far = 0.0;
  for (int cx : {0, j.nx - 1})
    for (int cy : {0, j.ny - 1}) {
      const double dx = j.x[cx] - origin[0], dy = j.y[cy] - origin[1];
      const double c = sqrt(dx * dx + dy * dy) * j.inv_d + 0.5;
      if (!(c <= far)) far = c;  // (a NaN stays: the caller refuses it)
    }
  return far;
}

int viewshed_run(const ViewshedJob& j) {
  const size_t n = (size_t)j.nx * j.ny;
  // the ring numbers of every origin fit a histogram sized before anything is allocated
  int nbins = 1;
  for (int o = 0; o < j.m; ++o) {
    const double far = viewshed_farthest_cells(j, j.origins + 3 * o);
    if (!(far < (double)VS_MAX_RINGS))
      return fail(GLH_E_UNSUPPORTED, "viewshed: origin %d is %g cells from the farthest cell (fewer than %d are served)",
                  o, far, VS_MAX_RINGS);
    if ((int)far + 2 > nbins) nbins = (int)far + 2;
  }
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<6> ev;
  CHK(ev.create());
  const size_t zbytes = n * (j.f32 ? 4 : 8);
  DevBuf dz, dx, dy, hkey, kbuf, elev, ring, idxa, idxb, rka, rkb, es, ms, vis, hist, flags, small, temp;
  CHK(dz.alloc(zbytes));
  CHK(dx.alloc((size_t)j.nx * 8));
  CHK(dy.alloc((size_t)j.ny * 8));
  CHK(hkey.alloc(n * 8));
  CHK(kbuf.alloc(n * 8));  // the first sort's sorted keys, then the sorted headings
  CHK(elev.alloc(n * 8));
  CHK(ring.alloc(n * 4));
  CHK(idxa.alloc(n * 4));
  CHK(idxb.alloc(n * 4));
  CHK(rka.alloc(n * 4));
  CHK(rkb.alloc(n * 4));
  CHK(es.alloc(n * 8));
  CHK(ms.alloc(n * 8));
  CHK(vis.alloc(n));
  CHK(hist.alloc((size_t)nbins * 4));
  CHK(flags.alloc(4));  // the per-cell kernel's error word
  int ring_bits = 1;
  while ((1ll << ring_bits) < nbins) ++ring_bits;
  size_t t1 = 0, t2 = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, t1, hkey.as<uint64_t>(), kbuf.as<uint64_t>(), idxa.as<uint32_t>(),
                                   idxb.as<uint32_t>(), n, 0, 64, s));
  HIPCHK(rocprim::radix_sort_pairs(nullptr, t2, rka.as<uint32_t>(), rkb.as<uint32_t>(), idxb.as<uint32_t>(),
                                   idxa.as<uint32_t>(), n, 0, ring_bits, s));
  const size_t tbytes = t1 > t2 ? t1 : t2;
  CHK(temp.alloc(tbytes));

  double t_ms[5] = {0, 0, 0, 0, 0};
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dz.p, j.z, zbytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx.p, j.x, (size_t)j.nx * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy.p, j.y, (size_t)j.ny * 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  HIPCHK(hipEventSynchronize(ev.e[1]));
  t_ms[0] += ev.ms(0, 1);

  std::vector<uint32_t> h_hist(nbins);
  std::vector<size_t> r_start, r_end;
  std::vector<int> preset;
  const unsigned nblocks = (unsigned)((n + VS_TB - 1) / VS_TB);
  long long rings_done = 0, launches = 0;
  for (int o = 0; o < j.m; ++o) {
    const double* org = j.origins + 3 * o;
    uint8_t* out = j.visible + (size_t)o * n;
    // ---- 1: per cell
    CHK(ev.record(0, s));
    HIPCHK(hipMemsetAsync(hist.p, 0, (size_t)nbins * 4, s));
    HIPCHK(hipMemsetAsync(flags.p, 0, 4, s));
    VsCellArgs ca{dz.p, dx.as<double>(), dy.as<double>(), j.nx, j.ny, j.f32, j.correction, j.inv_d, org[0], org[1], org[2],
                  j.refraction - 1.0, 2.0 * j.radius, hkey.as<uint64_t>(), elev.as<double>(), ring.as<uint32_t>(),
                  idxa.as<uint32_t>(), hist.as<uint32_t>(), nbins, flags.as<int>()};
    hipLaunchKernelGGL(k_vs_cells, dim3((j.nx + VS_TB - 1) / VS_TB, j.ny), dim3(VS_TB), 0, s, ca);
    HIPCHK(hipGetLastError());
    CHK(ev.record(1, s));
    // ---- 2: np.lexsort((heading, ring)): stable by heading, then stable by ring
    HIPCHK(rocprim::radix_sort_pairs(temp.p, t1, hkey.as<uint64_t>(), kbuf.as<uint64_t>(), idxa.as<uint32_t>(),
                                     idxb.as<uint32_t>(), n, 0, 64, s));
    hipLaunchKernelGGL(k_vs_gather_ring, dim3(nblocks), dim3(VS_TB), 0, s, ring.as<uint32_t>(), idxb.as<uint32_t>(),
                       rka.as<uint32_t>(), n);
    HIPCHK(rocprim::radix_sort_pairs(temp.p, t2, rka.as<uint32_t>(), rkb.as<uint32_t>(), idxb.as<uint32_t>(),
                                     idxa.as<uint32_t>(), n, 0, ring_bits, s));
    hipLaunchKernelGGL(k_vs_gather_sorted, dim3(nblocks), dim3(VS_TB), 0, s, hkey.as<uint64_t>(), elev.as<double>(),
                       idxa.as<uint32_t>(), kbuf.as<double>(), es.as<double>(), n);
    HIPCHK(hipGetLastError());
    CHK(ev.record(2, s));
    // the ring sizes come back once, to shape the launches
    int kernel_err = 0;
    CHK(hist.down(h_hist.data(), (size_t)nbins * 4));
    CHK(flags.down(&kernel_err, 4));
    if (kernel_err) return fail(GLH_E_INVALID, "viewshed: a ring number beyond the %d the corners allow", nbins);
    // the processed rings: every non-empty ring but ring 0 (raster.py:1333-1346: with a ring 0 `rings` starts at ring 1)
    r_start.clear();
    r_end.clear();
    size_t at = 0;
    for (int b = 0; b < nbins; ++b) {
      if (h_hist[b] && b > 0) {
        r_start.push_back(at);
        r_end.push_back(at + h_hist[b]);
      }
      at += h_hist[b];
    }
    if (at != n) return fail(GLH_E_HIP, "viewshed: the ring histogram counts %zu of %zu cells", at, n);
    const int nr = (int)r_start.size();
    CHK(ev.record(3, s));
    if (nr == 0) {
      // "Single co-located pixel, return all visible" (raster.py:1344-1345)
      HIPCHK(hipMemsetAsync(vis.p, 1, n, s));
    } else {
      HIPCHK(hipMemsetAsync(vis.p, 0, n, s));  // (ring 0 beside other rings is never processed: it stays False)
      // per ring: rot preset to the ring's size ("no non-negative heading"), flag, two counters
      preset.assign((size_t)4 * nr, 0);
      for (int k = 0; k < nr; ++k) preset[k] = (int)(r_end[k] - r_start[k]);
      CHK(small.alloc((size_t)16 * nr));
      HIPCHK(hipMemcpy(small.p, preset.data(), (size_t)16 * nr, hipMemcpyHostToDevice));
      VsSweepArgs sa{kbuf.as<double>(), es.as<double>(), ms.as<double>(), idxa.as<uint32_t>(), vis.as<uint8_t>(),
                     small.as<int>(), small.as<int>() + nr, small.as<uint32_t>() + 2 * nr, small.as<uint32_t>() + 3 * nr};
      for (int k = 0; k < nr; ++k) {
        const size_t cnt = r_end[k] - r_start[k];
        hipLaunchKernelGGL(k_vs_ring, dim3((unsigned)((cnt + VS_TB - 1) / VS_TB)), dim3(VS_TB), 0, s, sa, k,
                           k ? r_start[k - 1] : r_start[k], r_start[k], r_end[k]);
      }
      HIPCHK(hipGetLastError());
    }
    CHK(ev.record(4, s));
    CHK(vis.down(out, n));
    CHK(ev.record(5, s));
    HIPCHK(hipEventSynchronize(ev.e[5]));
    if (small.p) {
      HIPCHK(hipFree(small.p));
      small.p = nullptr;
    }
    t_ms[1] += ev.ms(0, 1);
    t_ms[2] += ev.ms(1, 2);
    t_ms[3] += ev.ms(3, 4);
    t_ms[4] += ev.ms(4, 5);
    rings_done += nr;
    launches += nr;
  }
  if (j.times_ms) {
    for (int k = 0; k < 5; ++k) j.times_ms[k] = t_ms[k];
    j.times_ms[5] = (double)rings_done;
    j.times_ms[6] = (double)launches;
    j.times_ms[7] = (double)tbytes;
  }
  return GLH_OK;
}

}  // namespace glh
