// glh_filters.hip -- helpers.maximum_filter, helpers.gaussian_filter (helpers.py:347-430) and Raster.fill_crevasses
// (raster.py:1266-1291) on the device: the work behind glh_stage_max_filter, glh_stage_gaussian_filter and
// glh_stage_fill_crevasses (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls filters_run).
//
// What the reference computes, and so what is computed here, operation by operation:
//   maximum   scipy.ndimage.maximum_filter(size): the maximum over a window of size_y x size_x cells that reaches
//             size // 2 cells back and size - 1 - size // 2 cells forward, the array extended by the boundary mode.  With a
//             mask, excluded cells count as the dtype's lowest finite value; afterwards the array's own values are put back
//             at the excluded cells (fill false) or at the cells whose result is that lowest value (fill true).
//   Gaussian  scipy.ndimage.gaussian_filter: one correlation per axis, axis 0 (rows) then axis 1 (columns), each in
//             SciPy's symmetric form  tmp = in[0] w[0];  for j = -r .. -1:  tmp += (in[j] + in[-j]) w[j]  in float64 and in
//             that order, rounded to the array's dtype after each axis.  With a mask: xf = G(array, 0 at excluded cells),
//             xf_sum = G(1 at included cells, 0 elsewhere), the result xf / xf_sum in the array's dtype, and the array's own
//             values put back at excluded cells when fill is false (fill true leaves 0 / 0 = NaN out of reach).
// The weight tables are made on the host (NumPy's exp); the device only adds, multiplies and divides, each correctly
// rounded (the library is built with -ffp-contract=off, and the sums use the explicit round-to-nearest intrinsics), so the
// results equal SciPy's in every bit.
//
// Kernels: k_fl_max loads a tile of 64 x 16 outputs with its halo into LDS (mask-on-load), takes the column maximum, then
// the row maximum, and applies the put-back rule on store.  k_fl_gauss is one pass along either axis: a thread per output
// cell, the half weight table in LDS, the taps read straight from memory -- neighbouring lanes are neighbouring columns
// along both axes, so every tap is a coalesced row segment, and the 2 r + 1 rows (or the row itself) a workgroup walks are
// served by the caches.  The first pass forms the indicator from the mask it reads anyway; the last pass divides and puts
// back.  (A tile of rows in LDS does not hold radius 128: 2 r + rows x 64 columns x two float64 arrays.)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_filters.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int FL_TB = 256;
constexpr int FL_TW = 64, FL_TH = 16;  // outputs of one maximum tile (columns, rows)

template <typename T>
struct Lowest;  // np.finfo(dtype).min (helpers.numpy_dtype_minmax)
template <>
struct Lowest<double> {
  static constexpr double value = -DBL_MAX;
};
template <>
struct Lowest<float> {
  static constexpr float value = -FLT_MAX;
};

// the boundary map; a cell inside the array is itself (no fold, no division)
__device__ __forceinline__ int fl_border(int i, int n, int mode) {
  return (unsigned)i < (unsigned)n ? i : border_index(i, n, mode);
}

// ---- maximum -----------------------------------------------------------------------------------------------------------
struct FlMaxArgs {
  const void* a;        // [ny][nx]
  const uint8_t* mask;  // [ny][nx] or null
  void* out;            // [ny][nx]
  int nx, ny;
  int wy, wx;  // window (rows, columns)
  int mode;
  int fill;
  int tiles_x;
};

template <typename T>
__global__ void __launch_bounds__(FL_TB) k_fl_max(FlMaxArgs p) {
  extern __shared__ double fl_lds[];
  const int aw = FL_TW + p.wx - 1, ah = FL_TH + p.wy - 1;
  T* A = reinterpret_cast<T*>(fl_lds);  // [ah][aw] the tile and its halo
  T* B = A + ah * aw;                   // [FL_TH][aw] column maxima
  const T* src = static_cast<const T*>(p.a);
  const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
  const int r0 = ty * FL_TH, c0 = tx * FL_TW;
  const int ly = p.wy / 2, lx = p.wx / 2;  // SciPy centres an even window at size // 2
  const int tid = threadIdx.x;
  for (int k = tid; k < ah * aw; k += FL_TB) {
    const int rr = k / aw, cc = k - rr * aw;
    const size_t g = (size_t)fl_border(r0 - ly + rr, p.ny, p.mode) * p.nx + fl_border(c0 - lx + cc, p.nx, p.mode);
    T v = src[g];
    if (p.mask && !p.mask[g]) v = Lowest<T>::value;
    A[k] = v;
  }
  __syncthreads();
  for (int k = tid; k < FL_TH * aw; k += FL_TB) {
    T m = A[k];
    for (int d = 1; d < p.wy; ++d) {
      const T v = A[k + d * aw];
      m = v > m ? v : m;
    }
    B[k] = m;
  }
  __syncthreads();
  T* out = static_cast<T*>(p.out);
  for (int k = tid; k < FL_TH * FL_TW; k += FL_TB) {
    const int orow = k / FL_TW, oc = k - orow * FL_TW;
    const int r = r0 + orow, c = c0 + oc;
    if (r >= p.ny || c >= p.nx) continue;
    const T* b = B + orow * aw + oc;
    T m = b[0];
    for (int d = 1; d < p.wx; ++d) {
      const T v = b[d];
      m = v > m ? v : m;
    }
    const size_t g = (size_t)r * p.nx + c;
    if (p.mask) {
      // helpers.py:427-429: the array's own values at the excluded cells, or (fill) where the whole window was excluded
      const bool own = p.fill ? m == Lowest<T>::value : !p.mask[g];
      if (own) m = src[g];
    }
    out[g] = m;
  }
}

// ---- Gaussian ----------------------------------------------------------------------------------------------------------
struct FlGaussArgs {
  const void* v;        // [ny][nx] the values this pass filters
  const void* s;        // [ny][nx] the indicator's earlier pass (masked, not the first pass)
  const uint8_t* mask;  // [ny][nx] or null
  const void* own;      // [ny][nx] the values put back at excluded cells (last pass, masked, fill false)
  void* out_v;
  void* out_s;      // (masked, not the last pass)
  const double* w;  // [2 r + 1]; the weights are symmetric and the pass reads w[0 .. r]
  int r;
  int nx, ny;
  int axis;
  int mode;
  int first;  // the values are the array itself: excluded cells read as 0, the indicator comes from the mask
  int last;   // divide and put back
  int fill;
};

template <typename T, bool MASKED>
__global__ void __launch_bounds__(FL_TB) k_fl_gauss(FlGaussArgs p) {
  extern __shared__ double fl_w[];  // [r + 1]: fl_w[r + j] is SciPy's fw[j], j = -r .. 0
  for (int k = threadIdx.x; k <= p.r; k += FL_TB) fl_w[k] = p.w[k];
  __syncthreads();
  const size_t n = (size_t)p.nx * p.ny;
  const size_t i = (size_t)blockIdx.x * FL_TB + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / p.nx), col = (int)(i - (size_t)row * p.nx);
  const int pos = p.axis == 0 ? row : col, len = p.axis == 0 ? p.ny : p.nx;
  const size_t stride = p.axis == 0 ? (size_t)p.nx : 1, base = i - (size_t)pos * stride;
  const T* V = static_cast<const T*>(p.v);
  const T* S = static_cast<const T*>(p.s);
  const bool from_mask = MASKED && p.first;
  double xv = 0.0, xs = 0.0;
  auto tap = [&](int q, double& tv, double& ts) {
    const size_t g = base + (size_t)fl_border(q, len, p.mode) * stride;
    if (from_mask) {
      const bool in = p.mask[g] != 0;
      tv = in ? (double)V[g] : 0.0;
      ts = in ? 1.0 : 0.0;
    } else {
      tv = (double)V[g];
      if (MASKED) ts = (double)S[g];
    }
  };
  tap(pos, xv, xs);
  const double wc = fl_w[p.r];
  double acc_v = __dmul_rn(xv, wc), acc_s = MASKED ? __dmul_rn(xs, wc) : 0.0;
  for (int j = -p.r; j < 0; ++j) {
    const double wj = fl_w[p.r + j];
    double av = 0.0, as = 0.0, bv = 0.0, bs = 0.0;
    tap(pos + j, av, as);
    tap(pos - j, bv, bs);
    acc_v = __dadd_rn(acc_v, __dmul_rn(__dadd_rn(av, bv), wj));
    if (MASKED) acc_s = __dadd_rn(acc_s, __dmul_rn(__dadd_rn(as, bs), wj));
  }
  const T rv = (T)acc_v, rs = (T)acc_s;  // rounded to the array's dtype after every axis
  T* out = static_cast<T*>(p.out_v);
  if (!p.last) {
    out[i] = rv;
    if (MASKED) static_cast<T*>(p.out_s)[i] = rs;
    return;
  }
  if (!MASKED) {
    out[i] = rv;
    return;
  }
  // xf / xf_sum in the array's dtype.  float32: the float64 quotient of two float32 rounded to float32 is the correctly
  // rounded float32 quotient (53 >= 2 * 24 + 2 bits), whatever the device's float32 division does with denormals.
  T res = (T)__ddiv_rn((double)rv, (double)rs);
  if (!p.fill && !p.mask[i]) res = static_cast<const T*>(p.own)[i];
  out[i] = res;
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct Pass {
  int axis;
  const double* w;  // device
  int r;
};

}  // namespace

int filters_run(const FiltersJob& j) {
  const size_t n = (size_t)j.nx * j.ny, bytes = n * (j.f32 ? 4 : 8);
  const bool masked = j.mask != nullptr;
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<6> ev;
  CHK(ev.create());

  // the Gaussian's passes: axis 0, then axis 1; with both axes skipped one pass with the weight 1 (x * 1.0 is x) still
  // divides and puts back, as the reference's gaussian_filter does around SciPy's copy
  static const double one = 1.0;
  const double* host_w[2] = {j.w0, j.w1};
  const int radius[2] = {j.r0, j.r1};
  DevBuf da, dm, dmax, dxf, dxs, dout, dw[2], done;
  Pass pass[2];
  int n_pass = 0;
  CHK(da.alloc(bytes));
  if (masked) CHK(dm.alloc(n));
  CHK(dout.alloc(bytes));
  if (j.do_max && j.do_gauss) CHK(dmax.alloc(bytes));
  if (j.do_gauss) {
    for (int ax = 0; ax < 2; ++ax)
      if (host_w[ax]) {
        CHK(dw[ax].alloc((size_t)(2 * radius[ax] + 1) * 8));
        pass[n_pass++] = Pass{ax, dw[ax].as<const double>(), radius[ax]};
      }
    if (n_pass == 0) {
      CHK(done.alloc(8));
      pass[n_pass++] = Pass{1, done.as<const double>(), 0};
    }
    if (n_pass == 2) {
      CHK(dxf.alloc(bytes));
      if (masked) CHK(dxs.alloc(bytes));
    }
  }

  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(da.p, j.a, bytes, hipMemcpyHostToDevice));
  if (masked) HIPCHK(hipMemcpy(dm.p, j.mask, n, hipMemcpyHostToDevice));
  for (int ax = 0; ax < 2; ++ax)
    if (dw[ax].p) HIPCHK(hipMemcpy(dw[ax].p, host_w[ax], (size_t)(2 * radius[ax] + 1) * 8, hipMemcpyHostToDevice));
  if (done.p) HIPCHK(hipMemcpy(done.p, &one, 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));

  const void* cur = da.p;
  if (j.do_max) {
    void* dst = j.do_gauss ? dmax.p : dout.p;
    const int tiles_x = (j.nx + FL_TW - 1) / FL_TW, tiles_y = (j.ny + FL_TH - 1) / FL_TH;
    const FlMaxArgs ma{da.p, dm.as<const uint8_t>(), dst, j.nx, j.ny, j.size_y, j.size_x, j.max_mode, j.fill, tiles_x};
    const size_t lds = (size_t)(FL_TH + j.size_y - 1 + FL_TH) * (FL_TW + j.size_x - 1) * (j.f32 ? 4 : 8);
    const dim3 grid((unsigned)((size_t)tiles_x * tiles_y));
    if (j.f32)
      hipLaunchKernelGGL(k_fl_max<float>, grid, dim3(FL_TB), lds, s, ma);
    else
      hipLaunchKernelGGL(k_fl_max<double>, grid, dim3(FL_TB), lds, s, ma);
    HIPCHK(hipGetLastError());
    cur = dst;
  }
  CHK(ev.record(2, s));
  int timed_axis[2] = {-1, -1};  // which event pair holds which axis
  const void* own = cur;         // the Gaussian's own input: what it puts back at excluded cells
  const void* cur_s = nullptr;
  for (int k = 0; k < n_pass; ++k) {
    const bool last = k == n_pass - 1;
    const FlGaussArgs ga{cur, cur_s, dm.as<const uint8_t>(), own, last ? dout.p : dxf.p, last ? nullptr : dxs.p,
                         pass[k].w, pass[k].r, j.nx, j.ny, pass[k].axis, j.gauss_mode, k == 0, last, j.fill};
    const dim3 grid((unsigned)((n + FL_TB - 1) / FL_TB));
    const size_t lds = (size_t)(pass[k].r + 1) * 8;
    if (j.f32) {
      if (masked)
        hipLaunchKernelGGL((k_fl_gauss<float, true>), grid, dim3(FL_TB), lds, s, ga);
      else
        hipLaunchKernelGGL((k_fl_gauss<float, false>), grid, dim3(FL_TB), lds, s, ga);
    } else {
      if (masked)
        hipLaunchKernelGGL((k_fl_gauss<double, true>), grid, dim3(FL_TB), lds, s, ga);
      else
        hipLaunchKernelGGL((k_fl_gauss<double, false>), grid, dim3(FL_TB), lds, s, ga);
    }
    HIPCHK(hipGetLastError());
    cur = dxf.p;
    cur_s = dxs.p;
    timed_axis[k] = pass[k].axis;
    CHK(ev.record(3 + k, s));
  }
  for (int k = n_pass; k < 2; ++k) CHK(ev.record(3 + k, s));
  CHK(dout.down(j.out, bytes));
  CHK(ev.record(5, s));
  HIPCHK(hipEventSynchronize(ev.e[5]));
  if (j.times_ms) {
    ev.report(j.times_ms, 2, FL_TIMES);  // upload, max; then the Gaussian's spans by axis, and the download
    for (int k = 0; k < 2; ++k)
      if (timed_axis[k] >= 0) j.times_ms[2 + timed_axis[k]] += ev.ms(2 + k, 3 + k);
    j.times_ms[4] = ev.ms(4, 5);
  }
  return GLH_OK;
}

}  // namespace glh
