// glh_rpj_sample.h -- one sample of a frame at image coordinates (u, v), as scipy.interpolate.RegularGridInterpolator
// over the pixel centres evaluates it.  Shared by k_reproject (glh_kernels.h: Image.project) and k_orthorectify
// (glh_ortho.hip: Image.orthorectify), so that both pick the same corners and round in the same places.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "glh_math.h"

namespace glh {

constexpr int RPJ_BX = 32, RPJ_BY = 8;  // one workgroup: 32 x 8 target pixels, a wave = two rows of 32 neighbours
enum { RPJ_LINEAR = 0, RPJ_NEAREST = 1 };

// find_indices of scipy's RegularGridInterpolator (interpolate/_rgi_cython.pyx) on the grid of pixel centres
// g[j] = j + 0.5 (np.linspace(0.5, n - 0.5, n): step exactly 1, so g[j] is exact): the interval i with g[i] <= x < g[i + 1],
// clipped to [0, n - 2]; t = (x - g[i]) / (g[i + 1] - g[i]), whose denominator is exactly 1.  The caller has tested
// 0.5 <= x <= n - 0.5 (x - 0.5 is exact there).
GLH_HD int rpj_interval(double x, int n, double& t) {
  int i = (int)floor(x - 0.5);
  i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
  t = x - ((double)i + 0.5);
  return i;
}

// The C channels of the frame `src` [sh][sw][C] at (u, v), bilinear or nearest, as RegularGridInterpolator((pv, pu),
// array[:, :, c], method, bounds_error=False) evaluates them, each converted to Out: o[0 .. C).  False, and nothing
// written, where the interpolator answers its fill value: outside 0.5 <= u <= sw - 0.5, 0.5 <= v <= sh - 0.5, or a NaN
// coordinate (behind the camera), which fails every comparison.
//  * 8 / 16-bit and float64 frames take scipy's two-dimensional float64 path (evaluate_linear_2d): every corner is
//    value * w_row * w_col, left to right, summed in the order (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1);
//  * float32 frames take its general path: value * (w_row * w_col) in float64, summed from 0.0 in the same order.
// The conversion to Out is NumPy's assignment into the result: one rounding to float32, a truncation toward zero to an
// unsigned integer, nothing for float64.  "nearest" hands the chosen pixel over as it is.
template <typename T, int C, typename Out>
GLH_HD bool rpj_sample(const T* __restrict__ src, int sw, int sh, double u, double v, int method, Out* __restrict__ o) {
  if (!(u >= 0.5 && u <= (double)sw - 0.5 && v >= 0.5 && v <= (double)sh - 0.5)) return false;
  double tu, tv;
  const int iu = rpj_interval(u, sw, tu), iv = rpj_interval(v, sh, tv);
  if (method == RPJ_NEAREST) {
    const T* s = src + ((size_t)(tv <= 0.5 ? iv : iv + 1) * sw + (tu <= 0.5 ? iu : iu + 1)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (Out)s[c];
    return true;
  }
  const T* s0 = src + ((size_t)iv * sw + iu) * C;
  const T* s1 = s0 + (size_t)sw * C;
  const double wv0 = 1.0 - tv, wu0 = 1.0 - tu;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double a00 = (double)s0[c], a01 = (double)s0[C + c], a10 = (double)s1[c], a11 = (double)s1[C + c];
    double r;
    if constexpr (sizeof(T) == 4) {
      r = 0.0;
      r += a00 * (wv0 * wu0);
      r += a01 * (wv0 * tu);
      r += a10 * (tv * wu0);
      r += a11 * (tv * tu);
    } else {
      r = 0.0;
      r += a00 * wv0 * wu0;
      r += a01 * wv0 * tu;
      r += a10 * tv * wu0;
      r += a11 * tv * tu;
    }
    o[c] = (Out)r;
  }
  return true;
}

}  // namespace glh
