// glh_sift.hip -- SIFT keypoint detection and description on the device (optimize.SIFT, optimize.detect_keypoints with
// method=optimize.SIFT): the work behind glh_sift_create / _detect / _read / _counts / _layer / _destroy
// (include/glimpse_hip.h; glimpse_hip.hip validates the arguments).  Lowe 2004 with the structure and constants of OpenCV's
// implementation; the rule is written out in INPUTS.md ("SIFT: the rule") and restated in NumPy by tests/sift_restated.py,
// which this file equals in every bit:
//   * the pyramid is float32.  A blur pass is the arithmetic of glh_filters.hip's Gaussian pass (SciPy's correlate1d in its
//     symmetric form, float64 sums in tap order, rounded to float32 after each axis, boundary "mirror") on layers that stay on
//     the device; the weight tables come from the host (NumPy's exp);
//   * everything per keypoint is float64 made of + - x /, sqrt, rint, floor and ldexp alone (the library is built with
//     -ffp-contract=off); exp, 2^x, atan2, sin and cos are the functions below, not the maths library's;
//   * the 36-bin and the 360-bin histograms are summed in fixed point: every contribution is rint(v 2^20) added as a 64-bit
//     integer with an LDS atomic, so the sums do not depend on the order of the lanes.  A contribution is below 361 x 2^20
//     (the magnitude of a gradient of values in 0 .. 255 is below 361, the weights are at most 1) and a layer has fewer than
//     2^31 cells: every sum stays below 2^60;
//   * the candidate list and the keypoint list are appended through atomic counters and sorted by their keys (rocPRIM's radix
//     sort) before anything reads them.  Keypoints of equal keys are equal in every field.
//
// Kernels: k_sf_base (uint8 -> the doubled float32 image), k_sf_blur (one pass along an axis: a thread per cell, the half
// table in LDS, taps from memory -- neighbouring lanes are neighbouring columns on both axes), k_sf_decimate, k_sf_dog,
// k_sf_extrema (a thread per interior cell and layer, appending keys), k_sf_refine (a wave per candidate: lane 0 fits the
// quadratic, all lanes fill the orientation histogram, lane 0 smooths it and appends one keypoint per peak), k_sf_describe
// (a wave per keypoint: all lanes spread the window's gradients over the 6 x 6 x 10 histogram in LDS, lane 0 normalises).
// The windows are read from memory: a keypoint's window is a few thousand cells that the caches hold.
#include <hip/hip_runtime.h>

#include <cstring>  // (before rocPRIM: its headers call the host memset)

#include <rocprim/device/device_radix_sort.hpp>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_sift.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int SF_TB = 256;
constexpr int SF_WAVE = 64;
constexpr int SF_BORDER = 5;
constexpr int SF_MAX_STEPS = 5;
constexpr double SF_FIX = 1048576.0;  // 2^20
constexpr double SF_IS = 1.0 / 255.0;
constexpr double SF_EPS = 0x1p-52;
constexpr double SF_ANGLE_EPS = 0x1p-23;

// ---- the rule's own elementary functions (tests/sift_restated.py repeats them operation for operation) ------------------
// e^x: x = k ln 2 + r with k = rint(x / ln 2) and ln 2 in two parts, the degree-13 Taylor polynomial of r by Horner, scaled
// by 2^k.  0 below -700.
__device__ __forceinline__ double sf_exp(double x) {
  if (x < -700.0) return 0.0;
  const double kf = __builtin_rint(x * 0x1.71547652b82fep+0);
  const double r = (x - kf * 0x1.62e42fee00000p-1) - kf * 0x1.a39ef35793c76p-33;
  double p = 0x1.6124613a86d09p-33;  // 1 / 13!
  p = p * r + 0x1.1eed8eff8d898p-29;
  p = p * r + 0x1.ae64567f544e4p-26;
  p = p * r + 0x1.27e4fb7789f5cp-22;
  p = p * r + 0x1.71de3a556c734p-19;
  p = p * r + 0x1.a01a01a01a01ap-16;
  p = p * r + 0x1.a01a01a01a01ap-13;
  p = p * r + 0x1.6c16c16c16c17p-10;
  p = p * r + 0x1.1111111111111p-7;
  p = p * r + 0x1.5555555555555p-5;
  p = p * r + 0x1.5555555555555p-3;
  p = p * r + 0x1.0000000000000p-1;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)kf);
}
__device__ __forceinline__ double sf_pow2(double x) { return sf_exp(x * 0x1.62e42fefa39efp-1); }

// the angle of (x, y) in degrees, [0, 360]: OpenCV's fastAtan2 polynomial in float64
__device__ __forceinline__ double sf_atan2(double y, double x) {
  const double ax = fabs(x), ay = fabs(y);
  const bool big = ax >= ay;
  const double c = (big ? ay : ax) / ((big ? ax : ay) + SF_EPS);
  const double c2 = c * c;
  double a = (((-0x1.4515b1b4863e3p+1 * c2 + 0x1.1d3f7d350aa15p+3) * c2 + -0x1.2aaddbf772879p+4) * c2 + 0x1.ca44dc8279760p+5) * c;
  if (!big) a = 90.0 - a;
  if (x < 0.0) a = 180.0 - a;
  if (y < 0.0) a = 360.0 - a;
  return a;
}

// (sin, cos) of an angle in degrees, 0 <= deg <= 360: quadrant k = rint(rad 2 / pi), Taylor polynomials of the rest
__device__ __forceinline__ void sf_sincos(double deg, double& sn, double& cs) {
  const double rad = deg * 0x1.1df46a2529d39p-6;
  const double k = __builtin_rint(rad * 0x1.45f306dc9c883p-1);
  const double r = (rad - k * 0x1.921fb54400000p+0) - k * 0x1.0b4611a626331p-34;
  const double z = r * r;
  double s = 0x1.952c77030ad4ap-49, c = 0x1.ae7f3e733b81fp-45;
  s = s * z + -0x1.ae7f3e733b81fp-41;
  c = c * z + -0x1.93974a8c07c9dp-37;
  s = s * z + 0x1.6124613a86d09p-33;
  c = c * z + 0x1.1eed8eff8d898p-29;
  s = s * z + -0x1.ae64567f544e4p-26;
  c = c * z + -0x1.27e4fb7789f5cp-22;
  s = s * z + 0x1.71de3a556c734p-19;
  c = c * z + 0x1.a01a01a01a01ap-16;
  s = s * z + -0x1.a01a01a01a01ap-13;
  c = c * z + -0x1.6c16c16c16c17p-10;
  s = s * z + 0x1.1111111111111p-7;
  c = c * z + 0x1.5555555555555p-5;
  s = s * z + -0x1.5555555555555p-3;
  c = c * z + -0x1.0000000000000p-1;
  s = s * z + 1.0;
  c = c * z + 1.0;
  s = s * r;
  const int q = (int)k & 3;
  sn = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
  cs = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
}

// ---- the pyramid --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sf_double_axis(int i, int n, int& i0, int& i1, float& w0, float& w1) {
  const int k = i >> 1;
  if ((i & 1) == 0) {
    i0 = k > 0 ? k - 1 : 0;
    i1 = k;
    w0 = 0.25f;
  } else {
    i0 = k;
    i1 = k + 1 < n ? k + 1 : n - 1;
    w0 = 0.75f;
  }
  w1 = 1.0f - w0;
}

__global__ void __launch_bounds__(SF_TB) k_sf_base(const uint8_t* img, int h, int w, float* out) {
  const size_t n = (size_t)(2 * h) * (size_t)(2 * w);
  const size_t i = (size_t)blockIdx.x * SF_TB + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / (size_t)(2 * w)), col = (int)(i - (size_t)row * (2 * w));
  int r0, r1, c0, c1;
  float wr0, wr1, wc0, wc1;
  sf_double_axis(row, h, r0, r1, wr0, wr1);
  sf_double_axis(col, w, c0, c1, wc0, wc1);
  const float t0 = (float)img[(size_t)r0 * w + c0] * wc0 + (float)img[(size_t)r0 * w + c1] * wc1;
  const float t1 = (float)img[(size_t)r1 * w + c0] * wc0 + (float)img[(size_t)r1 * w + c1] * wc1;
  out[i] = t0 * wr0 + t1 * wr1;
}

// one pass of a blur along `axis` (0: rows): glh_filters.hip's k_fl_gauss without its mask, float32 in and out
__global__ void __launch_bounds__(SF_TB) k_sf_blur(const float* in, float* out, const double* wt, int r, int nx, int ny,
                                                   int axis) {
  extern __shared__ double sf_w[];  // [r + 1]: sf_w[r + j] is the weight of taps -j and j, j = -r .. 0
  for (int k = threadIdx.x; k <= r; k += SF_TB) sf_w[k] = wt[k];
  __syncthreads();
  const size_t n = (size_t)nx * ny;
  const size_t i = (size_t)blockIdx.x * SF_TB + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / nx), col = (int)(i - (size_t)row * nx);
  const int pos = axis == 0 ? row : col, len = axis == 0 ? ny : nx;
  const size_t stride = axis == 0 ? (size_t)nx : 1, base = i - (size_t)pos * stride;
  auto tap = [&](int q) {
    const int b = (unsigned)q < (unsigned)len ? q : border_index(q, len, GLH_HP_MIRROR);
    return (double)in[base + (size_t)b * stride];
  };
  double acc = __dmul_rn(tap(pos), sf_w[r]);
  for (int j = -r; j < 0; ++j) acc = __dadd_rn(acc, __dmul_rn(__dadd_rn(tap(pos + j), tap(pos - j)), sf_w[r + j]));
  out[i] = (float)acc;
}

__global__ void __launch_bounds__(SF_TB) k_sf_decimate(const float* in, int W, float* out, int W2, int H2) {
  const size_t n = (size_t)W2 * H2;
  const size_t i = (size_t)blockIdx.x * SF_TB + threadIdx.x;
  if (i >= n) return;
  const int row = (int)(i / W2), col = (int)(i - (size_t)row * W2);
  out[i] = in[(size_t)(2 * row) * W + 2 * col];
}

// d[i] = g[i + 1] - g[i] for the S + 2 differences of an octave (layers of `cells` cells, contiguous)
__global__ void __launch_bounds__(SF_TB) k_sf_dog(const float* g, float* d, size_t cells, size_t total) {
  const size_t i = (size_t)blockIdx.x * SF_TB + threadIdx.x;
  if (i >= total) return;
  d[i] = g[i + cells] - g[i];
}

struct SfPyr {  // where the layers of every octave are
  const float* g[SF_MAX_OCTAVES];  // [S + 3][H][W]
  const float* d[SF_MAX_OCTAVES];  // [S + 2][H][W]
  int W[SF_MAX_OCTAVES], H[SF_MAX_OCTAVES];
  int n_oct, S;
};

__device__ __forceinline__ uint64_t sf_key(int o, int l, int r, int c) {
  return ((uint64_t)o << 56) | ((uint64_t)l << 48) | ((uint64_t)r << 24) | (uint64_t)c;
}

// a thread per cell of layers 1 .. S inside the border: appends the key of every extremum above the contrast floor; the
// counter goes on counting past `cap` (the host then runs this again with room)
__global__ void __launch_bounds__(SF_TB) k_sf_extrema(const float* d, int W, int H, int S, float thr, int o, uint64_t* keys,
                                                      unsigned* counter, unsigned cap) {
  const int iw = W - 2 * SF_BORDER, ih = H - 2 * SF_BORDER;
  const size_t per = (size_t)iw * ih, n = per * S;
  const size_t i = (size_t)blockIdx.x * SF_TB + threadIdx.x;
  if (i >= n) return;
  const int l = (int)(i / per) + 1;
  const size_t rem = i - (size_t)(l - 1) * per;
  const int r = (int)(rem / iw) + SF_BORDER, c = (int)(rem - (size_t)(r - SF_BORDER) * iw) + SF_BORDER;
  const size_t cells = (size_t)W * H;
  const float* p = d + (size_t)l * cells + (size_t)r * W + c;
  const float v = *p;
  if (!(fabsf(v) > thr)) return;
  bool ge = true, le = true;
  for (int dl = -1; dl <= 1; ++dl)
    for (int dr = -1; dr <= 1; ++dr)
      for (int dc = -1; dc <= 1; ++dc) {
        const float q = p[(ptrdiff_t)dl * (ptrdiff_t)cells + (ptrdiff_t)dr * W + dc];
        ge = ge && v >= q;
        le = le && v <= q;
      }
  if ((v > 0.f && ge) || (v < 0.f && le)) {
    const unsigned slot = atomicAdd(counter, 1u);
    if (slot < cap) keys[slot] = sf_key(o, l, r, c);
  }
}

// ---- refinement and orientation -------------------------------------------------------------------------------------------
struct SfKp {
  double ptx, pty, size, angle, response, octave, scl;
  int32_t o, l, r, c, bin, pad_;
};

// x of the 3 x 4 augmented system by Gaussian elimination, in each column the pivot the row of largest |entry| (the first of
// equals); false when a pivot is zero
__device__ bool sf_solve3(double a[3][4], double* x) {
  for (int k = 0; k < 3; ++k) {
    int p = k;
    for (int i = k + 1; i < 3; ++i)
      if (fabs(a[i][k]) > fabs(a[p][k])) p = i;
    if (a[p][k] == 0.0) return false;
    if (p != k)
      for (int j = 0; j < 4; ++j) {
        const double t = a[k][j];
        a[k][j] = a[p][j];
        a[p][j] = t;
      }
    for (int i = k + 1; i < 3; ++i) {
      const double f = a[i][k] / a[k][k];
      for (int j = k; j < 4; ++j) a[i][j] = a[i][j] - f * a[k][j];
    }
  }
  x[2] = a[2][3] / a[2][2];
  x[1] = (a[1][3] - a[1][2] * x[2]) / a[1][1];
  x[0] = (a[0][3] - a[0][1] * x[1] - a[0][2] * x[2]) / a[0][0];
  return true;
}

struct SfFit {
  int status, l, r, c;
  double xc, xr, xi, contr, size, ptx, pty, scl;
};

// the quadratic fit of one candidate (one lane)
__device__ void sf_refine_one(const float* d, int W, int H, int S, double contrast, double edge, double sigma, int o, int l,
                              int r, int c, SfFit& f) {
  const size_t cells = (size_t)W * H;
  const double ds = SF_IS * 0.5, ss = SF_IS, cs = SF_IS * 0.25;
  double dx = 0, dy = 0, dz = 0, dxx = 0, dyy = 0, dxy = 0, xc = 0, xr = 0, xi = 0, v = 0;
  bool settled = false;
  f.status = 0;
  for (int step = 0; step < SF_MAX_STEPS; ++step) {
    const float* p = d + (size_t)l * cells + (size_t)r * W + c;
    auto D = [&](int dl, int dr, int dc) { return (double)p[(ptrdiff_t)dl * (ptrdiff_t)cells + (ptrdiff_t)dr * W + dc]; };
    v = D(0, 0, 0);
    dx = (D(0, 0, 1) - D(0, 0, -1)) * ds;
    dy = (D(0, 1, 0) - D(0, -1, 0)) * ds;
    dz = (D(1, 0, 0) - D(-1, 0, 0)) * ds;
    const double v2 = v * 2.0;
    dxx = (D(0, 0, 1) + D(0, 0, -1) - v2) * ss;
    dyy = (D(0, 1, 0) + D(0, -1, 0) - v2) * ss;
    const double dss = (D(1, 0, 0) + D(-1, 0, 0) - v2) * ss;
    dxy = (D(0, 1, 1) - D(0, 1, -1) - D(0, -1, 1) + D(0, -1, -1)) * cs;
    const double dxs = (D(1, 0, 1) - D(1, 0, -1) - D(-1, 0, 1) + D(-1, 0, -1)) * cs;
    const double dys = (D(1, 1, 0) - D(1, -1, 0) - D(-1, 1, 0) + D(-1, -1, 0)) * cs;
    double a[3][4] = {{dxx, dxy, dxs, dx}, {dxy, dyy, dys, dy}, {dxs, dys, dss, dz}};
    double X[3];
    if (!sf_solve3(a, X)) {
      f.status = 1;
      return;
    }
    xc = -X[0];
    xr = -X[1];
    xi = -X[2];
    if (fabs(xc) < 0.5 && fabs(xr) < 0.5 && fabs(xi) < 0.5) {
      settled = true;
      break;
    }
    if (!(fabs(xc) <= 1e6 && fabs(xr) <= 1e6 && fabs(xi) <= 1e6)) {
      f.status = 6;
      return;
    }
    c += (int)__builtin_rint(xc);
    r += (int)__builtin_rint(xr);
    l += (int)__builtin_rint(xi);
    if (l < 1 || l > S || c < SF_BORDER || c >= W - SF_BORDER || r < SF_BORDER || r >= H - SF_BORDER) {
      f.status = 2;
      return;
    }
  }
  if (!settled) {
    f.status = 3;
    return;
  }
  const double contr = v * SF_IS + (dx * xc + dy * xr + dz * xi) * 0.5;
  if (fabs(contr) * (double)S < contrast) {
    f.status = 4;
    return;
  }
  const double tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
  if (det <= 0.0 || tr * tr * edge >= (edge + 1.0) * (edge + 1.0) * det) {
    f.status = 5;
    return;
  }
  f.l = l;
  f.r = r;
  f.c = c;
  f.xc = xc;
  f.xr = xr;
  f.xi = xi;
  f.contr = contr;
  f.scl = sigma * sf_pow2(((double)l + xi) / (double)S);
  const double oscale = ldexp(0.5, o);
  f.size = f.scl * ldexp(1.0, o);
  f.ptx = ((double)c + xc) * oscale;
  f.pty = ((double)r + xr) * oscale;
}

__device__ __forceinline__ void sf_gradient(const float* g, int W, int y, int x, double& dx, double& dy) {
  const float* p = g + (size_t)y * W + x;
  dx = (double)p[1] - (double)p[-1];
  dy = (double)p[-(ptrdiff_t)W] - (double)p[W];
}

// a wave per candidate (sorted keys)
__global__ void __launch_bounds__(SF_WAVE) k_sf_refine(SfPyr pyr, const uint64_t* keys, int n_cand, double contrast,
                                                       double edge, double sigma, double* refined, SfKp* kps,
                                                       uint64_t* kp_keys, unsigned* counter, unsigned cap) {
  __shared__ SfFit fit;
  __shared__ unsigned long long hist[36];
  const int cand = blockIdx.x, lane = threadIdx.x;
  if (cand >= n_cand) return;
  const uint64_t key = keys[cand];
  const int o = (int)(key >> 56), l0 = (int)((key >> 48) & 255), r0 = (int)((key >> 24) & 0xffffff), c0 = (int)(key & 0xffffff);
  const int W = pyr.W[o], H = pyr.H[o], S = pyr.S;
  if (lane < 36) hist[lane] = 0ull;
  if (lane == 0) {
    sf_refine_one(pyr.d[o], W, H, S, contrast, edge, sigma, o, l0, r0, c0, fit);
    double* out = refined + (size_t)cand * SF_REFINED_COLS;
    const bool ok = fit.status == 0;
    out[0] = (double)fit.status;
    out[1] = ok ? (double)o : 0.0;
    out[2] = ok ? (double)fit.l : 0.0;
    out[3] = ok ? (double)fit.r : 0.0;
    out[4] = ok ? (double)fit.c : 0.0;
    out[5] = ok ? fit.xc : 0.0;
    out[6] = ok ? fit.xr : 0.0;
    out[7] = ok ? fit.xi : 0.0;
    out[8] = ok ? fit.contr : 0.0;
    out[9] = ok ? fit.size : 0.0;
    out[10] = ok ? fit.ptx : 0.0;
    out[11] = ok ? fit.pty : 0.0;
  }
  __syncthreads();
  if (fit.status != 0) return;  // (uniform)
  const int l = fit.l, r = fit.r, c = fit.c;
  const double scl = fit.scl;
  const float* g = pyr.g[o] + (size_t)l * ((size_t)W * H);
  const long long rad = (long long)__builtin_rint(4.5 * scl);
  const double sig = 1.5 * scl;
  const double escale = -1.0 / (2.0 * sig * sig);
  const long long side = 2 * rad + 1, n = side * side;
  for (long long t = lane; t < n; t += SF_WAVE) {
    const long long i = t / side - rad, j = t % side - rad;
    const long long y = r + i, x = c + j;
    if (y <= 0 || y >= H - 1 || x <= 0 || x >= W - 1) continue;
    double dx, dy;
    sf_gradient(g, W, (int)y, (int)x, dx, dy);
    const double w = sf_exp((double)(i * i + j * j) * escale);
    const double mag = __dsqrt_rn(dx * dx + dy * dy);
    int b = (int)__builtin_rint(sf_atan2(dy, dx) * (36.0 / 360.0));
    if (b >= 36) b -= 36;
    if (b < 0) b += 36;
    atomicAdd(&hist[b], (unsigned long long)(long long)__builtin_rint(w * mag * SF_FIX));
  }
  __syncthreads();
  if (lane != 0) return;
  double t[36], h[36];
  for (int k = 0; k < 36; ++k) t[k] = (double)(long long)hist[k] / SF_FIX;
  double top = 0.0;
  for (int k = 0; k < 36; ++k) {
    h[k] = (t[(k + 34) % 36] + t[(k + 2) % 36]) * (1.0 / 16.0) + (t[(k + 35) % 36] + t[(k + 1) % 36]) * (4.0 / 16.0) +
           t[k] * (6.0 / 16.0);
    top = k == 0 || h[k] > top ? h[k] : top;
  }
  const double thr = top * 0.8;
  for (int k = 0; k < 36; ++k) {
    const double a = h[(k + 35) % 36], z = h[(k + 1) % 36];
    if (!(h[k] > a && h[k] > z && h[k] >= thr)) continue;
    double b = (double)k + 0.5 * (a - z) / (a - 2.0 * h[k] + z);
    if (b < 0.0) b = b + 36.0;
    if (b >= 36.0) b = b - 36.0;
    double angle = 360.0 - 10.0 * b;
    if (fabs(angle - 360.0) < SF_ANGLE_EPS) angle = 0.0;
    const unsigned slot = atomicAdd(counter, 1u);
    if (slot >= cap) continue;
    SfKp kp;
    kp.ptx = fit.ptx;
    kp.pty = fit.pty;
    kp.size = fit.size;
    kp.angle = angle;
    kp.response = fabs(fit.contr);
    kp.octave = (double)(((o - 1) & 255) | (l << 8) | ((int)__builtin_rint((fit.xi + 0.5) * 255.0) << 16));
    kp.scl = scl;
    kp.o = o;
    kp.l = l;
    kp.r = r;
    kp.c = c;
    kp.bin = k;
    kp.pad_ = 0;
    kps[slot] = kp;
    // (octave 5 bits, layer 4, row 24, column 24, bin 6)
    kp_keys[slot] = ((uint64_t)o << 58) | ((uint64_t)l << 54) | ((uint64_t)r << 30) | ((uint64_t)c << 6) | (uint64_t)k;
  }
}

// ---- the descriptor -------------------------------------------------------------------------------------------------------
// a wave per keypoint of the sorted list: writes the keypoint at its sorted place and its 128 bytes
__global__ void __launch_bounds__(SF_WAVE) k_sf_describe(SfPyr pyr, const SfKp* kps, const uint32_t* order, int n_kp,
                                                         SfKp* sorted, uint8_t* desc) {
  __shared__ unsigned long long hist[360];
  __shared__ double dst[128];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= n_kp) return;
  const SfKp kp = kps[order[k]];
  for (int b = lane; b < 360; b += SF_WAVE) hist[b] = 0ull;
  __syncthreads();
  const int W = pyr.W[kp.o], H = pyr.H[kp.o];
  const float* g = pyr.g[kp.o] + (size_t)kp.l * ((size_t)W * H);
  double ori = 360.0 - kp.angle;
  if (fabs(ori - 360.0) < SF_ANGLE_EPS) ori = 0.0;
  double sin_t, cos_t;
  sf_sincos(ori, sin_t, cos_t);
  const double width = 3.0 * kp.scl;
  const double want = __builtin_rint(width * 1.4142135623730951 * 2.5);
  const double diag = floor(__dsqrt_rn((double)W * (double)W + (double)H * (double)H));
  const long long radius = (long long)(want < diag ? want : diag);
  cos_t = cos_t / width;
  sin_t = sin_t / width;
  const long long side = 2 * radius + 1, n = side * side;
  for (long long t = lane; t < n; t += SF_WAVE) {
    const long long i = t / side - radius, j = t % side - radius;
    const double fi = (double)i, fj = (double)j;
    const double c_rot = fj * cos_t - fi * sin_t, r_rot = fj * sin_t + fi * cos_t;
    double rbin = r_rot + 1.5, cbin = c_rot + 1.5;
    const long long y = kp.r + i, x = kp.c + j;
    if (!(rbin > -1.0 && rbin < 4.0 && cbin > -1.0 && cbin < 4.0)) continue;
    if (y <= 0 || y >= H - 1 || x <= 0 || x >= W - 1) continue;
    double dx, dy;
    sf_gradient(g, W, (int)y, (int)x, dx, dy);
    const double w = sf_exp((c_rot * c_rot + r_rot * r_rot) * -0.125);
    const double mag = __dsqrt_rn(dx * dx + dy * dy) * w;
    double obin = (sf_atan2(dy, dx) - ori) * (8.0 / 360.0);
    const double fr0 = floor(rbin), fc0 = floor(cbin), fo0 = floor(obin);
    rbin = rbin - fr0;
    cbin = cbin - fc0;
    obin = obin - fo0;
    const int rr0 = (int)fr0, cc0 = (int)fc0;
    int o0 = (int)fo0;
    if (o0 < 0) o0 += 8;
    if (o0 >= 8) o0 -= 8;
    const double v_r1 = mag * rbin, v_r0 = mag - v_r1;
    const double v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
    const double v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
    const int base = ((rr0 + 1) * 6 + cc0 + 1) * 10 + o0;  // 0 .. 288 (rr0, cc0 in -1 .. 3, o0 in 0 .. 7)
    const double vs[4] = {v_rc00, v_rc01, v_rc10, v_rc11};
    const int offs[4] = {0, 10, 60, 70};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double v1 = vs[q] * obin, v0 = vs[q] - v1;
      atomicAdd(&hist[base + offs[q]], (unsigned long long)(long long)__builtin_rint(v0 * SF_FIX));
      atomicAdd(&hist[base + offs[q] + 1], (unsigned long long)(long long)__builtin_rint(v1 * SF_FIX));
    }
  }
  __syncthreads();
  for (int b = lane; b < 128; b += SF_WAVE) {
    const int cell = b >> 3, kk = b & 7;
    const int idx = (((cell >> 2) + 1) * 6 + (cell & 3) + 1) * 10 + kk;
    unsigned long long q = hist[idx];
    if (kk < 2) q += hist[idx + 8];  // the orientation axis is circular
    dst[b] = (double)(long long)q / SF_FIX;
  }
  __syncthreads();
  if (lane != 0) return;
  double s = 0.0;
  for (int b = 0; b < 128; ++b) s = s + dst[b] * dst[b];
  const double thr = __dsqrt_rn(s) * 0.2;
  s = 0.0;
  for (int b = 0; b < 128; ++b) {
    const double val = dst[b] < thr ? dst[b] : thr;
    dst[b] = val;
    s = s + val * val;
  }
  const double root = __dsqrt_rn(s);
  const double nrm = 512.0 / (root > SF_ANGLE_EPS ? root : SF_ANGLE_EPS);
  uint8_t* out = desc + (size_t)k * 128;
  for (int b = 0; b < 128; ++b) {
    const double q = __builtin_rint(dst[b] * nrm);
    out[b] = (uint8_t)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
  }
  sorted[k] = kp;
}

__global__ void __launch_bounds__(SF_TB) k_sf_iota(uint32_t* out, unsigned n) {
  const unsigned i = blockIdx.x * SF_TB + threadIdx.x;
  if (i < n) out[i] = i;
}

unsigned blocks_for(size_t n) { return (unsigned)((n + SF_TB - 1) / SF_TB); }

}  // namespace
}  // namespace glh

struct glh_sift : glh::DeviceObject {
  // (they keep their memory between the images of one size)
  glh::GrowBuf image, pyramid, temp, tables, keys_a, keys_b, refined, kps, kp_keys, kp_keys_b, order_a, order_b, sorted, desc,
      counters, sort_temp;
  glh::StageEvents<glh::SF_TIMES + 1> ev;
  glh::SfPyr pyr{};
  size_t g_off[glh::SF_MAX_OCTAVES] = {}, d_off[glh::SF_MAX_OCTAVES] = {};
  int w = 0, h = 0;  // of the last image
  int n_cand = 0, n_kp = 0;
  bool have = false;  // a detection has been made
  std::vector<double> host_kp;
  std::vector<uint8_t> host_desc;
  std::vector<int32_t> host_cells;
};

namespace glh {

int sift_create(int device, glh_sift** out) {
  return create_object("sift", device, out, [](glh_sift* h) { return h->ev.create(); });
}

void sift_destroy(glh_sift* h) { destroy_object(h); }

void sift_counts(const glh_sift* h, int32_t* out) {
  out[0] = h->have ? h->pyr.n_oct : 0;
  out[1] = h->have ? h->n_cand : 0;
  out[2] = h->have ? h->n_kp : 0;
  out[3] = h->have ? h->pyr.S : 0;
  out[4] = h->have ? 2 * h->w : 0;
  out[5] = h->have ? 2 * h->h : 0;
}

// one blur of `in` into `out` through the handle's temporary layer
static int sift_blur(glh_sift* h, const float* in, float* out, const double* table, int r, int W, int H, hipStream_t s) {
  const size_t n = (size_t)W * H, lds = (size_t)(r + 1) * 8;
  hipLaunchKernelGGL(k_sf_blur, dim3(blocks_for(n)), dim3(SF_TB), lds, s, in, h->temp.as<float>(), table, r, W, H, 0);
  hipLaunchKernelGGL(k_sf_blur, dim3(blocks_for(n)), dim3(SF_TB), lds, s, (const float*)h->temp.as<float>(), out, table, r, W,
                     H, 1);
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

static int sift_detect_run(glh_sift* h, const uint8_t* image, int w, int h_px, const SiftParams& p, int* n_out,
                           double* times_ms);
static int sift_layer_run(glh_sift* h, int kind, int octave, int index, void* out);

// (the host lists are std::vectors: an allocation that fails there is reported like one that fails on the device)
int sift_detect(glh_sift* h, const uint8_t* image, int w, int h_px, const SiftParams& p, int* n_out, double* times_ms) {
  try {
    return sift_detect_run(h, image, w, h_px, p, n_out, times_ms);
  } catch (const std::bad_alloc&) {
    h->have = false;
    return fail(GLH_E_NOMEM, "sift: no host memory for the lists of a %d x %d image", w, h_px);
  }
}

int sift_layer(glh_sift* h, int kind, int octave, int index, void* out) {
  try {
    return sift_layer_run(h, kind, octave, index, out);
  } catch (const std::bad_alloc&) {
    return fail(GLH_E_NOMEM, "sift: no host memory to read back %d candidates", h->n_cand);
  }
}

static int sift_detect_run(glh_sift* h, const uint8_t* image, int w, int h_px, const SiftParams& p, int* n_out,
                           double* times_ms) {
  CHK(h->use());
  hipStream_t s = h->stream;
  StageEvents<SF_TIMES + 1>& ev = h->ev;
  h->have = false;
  const int S = p.S;
  // the octaves: while the smaller side holds 12 cells
  SfPyr& pyr = h->pyr;
  pyr = SfPyr{};
  pyr.S = S;
  size_t floats = 0;
  for (int W = 2 * w, H = 2 * h_px; (W < H ? W : H) >= 12 && pyr.n_oct < SF_MAX_OCTAVES; W = (W + 1) / 2, H = (H + 1) / 2) {
    const int o = pyr.n_oct++;
    pyr.W[o] = W;
    pyr.H[o] = H;
    h->g_off[o] = floats;
    floats += (size_t)(S + 3) * W * H;
    h->d_off[o] = floats;
    floats += (size_t)(S + 2) * W * H;
  }
  h->w = w;
  h->h = h_px;
  h->n_cand = h->n_kp = 0;
  h->host_kp.clear();
  h->host_desc.clear();
  h->host_cells.clear();
  if (pyr.n_oct == 0) {
    h->have = true;
    *n_out = 0;
    if (times_ms)
      for (int k = 0; k < SF_TIMES; ++k) times_ms[k] = 0.0;
    return GLH_OK;
  }
  const size_t cells0 = (size_t)pyr.W[0] * pyr.H[0];
  CHK(h->image.reserve((size_t)w * h_px));
  CHK(h->pyramid.reserve(floats * 4));
  CHK(h->temp.reserve(cells0 * 4));
  CHK(h->counters.reserve(8));
  size_t table_doubles = 0, table_off[SF_MAX_LAYERS + 3];
  for (int i = 0; i < S + 3; ++i) {
    table_off[i] = table_doubles;
    table_doubles += (size_t)(2 * p.radius[i] + 1);
  }
  CHK(h->tables.reserve(table_doubles * 8));
  for (int o = 0; o < pyr.n_oct; ++o) {
    pyr.g[o] = h->pyramid.as<float>() + h->g_off[o];
    pyr.d[o] = h->pyramid.as<float>() + h->d_off[o];
  }

  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(h->image.p, image, (size_t)w * h_px, hipMemcpyHostToDevice));
  for (int i = 0; i < S + 3; ++i)
    HIPCHK(hipMemcpy(h->tables.as<double>() + table_off[i], p.table[i], (size_t)(2 * p.radius[i] + 1) * 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));

  // the base: doubled into the slot of layer 1 (which the first blur of the octave overwrites later), blurred into layer 0
  float* g0 = h->pyramid.as<float>() + h->g_off[0];
  hipLaunchKernelGGL(k_sf_base, dim3(blocks_for(cells0)), dim3(SF_TB), 0, s, h->image.as<const uint8_t>(), h_px, w, g0 + cells0);
  HIPCHK(hipGetLastError());
  CHK(sift_blur(h, g0 + cells0, g0, h->tables.as<double>() + table_off[0], p.radius[0], pyr.W[0], pyr.H[0], s));
  CHK(ev.record(2, s));

  for (int o = 0; o < pyr.n_oct; ++o) {
    const int W = pyr.W[o], H = pyr.H[o];
    const size_t cells = (size_t)W * H;
    float* g = h->pyramid.as<float>() + h->g_off[o];
    float* d = h->pyramid.as<float>() + h->d_off[o];
    if (o > 0) {
      const float* from = pyr.g[o - 1] + (size_t)S * ((size_t)pyr.W[o - 1] * pyr.H[o - 1]);
      hipLaunchKernelGGL(k_sf_decimate, dim3(blocks_for(cells)), dim3(SF_TB), 0, s, from, pyr.W[o - 1], g, W, H);
      HIPCHK(hipGetLastError());
    }
    for (int i = 1; i < S + 3; ++i)
      CHK(sift_blur(h, g + (size_t)(i - 1) * cells, g + (size_t)i * cells, h->tables.as<double>() + table_off[i], p.radius[i], W, H,
                    s));
    const size_t total = (size_t)(S + 2) * cells;
    hipLaunchKernelGGL(k_sf_dog, dim3(blocks_for(total)), dim3(SF_TB), 0, s, (const float*)g, d, cells, total);
    HIPCHK(hipGetLastError());
  }
  CHK(ev.record(3, s));

  // the candidates: appended, counted, appended again if the list was too short, sorted
  const float thr = (float)floor(0.5 * p.contrast / (double)S * 255.0);
  unsigned* counters = h->counters.as<unsigned>();
  unsigned cap = (unsigned)(h->keys_a.cap / 8);
  if (cap < 4096) cap = 4096;
  unsigned found = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    CHK(h->keys_a.reserve((size_t)cap * 8));
    HIPCHK(hipMemsetAsync(counters, 0, 8, s));
    for (int o = 0; o < pyr.n_oct; ++o) {
      const int W = pyr.W[o], H = pyr.H[o];
      if (W <= 2 * SF_BORDER || H <= 2 * SF_BORDER) continue;
      const size_t n = (size_t)(W - 2 * SF_BORDER) * (H - 2 * SF_BORDER) * S;
      hipLaunchKernelGGL(k_sf_extrema, dim3(blocks_for(n)), dim3(SF_TB), 0, s, pyr.d[o], W, H, S, thr, o, h->keys_a.as<uint64_t>(),
                         counters, cap);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpy(&found, counters, 4, hipMemcpyDeviceToHost));
    if (found <= cap) break;
    cap = found;
  }
  h->n_cand = (int)found;
  const uint64_t* cand_keys = nullptr;
  if (found) {
    CHK(h->keys_b.reserve((size_t)found * 8));
    size_t tb = 0;
    HIPCHK(rocprim::radix_sort_keys(nullptr, tb, h->keys_a.as<uint64_t>(), h->keys_b.as<uint64_t>(), (size_t)found, 0, 64, s));
    CHK(h->sort_temp.reserve(tb));
    HIPCHK(rocprim::radix_sort_keys(h->sort_temp.p, tb, h->keys_a.as<uint64_t>(), h->keys_b.as<uint64_t>(), (size_t)found, 0, 64, s));
    cand_keys = h->keys_b.as<uint64_t>();
  }
  CHK(ev.record(4, s));

  // refinement and orientation: the keypoints appended, counted, sorted by (octave, layer, row, column, bin)
  unsigned n_kp = 0;
  if (found) {
    CHK(h->refined.reserve((size_t)found * SF_REFINED_COLS * 8));
    unsigned kcap = (unsigned)(h->kps.cap / sizeof(SfKp));
    if (kcap < 2 * found + 64) kcap = 2 * found + 64;
    for (int attempt = 0; attempt < 2; ++attempt) {
      CHK(h->kps.reserve((size_t)kcap * sizeof(SfKp)));
      CHK(h->kp_keys.reserve((size_t)kcap * 8));
      HIPCHK(hipMemsetAsync(counters + 1, 0, 4, s));
      hipLaunchKernelGGL(k_sf_refine, dim3(found), dim3(SF_WAVE), 0, s, pyr, cand_keys, (int)found, p.contrast, p.edge, p.sigma,
                         h->refined.as<double>(), h->kps.as<SfKp>(), h->kp_keys.as<uint64_t>(), counters + 1, kcap);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpy(&n_kp, counters + 1, 4, hipMemcpyDeviceToHost));
      if (n_kp <= kcap) break;
      kcap = n_kp;
    }
  }
  h->n_kp = (int)n_kp;
  CHK(ev.record(5, s));

  if (n_kp) {
    CHK(h->order_a.reserve((size_t)n_kp * 4));
    CHK(h->order_b.reserve((size_t)n_kp * 4));
    CHK(h->kp_keys_b.reserve((size_t)n_kp * 8));
    CHK(h->sorted.reserve((size_t)n_kp * sizeof(SfKp)));
    CHK(h->desc.reserve((size_t)n_kp * 128));
    hipLaunchKernelGGL(k_sf_iota, dim3(blocks_for(n_kp)), dim3(SF_TB), 0, s, h->order_a.as<uint32_t>(), n_kp);
    HIPCHK(hipGetLastError());
    size_t tb = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, h->kp_keys.as<uint64_t>(), h->kp_keys_b.as<uint64_t>(), h->order_a.as<uint32_t>(),
                                     h->order_b.as<uint32_t>(), (size_t)n_kp, 0, 64, s));
    CHK(h->sort_temp.reserve(tb));
    HIPCHK(rocprim::radix_sort_pairs(h->sort_temp.p, tb, h->kp_keys.as<uint64_t>(), h->kp_keys_b.as<uint64_t>(),
                                     h->order_a.as<uint32_t>(), h->order_b.as<uint32_t>(), (size_t)n_kp, 0, 64, s));
    hipLaunchKernelGGL(k_sf_describe, dim3(n_kp), dim3(SF_WAVE), 0, s, pyr, (const SfKp*)h->kps.as<SfKp>(),
                       (const uint32_t*)h->order_b.as<uint32_t>(), (int)n_kp, h->sorted.as<SfKp>(), h->desc.as<uint8_t>());
    HIPCHK(hipGetLastError());
  }
  CHK(ev.record(6, s));

  if (n_kp) {
    std::vector<SfKp> kp(n_kp);
    h->host_desc.resize((size_t)n_kp * 128);
    HIPCHK(hipMemcpy(kp.data(), h->sorted.p, (size_t)n_kp * sizeof(SfKp), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->host_desc.data(), h->desc.p, (size_t)n_kp * 128, hipMemcpyDeviceToHost));
    h->host_kp.resize((size_t)n_kp * SF_KEYPOINT_COLS);
    h->host_cells.resize((size_t)n_kp * SF_CELL_COLS);
    for (unsigned k = 0; k < n_kp; ++k) {
      double* a = &h->host_kp[(size_t)k * SF_KEYPOINT_COLS];
      a[0] = kp[k].ptx;
      a[1] = kp[k].pty;
      a[2] = kp[k].size;
      a[3] = kp[k].angle;
      a[4] = kp[k].response;
      a[5] = kp[k].octave;
      int32_t* c = &h->host_cells[(size_t)k * SF_CELL_COLS];
      c[0] = kp[k].o;
      c[1] = kp[k].l;
      c[2] = kp[k].r;
      c[3] = kp[k].c;
      c[4] = kp[k].bin;
    }
  }
  CHK(ev.record(7, s));
  HIPCHK(hipEventSynchronize(ev.e[7]));
  ev.report(times_ms, SF_TIMES, SF_TIMES);
  h->have = true;
  *n_out = (int)n_kp;
  return GLH_OK;
}

int sift_read(const glh_sift* h, double* keypoints, uint8_t* descriptors) {
  if (!h->have) return fail(GLH_E_INVALID, "sift: nothing has been detected on this handle");
  if (h->n_kp) {
    memcpy(keypoints, h->host_kp.data(), h->host_kp.size() * 8);
    memcpy(descriptors, h->host_desc.data(), h->host_desc.size());
  }
  return GLH_OK;
}

static int sift_layer_run(glh_sift* h, int kind, int octave, int index, void* out) {
  if (!h->have) return fail(GLH_E_INVALID, "sift: nothing has been detected on this handle");
  CHK(h->use());
  const SfPyr& pyr = h->pyr;
  if (kind == GLH_SIFT_GAUSS || kind == GLH_SIFT_DOG) {
    const int layers = kind == GLH_SIFT_GAUSS ? pyr.S + 3 : pyr.S + 2;
    if (octave < 0 || octave >= pyr.n_oct || index < 0 || index >= layers)
      return fail(GLH_E_INVALID, "sift: layer %d of octave %d: the pyramid has %d octaves of %d layers", index, octave, pyr.n_oct,
                  layers);
    const size_t cells = (size_t)pyr.W[octave] * pyr.H[octave];
    const float* from = (kind == GLH_SIFT_GAUSS ? pyr.g[octave] : pyr.d[octave]) + (size_t)index * cells;
    HIPCHK(hipMemcpy(out, from, cells * 4, hipMemcpyDeviceToHost));
    return GLH_OK;
  }
  if (kind == GLH_SIFT_CANDIDATES) {
    if (!h->n_cand) return GLH_OK;
    std::vector<uint64_t> keys((size_t)h->n_cand);
    HIPCHK(hipMemcpy(keys.data(), h->keys_b.p, keys.size() * 8, hipMemcpyDeviceToHost));
    int32_t* o = static_cast<int32_t*>(out);
    for (size_t k = 0; k < keys.size(); ++k) {
      o[4 * k + 0] = (int32_t)(keys[k] >> 56);
      o[4 * k + 1] = (int32_t)((keys[k] >> 48) & 255);
      o[4 * k + 2] = (int32_t)((keys[k] >> 24) & 0xffffff);
      o[4 * k + 3] = (int32_t)(keys[k] & 0xffffff);
    }
    return GLH_OK;
  }
  if (kind == GLH_SIFT_REFINED) {
    if (h->n_cand) HIPCHK(hipMemcpy(out, h->refined.p, (size_t)h->n_cand * SF_REFINED_COLS * 8, hipMemcpyDeviceToHost));
    return GLH_OK;
  }
  if (kind == GLH_SIFT_CELLS) {
    if (h->n_kp) memcpy(out, h->host_cells.data(), h->host_cells.size() * 4);
    return GLH_OK;
  }
  return fail(GLH_E_INVALID, "sift: unknown kind %d", kind);
}

}  // namespace glh
