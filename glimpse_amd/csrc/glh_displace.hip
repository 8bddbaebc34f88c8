// glh_displace.hip -- dense template matching between frames on the device: the work behind glh_stage_displacements
// (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls displacements_run).  For every point of a
// grid a template is cut from one frame and looked for in another by zero-normalised cross-correlation; the peak of the
// score surface, refined by a parabola per axis, is the displacement.  The reference leaves this to its users, so the
// rule is the contract: INPUTS.md, "Displacements: the rule", restated in NumPy in tests/displacement_rule.py, which both
// kernels equal bit for bit.  In short, with n = w h and the sums over the template T and the window S of an offset:
//
//   vt = n sum(T^2) - sum(T)^2,  vs = n sum(S^2) - sum(S)^2,  num = n sum(T S) - sum(T) sum(S)
//   score = num / sqrt(vt vs)   one product, one correctly rounded square root and division, float64
//
// One workgroup of DP_TB threads per (point, pair), blockIdx.y the pair.  The template and the (w + 2 rx) x (h + 2 ry)
// search window are staged in LDS once, each thread owns whole offsets, the score surface stays in LDS for the sub-pixel
// term, and the peak comes from an ordered reduction (larger score, lower index on ties): no atomics.
//
//   k_displace_u8   the integer path.  Every sum is an exact integer, so the order is free: pixels stay packed four to a
//                   word, a window row at byte phase (l + g_u + i) mod 4 is assembled from neighbouring LDS words with
//                   v_alignbyte_b32 and multiplied with v_dot4_u32_u8, four template words (one 16-byte read) against
//                   five window words a step.  A template row is zero from w to its pitch, which masks the product
//                   (the window operand needs no mask of its own: sum(S) does not come from it).  sum(S) and sum(S^2) of every offset come from running sums: along the rows
//                   first (dp_row_sums), then down the columns (dp_column_sums), two LDS reads per offset and step.
//                   LDS rows of the window are `wstride` words apart, chosen by dp_pitch_u8: the lanes of a 32-lane
//                   group, which own consecutive offsets, read one bank range per row of offsets, and the pitch keeps
//                   the ranges of the rows a group reaches over apart, for every byte phase.
//   k_displace_f32  the float path.  The order of summation is part of the rule (row-major, float64 accumulators; the
//                   product of two float32 is exact in float64, so fma is the stated multiply-add), so each offset is
//                   one serial chain per sum; a thread runs DP_FB offsets at once for ILP.  Rows are `wstride` floats
//                   apart with wstride = nxo (mod 32), which makes the addresses of consecutive offsets consecutive
//                   banks across a row change.
//
// Where the parts of a workgroup's LDS lie and how far apart the rows are is glh_displace_plan.h's (dp_layout, dp_plan),
// checked on the CPU for every template and reach by tests/hostcheck/displace_plan_hostcheck.cpp.
//
// Every loop is bounded by the template and reach, both checked by the caller (DP_MAX_SIDE, DP_MAX_REACH); every global
// read is bounds-checked against the frame (pixels outside are staged as 0 and their offsets are invalid by geometry).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/glimpse_hip.h"
#include "glh_displace.h"
#include "glh_displace_plan.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int DP_WAVES = DP_TB / 64;
constexpr int DP_FB = 4;  // offsets a thread of the float path runs at once

struct DpArgs {
  const void* frames;
  int width, height;
  const int32_t* pairs;
  const int32_t* corners;
  const uint8_t* valid;
  int n;
  const int32_t* guess;
  int guess_pair_stride;  // 0, or 2 n when every pair has its own guesses
  int w, h, rx, ry, subpixel;
  int wstride;  // LDS row pitch of the search window: words (integer path) or floats
  double* duv;
  double* score;
  uint8_t* status;
  double* surface;
};

// What a workgroup learns about its point before it touches a pixel.
struct DpPoint {
  size_t out;    // pair * n + point
  int fa, fb;    // the frames of the pair
  int l, t;      // the template's corner
  int gu, gv;    // the integer guess
  int ok;        // the template lies in the frame
};

__device__ __forceinline__ DpPoint dp_point(const DpArgs& a) {
  DpPoint p;
  const int point = (int)blockIdx.x, pair = (int)blockIdx.y;
  p.out = (size_t)pair * a.n + point;
  p.fa = a.pairs[2 * pair], p.fb = a.pairs[2 * pair + 1];
  p.l = a.corners[2 * point], p.t = a.corners[2 * point + 1];
  p.ok = a.valid[point] != 0 && p.l >= 0 && p.t >= 0 && p.l + a.w <= a.width && p.t + a.h <= a.height;
  p.gu = p.gv = 0;
  if (a.guess) {
    const int32_t* g = a.guess + (size_t)pair * a.guess_pair_stride + 2 * (size_t)point;
    p.gu = g[0], p.gv = g[1];
  }
  return p;
}

// Status `status` without a result: NaN everywhere.
__device__ void dp_no_result(const DpArgs& a, const DpPoint& p, int status) {
  const int noff = (2 * a.rx + 1) * (2 * a.ry + 1);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (a.surface)
    for (int o = (int)threadIdx.x; o < noff; o += DP_TB) a.surface[p.out * noff + o] = nan;
  if (threadIdx.x == 0) {
    a.duv[2 * p.out] = a.duv[2 * p.out + 1] = nan;
    a.score[p.out] = nan;
    a.status[p.out] = (uint8_t)status;
  }
}

__device__ __forceinline__ double dp_score(double num, double vt, double vs) {
  return __ddiv_rn(num, __dsqrt_rn(vt * vs));
}

// The parabola through the peak c and its neighbours a (before) and b (after) on one axis: the offset of its vertex.
__device__ __forceinline__ double dp_vertex(double av, double cv, double bv) {
  const double den = (av - 2.0 * cv) + bv;
  return den < 0.0 ? __ddiv_rn(av - bv, 2.0 * den) : 0.0;
}

// The end of both kernels.  surf [nyo][nxo] in LDS holds every offset's score (NaN: invalid), `best` / `bidx` the
// largest valid score among the calling thread's offsets and the first offset that has it (bidx < 0: none).  Reduces
// them over the workgroup in a fixed order and lets the last wave write the point's result.
__device__ void dp_finish(const DpArgs& a, const DpPoint& p, char* lds, const double* surf, double best, int bidx) {
  double* red_s = reinterpret_cast<double*>(lds + DP_RED_SCORE);
  int* red_i = reinterpret_cast<int*>(lds + DP_RED_INDEX);
  const int nxo = 2 * a.rx + 1, nyo = 2 * a.ry + 1;
  for (int d = 32; d >= 1; d >>= 1) {
    const double os = __shfl_down(best, d, 64);
    const int oi = __shfl_down(bidx, d, 64);
    if (oi >= 0 && (bidx < 0 || os > best || (os == best && oi < bidx))) best = os, bidx = oi;
  }
  if ((threadIdx.x & 63) == 0) red_s[threadIdx.x >> 6] = best, red_i[threadIdx.x >> 6] = bidx;
  __syncthreads();  // (also: every score of surf is written)
  if (threadIdx.x != DP_TB - 64) return;
  best = red_s[0], bidx = red_i[0];
  for (int k = 1; k < DP_WAVES; ++k)
    if (red_i[k] >= 0 && (bidx < 0 || red_s[k] > best || (red_s[k] == best && red_i[k] < bidx))) best = red_s[k], bidx = red_i[k];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (bidx < 0) {
    a.duv[2 * p.out] = a.duv[2 * p.out + 1] = nan;
    a.score[p.out] = nan;
    a.status[p.out] = GLH_DISPLACE_NO_OFFSET;
    return;
  }
  const int j = bidx / nxo, i = bidx - j * nxo;
  double du = 0.0, dv = 0.0;
  int edge = 0;
  if (a.subpixel) {
    const double c = surf[bidx];
    if (i == 0 || i == nxo - 1 || surf[bidx - 1] != surf[bidx - 1] || surf[bidx + 1] != surf[bidx + 1])
      edge = 1;
    else
      du = dp_vertex(surf[bidx - 1], c, surf[bidx + 1]);
    if (j == 0 || j == nyo - 1 || surf[bidx - nxo] != surf[bidx - nxo] || surf[bidx + nxo] != surf[bidx + nxo])
      edge = 1;
    else
      dv = dp_vertex(surf[bidx - nxo], c, surf[bidx + nxo]);
  }
  a.duv[2 * p.out] = (double)(p.gu + i - a.rx) + du;
  a.duv[2 * p.out + 1] = (double)(p.gv + j - a.ry) + dv;
  a.score[p.out] = best;
  a.status[p.out] = edge ? GLH_DISPLACE_EDGE : GLH_DISPLACE_MATCHED;
}

// Is the w x h window of offset (i, j) inside the searched frame?
__device__ __forceinline__ bool dp_inside(const DpArgs& a, const DpPoint& p, int i, int j) {
  const int x = p.l + p.gu + i - a.rx, y = p.t + p.gv + j - a.ry;
  return x >= 0 && y >= 0 && x + a.w <= a.width && y + a.h <= a.height;
}

// ---- the integer path ------------------------------------------------------------------------------------------------------

// rows[y][i] = (sum, sum of squares) of the w bytes of window row y from column i on, i < nxo: one running sum per thread
// over a stretch of a row.  win: the staged window (bytes), cb0: the byte of its first column.
__device__ void dp_row_sums(const uint8_t* win, int pitch, int cb0, int sh, int w, int nxo, uint2* rows) {
  const int nseg = DP_TB / sh > 0 ? DP_TB / sh : 1;
  const int len = (nxo + nseg - 1) / nseg;
  for (int t = (int)threadIdx.x; t < sh * nseg; t += DP_TB) {
    const int y = t % sh, i0 = (t / sh) * len, i1 = min(nxo, i0 + len);
    if (i0 >= i1) continue;
    const uint8_t* row = win + (size_t)y * pitch + cb0;
    uint32_t s = 0, q = 0;
    for (int c = 0; c < w; ++c) {
      const uint32_t v = row[i0 + c];
      s += v, q += v * v;
    }
    for (int i = i0; i < i1; ++i) {
      rows[y * nxo + i] = make_uint2(s, q);
      const uint32_t out = row[i], in = row[i + w];  // (the last step reads inside the pitch; its sums are not kept)
      s += in - out, q += in * in - out * out;
    }
  }
}

// sums[j][i] = the h rows of rows[][i] from row j on, j < nyo: the same running sum down a stretch of a column.
__device__ void dp_column_sums(const uint2* rows, int h, int nxo, int nyo, uint2* sums) {
  const int nseg = DP_TB / nxo > 0 ? DP_TB / nxo : 1;
  const int len = (nyo + nseg - 1) / nseg;
  for (int t = (int)threadIdx.x; t < nxo * nseg; t += DP_TB) {
    const int i = t % nxo, j0 = (t / nxo) * len, j1 = min(nyo, j0 + len);
    if (j0 >= j1) continue;
    uint32_t s = 0, q = 0;
    for (int r = 0; r < h; ++r) {
      const uint2 v = rows[(j0 + r) * nxo + i];
      s += v.x, q += v.y;
    }
    for (int j = j0; j < j1; ++j) {
      sums[j * nxo + i] = make_uint2(s, q);
      if (j + 1 < j1) {
        const uint2 out = rows[j * nxo + i], in = rows[(j + h) * nxo + i];
        s += in.x - out.x, q += in.y - out.y;
      }
    }
  }
}

// sum(T S) of the offset whose window starts at word `base` of the staged window, byte phase `ph`.  Four words of a
// template row (one 16-byte read; a row's pitch `tw4` is a multiple of four words, zero beyond w) meet five of the window's
// per step: the eight reads are in flight together, and two accumulators halve the dependent chain of the dot products.
__device__ __forceinline__ uint32_t dp_dot(const uint32_t* win, const uint32_t* tpl, int base, uint32_t ph, int pitch,
                                           int h, int tw4) {
  uint32_t acc0 = 0, acc1 = 0;
  for (int r = 0; r < h; ++r) {
    const uint32_t* row = win + base + r * pitch;
    const uint4* trow = reinterpret_cast<const uint4*>(tpl + r * tw4);
    uint32_t lo = row[0];
    for (int k = 0; k < tw4; k += 4) {
      const uint4 t = trow[k >> 2];
      const uint32_t s1 = row[k + 1], s2 = row[k + 2], s3 = row[k + 3], s4 = row[k + 4];
      acc0 = __builtin_amdgcn_udot4(t.x, __builtin_amdgcn_alignbyte(s1, lo, ph), acc0, false);
      acc1 = __builtin_amdgcn_udot4(t.y, __builtin_amdgcn_alignbyte(s2, s1, ph), acc1, false);
      acc0 = __builtin_amdgcn_udot4(t.z, __builtin_amdgcn_alignbyte(s3, s2, ph), acc0, false);
      acc1 = __builtin_amdgcn_udot4(t.w, __builtin_amdgcn_alignbyte(s4, s3, ph), acc1, false);
      lo = s4;
    }
  }
  return acc0 + acc1;
}

__global__ __launch_bounds__(DP_TB) void k_displace_u8(const DpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char dp_lds[];
  const DpPoint p = dp_point(a);
  if (!p.ok) return dp_no_result(a, p, GLH_DISPLACE_OUTSIDE);
  const int nxo = 2 * a.rx + 1, nyo = 2 * a.ry + 1, noff = nxo * nyo;
  const int sh = a.h + 2 * a.ry, tw4 = dp_tpitch_u8(a.w), pitch = a.wstride;
  const DpLayout lay = dp_layout(false, a.h, a.rx, a.ry, pitch, tw4);
  uint2* trow_sums = reinterpret_cast<uint2*>(dp_lds + DP_TROWS);
  uint32_t* tpl = reinterpret_cast<uint32_t*>(dp_lds + lay.tpl);
  uint32_t* win = reinterpret_cast<uint32_t*>(dp_lds + lay.win);
  uint2* sums = reinterpret_cast<uint2*>(dp_lds + lay.sums);
  uint2* rows = reinterpret_cast<uint2*>(dp_lds + lay.surf);
  double* surf = reinterpret_cast<double*>(dp_lds + lay.surf);
  const int wx0 = p.l + p.gu - a.rx, wy0 = p.t + p.gv - a.ry;
  const int x0 = wx0 & ~3, cb0 = wx0 - x0;  // (the staged window starts on a word of the frame's columns)
  const size_t plane = (size_t)a.width * a.height;
  const uint8_t* fa = static_cast<const uint8_t*>(a.frames) + plane * p.fa;
  const uint8_t* fb = static_cast<const uint8_t*>(a.frames) + plane * p.fb;
  for (int idx = (int)threadIdx.x; idx < sh * pitch; idx += DP_TB) {
    const int y = idx / pitch, x = idx - y * pitch;
    const int gy = wy0 + y, gx = x0 + 4 * x;
    uint32_t word = 0;
    if (gy >= 0 && gy < a.height)
      for (int m = 0; m < 4; ++m)
        if (gx + m >= 0 && gx + m < a.width) word |= (uint32_t)fb[(size_t)gy * a.width + gx + m] << (8 * m);
    win[idx] = word;
  }
  for (int idx = (int)threadIdx.x; idx < a.h * tw4; idx += DP_TB) {
    const int r = idx / tw4, k = idx - r * tw4;
    uint32_t word = 0;
    for (int m = 0; m < 4; ++m)
      if (4 * k + m < a.w) word |= (uint32_t)fa[(size_t)(p.t + r) * a.width + p.l + 4 * k + m] << (8 * m);
    tpl[idx] = word;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.h) {
    uint32_t s = 0, q = 0;
    for (int k = 0; k < tw4; ++k) {
      const uint32_t v = tpl[threadIdx.x * tw4 + k];
      s = __builtin_amdgcn_udot4(v, 0x01010101u, s, false);
      q = __builtin_amdgcn_udot4(v, v, q, false);
    }
    trow_sums[threadIdx.x] = make_uint2(s, q);
  }
  dp_row_sums(reinterpret_cast<const uint8_t*>(win), 4 * pitch, cb0, sh, a.w, nxo, rows);
  __syncthreads();
  dp_column_sums(rows, a.h, nxo, nyo, sums);
  int64_t st = 0, stt = 0;
  for (int r = 0; r < a.h; ++r) st += trow_sums[r].x, stt += trow_sums[r].y;
  const int64_t n = (int64_t)a.w * a.h;
  const int64_t vt = n * stt - st * st;
  if (!(vt > 0)) return dp_no_result(a, p, GLH_DISPLACE_FLAT);  // (the same in every thread)
  __syncthreads();  // (rows is read out: the surface takes its place)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double best = 0.0;
  int bidx = -1;
  for (int o = (int)threadIdx.x; o < noff; o += DP_TB) {
    const int j = o / nxo, i = o - j * nxo;
    const int cb = cb0 + i;
    const uint32_t ts = dp_dot(win, tpl, j * pitch + (cb >> 2), (uint32_t)(cb & 3), pitch, a.h, tw4);
    const uint2 sq = sums[o];
    const int64_t vs = n * (int64_t)sq.y - (int64_t)sq.x * sq.x;
    const int64_t num = n * (int64_t)ts - st * (int64_t)sq.x;
    const double sc = dp_score((double)num, (double)vt, (double)vs);
    const bool ok = dp_inside(a, p, i, j) && vs > 0 && isfinite(sc);
    surf[o] = ok ? sc : nan;
    if (a.surface) a.surface[p.out * noff + o] = ok ? sc : nan;
    if (ok && (bidx < 0 || sc > best)) best = sc, bidx = o;
  }
  dp_finish(a, p, dp_lds, surf, best, bidx);
}

// ---- the float path --------------------------------------------------------------------------------------------------------

// The sums of DP_FB offsets at once over the template in row-major order; FIRST also forms the template's own.
template <bool FIRST>
__device__ __forceinline__ void dp_sums_f32(const float* win, const float* tpl, const int (&base)[DP_FB], int pitch, int w,
                                            int h, double (&ss)[DP_FB], double (&sq)[DP_FB], double (&sx)[DP_FB],
                                            double& st, double& stt) {
  for (int r = 0; r < h; ++r) {
    const float* trow = tpl + r * w;
    const int ro = r * pitch;
    for (int c = 0; c < w; ++c) {
      const double t = (double)trow[c];
      if (FIRST) st += t, stt = fma(t, t, stt);
#pragma unroll
      for (int k = 0; k < DP_FB; ++k) {
        const double s = (double)win[base[k] + ro + c];
        ss[k] += s;
        sq[k] = fma(s, s, sq[k]);
        sx[k] = fma(t, s, sx[k]);
      }
    }
  }
}

__global__ __launch_bounds__(DP_TB) void k_displace_f32(const DpArgs a) {
  extern __shared__ __attribute__((aligned(16))) char dp_lds[];
  int& flat = *reinterpret_cast<int*>(dp_lds + DP_FLAT);
  const DpPoint p = dp_point(a);
  if (!p.ok) return dp_no_result(a, p, GLH_DISPLACE_OUTSIDE);
  const int nxo = 2 * a.rx + 1, nyo = 2 * a.ry + 1, noff = nxo * nyo;
  const int sw = a.w + 2 * a.rx, sh = a.h + 2 * a.ry, pitch = a.wstride;
  const DpLayout lay = dp_layout(true, a.h, a.rx, a.ry, pitch, a.w);
  float* tpl = reinterpret_cast<float*>(dp_lds + lay.tpl);
  float* win = reinterpret_cast<float*>(dp_lds + lay.win);
  double* surf = reinterpret_cast<double*>(dp_lds + lay.surf);
  const int wx0 = p.l + p.gu - a.rx, wy0 = p.t + p.gv - a.ry;
  const size_t plane = (size_t)a.width * a.height;
  const float* fa = static_cast<const float*>(a.frames) + plane * p.fa;
  const float* fb = static_cast<const float*>(a.frames) + plane * p.fb;
  for (int idx = (int)threadIdx.x; idx < sh * sw; idx += DP_TB) {
    const int y = idx / sw, x = idx - y * sw;
    const int gy = wy0 + y, gx = wx0 + x;
    win[y * pitch + x] = gy >= 0 && gy < a.height && gx >= 0 && gx < a.width ? fb[(size_t)gy * a.width + gx] : 0.f;
  }
  for (int idx = (int)threadIdx.x; idx < a.h * a.w; idx += DP_TB) {
    const int r = idx / a.w, c = idx - r * a.w;
    tpl[idx] = fa[(size_t)(p.t + r) * a.width + p.l + c];
  }
  __syncthreads();
  const double n = (double)(a.w * a.h);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double st = 0.0, stt = 0.0, vt = 0.0, best = 0.0;
  int bidx = -1;
  bool first = true;
  for (int o0 = (int)threadIdx.x; o0 < noff; o0 += DP_FB * DP_TB) {
    int base[DP_FB];
    double ss[DP_FB], sq[DP_FB], sx[DP_FB];
#pragma unroll
    for (int k = 0; k < DP_FB; ++k) {
      const int o = o0 + k * DP_TB < noff ? o0 + k * DP_TB : o0;  // (past the end: the first again, not kept)
      const int j = o / nxo;
      base[k] = j * pitch + (o - j * nxo);
      ss[k] = sq[k] = sx[k] = 0.0;
    }
    if (first) {
      dp_sums_f32<true>(win, tpl, base, pitch, a.w, a.h, ss, sq, sx, st, stt);
      vt = n * stt - st * st;
      if (threadIdx.x == 0) flat = !(vt > 0.0);
      first = false;
    } else {
      dp_sums_f32<false>(win, tpl, base, pitch, a.w, a.h, ss, sq, sx, st, stt);
    }
#pragma unroll
    for (int k = 0; k < DP_FB; ++k) {
      const int o = o0 + k * DP_TB;
      if (o >= noff) break;
      const int j = o / nxo, i = o - j * nxo;
      const double vs = n * sq[k] - ss[k] * ss[k];
      const double num = n * sx[k] - st * ss[k];
      const double sc = dp_score(num, vt, vs);
      const bool ok = vt > 0.0 && dp_inside(a, p, i, j) && vs > 0.0 && isfinite(sc);
      surf[o] = ok ? sc : nan;
      if (a.surface) a.surface[p.out * noff + o] = ok ? sc : nan;
      if (ok && (bidx < 0 || sc > best)) best = sc, bidx = o;
    }
  }
  __syncthreads();  // (thread 0 always owns offset 0, so `flat` is written)
  if (flat) {
    if (threadIdx.x == 0) {
      a.duv[2 * p.out] = a.duv[2 * p.out + 1] = nan;
      a.score[p.out] = nan;
      a.status[p.out] = GLH_DISPLACE_FLAT;
    }
    return;
  }
  dp_finish(a, p, dp_lds, surf, best, bidx);
}

}  // namespace

int displacements_run(const DisplaceJob& j) {
  const size_t plane = (size_t)j.width * j.height, n = (size_t)j.n, np = (size_t)j.n_pairs;
  const size_t fbytes = plane * j.n_frames * (j.is_float ? 4 : 1);
  const int nxo = 2 * j.rx + 1, nyo = 2 * j.ry + 1, noff = nxo * nyo;
  const size_t gbytes = j.guess ? (j.guess_per_pair ? np : 1) * n * 8 : 0;
  const DpPlan plan = dp_plan(j.is_float != 0, j.w, j.h, j.rx, j.ry);
  const int pitch = plan.pitch;
  const size_t lds = plan.lds;
  if (lds > DP_LDS_LIMIT) return fail(GLH_E_UNSUPPORTED, "displacements: %zu bytes of LDS for one point", lds);
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernel)
  StageEvents<DP_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dframes, dpairs, dcorners, dvalid, dguess, dduv, dscore, dstatus, dsurf;
  CHK(dframes.alloc(fbytes));
  CHK(dpairs.alloc(np * 8));
  CHK(dcorners.alloc(n * 8));
  CHK(dvalid.alloc(n));
  CHK(dguess.alloc(gbytes));
  CHK(dduv.alloc(np * n * 16));
  CHK(dscore.alloc(np * n * 8));
  CHK(dstatus.alloc(np * n));
  if (j.surface) CHK(dsurf.alloc(np * n * noff * 8));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dframes.p, j.frames, fbytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dpairs.p, j.pairs, np * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dcorners.p, j.corners, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dvalid.p, j.valid, n, hipMemcpyHostToDevice));
  if (gbytes) HIPCHK(hipMemcpy(dguess.p, j.guess, gbytes, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  DpArgs a{};
  a.frames = dframes.p, a.width = j.width, a.height = j.height;
  a.pairs = dpairs.as<int32_t>(), a.corners = dcorners.as<int32_t>(), a.valid = dvalid.as<uint8_t>(), a.n = j.n;
  a.guess = gbytes ? dguess.as<int32_t>() : nullptr, a.guess_pair_stride = j.guess_per_pair ? 2 * j.n : 0;
  a.w = j.w, a.h = j.h, a.rx = j.rx, a.ry = j.ry, a.subpixel = j.subpixel, a.wstride = pitch;
  a.duv = dduv.as<double>(), a.score = dscore.as<double>(), a.status = dstatus.as<uint8_t>();
  a.surface = j.surface ? dsurf.as<double>() : nullptr;
  const void* kernel = j.is_float ? (const void*)k_displace_f32 : (const void*)k_displace_u8;
  if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)j.n, (unsigned)j.n_pairs);
  if (j.is_float)
    hipLaunchKernelGGL(k_displace_f32, grid, dim3(DP_TB), lds, s, a);
  else
    hipLaunchKernelGGL(k_displace_u8, grid, dim3(DP_TB), lds, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  CHK(dduv.down(j.duv, np * n * 16));
  CHK(dscore.down(j.score, np * n * 8));
  CHK(dstatus.down(j.status, np * n));
  if (j.surface) CHK(dsurf.down(j.surface, np * n * noff * 8));
  CHK(ev.record(3, s));
  HIPCHK(hipEventSynchronize(ev.e[3]));
  ev.report(j.times_ms, DP_TIMES, DP_TIMES);
  return GLH_OK;
}

}  // namespace glh
