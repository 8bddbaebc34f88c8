// glh_displace_plan.h -- the LDS plan of the displacement kernels (glh_displace.hip): where the parts of a workgroup's
// one dynamic region lie, how far apart the rows of the template and of the search window are, and how many bytes that
// takes.  The kernels read the layout, the launch (displacements_run) asks dp_plan for the pitches and the size.  Plain
// C++ without a HIP header, so that tests/hostcheck/displace_plan_hostcheck.cpp compiles the very same code for the CPU
// under the sanitizers and checks it for every template and reach the ABI accepts.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define GLH_DP_HD __host__ __device__ inline
#else
#define GLH_DP_HD inline
#endif

namespace glh {

constexpr int DP_TB = 256;
constexpr size_t DP_LDS_LIMIT = 160 * 1024;

// LDS is one dynamic region (no static beside it, which would shift its base off 16 bytes); every part starts on a
// multiple of 16 bytes.  The head is the reduction's scratch, the flat flag and the template's row sums; then the
// template, the window, the offsets' sums (integer path) and the score surface, which on the integer path first holds
// the row sums.
constexpr int DP_RED_SCORE = 0, DP_RED_INDEX = 32, DP_FLAT = 48, DP_TROWS = 64, DP_HEAD = DP_TROWS + 8 * 64;

struct DpLayout {
  int tpl, win, sums, surf, total;  // byte offsets into the region, and its size
};

GLH_DP_HD int dp_up16(int v) { return (v + 15) & ~15; }

// pitch: of a window row; tpitch: of a template row (both in 4-byte units)
GLH_DP_HD DpLayout dp_layout(bool is_float, int h, int rx, int ry, int pitch, int tpitch) {
  const int nxo = 2 * rx + 1, noff = nxo * (2 * ry + 1), sh = h + 2 * ry;
  DpLayout l;
  l.tpl = DP_HEAD;
  l.win = l.tpl + dp_up16(4 * h * tpitch);
  l.sums = l.win + dp_up16(4 * sh * pitch);
  l.surf = l.sums + (is_float ? 0 : dp_up16(8 * noff));
  l.total = l.surf + dp_up16(8 * (is_float ? noff : sh * nxo));  // (sh >= 2 ry + 1: the row sums are the larger)
  return l;
}

// The template's row pitch on the integer path: whole 16-byte reads.
GLH_DP_HD int dp_tpitch_u8(int w) { return (((w + 3) >> 2) + 3) & ~3; }

// The smallest pitch >= `need` that is `rem` modulo 32.
inline int dp_pitch(int need, int rem) { return need + ((rem - need) % 32 + 32) % 32; }

// The window's row pitch in words on the integer path.  The lanes of a 32-lane group own consecutive offsets: within one
// row of offsets they read `span` consecutive words (at most min(nxo, 32) + 3 bytes, whatever the phase), and they reach
// over `rows` rows of offsets, `pitch` words apart.  The smallest pitch >= `need` for which those bank ranges are
// pairwise disjoint modulo the 32 banks of a 4-byte read; an odd pitch where none is.
inline int dp_pitch_u8(int need, int nxo) {
  const int lanes = nxo < 32 ? nxo : 32;
  const int span = (lanes + 3 + 3) / 4, rows = nxo >= 32 ? 2 : 32 / nxo + 2;
  for (int p = need; p < need + 32; ++p) {
    bool ok = true;
    for (int k = 1; k < rows && ok; ++k) {
      const int d = (k * p) % 32;
      ok = d >= span && 32 - d >= span;
    }
    if (ok) return p;
  }
  return need | 1;
}

struct DpPlan {
  int pitch, tpitch;  // of a window row and of a template row, in 4-byte units
  size_t lds;         // bytes of the region
};

// What the launch uses for a template of w x h and a reach of (rx, ry).  displacements_run refuses a plan beyond
// DP_LDS_LIMIT; tests/hostcheck/displace_plan_hostcheck.cpp forms every plan of w, h in 3 .. 63 and rx, ry in 1 .. 32 and
// finds the largest at 125 296 bytes (integer path, w of 49 .. 63) and 115 808 bytes (float path, w = 63), both at h = 63
// with reach (32, 32): no argument the ABI accepts reaches the refusal or the float path's fallback to a pitch of sw,
// which stay as guards.
inline DpPlan dp_plan(bool is_float, int w, int h, int rx, int ry) {
  const int nxo = 2 * rx + 1;
  const int sw = w + 2 * rx;
  int pitch, tpitch;
  if (is_float) {
    pitch = dp_pitch(sw, nxo % 32), tpitch = w;
    if ((size_t)dp_layout(true, h, rx, ry, pitch, tpitch).total > DP_LDS_LIMIT) pitch = sw;
  } else {
    // (a row holds the bytes before the first column and every word the last step of dp_dot reads: the template's
    // padded row and one more)
    tpitch = dp_tpitch_u8(w);
    pitch = dp_pitch_u8((2 * rx + 3) / 4 + tpitch + 1, nxo);
  }
  return DpPlan{pitch, tpitch, (size_t)dp_layout(is_float, h, rx, ry, pitch, tpitch).total};
}

}  // namespace glh
