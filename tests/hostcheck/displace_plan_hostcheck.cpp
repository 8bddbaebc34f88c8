// displace_plan_hostcheck.cpp -- the LDS plan of the displacement kernels on the CPU: a stand-alone program, built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_displace_plan_host.py and run directly.  It drives the
// header the kernels and their launch include, csrc/glh_displace_plan.h, for every template of 3 .. 63 a side and every
// reach of 1 .. 32 per axis, on both paths, and requires of each plan what glh_displace.hip argues in its comments:
//   * every part of the layout starts on a multiple of 16 bytes, the parts follow one another without overlap, and each
//     is as large as what the kernels keep in it;
//   * every LDS word and byte the integer kernel's loops read in a window row lies inside the row's pitch;
//   * the float path's pitch holds a window row and is nxo modulo 32;
//   * the region stays within DP_LDS_LIMIT.
// It prints the largest region of each path ("largest integer ...", "largest float ...") and how often the float path's
// fallback was taken; the last line is "ok" unless something failed.
#include <cstdio>

#include "../../glimpse_amd/csrc/glh_displace.h"
#include "../../glimpse_amd/csrc/glh_displace_plan.h"

using namespace glh;

static long failures = 0;
#define EXPECT(cond)                                                                                        \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      if (failures < 20)                                                                                    \
        std::printf("FAILED line %d: %s (float %d, w %d, h %d, rx %d, ry %d)\n", __LINE__, #cond, (int)is_float, w, h, rx, ry); \
      ++failures;                                                                                           \
    }                                                                                                       \
  } while (0)

struct Largest {
  size_t lds = 0;
  int w = 0, h = 0, rx = 0, ry = 0;
};

static Largest largest[2];
static long fallbacks = 0, plans = 0;

static void check(bool is_float, int w, int h, int rx, int ry) {
  const int nxo = 2 * rx + 1, nyo = 2 * ry + 1, noff = nxo * nyo, sw = w + 2 * rx, sh = h + 2 * ry;
  const DpPlan plan = dp_plan(is_float, w, h, rx, ry);
  const DpLayout l = dp_layout(is_float, h, rx, ry, plan.pitch, plan.tpitch);
  ++plans;
  EXPECT(plan.lds == (size_t)l.total);
  // the head: the reduction's scores (one double a wave) and indices (one int a wave), the flat flag, and one pair of
  // 32-bit sums per template row (k_displace_u8: trow_sums[threadIdx.x] for threadIdx.x < h)
  EXPECT(DP_RED_SCORE + 8 * (DP_TB / 64) <= DP_RED_INDEX && DP_RED_INDEX + 4 * (DP_TB / 64) <= DP_FLAT);
  EXPECT(DP_FLAT + 4 <= DP_TROWS && DP_TROWS + 8 * h <= DP_HEAD);
  EXPECT(DP_RED_SCORE % 8 == 0 && DP_RED_INDEX % 4 == 0 && DP_FLAT % 4 == 0 && DP_TROWS % 8 == 0);
  // every part starts on a multiple of 16 bytes and ends where the next begins, or before
  EXPECT(l.tpl % 16 == 0 && l.win % 16 == 0 && l.sums % 16 == 0 && l.surf % 16 == 0 && l.total % 16 == 0);
  EXPECT(l.tpl >= DP_HEAD);
  EXPECT(l.tpl + 4 * h * plan.tpitch <= l.win);      // the template: h rows of tpitch words or floats
  EXPECT(l.win + 4 * sh * plan.pitch <= l.sums);     // the window: sh rows of pitch words or floats
  if (is_float) {
    EXPECT(l.surf == l.sums);                        // (no sums of offsets on the float path)
    EXPECT(l.surf + 8 * noff <= l.total);            // the surface: one double per offset
    // k_displace_f32 stages win[y * pitch + x] for x < sw and reads win[j * pitch + i + r * pitch + c] for i < nxo,
    // c < w (dp_sums_f32): column nxo - 1 + w - 1 = sw - 1 at most; a template row is w floats (tpl + r * w)
    EXPECT(plan.tpitch == w);
    EXPECT(plan.pitch >= sw);
    const bool fallback = plan.pitch == sw && sw % 32 != nxo % 32;
    if (fallback) ++fallbacks;
    EXPECT(fallback || (plan.pitch % 32 == nxo % 32 && plan.pitch < sw + 32));
  } else {
    EXPECT(l.sums + 8 * noff <= l.surf);             // the offsets' sums: one pair of 32-bit sums per offset
    EXPECT(l.surf + 8 * sh * nxo <= l.total);        // the row sums: sh * nxo pairs (dp_row_sums: rows[y * nxo + i]) ...
    EXPECT(sh * nxo >= noff);                        // ... where the surface of noff doubles later lies
    // a template row is whole 16-byte reads that hold its w bytes (dp_dot: trow[k >> 2] for k < tw4 in steps of 4)
    EXPECT(plan.tpitch % 4 == 0 && 4 * plan.tpitch >= w && plan.tpitch == dp_tpitch_u8(w));
    // dp_dot: row = win + j * pitch + ((cb0 + i) >> 2) with cb0 <= 3 and i <= 2 rx; it reads row[0] and row[k + 1] ..
    // row[k + 4] for k < tw4 in steps of 4, row[tw4] the last: word (3 + 2 rx) / 4 + tpitch of a window row at most
    const int last_word = (3 + 2 * rx) / 4 + plan.tpitch;
    EXPECT(last_word < plan.pitch);
    // dp_row_sums: row = win + y * pitch + cb0 (bytes); it reads row[i0 + c] for c < w and row[i], row[i + w] for
    // i < i1 <= nxo, row[nxo - 1 + w] the last: byte 3 + 2 rx + w of a window row at most
    const int last_byte = 3 + 2 * rx + w;
    EXPECT(last_byte < 4 * plan.pitch);
    // the rows the loops reach: j + r <= 2 ry + h - 1 = sh - 1 (dp_dot), j0 + r and j + h <= sh - 1 (dp_column_sums,
    // which steps only while j + 1 < j1 <= nyo)
    EXPECT(2 * ry + (h - 1) == sh - 1 && (nyo - 2) + h <= sh - 1);
  }
  EXPECT(plan.lds <= DP_LDS_LIMIT);
  Largest& big = largest[is_float ? 1 : 0];
  if (plan.lds > big.lds) big = Largest{plan.lds, w, h, rx, ry};
}

int main() {
  for (int is_float = 0; is_float < 2; ++is_float)
    for (int w = DP_MIN_SIDE; w <= DP_MAX_SIDE; ++w)
      for (int h = DP_MIN_SIDE; h <= DP_MAX_SIDE; ++h)
        for (int rx = 1; rx <= DP_MAX_REACH; ++rx)
          for (int ry = 1; ry <= DP_MAX_REACH; ++ry) check(is_float != 0, w, h, rx, ry);
  // the pitch steps of the template the kernel's comments name: 4, 8, 12, 16 words, at w = 16 / 17, 32 / 33, 48 / 49
  {
    const bool is_float = false;
    const int w = 0, h = 0, rx = 0, ry = 0;
    EXPECT(dp_tpitch_u8(3) == 4 && dp_tpitch_u8(16) == 4 && dp_tpitch_u8(17) == 8 && dp_tpitch_u8(32) == 8);
    EXPECT(dp_tpitch_u8(33) == 12 && dp_tpitch_u8(48) == 12 && dp_tpitch_u8(49) == 16 && dp_tpitch_u8(63) == 16);
    EXPECT(dp_pitch(65, 1) == 65 && dp_pitch(66, 1) == 97 && dp_pitch(5, 3) == 35 && dp_pitch(127, 1) == 129);
    EXPECT(plans == 2L * 61 * 61 * 32 * 32);
    EXPECT(fallbacks == 0);  // (no accepted argument takes the float path's fallback)
  }
  const char* names[2] = {"integer", "float"};
  for (int k = 0; k < 2; ++k)
    std::printf("largest %s %zu bytes at w %d h %d rx %d ry %d\n", names[k], largest[k].lds, largest[k].w, largest[k].h,
                largest[k].rx, largest[k].ry);
  std::printf("plans %ld, float fallbacks %ld\n", plans, fallbacks);
  if (failures) {
    std::printf("%ld failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
