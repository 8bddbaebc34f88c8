// glh_ransac_draw.h -- the RANSAC samples of optimize.ransac_pairs(samples="device") (INPUTS.md, "Device samples: the
// rule"): how many hypotheses a pair gets, the pairs that are enumerated, and the draw of one hypothesis.  Plain C++
// without a HIP header: glh_calib.hip's k_rg_draw and tests/hostcheck/ransac_draw_hostcheck.cpp, a CPU program under the
// sanitizers, compile the very same code.
//
// Pair k of the call has s rows, s > n.  C = C(s, n), exactly; H_k = min(iterations, C).  A pair with C <= iterations is
// ENUMERATED: its hypotheses are all C combinations in lexicographic order, made on the host.  Otherwise hypothesis h is
// DRAWN by Floyd's algorithm from the Philox block(s) of counter (h, k, i >> 2, RANSAC_DRAW_TAG) under the call's two seed
// words, and stored in ascending row order: a pure function of (seed, k, h, s, n).
#pragma once
#include <stdint.h>

#include "glh_math.h"

namespace glh {

constexpr uint32_t RANSAC_DRAW_TAG = 0x52414e53u;            // "RANS": the domain of these streams (counter word 3)
constexpr int64_t RANSAC_DRAW_LIMIT = ((int64_t)1 << 31) - 1;  // rows of a pair and `iterations`: at most this

// min(C(s, n), cap + 1) for 0 <= s, cap <= RANSAC_DRAW_LIMIT, exactly: the running value is C(s - m + i, i), m =
// min(n, s - n), an integer that does not decrease with i, so it is given up the moment it exceeds `cap` -- before that it
// is at most 2^31 - 1 and its product with a factor below 2^31 stays below 2^62.
GLH_HD int64_t rd_combinations(int64_t s, int64_t n, int64_t cap) {
  if (n < 0 || n > s) return 0;
  const int64_t m = n < s - n ? n : s - n;
  int64_t c = 1;
  for (int64_t i = 1; i <= m; ++i) {
    c = c * (s - m + i) / i;  // (exact: i consecutive integers hold a multiple of every number up to i)
    if (c > cap) return cap + 1;
  }
  return c;
}

// H_k of a pair of s rows; *enumerated: whether its hypotheses are all combinations.  A pair with s <= n has none.
GLH_HD int64_t rd_hypotheses(int64_t s, int64_t n, int64_t iterations, bool* enumerated) {
  *enumerated = false;
  if (s <= n || iterations < 0) return 0;
  const int64_t c = rd_combinations(s, n, iterations);
  *enumerated = c <= iterations;
  return c < iterations ? c : iterations;
}

// The first `count` combinations of n of s rows in lexicographic order: out [count][n].  count <= C(s, n).
inline void rd_enumerate(int64_t s, int n, int64_t count, int64_t* out) {
  for (int64_t q = 0; q < count; ++q) {
    int64_t* c = out + q * n;
    if (q == 0) {
      for (int i = 0; i < n; ++i) c[i] = i;
      continue;
    }
    const int64_t* before = c - n;
    int at = n - 1;  // the last place that can still move up
    while (at > 0 && before[at] == s - n + at) --at;
    for (int i = 0; i < at; ++i) c[i] = before[i];
    c[at] = before[at] + 1;
    for (int i = at + 1; i < n; ++i) c[i] = c[i - 1] + 1;
  }
}

// Hypothesis h of pair k, n of s rows (n < s <= RANSAC_DRAW_LIMIT): out[0 .. n) = base + row, ascending.  Floyd: for
// i = 0 .. n - 1, j = s - n + i and t = mulhi32(word_i, j + 1), a row of 0 .. j; j is taken if t is in the sample
// already, t otherwise.  The sample is kept sorted as it grows: j exceeds every row taken before it, so it goes to the
// end; t goes where the search for it stopped.
GLH_HD void rd_draw(uint32_t seed0, uint32_t seed1, uint32_t k, uint32_t h, uint32_t s, int n, int32_t base, int32_t* out) {
  uint32_t word[4];
  for (int i = 0; i < n; ++i) {
    if ((i & 3) == 0) philox4x32(h, k, (uint32_t)(i >> 2), RANSAC_DRAW_TAG, seed0, seed1, word);
    const uint32_t j = s - (uint32_t)n + (uint32_t)i;
    const int32_t t = base + (int32_t)mulhi32(word[i & 3], j + 1u);
    int lo = 0, hi = i;  // the first place whose row is not below t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (out[mid] < t) lo = mid + 1; else hi = mid;
    }
    if (lo < i && out[lo] == t) {
      out[i] = base + (int32_t)j;
    } else {
      for (int q = i; q > lo; --q) out[q] = out[q - 1];
      out[lo] = t;
    }
  }
}

}  // namespace glh
