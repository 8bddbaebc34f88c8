// ransac_draw_hostcheck.cpp -- the samples of optimize.ransac_pairs(samples="device") on the CPU: a stand-alone program,
// built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_ransac_draw_host.py and run directly.  It drives
// the headers the library includes, csrc/glh_ransac_draw.h (the count, the enumeration, the draw) and the part of
// csrc/glh_ransac_plan.h that serves glh_calib_ransac_groups_drawn:
//   * every drawn sample is checked here: n distinct rows below s, ascending;
//   * the samples, the counts and the enumerations are printed, one line each ("draw", "count", "enum"), and the test
//     compares every number with tests/ransac_draw_restated.py, math.comb and itertools.combinations;
//   * every refusal rg_check gained, with the calls either side of it that are served.
// The last line is "ok" unless something failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../../glimpse_amd/csrc/glh_ransac_draw.h"
#include "../../glimpse_amd/csrc/glh_ransac_plan.h"

using namespace glh;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static const uint32_t SEED0 = 0x9E3779B9u, SEED1 = 0x00C0FFEEu;  // (tests/test_ransac_draw_host.py: SEED)
static const int64_t LIMIT = RANSAC_DRAW_LIMIT;

// "draw s n k h base : rows": the pairs k and hypotheses h below for every s > n of the two lists.
static void check_draws() {
  const int ns[] = {1, 2, 4, 5, 12, 40, 65};
  const uint32_t ks[] = {0u, 7u, (1u << 24) - 1u};
  const uint32_t hs[] = {0u, 1u, 2u, 3u, 99u, 65536u, 0x7FFFFFFEu};
  for (int n : ns) {
    const int64_t sizes[] = {n + 1, 13, 63, 64, 65, 257, (int64_t)1 << 20, LIMIT};
    for (size_t q = 0; q < sizeof(sizes) / sizeof(sizes[0]); ++q) {
      const int64_t s = sizes[q];
      if (s <= n || (q > 0 && s == n + 1)) continue;
      for (uint32_t k : ks)
        for (uint32_t h : hs) {
          // (one more place either side: the draw writes its n and no other)
          std::vector<int32_t> row((size_t)n + 2, -7);
          const int32_t base = s < 1000 ? 1000 : 0;  // (a group's first row in the handle; rows stay below 2^31)
          rd_draw(SEED0, SEED1, k, h, (uint32_t)s, n, base, row.data() + 1);
          EXPECT(row[0] == -7 && row[(size_t)n + 1] == -7);
          bool fine = true;
          for (int i = 0; i < n; ++i) {
            const int64_t r = (int64_t)row[(size_t)i + 1] - base;
            fine = fine && r >= 0 && r < s && (i == 0 || row[(size_t)i + 1] > row[(size_t)i]);
          }
          EXPECT(fine);
          std::printf("draw %lld %d %u %u :", (long long)s, n, k, h);
          for (int i = 0; i < n; ++i) std::printf(" %lld", (long long)row[(size_t)i + 1] - base);
          std::printf("\n");
        }
    }
  }
}

// "count s n iterations : H enumerated C" with C = min(C(s, n), iterations + 1).
static void print_count(int64_t s, int64_t n, int64_t iterations) {
  bool all = false;
  const int64_t hyps = rd_hypotheses(s, n, iterations, &all);
  std::printf("count %lld %lld %lld : %lld %d %lld\n", (long long)s, (long long)n, (long long)iterations, (long long)hyps, all ? 1 : 0,
              (long long)rd_combinations(s, n, iterations));
}

static void check_counts() {
  const int64_t iterations[] = {0, 1, 2, 10, 100, 1000, 1000000, LIMIT};
  for (int64_t s = 1; s <= 40; ++s)
    for (int64_t n = 1; n <= s + 1; ++n)
      for (int64_t it : iterations) print_count(s, n, it);
  // C == iterations and C == iterations + 1: C(6, 2) = 15, C(13, 6) = 1716, C(13, 10) = 286 (n > s / 2), C(2^31 - 1, 1)
  for (int64_t it : {14, 15, 16}) print_count(6, 2, it);
  for (int64_t it : {1715, 1716, 1717}) print_count(13, 6, it);
  for (int64_t it : {285, 286, 287}) print_count(13, 10, it);
  for (int64_t it : {LIMIT - 1, LIMIT}) print_count(LIMIT, 1, it);
  // no overflow: the largest pair, samples of 64, of half of it and of all but one or two rows; 2^20 rows
  for (int64_t n : {(int64_t)2, (int64_t)64, (int64_t)65, LIMIT / 2, LIMIT - 2, LIMIT - 1, LIMIT})
    for (int64_t it : {(int64_t)100, LIMIT - 1, LIMIT}) print_count(LIMIT, n, it);
  for (int64_t n : {(int64_t)2, (int64_t)12, (int64_t)1 << 19, ((int64_t)1 << 20) - 2})
    for (int64_t it : {(int64_t)100, LIMIT}) print_count((int64_t)1 << 20, n, it);
  print_count(100, 50, LIMIT);
  print_count(65536, 2, LIMIT);  // (C = 2 147 450 880, the largest below the limit among samples of two)
  print_count(65537, 2, LIMIT);
  EXPECT(rd_combinations(5, -1, 100) == 0 && rd_combinations(5, 6, 100) == 0 && rd_combinations(0, 0, 100) == 1);
  bool all = true;
  EXPECT(rd_hypotheses(10, 2, -1, &all) == 0 && !all);
}

// "enum s n count : rows of every combination"
static void check_enumerations() {
  const int64_t cases[][3] = {{5, 2, 10}, {6, 3, 20}, {7, 1, 7}, {6, 5, 6}, {4, 4, 1}, {13, 2, 78}, {13, 3, 10}, {9, 4, 126}, {9, 4, 0},
                              {66, 65, 66}, {LIMIT, 2, 5}};
  for (const auto& c : cases) {
    const int64_t s = c[0], count = c[2];
    const int n = (int)c[1];
    std::vector<int64_t> out((size_t)(count * n) + 1, -7);
    rd_enumerate(s, n, count, out.data());
    EXPECT(out.back() == -7);
    std::printf("enum %lld %d %lld :", (long long)s, n, (long long)count);
    for (int64_t i = 0; i < count * n; ++i) std::printf(" %lld", (long long)out[(size_t)i]);
    std::printf("\n");
  }
}

// The handle and the call of ransac_pairs_hostcheck.cpp -- MATCHES (cameras 0, 1; 64 rows), ROTATION (1, 2; 65),
// ROTATION_XY (2, 3; 0 rows), POINTS (camera 3; 0 rows); groups over the first three, two parameters, samples of three
// rows -- as glh_calib_ransac_groups_drawn makes it: group 1 drawn, the others given.
struct Case {
  std::vector<int32_t> kind{2, 3, 4, 0}, cam_a{0, 1, 2, 3}, cam_b{1, 2, 3, 3};
  std::vector<int64_t> row_offset{0, 64, 129, 129, 129};
  std::vector<int32_t> group_control{0, 1, 2}, group_cam{1, 1, 3}, slots{3, 5};
  std::vector<double> x0{1, 2, 3, 4, 5, 6}, lb{0, 0, 0, 0, 0, 0}, ub{9, 9, 9, 9, 9, 9}, scale{1, 1, 1, 1, 1, 1};
  std::vector<int64_t> hyp_offset{0, 2, 5, 5};
  std::vector<int64_t> samples{0, 1, 63, 5, 5, 5, -1, 1 << 30, 0, 63, 129, 7, 0, 0, 0};  // (group 1's: not rows of its control)
  std::vector<int32_t> group_id{5, 0, 1 << 30};
  std::vector<uint8_t> drawn{0, 1, 0};
  int n_cams = 4, n_controls = 4, n_groups = 3, p = 2, n = 3, max_nfev = 10;
  bool draws = true, no_samples = false, no_ids = false, no_flags = false;
  // (what the check only asks to be there: the cameras' vectors, the observations of the ROTATION control, the outputs)
  double vectors[1] = {0.0}, observed[1] = {0.0}, f64[3] = {};
  int32_t i32[4] = {};
  uint8_t u8[1] = {};
  CalibTable table() const { return CalibTable{n_cams, n_controls, kind.data(), row_offset.data(), cam_a.data(), cam_b.data()}; }
  CalibRansac call() {
    return CalibRansac{{p, slots.data(), x0.data(), lb.data(), ub.data(), scale.data(), max_nfev, 1e-8, 1e-8, 1e-8}, nullptr, vectors,
                       n_groups, group_control.data(), group_cam.data(), nullptr, observed, hyp_offset.data(), n,
                       no_samples ? nullptr : samples.data(), 3.0, 0, f64, i32, i32 + 1, f64 + 1, i32 + 2, f64 + 2, i32 + 3, u8, nullptr,
                       draws, no_ids ? nullptr : group_id.data(), no_flags ? nullptr : drawn.data()};
  }
};

static char last[400];  // the message of the last refusal

static bool served(Case& c, const char* word = nullptr) {
  char* msg = last;
  msg[0] = 0;
  const bool ok = rg_check(c.table(), c.call(), msg, sizeof(last));
  if (!ok && std::strncmp(msg, "ransac groups:", 14) != 0) EXPECT(!"a refusal without a message");
  if (!ok && word && !std::strstr(msg, word)) {
    std::printf("FAILED: expected \"%s\" in \"%s\"\n", word, msg);
    ++failures;
  }
  return ok;
}

static void refused(const char* word, const std::function<void(Case&)>& change) {
  Case c;
  EXPECT(served(c));
  change(c);
  if (served(c, word)) {
    std::printf("FAILED: not refused: %s\n", word);
    ++failures;
  }
}

// The whole message of a refusal, as rg_check's format strings gave it before its checks were shared with fs_check.
static void says(const char* message, const std::function<void(Case&)>& change) {
  Case c;
  change(c);
  if (served(c) || std::strcmp(last, message) != 0) {
    std::printf("FAILED: expected \"%s\", got \"%s\"\n", message, last);
    ++failures;
  }
}

static void accepted(const std::function<void(Case&)>& change) {
  Case c;
  change(c);
  EXPECT(served(c));
}

static void check_plan() {
  refused("ids and drawn flags", [](Case& c) { c.no_ids = true; });
  refused("ids and drawn flags", [](Case& c) { c.no_flags = true; });
  refused("has the id", [](Case& c) { c.group_id[2] = -1; });
  refused("drawn flag", [](Case& c) { c.drawn[0] = 2; });
  refused("drawn flag", [](Case& c) { c.drawn[2] = 255; });
  // a drawn group has more rows than a sample: 65 rows serve samples of 64, not of 65 (every group drawn: no samples given)
  accepted([](Case& c) { c.drawn = {1, 1, 1}, c.no_samples = true, c.n = 63; });
  refused("more rows than that", [](Case& c) { c.drawn = {1, 1, 1}, c.no_samples = true, c.n = 64; });  // (group 0 has 64)
  accepted([](Case& c) { c.drawn = {0, 1, 0}, c.n = 3, c.hyp_offset = {0, 2, 2, 2}, c.row_offset = {0, 64, 67, 67, 67}; });
  refused("more rows than that", [](Case& c) { c.row_offset = {0, 64, 67, 67, 67}; });  // (group 1, drawn: 3 rows for samples of 3)
  accepted([](Case& c) { c.drawn = {0, 1, 1}; });  // (a drawn group without rows and without hypotheses)
  // the samples may be missing only if no group with a hypothesis reads them
  refused("null samples", [](Case& c) { c.no_samples = true; });
  refused("null samples", [](Case& c) { c.no_samples = true, c.drawn = {1, 0, 0}; });
  accepted([](Case& c) { c.no_samples = true, c.drawn = {1, 1, 0}; });  // (group 2 is given, and has no hypothesis)
  accepted([](Case& c) { c.no_samples = true, c.drawn = {1, 1, 1}; });
  // the rows of a group that is not drawn are checked as before, those of a drawn one are not read
  refused("samples row", [](Case& c) { c.samples[2] = 64; });
  refused("samples row", [](Case& c) { c.drawn = {0, 0, 0}; });
  accepted([](Case& c) { c.drawn = {1, 1, 0}, c.samples[2] = 64; });
  // glh_calib_ransac_groups' own call: ids and flags are not looked at, every row is
  refused("samples row", [](Case& c) { c.draws = false; });
  accepted([](Case& c) { c.draws = false, c.no_ids = c.no_flags = true, c.samples = {0, 1, 63, 5, 5, 5, 64, 65, 128, 100, 101, 102, 64, 64, 64}; });
  accepted([](Case& c) { c.n_groups = 0, c.row_offset = {0, 0, 0, 0, 0}, c.no_ids = c.no_flags = c.no_samples = true; });
  EXPECT(RANSAC_DRAWN_TIMES == RANSAC_TIMES + 1);
  // the whole messages of the refusals above
  says("ransac groups: null argument: the groups' ids and drawn flags", [](Case& c) { c.no_ids = true; });
  says("ransac groups: null argument: the groups' ids and drawn flags", [](Case& c) { c.no_flags = true; });
  says("ransac groups: group 2 has the id -1: ids are not negative", [](Case& c) { c.group_id[2] = -1; });
  says("ransac groups: group 0 has the drawn flag 2: 0 or 1", [](Case& c) { c.drawn[0] = 2; });
  says("ransac groups: group 2 has the drawn flag 255: 0 or 1", [](Case& c) { c.drawn[2] = 255; });
  says("ransac groups: group 0 draws samples of 64 of its 64 rows: a drawn group has more rows than that",
       [](Case& c) { c.drawn = {1, 1, 1}, c.no_samples = true, c.n = 64; });
  says("ransac groups: group 1 draws samples of 3 of its 3 rows: a drawn group has more rows than that",
       [](Case& c) { c.row_offset = {0, 64, 67, 67, 67}; });
  says("ransac groups: null samples", [](Case& c) { c.no_samples = true; });
  says("ransac groups: null samples", [](Case& c) { c.no_samples = true, c.drawn = {1, 0, 0}; });
  says("ransac groups: hypothesis 0 of group 0 samples row 64 outside its control's rows 0 .. 64", [](Case& c) { c.samples[2] = 64; });
  says("ransac groups: hypothesis 2 of group 1 samples row -1 outside its control's rows 64 .. 129", [](Case& c) { c.drawn = {0, 0, 0}; });
  says("ransac groups: hypothesis 2 of group 1 samples row -1 outside its control's rows 64 .. 129", [](Case& c) { c.draws = false; });
}

int main() {
  check_draws();
  check_counts();
  check_enumerations();
  check_plan();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
