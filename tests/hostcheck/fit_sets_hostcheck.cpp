// fit_sets_hostcheck.cpp -- what glh_calib_fit_sets checks before a device is touched (csrc/glh_ransac_plan.h: fs_check) on
// the CPU: a stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_fit_sets_host.py
// and run directly.  It drives the header the library includes: every refusal, with a valid call accepted before and after
// it, and the whole message of each.  The messages are literals: the format strings glimpse_hip.hip held when the checks
// were still written there, evaluated by hand for the case.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

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

// A handle of one camera and three controls -- POINTS (64 rows), ROTATION (1 row), LINES (no row) -- and a valid call:
// three parameters, two sets of the POINTS rows 0 .. 9, every row scored.
struct Case {
  std::vector<int32_t> kind{GLH_CALIB_POINTS, GLH_CALIB_ROTATION, GLH_CALIB_LINES}, cam{0, 0, 0};
  std::vector<int64_t> row_offset{0, 64, 65, 65};
  std::vector<int32_t> slots{3, 4, 5};
  std::vector<double> x0{10, 20, 30}, lb{0, 0, 0}, ub{100, 100, 100}, scale{1, 1, 1};
  std::vector<int64_t> set_offset{0, 4, 10}, set_rows{0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
  int n_cams = 1, fit_cam = 0, p = 3, n_sets = 2, max_nfev = 50, score = 1;
  double ftol = 1e-8, xtol = 1e-8, gtol = 1e-8, max_error = 3.0;
  int missing = -1;  // which of the pointers below is null
  // (what the check only asks to be there)
  double vectors[1] = {0.0}, observed[1] = {0.0}, x[1] = {0.0}, mean_error[1] = {0.0};
  int32_t status[1] = {0};
  uint8_t inlier[1] = {0};
  CalibTable table() const { return CalibTable{n_cams, (int)kind.size(), kind.data(), row_offset.data(), cam.data(), cam.data()}; }
  CalibFit call() {
    CalibFit f{{p, slots.data(), x0.data(), lb.data(), ub.data(), scale.data(), max_nfev, ftol, xtol, gtol}, nullptr, vectors, fit_cam,
               nullptr, observed, n_sets, set_offset.data(), set_rows.data(), score, max_error, x, status, mean_error, inlier, nullptr};
    const void** pointers[] = {(const void**)&f.vectors, (const void**)&f.slots, (const void**)&f.x0, (const void**)&f.lb,
                               (const void**)&f.ub, (const void**)&f.scale, (const void**)&f.set_offset, (const void**)&f.x,
                               (const void**)&f.status, (const void**)&f.mean_error, (const void**)&f.set_rows,
                               (const void**)&f.inlier, (const void**)&f.observed};
    if (missing >= 0) *pointers[missing] = nullptr;
    return f;
  }
};
static const int REQUIRED = 10;  // the first ten of call()'s pointers: "null argument"
static const int NO_SET_ROWS = 10, NO_INLIER = 11, NO_OBSERVED = 12;

static char last[400];  // the message of the last refusal

static bool served(Case& c) {
  last[0] = 0;
  return fs_check(c.table(), c.call(), last, sizeof(last));
}

static void refused(const char* message, const std::function<void(Case&)>& change) {
  Case c;
  EXPECT(served(c));
  change(c);
  if (served(c) || std::strcmp(last, message) != 0) {
    std::printf("FAILED: expected \"%s\", got \"%s\"\n", message, last);
    ++failures;
  }
  Case again;
  EXPECT(served(again));
}

static void accepted(const std::function<void(Case&)>& change) {
  Case c;
  change(c);
  if (!served(c)) {
    std::printf("FAILED: refused: \"%s\"\n", last);
    ++failures;
  }
}

static void lines_rows(Case& c) { c.row_offset = {0, 64, 65, 70}; }  // the LINES control with 5 rows

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // tests/test_gpu_ransac.py: test_bad_arguments_leave_the_handle_usable's `bad`, entry by entry
  refused("calib fit: camera 1 of 1", [](Case& c) { c.fit_cam = 1; });
  refused("calib fit: camera -1 of 1", [](Case& c) { c.fit_cam = -1; });
  refused("calib fit: parameter 2 is entry 6 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 4, 6}; });
  refused("calib fit: parameter 1 is entry 3 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 3, 5}; });
  refused("calib fit: parameter 2 is entry 20 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 4, 20}; });
  refused("calib fit: parameter 1 starts at 420 outside its bounds 0 .. 100", [inf](Case& c) { c.x0[1] += 400, c.ub = {inf, 100, inf}; });
  refused("calib fit: parameter 1 has scale 0", [](Case& c) { c.scale = {1, 0, 1}; });
  refused("calib fit: parameter 1 has scale nan", [nan](Case& c) { c.scale = {1, nan, 1}; });
  refused("calib fit: row 65 of 65", [](Case& c) { c.set_rows = {56, 57, 58, 59, 60, 61, 62, 63, 64, 65}; });  // (the last is past the end)
  refused("calib fit: row -1 of 65", [](Case& c) { c.set_rows = {0, -1, -2, -3, -4, -5, -6, -7, -8, -9}; });
  refused("calib fit: set_offset[0] is 1, not 0", [](Case& c) { c.set_offset = {1, 4, 10}; });
  refused("calib fit: set 1 ends at row 4 after 6: not decreasing, fewer than 2^31 rows in all", [](Case& c) { c.set_offset = {0, 6, 4}; });
  refused("calib fit: parameter 0 has the bounds 10 .. 10: the lower one must be below the upper one", [](Case& c) { c.lb = c.ub = c.x0; });
  refused("calib fit: parameter 1 starts at 20 outside its bounds 20 .. -20", [inf](Case& c) { c.lb = {-inf, 20, -inf}, c.ub = {inf, -20, inf}; });
  refused("calib fit: 0 evaluations, ftol 1e-08, xtol 1e-08, gtol 1e-08", [](Case& c) { c.max_nfev = 0; });
  refused("calib fit: 50 evaluations, ftol -1, xtol 1e-08, gtol 1e-08", [](Case& c) { c.ftol = -1.0; });
  refused("calib fit: 50 evaluations, ftol 1e-08, xtol nan, gtol 1e-08", [nan](Case& c) { c.xtol = nan; });
  refused("calib fit: 0 parameters: 1 .. 18 are served", [](Case& c) { c.p = 0, c.slots = {}, c.x0 = c.lb = c.ub = c.scale = {}; });
  refused("calib fit: 19 parameters: 1 .. 18 are served", [](Case& c) {
    c.p = 19, c.slots.resize(19), c.x0.assign(19, 0.0), c.lb.assign(19, -1.0), c.ub.assign(19, 1.0), c.scale.assign(19, 1.0);
    for (int i = 0; i < 19; ++i) c.slots[i] = i;
  });
  // a null for each required pointer
  for (int which = 0; which < REQUIRED; ++which) refused("calib fit: null argument", [which](Case& c) { c.missing = which; });
  refused("calib fit: null set rows", [](Case& c) { c.missing = NO_SET_ROWS; });
  accepted([](Case& c) { c.missing = NO_SET_ROWS, c.set_offset = {0, 0, 0}; });  // (no row in any set: none is read)
  // the sets
  refused("calib fit: -1 sets: fewer than 2^24 are served", [](Case& c) { c.n_sets = -1; });
  refused("calib fit: 16777216 sets: fewer than 2^24 are served", [](Case& c) { c.n_sets = 1 << 24; });
  accepted([](Case& c) { c.n_sets = 0; });
  refused("calib fit: set 1 ends at row 2147483648 after 4: not decreasing, fewer than 2^31 rows in all",
          [](Case& c) { c.set_offset = {0, 4, (int64_t)1 << 31}; });
  // Lines: no row of such a control is fitted, and a handle that holds one with rows is not scored
  refused("calib fit: row 66 belongs to control 2, a Lines control", [](Case& c) { lines_rows(c), c.score = 0, c.set_rows[9] = 66; });
  refused("calib fit: row 65 belongs to control 2, a Lines control", [](Case& c) { lines_rows(c), c.set_rows[0] = 65; });
  refused("calib fit: scoring covers every row, and the handle holds a Lines control", [](Case& c) { lines_rows(c); });
  accepted([](Case& c) { lines_rows(c), c.score = 0; });
  accepted([](Case& c) { lines_rows(c), c.score = 0, c.set_rows[9] = 64; });  // (the ROTATION control's row)
  // scoring
  refused("calib fit: max_error is NaN", [nan](Case& c) { c.max_error = nan; });
  accepted([nan](Case& c) { c.max_error = nan, c.score = 0; });
  refused("calib fit: null inlier output", [](Case& c) { c.missing = NO_INLIER; });
  accepted([](Case& c) { c.missing = NO_INLIER, c.score = 0; });
  const auto many = [](Case& c, int n_sets) {  // 2^20 + 1 rows, and sets without rows after the first two
    c.row_offset = {0, (int64_t)1 << 20, ((int64_t)1 << 20) + 1, ((int64_t)1 << 20) + 1};
    c.n_sets = n_sets;
    c.set_offset.resize((size_t)n_sets + 1, 10);
  };
  refused("calib fit: 2048 sets of 1048577 rows to score: fewer than 2^31 in all are served", [many](Case& c) { many(c, 2048); });
  accepted([many](Case& c) { many(c, 2047); });
  accepted([many](Case& c) { many(c, 2048), c.score = 0; });
  // a ROTATION control with rows reads `observed`
  refused("calib fit: control 1 is a ROTATION control, whose obs are camera coordinates: pass observed",
          [](Case& c) { c.missing = NO_OBSERVED; });
  accepted([](Case& c) { c.missing = NO_OBSERVED, c.row_offset = {0, 64, 64, 64}; });
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
