// ransac_pairs_hostcheck.cpp -- the host plan of glh_calib_ransac_groups (csrc/glh_ransac_plan.h) on the CPU: a stand-alone
// program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_ransac_pairs_host.py and run directly.
// It drives the header the library includes: every condition rg_check refuses (and a valid call it accepts before and
// after each), the mask offsets and the chunk boundaries for group sizes 0, 1, 63, 64, 65 and 2^20 against brute-force
// restatements, and the limits at 2^31 mask bytes.
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

// A handle of four controls -- MATCHES (cameras 0, 1; 64 rows), ROTATION (1, 2; 65), ROTATION_XY (2, 3; 0 rows), POINTS
// (camera 3; 0 rows) -- and a valid call over the first three: two parameters, samples of three rows.
struct Case {
  std::vector<int32_t> kind{2, 3, 4, 0}, cam_a{0, 1, 2, 3}, cam_b{1, 2, 3, 3};
  std::vector<int64_t> row_offset{0, 64, 129, 129, 129};
  std::vector<int32_t> group_control{0, 1, 2}, group_cam{1, 1, 3}, slots{3, 5};
  std::vector<double> x0{1, 2, 3, 4, 5, 6}, lb{0, 0, 0, 0, 0, 0}, ub{9, 9, 9, 9, 9, 9}, scale{1, 1, 1, 1, 1, 1};
  std::vector<int64_t> hyp_offset{0, 2, 5, 5};
  std::vector<int64_t> samples{0, 1, 63, 5, 5, 5, 64, 65, 128, 100, 101, 102, 64, 64, 64};
  int n_cams = 4, n_controls = 4, n_groups = 3, p = 2, n = 3, max_nfev = 10;
  double ftol = 1e-8, xtol = 1e-8, gtol = 1e-8, max_error = 3.0;
  bool outputs = true;
  // (what the check only asks to be there: the cameras' vectors, the observations of the ROTATION control, the outputs)
  double vectors[1] = {0.0}, observed[1] = {0.0}, f64[3] = {};
  int32_t i32[4] = {};
  uint8_t u8[1] = {};
  CalibTable table() const { return CalibTable{n_cams, n_controls, kind.data(), row_offset.data(), cam_a.data(), cam_b.data()}; }
  CalibRansac call() {
    return CalibRansac{{p, slots.data(), x0.data(), lb.data(), ub.data(), scale.data(), max_nfev, ftol, xtol, gtol}, nullptr, vectors,
                       n_groups, group_control.data(), group_cam.data(), nullptr, observed, hyp_offset.data(), n, samples.data(),
                       max_error, 0, f64, i32, i32 + 1, f64 + 1, i32 + 2, f64 + 2, i32 + 3, outputs ? u8 : nullptr, nullptr};
  }
};

static char last[400];  // the message of the last refusal

static bool served(Case& c, const char* word = nullptr) {
  char* msg = last;
  msg[0] = 0;
  const bool ok = rg_check(c.table(), c.call(), msg, sizeof(last));
  if (!ok && (std::strlen(msg) == 0 || std::strncmp(msg, "ransac groups:", 14) != 0)) EXPECT(!"a refusal without a message");
  if (!ok && word && !std::strstr(msg, word)) {
    std::printf("expected \"%s\" in \"%s\"\n", word, msg);
    ++failures;
  }
  return ok;
}

// The whole message of a refusal, as the format strings of rg_check gave it before its checks were shared with fs_check.
static void says(const char* message, const std::function<void(Case&)>& change) {
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

static void refused(const char* word, const std::function<void(Case&)>& change) {
  Case c;
  EXPECT(served(c));
  change(c);
  if (served(c, word)) {
    std::printf("FAILED: not refused: %s\n", word);
    ++failures;
  }
}

static void check_refusals() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  refused("null argument", [](Case& c) { c.outputs = false; });
  refused("groups", [](Case& c) { c.n_groups = -1; });
  refused("groups", [](Case& c) { c.n_groups = 1 << 24; });
  refused("parameters", [](Case& c) { c.p = 0; });
  refused("parameters", [](Case& c) { c.p = 19; });
  refused("entry", [](Case& c) { c.slots = {3, 3}; });
  refused("entry", [](Case& c) { c.slots = {3, 6}; });
  refused("entry", [](Case& c) { c.slots = {7, 4}; });
  refused("entry", [](Case& c) { c.slots = {3, 20}; });
  refused("entry", [](Case& c) { c.slots = {-1, 4}; });
  refused("samples of", [](Case& c) { c.n = 0; });
  refused("evaluations", [](Case& c) { c.max_nfev = 0; });
  refused("evaluations", [](Case& c) { c.ftol = -1.0; });
  refused("evaluations", [](Case& c) { c.ftol = 1.0; });
  refused("evaluations", [nan](Case& c) { c.xtol = nan; });
  refused("evaluations", [inf](Case& c) { c.gtol = inf; });
  refused("max_error", [nan](Case& c) { c.max_error = nan; });
  refused("hyp_offset[0]", [](Case& c) { c.hyp_offset[0] = 1; });
  refused("not decreasing", [](Case& c) { c.hyp_offset = {0, 3, 2, 5}; });
  refused("not decreasing", [](Case& c) { c.hyp_offset = {0, 2, (int64_t)1 << 31, (int64_t)1 << 31}; });
  refused("is control", [](Case& c) { c.group_control[2] = 4; });
  refused("is control", [](Case& c) { c.group_control[0] = -1; });
  refused("POINTS or LINES", [](Case& c) { c.group_control[2] = 3; });
  refused("POINTS or LINES", [](Case& c) { c.kind[1] = 1; });
  refused("ascending", [](Case& c) { c.group_control = {1, 0, 2}; });
  refused("ascending", [](Case& c) { c.group_control = {0, 1, 1}; });
  refused("fits camera", [](Case& c) { c.group_cam[0] = 4; });
  refused("fits camera", [](Case& c) { c.group_cam[0] = -1; });
  refused("neither camera", [](Case& c) { c.group_cam[0] = 2; });
  refused("neither camera", [](Case& c) { c.group_cam[2] = 0; });
  refused("outside its bounds", [](Case& c) { c.x0[3] = 10.0; });
  refused("outside its bounds", [](Case& c) { c.x0[0] = -1.0; });
  refused("outside its bounds", [nan](Case& c) { c.x0[5] = nan; });
  refused("outside its bounds", [inf](Case& c) { c.x0[5] = inf, c.ub[5] = inf; });
  refused("lower one", [](Case& c) { c.lb[2] = c.ub[2] = c.x0[2]; });
  refused("scale", [](Case& c) { c.scale[4] = 0.0; });
  refused("scale", [nan](Case& c) { c.scale[4] = nan; });
  refused("scale", [inf](Case& c) { c.scale[1] = inf; });
  refused("every row", [](Case& c) { c.n_groups = 1; });  // (control 1's rows are in no group)
  refused("samples row", [](Case& c) { c.samples[2] = 64; });   // (group 0's rows end at 63)
  refused("samples row", [](Case& c) { c.samples[6] = 63; });   // (group 1's begin at 64)
  refused("samples row", [](Case& c) { c.samples[14] = 129; });
  refused("samples row", [](Case& c) { c.samples[0] = -1; });
  {  // null pointers, one at a time
    Case c;
    const CalibTable t = c.table();
    char msg[400];
    for (int which = 0; which < 8; ++which) {
      CalibRansac r = c.call();
      const int32_t** i32[] = {&r.group_control, &r.group_cam, &r.slots};
      const double** f64[] = {&r.x0, &r.lb, &r.ub, &r.scale};
      if (which < 3)
        *i32[which] = nullptr;
      else if (which < 7)
        *f64[which - 3] = nullptr;
      else
        r.hyp_offset = nullptr;
      EXPECT(!rg_check(t, r, msg, sizeof(msg)) && std::strcmp(msg, "ransac groups: null argument") == 0);
    }
    for (int which = 0; which < 8; ++which) {  // every output is asked for
      CalibRansac r = c.call();
      void** out[] = {(void**)&r.x, (void**)&r.status, (void**)&r.consensus, (void**)&r.refit_x, (void**)&r.refit_status,
                      (void**)&r.mean_error, (void**)&r.winner, (void**)&r.inlier};
      *out[which] = nullptr;
      EXPECT(!rg_check(t, r, msg, sizeof(msg)) && std::strcmp(msg, "ransac groups: null argument") == 0);
    }
    CalibRansac r = c.call();
    r.samples = nullptr;
    EXPECT(!rg_check(t, r, msg, sizeof(msg)) && std::strcmp(msg, "ransac groups: null samples") == 0);
    r = c.call();
    r.observed = nullptr;  // (control 1 is a ROTATION control with rows)
    EXPECT(!rg_check(t, r, msg, sizeof(msg)) &&
           std::strcmp(msg, "ransac groups: control 1 is a ROTATION control, whose obs are camera coordinates: pass observed") == 0);
    CalibTable none = t;
    none.row_offset = nullptr;
    EXPECT(!rg_check(none, c.call(), msg, sizeof(msg)) && std::strcmp(msg, "ransac groups: a handle without controls") == 0);
    EXPECT(rg_check(t, c.call(), msg, sizeof(msg)));
  }
  // the whole messages of the refusals above, one fault each
  says("ransac groups: null argument", [](Case& c) { c.outputs = false; });
  says("ransac groups: -1 groups: fewer than 2^24 are served", [](Case& c) { c.n_groups = -1; });
  says("ransac groups: 16777216 groups: fewer than 2^24 are served", [](Case& c) { c.n_groups = 1 << 24; });
  says("ransac groups: 0 parameters: 1 .. 18 are served", [](Case& c) { c.p = 0; });
  says("ransac groups: 19 parameters: 1 .. 18 are served", [](Case& c) { c.p = 19; });
  says("ransac groups: parameter 1 is entry 3 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 3}; });
  says("ransac groups: parameter 1 is entry 6 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 6}; });
  says("ransac groups: parameter 0 is entry 7 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {7, 4}; });
  says("ransac groups: parameter 1 is entry 20 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {3, 20}; });
  says("ransac groups: parameter 0 is entry -1 of the camera vector: distinct ones of 0 .. 5, 8 .. 19", [](Case& c) { c.slots = {-1, 4}; });
  says("ransac groups: samples of 0 rows", [](Case& c) { c.n = 0; });
  says("ransac groups: 0 evaluations, ftol 1e-08, xtol 1e-08, gtol 1e-08", [](Case& c) { c.max_nfev = 0; });
  says("ransac groups: 10 evaluations, ftol -1, xtol 1e-08, gtol 1e-08", [](Case& c) { c.ftol = -1.0; });
  says("ransac groups: 10 evaluations, ftol 1, xtol 1e-08, gtol 1e-08", [](Case& c) { c.ftol = 1.0; });
  says("ransac groups: 10 evaluations, ftol 1e-08, xtol nan, gtol 1e-08", [nan](Case& c) { c.xtol = nan; });
  says("ransac groups: 10 evaluations, ftol 1e-08, xtol 1e-08, gtol inf", [inf](Case& c) { c.gtol = inf; });
  says("ransac groups: max_error is NaN", [nan](Case& c) { c.max_error = nan; });
  says("ransac groups: hyp_offset[0] is 1, not 0", [](Case& c) { c.hyp_offset[0] = 1; });
  says("ransac groups: group 1 ends at hypothesis 2 after 3: not decreasing, fewer than 2^31 in all",
       [](Case& c) { c.hyp_offset = {0, 3, 2, 5}; });
  says("ransac groups: group 1 ends at hypothesis 2147483648 after 2: not decreasing, fewer than 2^31 in all",
       [](Case& c) { c.hyp_offset = {0, 2, (int64_t)1 << 31, (int64_t)1 << 31}; });
  says("ransac groups: group 2 is control 4 of 4", [](Case& c) { c.group_control[2] = 4; });
  says("ransac groups: group 0 is control -1 of 4", [](Case& c) { c.group_control[0] = -1; });
  says("ransac groups: group 2 is control 3, a POINTS or LINES control: the match kinds are served", [](Case& c) { c.group_control[2] = 3; });
  says("ransac groups: group 1 is control 1, a POINTS or LINES control: the match kinds are served", [](Case& c) { c.kind[1] = 1; });
  says("ransac groups: group 1 is control 0 after control 1: the groups name distinct controls in ascending order",
       [](Case& c) { c.group_control = {1, 0, 2}; });
  says("ransac groups: group 2 is control 1 after control 1: the groups name distinct controls in ascending order",
       [](Case& c) { c.group_control = {0, 1, 1}; });
  says("ransac groups: group 0 fits camera 4 of 4", [](Case& c) { c.group_cam[0] = 4; });
  says("ransac groups: group 0 fits camera -1 of 4", [](Case& c) { c.group_cam[0] = -1; });
  says("ransac groups: group 0 fits camera 2, which is neither camera (0, 1) of its control", [](Case& c) { c.group_cam[0] = 2; });
  says("ransac groups: group 2 fits camera 0, which is neither camera (2, 3) of its control", [](Case& c) { c.group_cam[2] = 0; });
  says("ransac groups: group 1, parameter 1 starts at 10 outside its bounds 0 .. 9", [](Case& c) { c.x0[3] = 10.0; });
  says("ransac groups: group 0, parameter 0 starts at -1 outside its bounds 0 .. 9", [](Case& c) { c.x0[0] = -1.0; });
  says("ransac groups: group 2, parameter 1 starts at nan outside its bounds 0 .. 9", [nan](Case& c) { c.x0[5] = nan; });
  says("ransac groups: group 2, parameter 1 starts at inf outside its bounds 0 .. inf", [inf](Case& c) { c.x0[5] = inf, c.ub[5] = inf; });
  says("ransac groups: group 1, parameter 0 has the bounds 3 .. 3: the lower one must be below the upper one",
       [](Case& c) { c.lb[2] = c.ub[2] = c.x0[2]; });
  says("ransac groups: group 2, parameter 0 has scale 0", [](Case& c) { c.scale[4] = 0.0; });
  says("ransac groups: group 2, parameter 0 has scale nan", [nan](Case& c) { c.scale[4] = nan; });
  says("ransac groups: group 0, parameter 1 has scale inf", [inf](Case& c) { c.scale[1] = inf; });
  says("ransac groups: the groups hold 64 of the handle's 129 rows: every row belongs to exactly one group", [](Case& c) { c.n_groups = 1; });
  says("ransac groups: hypothesis 0 of group 0 samples row 64 outside its control's rows 0 .. 64", [](Case& c) { c.samples[2] = 64; });
  says("ransac groups: hypothesis 2 of group 1 samples row 63 outside its control's rows 64 .. 129", [](Case& c) { c.samples[6] = 63; });
  says("ransac groups: hypothesis 4 of group 1 samples row 129 outside its control's rows 64 .. 129", [](Case& c) { c.samples[14] = 129; });
  says("ransac groups: hypothesis 0 of group 0 samples row -1 outside its control's rows 0 .. 64", [](Case& c) { c.samples[0] = -1; });
  {  // no group and no row: served; a degenerate sample (one row n times) is the fit's business, not the plan's
    Case c;
    c.row_offset = {0, 0, 0, 0, 0};
    c.n_groups = 0;
    EXPECT(served(c));
  }
}

// 2^31 mask bytes: refused; one fewer: served.
static void check_mask_limit() {
  Case c;
  c.kind = {2};
  c.cam_a = {0}, c.cam_b = {1};
  c.n_controls = 1, c.n_groups = 1, c.n = 1;
  c.group_control = {0}, c.group_cam = {0};
  c.row_offset = {0, (int64_t)1 << 16};
  c.hyp_offset = {0, (int64_t)1 << 15};
  c.samples.assign((size_t)1 << 15, 7);
  EXPECT(!served(c, "2^31"));
  EXPECT(std::strcmp(last, "ransac groups: the consensus masks take 2^31 bytes or more: fewer are served in one call") == 0);
  c.hyp_offset = {0, ((int64_t)1 << 15) - 1};
  EXPECT(served(c));
  EXPECT(rg_mask_bytes((int64_t)1 << 16, (int64_t)1 << 15) == RANSAC_MASK_LIMIT);
  EXPECT(rg_mask_bytes((int64_t)1 << 16, ((int64_t)1 << 15) - 1) == RANSAC_MASK_LIMIT - ((int64_t)1 << 16));
  EXPECT(rg_mask_bytes(INT64_MAX, INT64_MAX) == RANSAC_MASK_LIMIT && rg_mask_bytes(0, INT64_MAX) == 0 && rg_mask_bytes(5, 0) == 0);
  EXPECT(rg_mask_bytes(3, (RANSAC_MASK_LIMIT - 1) / 3) < RANSAC_MASK_LIMIT && rg_mask_bytes(3, (RANSAC_MASK_LIMIT - 1) / 3 + 1) == RANSAC_MASK_LIMIT);
}

// The chunking, restated: group g opens a chunk unless the groups since the last opening, g included, stay at or below the
// budget together.
static std::vector<int32_t> chunks_restated(const std::vector<int64_t>& rows, const std::vector<int64_t>& hyps, int64_t budget) {
  std::vector<int32_t> out(rows.size());
  size_t opened = 0;
  int chunk = 0;
  for (size_t g = 0; g < rows.size(); ++g) {
    __int128 together = 0;
    for (size_t k = opened; k <= g; ++k) {
      const __int128 b = (__int128)rows[k] * hyps[k];
      together += b > RANSAC_MASK_LIMIT ? (__int128)RANSAC_MASK_LIMIT : b;
    }
    if (g > opened && together > budget) {
      opened = g;
      ++chunk;
    }
    out[g] = chunk;
  }
  return out;
}

static void check_offsets_and_chunks() {
  const int64_t sizes[] = {0, 1, 63, 64, 65, (int64_t)1 << 20};
  const int64_t hyp_counts[] = {0, 1, 4, 100};
  const int64_t budgets[] = {0, 1, 63, 64, 65, 256, 6400, (int64_t)1 << 20, (int64_t)1 << 30, RANSAC_MASK_LIMIT - 1};
  uint64_t state = 12345;
  auto next = [&state]() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
  };
  for (int trial = 0; trial < 400; ++trial) {
    const int G = trial < 6 ? 1 : 1 + (int)(next() % 40);
    std::vector<int64_t> rows(G), hyps(G), offset(G + 1);
    for (int g = 0; g < G; ++g) {
      rows[g] = trial < 6 ? sizes[trial] : sizes[next() % 6];
      hyps[g] = hyp_counts[next() % 4];
    }
    const int64_t total = rg_mask_offsets(G, rows.data(), hyps.data(), offset.data());
    __int128 at = 0;
    for (int g = 0; g < G; ++g) {
      EXPECT(offset[g] == (at > RANSAC_MASK_LIMIT ? RANSAC_MASK_LIMIT : (int64_t)at));
      at += (__int128)rows[g] * hyps[g];
    }
    EXPECT(total == (at > RANSAC_MASK_LIMIT ? RANSAC_MASK_LIMIT : (int64_t)at) && offset[G] == total);
    EXPECT(rg_mask_offsets(G, rows.data(), hyps.data(), nullptr) == total);
    for (int64_t budget : budgets) {
      std::vector<int32_t> chunk_of(G, -7);
      const int count = rg_chunks(G, rows.data(), hyps.data(), budget, chunk_of.data());
      const std::vector<int32_t> want = chunks_restated(rows, hyps, budget);
      EXPECT(chunk_of == want && count == want.back() + 1);
      // every chunk stays at or below the budget unless it is one group
      for (int ch = 0; ch < count; ++ch) {
        __int128 bytes = 0;
        int members = 0;
        for (int g = 0; g < G; ++g)
          if (chunk_of[g] == ch) bytes += (__int128)rows[g] * hyps[g], ++members;
        EXPECT(members >= 1 && (members == 1 || bytes <= budget));
      }
    }
  }
  int32_t none = 0;
  EXPECT(rg_chunks(0, nullptr, nullptr, 100, &none) == 0);
  // 2^20 groups of one row and one hypothesis, 64 bytes to a chunk
  const int many = 1 << 20;
  std::vector<int64_t> ones((size_t)many, 1);
  std::vector<int32_t> chunk_of((size_t)many);
  EXPECT(rg_chunks(many, ones.data(), ones.data(), 64, chunk_of.data()) == many / 64);
  bool fine = true;
  for (int g = 0; g < many; ++g) fine = fine && chunk_of[g] == g / 64;
  EXPECT(fine);
  std::vector<int64_t> offset((size_t)many + 1);
  EXPECT(rg_mask_offsets(many, ones.data(), ones.data(), offset.data()) == many && offset[12345] == 12345);
}

int main() {
  check_refusals();
  check_mask_limit();
  check_offsets_and_chunks();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
