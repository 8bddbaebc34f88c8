// velocity_plan_hostcheck.cpp -- the LDS plan of the velocity field's stack kernel on the CPU: a stand-alone program, built
// with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_velocity_plan_host.py and run directly.  It drives the
// header the kernel and its launch include, csrc/glh_velocity_plan.h, for every number of pairs the ABI accepts,
// 1 .. VF_MAX_PAIRS, and requires of each plan what glh_velocity.hip relies on:
//   * a list is a power of two long and holds every pair; a run is a power of two of 1 .. VF_MAX_RUN nodes, and twice as
//     long a run would not fit (or is beyond VF_MAX_RUN);
//   * every part of the layout starts on a multiple of 16 bytes, the parts follow one another without overlap, each as
//     large as what the kernel keeps in it, and the region stays within VF_LDS_LIMIT;
//   * every index the kernel forms -- a slot of a list, a flag, a count, a median, both ends of every compare-exchange of
//     the bitonic network -- lies inside its part: the program marks the bytes of a region of plan.lds bytes that the
//     kernel's index expressions reach, part by part, and the sanitizers watch the region's ends;
//   * the bitonic network, run on the CPU with the kernel's index expressions over a list of every length, sorts.
// It prints the plan at the steps ("pairs P: len L, nodes G, B bytes") and the largest region; the last line is "ok"
// unless something failed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../glimpse_amd/csrc/glh_velocity.h"
#include "../../glimpse_amd/csrc/glh_velocity_plan.h"

using namespace glh;

static long failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      if (failures < 20) std::printf("FAILED line %d: %s (pairs %d)\n", __LINE__, #cond, pairs); \
      ++failures;                                                                     \
    }                                                                                 \
  } while (0)

// The kernel's compare-exchange steps (glh_velocity.hip: vf_bitonic) over `nlists` lists in `region`; `touch` sees every
// byte range read and written.
template <typename Touch>
static void bitonic(double* lists, int nlists, int log_len, int pitch, Touch touch) {
  const int len = 1 << log_len, total = nlists * (len >> 1);
  for (int k = 2; k <= len; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
      for (int t = 0; t < total; ++t) {
        const int list = t >> (log_len - 1), q = t & ((len >> 1) - 1);
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
        double* b = lists + (size_t)list * pitch;
        touch(b + i), touch(b + l);
        const double x = b[i], y = b[l];
        const double lo = std::min(x, y), hi = std::max(x, y);
        const bool up = (i & k) == 0;
        b[i] = up ? lo : hi, b[l] = up ? hi : lo;
      }
}

static size_t largest = 0;
static int largest_pairs = 0;

static void check(int pairs) {
  const VfPlan plan = vf_plan(pairs);
  const VfLayout l = vf_layout(plan.len, plan.nodes);
  EXPECT(plan.len == 1 << plan.log_len && plan.len >= pairs && (plan.len == 1 || plan.len / 2 < pairs));
  EXPECT(plan.nodes == 1 << plan.log_nodes && plan.nodes >= 1 && plan.nodes <= VF_MAX_RUN);
  EXPECT(plan.nodes == VF_MAX_RUN || (size_t)vf_layout(plan.len, 2 * plan.nodes).total > VF_LDS_LIMIT);
  EXPECT(plan.lds == (size_t)l.total && plan.lds <= VF_LDS_LIMIT);
  EXPECT(l.pitch >= plan.len && l.fpitch >= plan.len);
  EXPECT(l.lists % 16 == 0 && l.flags % 16 == 0 && l.counts % 16 == 0 && l.meds % 16 == 0 && l.total % 16 == 0);
  EXPECT(l.lists == 0);
  EXPECT(l.lists + 8 * 2 * plan.nodes * l.pitch <= l.flags);  // 2 nodes lists of pitch doubles
  EXPECT(l.flags + plan.nodes * l.fpitch <= l.counts);        // nodes rows of fpitch bytes
  EXPECT(l.counts + 4 * plan.nodes <= l.meds);                // one int per node
  EXPECT(l.meds + 8 * 2 * plan.nodes <= l.total);             // one double per list
  // the run's segment of a pair's row: 16 bytes a node, and whole 128-byte lines from 8 nodes on
  EXPECT(plan.nodes < 8 || (16 * plan.nodes) % 128 == 0);
  if (plan.lds > largest) largest = plan.lds, largest_pairs = pairs;

  // the region itself, exactly plan.lds bytes on the heap: every index expression of k_vf_stack, each within its part
  std::vector<char> region(plan.lds);
  char* base = region.data();
  double* lists = reinterpret_cast<double*>(base + l.lists);
  uint8_t* flags = reinterpret_cast<uint8_t*>(base + l.flags);
  int* counts = reinterpret_cast<int*>(base + l.counts);
  double* meds = reinterpret_cast<double*>(base + l.meds);
  const int len = plan.len, nodes = plan.nodes, nlists = 2 * nodes;
  auto in_lists = [&](const double* p) {
    const char* c = reinterpret_cast<const char*>(p);
    if (!(c >= base + l.lists && c + 8 <= base + l.flags)) {
      if (failures < 20) std::printf("FAILED: a list element outside its part (pairs %d)\n", pairs);
      ++failures;
    }
  };
  // the fill: values that sort -- descending over the pairs, +inf beyond them
  for (int idx = 0; idx < len * nodes; ++idx) {
    const int p = idx >> plan.log_nodes, g = idx & (nodes - 1);
    const double x = p < pairs ? (double)((p * 7919 + g) % 1013) : std::numeric_limits<double>::infinity();
    in_lists(&lists[g * l.pitch + p]), in_lists(&lists[(nodes + g) * l.pitch + p]);
    lists[g * l.pitch + p] = x, lists[(nodes + g) * l.pitch + p] = -x;
    EXPECT(l.flags + g * l.fpitch + p < l.counts);
    flags[g * l.fpitch + p] = p < pairs;
  }
  for (int g = 0; g < nodes; ++g) {
    int c = 0;
    for (int p = 0; p < len; ++p) c += flags[g * l.fpitch + p];
    EXPECT(c == pairs);
    counts[g] = c;
  }
  bitonic(lists, nlists, plan.log_len, l.pitch, in_lists);
  for (int t = 0; t < nlists; ++t) {
    const double* b = lists + (size_t)t * l.pitch;
    EXPECT(std::is_sorted(b, b + len));
    meds[t] = b[counts[t & (nodes - 1)] >> 1];
  }
}

int main() {
  int pairs = 0;
  for (pairs = 1; pairs <= VF_MAX_PAIRS; ++pairs) check(pairs);
  for (int p : {1, 2, 3, 64, 128, 129, 256, 257, 512, 513, 1024}) {
    const VfPlan plan = vf_plan(p);
    std::printf("pairs %d: len %d, nodes %d, %zu bytes\n", p, plan.len, plan.nodes, plan.lds);
  }
  pairs = 0;
  EXPECT(vf_plan(256).nodes == 32 && vf_plan(257).nodes == 16 && vf_plan(512).nodes == 16 && vf_plan(513).nodes == 8);
  EXPECT(vf_plan(1024).nodes == 8 && vf_plan(1).len == 1 && vf_plan(1).nodes == VF_MAX_RUN);
  EXPECT(VF_LDS_LIMIT == 163840 && VF_MAX_PAIRS == 1024 && VF_MAX_NODES >= (1 << 24));
  std::printf("largest %zu bytes at %d pairs\n", largest, largest_pairs);
  if (failures) {
    std::printf("%ld failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
