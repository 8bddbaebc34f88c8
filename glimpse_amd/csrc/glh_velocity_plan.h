// glh_velocity_plan.h -- the LDS plan of the velocity field's stack kernel (glh_velocity.hip: k_vf_stack): how long a
// list is, how many adjacent nodes a workgroup takes, and where the parts of its one dynamic region lie.  The kernel
// reads the layout, the launch (velocity_field_run) asks vf_plan for the sizes.  Plain C++ without a HIP header, so that
// tests/hostcheck/velocity_plan_hostcheck.cpp compiles the very same code for the CPU and checks it for every number of
// pairs the ABI accepts.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define GLH_VF_HD __host__ __device__ inline
#else
#define GLH_VF_HD inline
#endif

namespace glh {

constexpr int VF_TB = 256;
constexpr size_t VF_LDS_LIMIT = 160 * 1024;  // 163 840 bytes: what the project allows itself of a CU's LDS
constexpr int VF_MAX_PAIRS = 1024;
constexpr int VF_MAX_RUN = 32;  // nodes of one workgroup at most

// A workgroup stacks a run of `nodes` adjacent nodes.  Each (component, node) has a list of `len` doubles, len the next
// power of two from the number of pairs, which the bitonic network sorts; list k * nodes + g (component k, node g)
// starts `pitch` doubles after the one before.  pitch = len + 1: the threads that fill the lists own consecutive nodes
// of one pair, so their 8-byte stores lie pitch doubles apart, 2 len + 2 dwords, which for len >= 16 is 2 modulo the 32
// banks of such a store -- sixteen lanes, sixteen bank pairs.  `flags` holds one byte per pair and node (kept or not),
// its rows fpitch = len + 4 bytes apart for the same reason; `counts` one int per node; `meds` one double per list.
struct VfLayout {
  int pitch, fpitch;                       // of a list (doubles) and of a row of flags (bytes)
  int lists, flags, counts, meds, total;  // byte offsets into the region, and its size
};

GLH_VF_HD int vf_up16(int v) { return (v + 15) & ~15; }

GLH_VF_HD VfLayout vf_layout(int len, int nodes) {
  VfLayout l;
  l.pitch = len + 1, l.fpitch = len + 4;
  l.lists = 0;
  l.flags = l.lists + vf_up16(8 * 2 * nodes * l.pitch);
  l.counts = l.flags + vf_up16(nodes * l.fpitch);
  l.meds = l.counts + vf_up16(4 * nodes);
  l.total = l.meds + vf_up16(8 * 2 * nodes);
  return l;
}

// log2 of the list's length: the smallest power of two that holds `pairs` values.
inline int vf_log_len(int pairs) {
  int b = 0;
  while ((1 << b) < pairs) ++b;
  return b;
}

struct VfPlan {
  int log_len, len;  // of a list
  int log_nodes, nodes;  // of a workgroup's run, a power of two so that a run's segment of a pair's row starts aligned
  size_t lds;        // bytes of the region
};

// What the launch uses for `pairs` pairs: the longest run of nodes, a power of two up to VF_MAX_RUN, whose region stays
// within VF_LDS_LIMIT.  tests/hostcheck/velocity_plan_hostcheck.cpp forms the plan of every pairs in 1 .. VF_MAX_PAIRS:
// 32 nodes up to 256 pairs (140 544 bytes at 129 .. 256), 16 up to 512 (139 904 bytes), 8 up to 1024 (139 584 bytes).
inline VfPlan vf_plan(int pairs) {
  VfPlan p;
  p.log_len = vf_log_len(pairs), p.len = 1 << p.log_len;
  p.log_nodes = 5;
  while (p.log_nodes > 0 && (size_t)vf_layout(p.len, 1 << p.log_nodes).total > VF_LDS_LIMIT) --p.log_nodes;
  p.nodes = 1 << p.log_nodes;
  p.lds = (size_t)vf_layout(p.len, p.nodes).total;
  return p;
}

}  // namespace glh
