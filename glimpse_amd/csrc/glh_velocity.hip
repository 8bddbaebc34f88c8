// glh_velocity.hip -- from displacements to a velocity field on the device: the work behind glh_stage_velocity_field
// (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls velocity_field_run).  The vectors of every
// image pair are tested against their neighbours on the grid (the normalised median test of Westerweel & Scarano, 2005),
// and what survives is stacked over the pairs into a median velocity, a robust spread (1.4826 x the median absolute
// deviation) and a count per node.  The reference has no such function, so the rule is the contract: INPUTS.md,
// "Velocity field: the rule", restated in NumPy in tests/velocity_field_rule.py, which both kernels equal bit for bit.
// Every operation is an IEEE float64 operation and no multiply feeds an add; every value has + 0.0 applied before it
// enters a sort, so that no -0.0 does and equal keys are equal in every bit, whatever order a network meets them in.
//
//   k_vf_test<R>  one thread per (pair, node), a workgroup per tile of VF_TW x VF_TH nodes, blockIdx.y the pair.  The
//                 tile and its halo of R nodes are staged in LDS once, as two planes of doubles (the components), with
//                 +inf where a node is no candidate or lies beyond the grid: status, score and duv of a node are read
//                 once a tile instead of up to 25 times.  A thread gathers the 8 or 24 neighbours of one component into
//                 registers, sorts them with the fixed network of glh_sort_networks.h (+inf sorts last, so the m
//                 neighbours that exist come first), picks s[m / 2 - 1] and s[m / 2] by a chain of selects on m, forms
//                 the deviations from the median (+inf stays +inf), sorts again and tests.  Consecutive lanes read
//                 consecutive doubles of a plane's row: no bank conflict in a group of 32 lanes; the second half of a
//                 wave is one row on, (VF_TW + 2 R) doubles = 4 or 8 banks modulo 64.  R = 0: kept = candidate, no LDS.
//   k_vf_stack    a workgroup takes a run of adjacent nodes (glh_velocity_plan.h: 8 .. 32, by the number of pairs), so
//                 that the threads that fill the lists read 16 x run contiguous bytes of every pair's row.  A slot p
//                 of list (component, node) gets the pair's velocity, or +inf when the pair is not kept or p is past
//                 the last pair: the sort itself compacts, the kept values come first.  All lists are sorted at once
//                 by a bitonic network over the next power of two, one compare-exchange per thread and step, a barrier
//                 between the steps.  A step of distance j reads runs of j consecutive doubles, 2 j apart: whole
//                 conflict-free groups from j = 32 on, two-way conflicts below (5 of log2(len) steps of the last
//                 merges).  Then the median, the list rewritten as deviations, the same sort, and v, sigma, count.  The
//                 count of a node comes from the flags of its pairs, summed by one wave in a fixed order.
//
// No atomics, no order that depends on timing.  Every global read and write is bounded by the grid (k_vf_test: r < rows,
// c < cols for the halo and the node) or by n and the number of pairs (k_vf_stack); every LDS index by the layout of
// glh_velocity_plan.h, checked on the CPU by tests/hostcheck/velocity_plan_hostcheck.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/glimpse_hip.h"
#include "glh_sort_networks.h"
#include "glh_stage.h"
#include "glh_velocity.h"
#include "glh_velocity_plan.h"

namespace glh {
namespace {

constexpr int VF_TW = 32, VF_TH = 8;  // a tile of the neighbour test: VF_TW * VF_TH == VF_TB
static_assert(VF_TW * VF_TH == VF_TB, "one thread per node of a tile");

struct VfArgs {
  const double* duv;
  const double* score;
  const uint8_t* status;
  int n_pairs, rows, cols, n;
  const double* dt;
  double scale[2];
  double min_score;
  int max_status, min_neighbors;
  double threshold, epsilon;
  int min_count;
  int log_len, log_nodes;  // of the stack's plan
  double* v;
  double* sigma;
  int32_t* count;
  uint8_t* kept;
};

__device__ __forceinline__ double vf_inf() { return __longlong_as_double(0x7ff0000000000000LL); }
__device__ __forceinline__ double vf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// ---- the neighbour test ----------------------------------------------------------------------------------------------------

// Is the vector of pair-and-node `at` a candidate?
__device__ __forceinline__ bool vf_candidate(const VfArgs& a, size_t at, double& x, double& y) {
  x = a.duv[2 * at], y = a.duv[2 * at + 1];
  return (int)a.status[at] <= a.max_status && a.score[at] >= a.min_score && isfinite(x) && isfinite(y);
}

#define GLH_VF_CE(i, j)                  \
  {                                      \
    const double lo_ = fmin(s[i], s[j]); \
    const double hi_ = fmax(s[i], s[j]); \
    s[i] = lo_;                          \
    s[j] = hi_;                          \
  }
template <int N>
__device__ __forceinline__ void vf_sort(double (&s)[N]) {
  static_assert(N == 8 || N == 24, "the networks of glh_sort_networks.h");
  if constexpr (N == 8) {
    GLH_SORT8_NETWORK(GLH_VF_CE)
  } else {
    GLH_SORT24_NETWORK(GLH_VF_CE)
  }
}
#undef GLH_VF_CE

// s[idx] by selects with compile-time indices (idx outside 0 .. N / 2: s[0]).  The empty asm after each select keeps the
// compiler from seeing the chain as s[idx], which it would serve from a copy of s in scratch.
template <int N>
__device__ __forceinline__ double vf_pick(const double (&s)[N], int idx) {
  double v = s[0];
#pragma unroll
  for (int k = 1; k <= N / 2; ++k) {  // (idx is at most m / 2 <= N / 2)
    v = idx == k ? s[k] : v;
    asm("" : "+v"(v));
  }
  return v;
}

// The median of the first m of the sorted s.
template <int N>
__device__ __forceinline__ double vf_median(const double (&s)[N], int m) {
  const double hi = vf_pick(s, m >> 1), lo = vf_pick(s, (m >> 1) - 1);
  return (m & 1) ? hi : (lo + hi) / 2.0;
}

// One component of the test: s the neighbours' values (+inf where there is none), m their number, x the node's own.
template <int N>
__device__ __forceinline__ bool vf_passes(double (&s)[N], int m, double x, double threshold, double epsilon) {
  vf_sort(s);
  const double med = vf_median(s, m);
#pragma unroll
  for (int q = 0; q < N; ++q) s[q] = fabs(s[q] - med) + 0.0;
  vf_sort(s);
  const double res = vf_median(s, m);
  return __ddiv_rn(fabs(x - med), res + epsilon) <= threshold;
}

template <int R>
__global__ __launch_bounds__(VF_TB) void k_vf_test(const VfArgs a) {
  constexpr int HW = VF_TW + 2 * R, HH = VF_TH + 2 * R, N = (2 * R + 1) * (2 * R + 1) - 1;
  const int tiles_x = (a.cols + VF_TW - 1) / VF_TW;
  const int tile_y = (int)blockIdx.x / tiles_x, tile_x = (int)blockIdx.x - tile_y * tiles_x;
  const int r0 = tile_y * VF_TH, c0 = tile_x * VF_TW;
  const size_t base = (size_t)blockIdx.y * a.n;
  const int tx = (int)threadIdx.x % VF_TW, ty = (int)threadIdx.x / VF_TW;
  const int r = r0 + ty, c = c0 + tx;
  if constexpr (R == 0) {
    if (r >= a.rows || c >= a.cols) return;
    const size_t at = base + (size_t)r * a.cols + c;
    double x, y;
    a.kept[at] = vf_candidate(a, at, x, y) ? 1 : 0;
  } else {
    __shared__ double plane[2][HH * HW];
    for (int idx = (int)threadIdx.x; idx < HH * HW; idx += VF_TB) {
      const int hr = idx / HW, hc = idx - hr * HW;
      const int gr = r0 - R + hr, gc = c0 - R + hc;
      double x = vf_inf(), y = vf_inf();
      if (gr >= 0 && gr < a.rows && gc >= 0 && gc < a.cols) {
        double vx, vy;
        if (vf_candidate(a, base + (size_t)gr * a.cols + gc, vx, vy)) x = vx + 0.0, y = vy + 0.0;
      }
      plane[0][idx] = x, plane[1][idx] = y;
    }
    __syncthreads();
    if (r >= a.rows || c >= a.cols) return;
    const int centre = (ty + R) * HW + tx + R;
    bool keep = plane[0][centre] < vf_inf();  // (a candidate's components are finite)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double s[N];
      int m = 0;
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int cell = q < N / 2 ? q : q + 1;  // (the window's cells in row-major order without the centre)
        const int dy = cell / (2 * R + 1) - R, dx = cell % (2 * R + 1) - R;
        s[q] = plane[k][centre + dy * HW + dx];
        m += s[q] < vf_inf() ? 1 : 0;
      }
      // (m is the same for both components; with m == 0 the medians are formed from +inf and not used)
      const bool ok = vf_passes(s, m, plane[k][centre], a.threshold, a.epsilon);
      keep = keep && m >= a.min_neighbors && ok;
    }
    a.kept[base + (size_t)r * a.cols + c] = keep ? 1 : 0;
  }
}

// ---- the stack ---------------------------------------------------------------------------------------------------------------

// Sorts `nlists` lists of 1 << log_len doubles, `pitch` apart, ascending: the bitonic network, every list at once, one
// compare-exchange per thread and step.  Ends on a barrier.
__device__ void vf_bitonic(double* lists, int nlists, int log_len, int pitch) {
  const int len = 1 << log_len, total = nlists * (len >> 1);
  for (int k = 2; k <= len; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = (int)threadIdx.x; t < total; t += VF_TB) {
        const int list = t >> (log_len - 1), q = t & ((len >> 1) - 1);
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
        double* b = lists + list * pitch;
        const double x = b[i], y = b[l];
        const double lo = fmin(x, y), hi = fmax(x, y);
        const bool up = (i & k) == 0;
        b[i] = up ? lo : hi, b[l] = up ? hi : lo;
      }
      __syncthreads();
    }
}

// The median of the first c (>= 1) of a sorted list.
__device__ __forceinline__ double vf_list_median(const double* b, int c) {
  return (c & 1) ? b[c >> 1] : (b[(c >> 1) - 1] + b[c >> 1]) / 2.0;
}

__global__ __launch_bounds__(VF_TB) void k_vf_stack(const VfArgs a) {
  extern __shared__ __attribute__((aligned(16))) char vf_lds[];
  const int len = 1 << a.log_len, nodes = 1 << a.log_nodes, nlists = 2 * nodes;
  const VfLayout lay = vf_layout(len, nodes);
  double* lists = reinterpret_cast<double*>(vf_lds + lay.lists);
  uint8_t* flags = reinterpret_cast<uint8_t*>(vf_lds + lay.flags);
  int* counts = reinterpret_cast<int*>(vf_lds + lay.counts);
  double* meds = reinterpret_cast<double*>(vf_lds + lay.meds);
  const int i0 = (int)blockIdx.x << a.log_nodes;  // (n <= 2^24: no overflow)
  const int here = min(nodes, a.n - i0);
  // the lists: slot p of list (k, g) is pair p's velocity at node i0 + g, +inf where it is not kept or there is no pair
  for (int idx = (int)threadIdx.x; idx < len * nodes; idx += VF_TB) {
    const int p = idx >> a.log_nodes, g = idx & (nodes - 1);
    double x = vf_inf(), y = vf_inf();
    uint8_t f = 0;
    if (p < a.n_pairs && g < here) {
      const size_t at = (size_t)p * a.n + i0 + g;
      f = a.kept[at] != 0;
      if (f) {
        const double dt = a.dt[p];
        x = __ddiv_rn(a.duv[2 * at] * a.scale[0], dt) + 0.0;
        y = __ddiv_rn(a.duv[2 * at + 1] * a.scale[1], dt) + 0.0;
      }
    }
    lists[g * lay.pitch + p] = x;
    lists[(nodes + g) * lay.pitch + p] = y;
    flags[g * lay.fpitch + p] = f;
  }
  __syncthreads();
  // the counts: a wave per node, lanes over the pairs, then the wave's sum
  for (int g = (int)threadIdx.x >> 6; g < nodes; g += VF_TB / 64) {
    int c = 0;
    for (int p = (int)threadIdx.x & 63; p < len; p += 64) c += flags[g * lay.fpitch + p];
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) counts[g] = c;
  }
  vf_bitonic(lists, nlists, a.log_len, lay.pitch);  // (its barrier also publishes the counts; len == 1: none, see below)
  if (len == 1) __syncthreads();
  if ((int)threadIdx.x < nlists) {
    const int c = counts[threadIdx.x & (nodes - 1)];
    meds[threadIdx.x] = c >= a.min_count ? vf_list_median(lists + threadIdx.x * lay.pitch, c) : vf_nan();
  }
  __syncthreads();
  for (int idx = (int)threadIdx.x; idx < nlists * len; idx += VF_TB) {
    const int list = idx >> a.log_len, q = idx & (len - 1);
    if (q < counts[list & (nodes - 1)]) {
      double* b = lists + list * lay.pitch;
      b[q] = fabs(b[q] - meds[list]) + 0.0;
    }
  }
  __syncthreads();
  vf_bitonic(lists, nlists, a.log_len, lay.pitch);
  if ((int)threadIdx.x < nlists) {
    const int k = (int)threadIdx.x >> a.log_nodes, g = (int)threadIdx.x & (nodes - 1);
    if (g < here) {
      const int c = counts[g];
      const bool ok = c >= a.min_count;
      const size_t out = 2 * (size_t)(i0 + g) + k;
      a.v[out] = meds[threadIdx.x];
      a.sigma[out] = ok ? 1.4826 * vf_list_median(lists + threadIdx.x * lay.pitch, c) : vf_nan();
      if (k == 0) a.count[i0 + g] = c;
    }
  }
}

}  // namespace

int velocity_field_run(const VelocityJob& j) {
  const size_t n = (size_t)j.rows * j.cols, np = (size_t)j.n_pairs;
  const VfPlan plan = vf_plan(j.n_pairs);
  if (plan.lds > VF_LDS_LIMIT) return fail(GLH_E_UNSUPPORTED, "velocity_field: %zu bytes of LDS for one node", plan.lds);
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<VF_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dduv, dscore, dstatus, ddt, dkept, dv, dsigma, dcount;
  CHK(dduv.alloc(np * n * 16));
  CHK(dscore.alloc(np * n * 8));
  CHK(dstatus.alloc(np * n));
  CHK(ddt.alloc(np * 8));
  CHK(dkept.alloc(np * n));
  CHK(dv.alloc(n * 16));
  CHK(dsigma.alloc(n * 16));
  CHK(dcount.alloc(n * 4));
  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dduv.p, j.duv, np * n * 16, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dscore.p, j.score, np * n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dstatus.p, j.status, np * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ddt.p, j.dt, np * 8, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  VfArgs a{};
  a.duv = dduv.as<double>(), a.score = dscore.as<double>(), a.status = dstatus.as<uint8_t>();
  a.n_pairs = j.n_pairs, a.rows = j.rows, a.cols = j.cols, a.n = (int)n;
  a.dt = ddt.as<double>(), a.scale[0] = j.scale[0], a.scale[1] = j.scale[1];
  a.min_score = j.min_score, a.max_status = j.max_status, a.min_neighbors = j.min_neighbors;
  a.threshold = j.threshold, a.epsilon = j.epsilon, a.min_count = j.min_count;
  a.log_len = plan.log_len, a.log_nodes = plan.log_nodes;
  a.v = dv.as<double>(), a.sigma = dsigma.as<double>(), a.count = dcount.as<int32_t>(), a.kept = dkept.as<uint8_t>();
  const unsigned tiles = (unsigned)((j.cols + VF_TW - 1) / VF_TW) * (unsigned)((j.rows + VF_TH - 1) / VF_TH);
  const dim3 grid(tiles, (unsigned)j.n_pairs);
  if (j.radius == 0)
    hipLaunchKernelGGL(k_vf_test<0>, grid, dim3(VF_TB), 0, s, a);
  else if (j.radius == 1)
    hipLaunchKernelGGL(k_vf_test<1>, grid, dim3(VF_TB), 0, s, a);
  else
    hipLaunchKernelGGL(k_vf_test<2>, grid, dim3(VF_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  if (plan.lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute((const void*)k_vf_stack, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
  hipLaunchKernelGGL(k_vf_stack, dim3((unsigned)((n + plan.nodes - 1) / plan.nodes)), dim3(VF_TB), plan.lds, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  CHK(dv.down(j.v, n * 16));
  CHK(dsigma.down(j.sigma, n * 16));
  CHK(dcount.down(j.count, n * 4));
  CHK(dkept.down(j.kept, np * n));
  CHK(ev.record(4, s));
  HIPCHK(hipEventSynchronize(ev.e[4]));
  ev.report(j.times_ms, VF_TIMES, VF_TIMES);
  return GLH_OK;
}

}  // namespace glh
