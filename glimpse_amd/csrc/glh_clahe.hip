// glh_clahe.hip -- optimize.CLAHE on the device: contrast-limited adaptive histogram equalisation of an 8-bit image, the
// work behind glh_stage_clahe (include/glimpse_hip.h; glimpse_hip.hip validates the arguments and calls clahe_run).
//
// The rule is INPUTS.md's "CLAHE: the rule" (OpenCV's clahe.cpp for 8-bit input, written out); tests/clahe_restated.py
// restates it in NumPy and the results equal it in every bit.  The histograms are integers, so their sums do not depend
// on the order of the pixels; every pixel's blend is one float32 expression whose products and sums are each rounded on
// their own (the explicit round-to-nearest intrinsics: no contraction), with the two quotients it needs (1 / tw, 1 / th,
// 255 / area) made on the host.
//
// Kernels:
//   k_clahe_hist   a workgroup per (tile, slice of the tile's rows): the slices keep every CU busy when the grid has few
//                  tiles.  A thread walks the slice's cells, reads the source at the reflected coordinates (closed form; no
//                  padded copy), forms the channel mean -- and writes it to the gray plane where the cell is the image's own
//                  and not a reflection, so every gray cell is written once -- and counts into its wave's 256-bin table in
//                  LDS.  The four tables are added up and go to the tile's global histogram with one atomicAdd per bin
//                  that is not empty.
//   k_clahe_lut    a workgroup of 256 threads per tile, a bin per thread: clips, sums the excess over the workgroup, hands
//                  it back by the closed form of the rule's residual loop, scans, scales and rounds.
//   k_clahe_apply  a thread per four pixels of a row (one 32-bit load and store where the width is a multiple of four,
//                  bytes otherwise): the row's and each column's two tiles and weights in registers, four table reads per
//                  pixel (the tables are 256 bytes a tile and stay in the caches).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glimpse_hip.h"
#include "glh_clahe.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int CL_TB = 256;
constexpr int CL_WAVES = CL_TB / 64;
constexpr int CL_TARGET_BLOCKS = 1024;  // of k_clahe_hist: four workgroups for each of the 256 CUs
constexpr int CL_MAX_SLICES = 65535;    // gridDim.y

struct ClaheArgs {
  const uint8_t* src;  // [h][w][C]
  uint8_t* gray;       // [h][w]: written by k_clahe_hist when C > 1; with one channel it is src itself
  uint32_t* hist;      // [tiles][256], zero before k_clahe_hist
  uint8_t* luts;       // [tiles][256]
  uint8_t* dst;        // [h][w]
  int w, h;
  int tiles_x, tiles_y;
  int tw, th;
  int slice_rows;  // rows of a tile that one workgroup of k_clahe_hist counts
  uint32_t lim;    // 0: no clipping
  float scale;     // float32(255) / float32(area)
  float inv_tw, inv_th;
};

// Step 1: index i >= 0 of an axis of n cells extended by reflection without the edge cell.  At most n cells are added
// (tiles <= n), so beyond the axis 2 (n - 1) - i is at least -1; -1 reflects once more, to 1, and an axis of one cell
// repeats it (BORDER_REFLECT_101 and np.pad's "reflect" agree on both).
__device__ __forceinline__ int cl_reflect(int i, int n) {
  if (i < n) return i;
  if (n == 1) return 0;
  const long long r = 2LL * (n - 1) - i;  // (n may be above 2^30)
  return (int)(r < 0 ? -r : r);
}

template <int C>
__global__ void __launch_bounds__(CL_TB) k_clahe_hist(ClaheArgs p) {
  __shared__ uint32_t sub[CL_WAVES][CL_BINS];
  const int tid = threadIdx.x;
  for (int k = tid; k < CL_WAVES * CL_BINS; k += CL_TB) (&sub[0][0])[k] = 0u;
  __syncthreads();
  const int tile = blockIdx.x;
  const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
  const int r0 = blockIdx.y * p.slice_rows;
  const int r1 = min(r0 + p.slice_rows, p.th);
  const int n = (r1 - r0) * p.tw;  // (at most a tile's area, below 2^31)
  uint32_t* mine = sub[tid >> 6];
  // cell k of the slice is row k / tw, column k % tw; the next one of this thread is CL_TB further on
  const int dr = CL_TB / p.tw, dc = CL_TB - dr * p.tw;
  int r = tid / p.tw, c = tid - r * p.tw;
  for (int k = tid; k < n; k += CL_TB) {
    const int ey = ty * p.th + r0 + r, ex = tx * p.tw + c;
    const size_t g = (size_t)cl_reflect(ey, p.h) * p.w + cl_reflect(ex, p.w);
    uint32_t v;
    if (C == 1) {
      v = p.src[g];
    } else {
      const uint8_t* s = p.src + g * C;
      uint32_t sum = s[0];
#pragma unroll
      for (int q = 1; q < C; ++q) sum += s[q];
      v = sum / C;
      if (ey < p.h && ex < p.w) p.gray[g] = (uint8_t)v;
    }
    atomicAdd(&mine[v], 1u);
    r += dr, c += dc;
    if (c >= p.tw) c -= p.tw, ++r;
  }
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int q = 0; q < CL_WAVES; ++q) total += sub[q][tid];
  if (total) atomicAdd(&p.hist[(size_t)tile * CL_BINS + tid], total);
}

__global__ void __launch_bounds__(CL_TB) k_clahe_lut(ClaheArgs p) {
  __shared__ uint32_t part[CL_WAVES];
  __shared__ uint32_t scan[2][CL_BINS];
  const int t = threadIdx.x;
  const size_t tile = blockIdx.x;
  uint32_t hv = p.hist[tile * CL_BINS + t];
  if (p.lim > 0) {
    // step 3: what lies above the limit, summed over the 256 bins
    uint32_t excess = hv > p.lim ? hv - p.lim : 0u;
    for (int off = 32; off > 0; off >>= 1) excess += __shfl_down(excess, off, 64);
    if ((t & 63) == 0) part[t >> 6] = excess;
    __syncthreads();
    uint32_t clipped = 0;
#pragma unroll
    for (int q = 0; q < CL_WAVES; ++q) clipped += part[q];
    const uint32_t batch = clipped / CL_BINS, residual = clipped % CL_BINS;
    hv = min(hv, p.lim) + batch;
    if (residual != 0) {
      const uint32_t step = max((uint32_t)CL_BINS / residual, 1u);
      const uint32_t q = (uint32_t)t / step;
      if ((uint32_t)t - q * step == 0 && q < residual) ++hv;
    }
  }
  // step 4: the inclusive sum of the bins up to this one (integers: any order gives the same)
  int cur = 0;
  scan[0][t] = hv;
  __syncthreads();
  for (int off = 1; off < CL_BINS; off <<= 1) {
    const uint32_t s = scan[cur][t] + (t >= off ? scan[cur][t - off] : 0u);
    scan[cur ^ 1][t] = s;
    cur ^= 1;
    __syncthreads();
  }
  const float f = rintf(__fmul_rn((float)scan[cur][t], p.scale));
  p.luts[tile * CL_BINS + t] = (uint8_t)fminf(fmaxf(f, 0.f), 255.f);
}

// Step 5 along one axis: cell i of the source, tiles of 1 / inv cells, `tiles` of them.
struct ClAxis {
  int i1, i2;
  float a, a1;
};

__device__ __forceinline__ ClAxis cl_axis(int i, float inv, int tiles) {
  ClAxis o;
  const float f = __fsub_rn(__fmul_rn((float)i, inv), 0.5f);
  const float fl = floorf(f);
  o.a = __fsub_rn(f, fl);  // (before clamping)
  o.a1 = __fsub_rn(1.f, o.a);
  const int i1 = (int)fl;
  o.i2 = min(i1 + 1, tiles - 1);
  // (the upper bound changes nothing the rule computes: i1 <= tiles - 1 wherever float32 holds the cell index exactly; it
  // keeps the table reads in bounds beyond that)
  o.i1 = min(max(i1, 0), tiles - 1);
  return o;
}

__device__ __forceinline__ uint32_t cl_pixel(const uint8_t* __restrict__ top, const uint8_t* __restrict__ bottom,
                                             const ClAxis& ax, const ClAxis& ay, uint32_t v) {
  const size_t o1 = (size_t)ax.i1 * CL_BINS + v, o2 = (size_t)ax.i2 * CL_BINS + v;
  const float a = __fadd_rn(__fmul_rn((float)top[o1], ax.a1), __fmul_rn((float)top[o2], ax.a));
  const float b = __fadd_rn(__fmul_rn((float)bottom[o1], ax.a1), __fmul_rn((float)bottom[o2], ax.a));
  const float res = __fadd_rn(__fmul_rn(a, ay.a1), __fmul_rn(b, ay.a));
  return (uint32_t)fminf(fmaxf(rintf(res), 0.f), 255.f);
}

// VEC: the width is a multiple of four (and the planes come from hipMalloc), so a thread's four pixels are one aligned word.
template <bool VEC>
__global__ void __launch_bounds__(CL_TB) k_clahe_apply(ClaheArgs p) {
  const int quads = (p.w + 3) >> 2;  // a row's
  const size_t i = (size_t)blockIdx.x * CL_TB + threadIdx.x;
  if (i >= (size_t)p.h * quads) return;
  const int y = (int)(i / quads), x0 = (int)(i - (size_t)y * quads) * 4;
  const ClAxis ay = cl_axis(y, p.inv_th, p.tiles_y);
  const uint8_t* top = p.luts + (size_t)ay.i1 * p.tiles_x * CL_BINS;
  const uint8_t* bottom = p.luts + (size_t)ay.i2 * p.tiles_x * CL_BINS;
  const size_t g = (size_t)y * p.w + x0;
  if (VEC) {
    const uint32_t in = *reinterpret_cast<const uint32_t*>(p.gray + g);
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      out |= cl_pixel(top, bottom, cl_axis(x0 + j, p.inv_tw, p.tiles_x), ay, (in >> (8 * j)) & 255u) << (8 * j);
    *reinterpret_cast<uint32_t*>(p.dst + g) = out;
  } else {
    for (int j = 0; j < 4 && x0 + j < p.w; ++j)
      p.dst[g + j] = (uint8_t)cl_pixel(top, bottom, cl_axis(x0 + j, p.inv_tw, p.tiles_x), ay, p.gray[g + j]);
  }
}

}  // namespace

int clahe_run(const ClaheJob& j) {
  const size_t n = (size_t)j.w * j.h;
  const size_t tiles = (size_t)j.tiles_x * j.tiles_y;  // (at most n, below 2^31)
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<CL_TIMES + 1> ev;
  CHK(ev.create());
  DevBuf dsrc, dgray, dhist, dlut, ddst;
  CHK(dsrc.alloc(n * j.channels));
  if (j.channels > 1) CHK(dgray.alloc(n));
  CHK(dhist.alloc(tiles * CL_BINS * sizeof(uint32_t)));
  CHK(dlut.alloc(tiles * CL_BINS));
  CHK(ddst.alloc(n));

  ClaheArgs a{};
  a.src = dsrc.as<const uint8_t>();
  a.gray = j.channels > 1 ? dgray.as<uint8_t>() : dsrc.as<uint8_t>();  // (one channel: read, never written)
  a.hist = dhist.as<uint32_t>();
  a.luts = dlut.as<uint8_t>();
  a.dst = ddst.as<uint8_t>();
  a.w = j.w, a.h = j.h;
  a.tiles_x = j.tiles_x, a.tiles_y = j.tiles_y;
  a.tw = (int)j.geo.tw, a.th = (int)j.geo.th;
  a.lim = (uint32_t)j.geo.lim;
  a.scale = 255.0f / (float)j.geo.area;
  a.inv_tw = 1.0f / (float)a.tw;
  a.inv_th = 1.0f / (float)a.th;
  // the slices of a tile: enough workgroups for the device, at least one row each, and no more than a grid holds
  size_t slices = (CL_TARGET_BLOCKS + tiles - 1) / tiles;
  if (slices > (size_t)a.th) slices = (size_t)a.th;
  if (slices > (size_t)CL_MAX_SLICES) slices = CL_MAX_SLICES;
  a.slice_rows = (int)((a.th + slices - 1) / slices);
  slices = (size_t)(a.th + a.slice_rows - 1) / a.slice_rows;  // (none of them empty)

  CHK(ev.record(0, s));
  HIPCHK(hipMemcpy(dsrc.p, j.src, n * j.channels, hipMemcpyHostToDevice));
  CHK(ev.record(1, s));
  HIPCHK(hipMemsetAsync(dhist.p, 0, tiles * CL_BINS * sizeof(uint32_t), s));
  const dim3 hgrid((unsigned)tiles, (unsigned)slices);
  switch (j.channels) {
    case 1: hipLaunchKernelGGL(k_clahe_hist<1>, hgrid, dim3(CL_TB), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_clahe_hist<2>, hgrid, dim3(CL_TB), 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_clahe_hist<3>, hgrid, dim3(CL_TB), 0, s, a); break;
    default: hipLaunchKernelGGL(k_clahe_hist<4>, hgrid, dim3(CL_TB), 0, s, a); break;
  }
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  hipLaunchKernelGGL(k_clahe_lut, dim3((unsigned)tiles), dim3(CL_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  const size_t threads = (size_t)j.h * ((j.w + 3) / 4);
  const dim3 agrid((unsigned)((threads + CL_TB - 1) / CL_TB));
  if (j.w % 4 == 0)
    hipLaunchKernelGGL(k_clahe_apply<true>, agrid, dim3(CL_TB), 0, s, a);
  else
    hipLaunchKernelGGL(k_clahe_apply<false>, agrid, dim3(CL_TB), 0, s, a);
  HIPCHK(hipGetLastError());
  CHK(ev.record(4, s));
  CHK(ddst.down(j.dst, n));
  if (j.luts) CHK(dlut.down(j.luts, tiles * CL_BINS));
  CHK(ev.record(5, s));
  HIPCHK(hipEventSynchronize(ev.e[5]));
  ev.report(j.times_ms, CL_TIMES, CL_TIMES);
  return GLH_OK;
}

}  // namespace glh
