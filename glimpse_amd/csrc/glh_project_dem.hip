// glh_project_dem.hip -- Camera.project_dem (camera.py:967-1129) and Camera.rasterize (camera.py:858-883) on the device:
// the work behind glh_stage_project_dem and glh_stage_rasterize (include/glimpse_hip.h; glimpse_hip.hip validates the
// arguments and calls project_dem_run / rasterize_run).  A translation unit of its own, like glh_viewshed.hip: it includes
// rocPRIM (the device radix sort).
//
// The reference walks the DEM tile by tile (Grid.tile_indices): it projects a tile's cells, groups them by the pixel they
// truncate to (np.unique), sums each layer per pixel in float64 in the order the cells appear (np.bincount), multiplies by
// 1 / count, and writes the tile's pixels over whatever earlier tiles left there -- no depth test.  A pixel therefore holds
// the mean of the LAST tile that reached it, of that tile's cells alone, summed row-major.  Here:
//   1. project: one thread per membership (a cell once per tile it belongs to; tiles overlap).  Memberships are numbered
//      tile after tile and row-major within a tile -- the reference's order.  project_f in exact arithmetic gives the
//      pixel and the depth; atomicMax leaves each pixel's last tile in `winner`.
//   2. order: a membership whose tile is not its pixel's winner loses its pixel; rocPRIM's stable radix sort on the pixel
//      brings the rest into pixel order with every pixel's cells still in the reference's order; one pass marks where each
//      pixel's run begins and ends.
//   3. reduce: per (pixel, layer) the run is summed sequentially in float64, one rounded addition per cell (the library
//      is built with -ffp-contract=off and the sum uses the explicit round-to-nearest intrinsics), times 1 / count.
// The value layers are inputs passed through, so they come out bit for bit as the reference has them, call after call.
// Camera.rasterize is stages 2 and 3 on keys the caller supplies.
#include <hip/hip_runtime.h>

#include <cstring>  // (before rocPRIM: its headers call the host memset)

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_project_dem.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int PD_TB = 256;
// A pixel with at least this many cells is summed by its whole wavefront (the lanes fetch, one running sum is carried
// through them in order); a shorter run is one thread's loop.
constexpr uint32_t PD_LONG = 64;

// ---- the tiling on the device ------------------------------------------------------------------------------------------
// The tiles are the cross product of the row slices and the column slices, so the memberships form an SY x SX grid of
// "expanded" rows and columns (a DEM row or column once per slice that holds it).  The host lays the slices out; the
// device only looks up.
struct PdGeom {
  const int32_t* col_slice;  // [SX] the column slice of an expanded column
  const int32_t* row_slice;  // [SY]
  const int32_t* xt;         // [ntx][3] per column slice: first DEM column, first expanded column, width
  const int32_t* yt;         // [nty][3] per row slice: first DEM row, first expanded row, height
  int SX, SY, ntx;
};
struct PdWhere {
  uint32_t m;     // membership number: tile-major, row-major within the tile
  uint32_t tile;  // row-major tile number + 1
  uint32_t cell;  // row * nx + col of the DEM
};
__device__ __forceinline__ PdWhere pd_locate(const PdGeom& g, int nx, int ex, int ey) {
  const int tx = g.col_slice[ex], ty = g.row_slice[ey];
  const int x0 = g.xt[3 * tx], xo = g.xt[3 * tx + 1], w = g.xt[3 * tx + 2];
  const int y0 = g.yt[3 * ty], yo = g.yt[3 * ty + 1], h = g.yt[3 * ty + 2];
  const int c = ex - xo, r = ey - yo;
  PdWhere o;
  // the tiles of the row slices above hold yo * SX memberships, the tiles to the left in this row slice h * xo
  o.m = (uint32_t)((int64_t)yo * g.SX + (int64_t)h * xo + (int64_t)r * w + c);
  o.tile = (uint32_t)(ty * g.ntx + tx) + 1u;
  o.cell = (uint32_t)((int64_t)(y0 + r) * nx + (x0 + c));
  return o;
}

// ---- stage 1 -----------------------------------------------------------------------------------------------------------
struct PdProjectArgs {
  CamDev cam;
  uint32_t flags;  // cam_flags(cam)
  int width, height;
  PdGeom g;
  const double* xc;  // [SX] the x of every expanded column: each tile's own Grid.x
  const double* yc;  // [SY]
  const void* z;
  int z_f32;
  int nx;
  const uint8_t* mask;  // or null
  uint32_t* key;        // [M] pixel (row * width + column), or npix: none
  uint32_t* cell;       // [M]
  double* depth;        // [M], or null
  uint32_t* winner;     // [npix] the last tile (+ 1) that reached the pixel; 0: none
  uint32_t npix;
};

__global__ void __launch_bounds__(PD_TB) k_pd_project(PdProjectArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * PD_TB + threadIdx.x;
  if (gid >= (int64_t)a.g.SX * a.g.SY) return;
  const int ey = (int)(gid / a.g.SX), ex = (int)(gid - (int64_t)ey * a.g.SX);
  const PdWhere w = pd_locate(a.g, a.nx, ex, ey);
  uint32_t key = a.npix;
  double depth = NAN;
  if (!a.mask || a.mask[w.cell]) {
    const double z = a.z_f32 ? (double)static_cast<const float*>(a.z)[w.cell] : static_cast<const double*>(a.z)[w.cell];
    double u, v;
    project_f(a.cam, a.flags, a.xc[ex], a.yc[ey], z, u, v, &depth);  // (a NaN elevation or a cell behind: u, v NaN)
    // Camera.inframe is 0 <= uv <= imgsz; a cell exactly on the far edge makes the reference raise: out of frame here
    if (u >= 0.0 && u < (double)a.width && v >= 0.0 && v < (double)a.height) {
      key = (uint32_t)(int)v * (uint32_t)a.width + (uint32_t)(int)u;  // astype(int) truncates
      atomicMax(a.winner + key, w.tile);
    }
  }
  a.key[w.m] = key;
  a.cell[w.m] = w.cell;
  if (a.depth) a.depth[w.m] = depth;
}

// ---- stage 2 -----------------------------------------------------------------------------------------------------------
// array[idx] = values (camera.py:1124): only the last tile's cells stay on a pixel
__global__ void __launch_bounds__(PD_TB) k_pd_keep_winners(PdGeom g, int nx, uint32_t* key, const uint32_t* winner,
                                                          uint32_t npix, uint32_t* idx, uint32_t* kept) {
  const int64_t gid = (int64_t)blockIdx.x * PD_TB + threadIdx.x;
  if (gid >= (int64_t)g.SX * g.SY) return;
  const int ey = (int)(gid / g.SX), ex = (int)(gid - (int64_t)ey * g.SX);
  const PdWhere w = pd_locate(g, nx, ex, ey);
  const uint32_t k = key[w.m];
  idx[w.m] = w.m;
  if (k >= npix) return;
  if (winner[k] == w.tile)
    atomicAdd(kept, 1u);
  else
    key[w.m] = npix;
}

__global__ void __launch_bounds__(PD_TB) k_pd_iota(uint32_t* idx, uint32_t n) {
  const size_t i = (size_t)blockIdx.x * PD_TB + threadIdx.x;
  if (i < n) idx[i] = (uint32_t)i;
}

// where each pixel's run of the sorted keys begins and ends (both preset to 0: an empty run)
__global__ void __launch_bounds__(PD_TB) k_pd_runs(const uint32_t* ks, uint32_t n, uint32_t npix, uint32_t* run_start,
                                                  uint32_t* run_end) {
  const size_t i = (size_t)blockIdx.x * PD_TB + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = ks[i];
  if (k >= npix) return;
  if (i == 0 || ks[i - 1] != k) run_start[k] = (uint32_t)i;
  if (i + 1 == n || ks[i + 1] != k) run_end[k] = (uint32_t)i + 1u;
}

// ---- stage 3 -----------------------------------------------------------------------------------------------------------
struct PdReduceArgs {
  const uint32_t* run_start;  // [npix]
  const uint32_t* run_end;    // [npix]
  const uint32_t* order;      // [n] sorted position -> item (membership, or point)
  const uint32_t* cell;       // [items] item -> row of `values`, or null: the item itself
  const void* values;         // [rows][layers] of v_dtype
  int v_dtype, layers;
  const double* depth;        // [items] the layer after the value layers, or null
  double* out;                // [npix][nl]
  int nl;                     // layers + (depth ? 1 : 0)
  int64_t total;              // npix * nl
};

__device__ __forceinline__ double pd_value(const PdReduceArgs& a, uint32_t at, int layer) {
  const uint32_t item = a.order[at];
  if (layer >= a.layers) return a.depth[item];
  const size_t i = (size_t)(a.cell ? a.cell[item] : item) * a.layers + layer;
  switch (a.v_dtype) {
    case GLH_PD_F64: return static_cast<const double*>(a.values)[i];
    case GLH_PD_F32: return (double)static_cast<const float*>(a.values)[i];
    case GLH_PD_U16: return (double)static_cast<const uint16_t*>(a.values)[i];
    default: return (double)static_cast<const uint8_t*>(a.values)[i];
  }
}

// One thread per (pixel, layer), the layer fastest: neighbouring threads read neighbouring values of one cell.  The sum
// is np.bincount's: from +0.0, one cell after another.  A run of PD_LONG cells or more is taken over by the wavefront,
// one such run at a time: the lanes fetch 64 cells at once and the sum walks through the lanes in order, so the long
// far-field runs cost their additions but not one memory round trip per cell.
__global__ void __launch_bounds__(PD_TB) k_pd_reduce(PdReduceArgs a) {
  const int64_t w = (int64_t)blockIdx.x * PD_TB + threadIdx.x;
  const bool valid = w < a.total;
  const int lane = threadIdx.x & 63;
  uint32_t s = 0, n = 0;
  int layer = 0;
  if (valid) {
    const int64_t pix = w / a.nl;
    layer = (int)(w - pix * a.nl);
    s = a.run_start[pix];
    n = a.run_end[pix] - s;
  }
  double acc = 0.0;
  if (n < PD_LONG)
    for (uint32_t k = 0; k < n; ++k) acc = __dadd_rn(acc, pd_value(a, s + k, layer));
  unsigned long long todo = __ballot(n >= PD_LONG);
  while (todo) {  // (uniform over the wavefront: every lane takes part, also those beyond `total`)
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const uint32_t s0 = __shfl(s, src), n0 = __shfl(n, src);
    const int l0 = __shfl(layer, src);
    double sum = 0.0;
    for (uint32_t base = 0; base < n0; base += 64) {
      const uint32_t k = base + (uint32_t)lane;
      const double v = k < n0 ? pd_value(a, s0 + k, l0) : 0.0;
      const int lim = n0 - base < 64u ? (int)(n0 - base) : 64;
      for (int j = 0; j < lim; ++j) sum = __dadd_rn(sum, __shfl(v, j));
    }
    if (lane == src) acc = sum;
  }
  if (valid) a.out[w] = n ? __dmul_rn(acc, __ddiv_rn(1.0, (double)n)) : NAN;  // sums * (1 / counts) (helpers.py:1690)
}

// ---- host --------------------------------------------------------------------------------------------------------------
unsigned blocks_for(int64_t n) { return (unsigned)((n + PD_TB - 1) / PD_TB); }

// Stages 2 (from the sort on) and 3, the download and the times: what project_dem and rasterize share.  key [n] holds a
// pixel or npix, idx [n] the items; ev.e[0 .. 2] are recorded (upload began, upload done, keys done).
int order_reduce_download(hipStream_t s, StageEvents<6>& ev, uint32_t* key, uint32_t* idx, uint32_t n,
                          uint32_t npix, PdReduceArgs ra, double* out, double* times_ms, double items, const uint32_t* kept) {
  DevBuf ks, order, run_start, run_end, dout, temp;
  CHK(ks.alloc((size_t)n * 4));
  CHK(order.alloc((size_t)n * 4));
  CHK(run_start.alloc((size_t)npix * 4));
  CHK(run_end.alloc((size_t)npix * 4));
  CHK(dout.alloc((size_t)ra.total * 8));
  int bits = 1;
  while ((1ull << bits) <= npix) ++bits;  // (npix itself, "no pixel", sorts last)
  size_t tbytes = 0;
  HIPCHK(rocprim::radix_sort_pairs(nullptr, tbytes, key, ks.as<uint32_t>(), idx, order.as<uint32_t>(), n, 0, bits, s));
  CHK(temp.alloc(tbytes));
  HIPCHK(rocprim::radix_sort_pairs(temp.p, tbytes, key, ks.as<uint32_t>(), idx, order.as<uint32_t>(), n, 0, bits, s));
  HIPCHK(hipMemsetAsync(run_start.p, 0, (size_t)npix * 4, s));
  HIPCHK(hipMemsetAsync(run_end.p, 0, (size_t)npix * 4, s));
  hipLaunchKernelGGL(k_pd_runs, dim3(blocks_for(n)), dim3(PD_TB), 0, s, ks.as<uint32_t>(), n, npix,
                     run_start.as<uint32_t>(), run_end.as<uint32_t>());
  HIPCHK(hipGetLastError());
  CHK(ev.record(3, s));
  ra.run_start = run_start.as<uint32_t>();
  ra.run_end = run_end.as<uint32_t>();
  ra.order = order.as<uint32_t>();
  ra.out = dout.as<double>();
  hipLaunchKernelGGL(k_pd_reduce, dim3(blocks_for(ra.total)), dim3(PD_TB), 0, s, ra);
  HIPCHK(hipGetLastError());
  CHK(ev.record(4, s));
  CHK(dout.down(out, (size_t)ra.total * 8));
  uint32_t h_kept = n;
  if (kept) HIPCHK(hipMemcpy(&h_kept, kept, 4, hipMemcpyDeviceToHost));
  CHK(ev.record(5, s));
  HIPCHK(hipEventSynchronize(ev.e[5]));
  if (times_ms) {
    ev.report(times_ms, 5, 5);
    times_ms[5] = items;
    times_ms[6] = (double)h_kept;
    times_ms[7] = (double)tbytes;
  }
  return GLH_OK;
}

// an axis laid out for the device: slice of every expanded row or column, and per slice (first cell, first expanded, size)
void lay_out(const PdAxis& ax, std::vector<int32_t>& slice_of, std::vector<int32_t>& table) {
  slice_of.clear();
  table.clear();
  for (int k = 0; k < ax.n; ++k) {
    const int32_t size = ax.end[k] - ax.start[k];
    table.push_back(ax.start[k]);
    table.push_back((int32_t)slice_of.size());
    table.push_back(size);
    slice_of.insert(slice_of.end(), (size_t)size, k);
  }
}

}  // namespace

int64_t project_dem_memberships(const ProjectDemJob& j) {
  int64_t sx = 0, sy = 0;
  for (int k = 0; k < j.tx.n; ++k) sx += j.tx.end[k] - j.tx.start[k];
  for (int k = 0; k < j.ty.n; ++k) sy += j.ty.end[k] - j.ty.start[k];
  return sx * sy;
}

int project_dem_run(const ProjectDemJob& j) {
  std::vector<int32_t> col_slice, row_slice, xt, yt;
  lay_out(j.tx, col_slice, xt);
  lay_out(j.ty, row_slice, yt);
  const int SX = (int)col_slice.size(), SY = (int)row_slice.size();
  const int64_t M = (int64_t)SX * SY;
  const uint32_t npix = (uint32_t)j.width * (uint32_t)j.height;
  const size_t ncell = (size_t)j.nx * j.ny;
  const int nl = j.layers + (j.return_depth ? 1 : 0);
  static const size_t v_size[] = {8, 4, 1, 2};  // GLH_PD_F64, _F32, _U8, _U16

  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;  // (the null stream: every copy below is ordered with the kernels)
  StageEvents<6> ev;
  CHK(ev.create());
  DevBuf dz, dmask, dvals, dxc, dyc, dcs, drs, dxt, dyt, key, idx, cell, depth, winner, kept;
  CHK(ev.record(0, s));
  CHK(dz.up(j.z, ncell * (j.z_f32 ? 4 : 8)));
  if (j.mask) CHK(dmask.up(j.mask, ncell));
  if (j.layers) CHK(dvals.up(j.values, ncell * j.layers * v_size[j.v_dtype]));
  CHK(dxc.up(j.tx.coords, (size_t)SX * 8));
  CHK(dyc.up(j.ty.coords, (size_t)SY * 8));
  CHK(dcs.up(col_slice.data(), (size_t)SX * 4));
  CHK(drs.up(row_slice.data(), (size_t)SY * 4));
  CHK(dxt.up(xt.data(), xt.size() * 4));
  CHK(dyt.up(yt.data(), yt.size() * 4));
  CHK(key.alloc((size_t)M * 4));
  CHK(idx.alloc((size_t)M * 4));
  CHK(cell.alloc((size_t)M * 4));
  if (j.return_depth) CHK(depth.alloc((size_t)M * 8));
  CHK(winner.alloc((size_t)npix * 4));
  CHK(kept.alloc(4));
  CHK(ev.record(1, s));

  const PdGeom g{dcs.as<int32_t>(), drs.as<int32_t>(), dxt.as<int32_t>(), dyt.as<int32_t>(), SX, SY, j.tx.n};
  HIPCHK(hipMemsetAsync(winner.p, 0, (size_t)npix * 4, s));
  HIPCHK(hipMemsetAsync(kept.p, 0, 4, s));
  PdProjectArgs pa{*j.cam, cam_flags(*j.cam), j.width, j.height, g, dxc.as<double>(), dyc.as<double>(), dz.p, j.z_f32, j.nx,
                   dmask.as<uint8_t>(), key.as<uint32_t>(), cell.as<uint32_t>(), depth.as<double>(), winner.as<uint32_t>(),
                   npix};
  hipLaunchKernelGGL(k_pd_project, dim3(blocks_for(M)), dim3(PD_TB), 0, s, pa);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  hipLaunchKernelGGL(k_pd_keep_winners, dim3(blocks_for(M)), dim3(PD_TB), 0, s, g, j.nx, key.as<uint32_t>(),
                     winner.as<uint32_t>(), npix, idx.as<uint32_t>(), kept.as<uint32_t>());
  HIPCHK(hipGetLastError());

  PdReduceArgs ra{};
  ra.cell = cell.as<uint32_t>();
  ra.values = dvals.p;
  ra.v_dtype = j.v_dtype;
  ra.layers = j.layers;
  ra.depth = depth.as<double>();
  ra.nl = nl;
  ra.total = (int64_t)npix * nl;
  return order_reduce_download(s, ev, key.as<uint32_t>(), idx.as<uint32_t>(), (uint32_t)M, npix, ra, j.out, j.times_ms,
                               (double)M, kept.as<uint32_t>());
}

int rasterize_run(const RasterizeJob& j) {
  const uint32_t n = (uint32_t)j.n, npix = (uint32_t)j.n_pixels;
  HIPCHK(hipSetDevice(j.device));
  hipStream_t s = nullptr;
  StageEvents<6> ev;
  CHK(ev.create());
  DevBuf key, idx, dvals;
  CHK(ev.record(0, s));
  CHK(key.up(j.keys, (size_t)n * 4));  // (checked to lie in [0, n_pixels): the bits of a uint32 pixel)
  CHK(dvals.up(j.values, (size_t)n * j.layers * 8));
  CHK(idx.alloc((size_t)n * 4));
  CHK(ev.record(1, s));
  hipLaunchKernelGGL(k_pd_iota, dim3(blocks_for(n)), dim3(PD_TB), 0, s, idx.as<uint32_t>(), n);
  HIPCHK(hipGetLastError());
  CHK(ev.record(2, s));
  PdReduceArgs ra{};
  ra.values = dvals.p;
  ra.v_dtype = GLH_PD_F64;
  ra.layers = j.layers;
  ra.nl = j.layers;
  ra.total = (int64_t)npix * j.layers;
  return order_reduce_download(s, ev, key.as<uint32_t>(), idx.as<uint32_t>(), n, npix, ra, j.out, j.times_ms, (double)n,
                               nullptr);
}

}  // namespace glh
