// glh_ortho.hip -- Image.orthorectify on the device: the work behind glh_stage_orthorectify (include/glimpse_hip.h;
// glimpse_hip.hip validates the arguments and calls orthorectify_run).  A calibrated, oriented oblique frame and the DEM
// give the frame's pixels on the DEM's grid -- the inverse of Camera.project_dem (glh_project_dem.hip), which drapes
// per-cell values into the image.  The reference has no single function for it; the rule (INPUTS.md, "Orthorectification:
// the rule") is composed of reference calls, and for every cell (r, c) of the DEM reads:
//   xyz = (x[c], y[r], z[r, c]);  uv = Camera.xyz_to_uv(xyz);
//   seen = z is not NaN  and  Camera.inframe(uv)  and  the caller's mask and viewshed at the cell;
//   value = RegularGridInterpolator((pv, pu), frame[:, :, ch], method, bounds_error=False)(uv[::-1]) where seen, else NaN.
// The interpolator answers NaN outside the pixel centres 0.5 .. n - 0.5, which lie inside the frame, and a NaN elevation
// or a cell behind the camera projects to NaN: the sampler's own domain test is the whole of `seen` but the mask.
//
// One thread per cell, all channels of it; one launch per frame, through the staging ring of glh_frame_ring.h, so that a
// frame's copies overlap its neighbours' kernels.  The DEM, its coordinates and the masks are uploaded once.  The
// projection is the exact-arithmetic project_f (glh_math.h: what glh_stage_project runs) and the sampler is k_reproject's
// (glh_rpj_sample.h), so a cell's value is a function of the inputs alone: no atomics, no LDS, no dependence on the launch
// geometry.  No LDS because nothing is shared: a cell reads its own elevation once, and the frame pixels neighbouring
// cells gather overlap only through the projective map, which the caches serve.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/glimpse_hip.h"
#include "glh_frame_ring.h"
#include "glh_math.h"
#include "glh_ortho.h"
#include "glh_rpj_sample.h"
#include "glh_stage.h"

namespace glh {
namespace {

// One workgroup: RPJ_BX x RPJ_BY cells, a wave two rows of 32 neighbours -- their elevations are two coalesced runs, and
// they gather neighbouring frame pixels.
struct OrthoArgs {
  CamDev cam;      // by value: the kernel reads it from scalar registers
  uint32_t flags;  // cam_flags(cam)
  int z_f32;
  const void* z;
  const double* x;
  const double* y;
  const uint8_t* seen;  // or null
  const void* frame;
  void* out;
  int nx, ny, fw, fh, method;
};

// float32 frames give float32 (the float64 sample rounded once, as Image.project returns it), every other frame float64
template <typename T>
using ortho_out_t = std::conditional_t<std::is_same<T, float>::value, float, double>;

template <typename T, int C>
__global__ __launch_bounds__(RPJ_BX * RPJ_BY) void k_orthorectify(const OrthoArgs a) {
  using Out = ortho_out_t<T>;
  const int col = blockIdx.x * RPJ_BX + threadIdx.x, row = blockIdx.y * RPJ_BY + threadIdx.y;
  if (col >= a.nx || row >= a.ny) return;
  const size_t cell = (size_t)row * a.nx + col;
  const double z = a.z_f32 ? (double)static_cast<const float*>(a.z)[cell] : static_cast<const double*>(a.z)[cell];
  const bool masked = a.seen && !a.seen[cell];
  double u, v;
  project_f(a.cam, a.flags, a.x[col], a.y[row], z, u, v);  // (a NaN elevation or a cell behind: u, v NaN)
  Out* o = static_cast<Out*>(a.out) + cell * C;
  if (masked || !rpj_sample<T, C, Out>(static_cast<const T*>(a.frame), a.fw, a.fh, u, v, a.method, o)) {
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (Out)NAN;
  }
}

template <typename T>
void launch_orthorectify(hipStream_t s, int channels, const OrthoArgs& a) {
  const dim3 grid((a.nx + RPJ_BX - 1) / RPJ_BX, (a.ny + RPJ_BY - 1) / RPJ_BY), block(RPJ_BX, RPJ_BY);
  if (channels == 1)
    hipLaunchKernelGGL((k_orthorectify<T, 1>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((k_orthorectify<T, 3>), grid, block, 0, s, a);
}

}  // namespace

int orthorectify_run(const OrthoJob& j) {
  const size_t ncell = (size_t)j.nx * j.ny;
  const size_t in_bytes = (size_t)j.width * j.height * j.channels * (j.depth_bits / 8);
  const size_t out_bytes = ncell * j.channels * (j.depth_bits == 32 ? 4 : 8);
  HIPCHK(hipSetDevice(j.device));
  DevBuf dz, dx, dy, dseen;
  CHK(dz.up(j.z, ncell * (j.z_f32 ? 4 : 8)));
  CHK(dx.up(j.x, (size_t)j.nx * 8));
  CHK(dy.up(j.y, (size_t)j.ny * 8));
  if (j.seen) CHK(dseen.up(j.seen, ncell * j.n_seen));
  FrameRing r;
  CHK(r.open(j.n_frames, in_bytes, out_bytes, j.kernel_ms != nullptr));
  auto launch = [&](int i, int k) {
    OrthoArgs a;
    a.cam = j.cams[i];
    a.flags = cam_flags(a.cam);
    a.z_f32 = j.z_f32;
    a.z = dz.p;
    a.x = dx.as<double>();
    a.y = dy.as<double>();
    a.seen = j.seen ? dseen.as<uint8_t>() + ncell * (j.seen_of ? j.seen_of[i] : 0) : nullptr;
    a.frame = r.dev_in[k];
    a.out = r.dev_out[k];
    a.nx = j.nx, a.ny = j.ny, a.fw = j.width, a.fh = j.height, a.method = j.method;
    if (j.depth_bits == 8)
      launch_orthorectify<uint8_t>(r.run, j.channels, a);
    else if (j.depth_bits == 16)
      launch_orthorectify<uint16_t>(r.run, j.channels, a);
    else if (j.depth_bits == 32)
      launch_orthorectify<float>(r.run, j.channels, a);
    else
      launch_orthorectify<double>(r.run, j.channels, a);
  };
  return r.process(j.frames, j.n_frames, j.out, launch, j.kernel_ms);
}

}  // namespace glh
