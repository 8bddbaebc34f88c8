// glh_orient.hip -- the objective and gradient of optimize.ObserverCameras.fit (optimize.py:2047-2072) on the device:
// the work behind glh_orient_create / _eval / _destroy (include/glimpse_hip.h; glimpse_hip.hip validates the arguments).
// Camera._uv_to_xy (camera.py:1510-1519, glh_stage_uv_to_xy), which makes the matches' camera coordinates, is here too.
//
// The reference loops over the image pairs in Python; per pair (i, j) with matches n it forms the unit ray directions
// d_i = R_i^T [x, y, 1] / |.| of both sides (RotationMatchesXYZ.predicted, :954-970), adds sum |d_i - d_j| to the objective
// and  g[w] = sum_n sum_r sign(d_i - d_j)[r] * (Rprime_i[r, w, :] . [x, y, 1])  to image i's gradient, minus g to image j's.
// Its quirks are kept: only Rprime of image i, no derivative of the normalisation, no weights.
//
//   create.  The matches' camera coordinates of both sides, interleaved [N][2] in pair order, are uploaded once.  Every
//   pair is cut into chunks of OR_CHUNK matches (the last one shorter; a pair without matches has none), and every image
//   gets the list of the pairs it is part of, in pair order.
//
//   k_orient_map, a workgroup of 256 per chunk.  The chunk's pair, hence R_i, R_j and Rprime_i, are the same for the whole
//   workgroup: they are read through uniform addresses (scalar loads).  Lane t takes matches t, t + 256, ... of the chunk
//   in order, one 16-byte load per side, and keeps four running sums (objective, g[0..2]) that start at +0.  The 256 sums
//   are added by block_sum4: a butterfly over the wave (lane ^ 32, 16, ... 1; a + b == b + a, so every lane ends with the
//   same bits), then waves 0 .. 3 in order through LDS.  One [4] partial per chunk.
//
//   k_orient_reduce.  Thread m < n_images walks image m's incidence list in pair order: a pair's g is the sum of its
//   chunks' partials in chunk order from +0; it is added where the image is i and subtracted where it is j.  The last
//   workgroup makes the objective: lane t adds the pairs t, t + 256, ... in order (each the sum of its chunks as above),
//   then block_sum4.
//
// No floating-point atomics; the order of every sum is a function of the pair sizes alone, so two evaluations give the
// same bytes and tests/orient_restated.py restates them in NumPy bit for bit.  Every float64 expression is evaluated
// operation by operation as NumPy does (explicit round-to-nearest intrinsics; the library is built with
// -ffp-contract=off besides); sqrt and / are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_math.h"
#include "glh_orient.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int OR_TB = 256, OR_WAVE = 64;

struct OrChunk {
  int64_t start;  // first match, in the uploaded order
  int32_t pair;
  int32_t count;  // 1 .. OR_CHUNK
};

// The sum of the workgroup's 256 values of each of v[0..3], in thread 0 (every lane of wave 0 holds the wave's own sum).
__device__ __forceinline__ void block_sum4(double v[4]) {
  for (int off = OR_WAVE / 2; off; off >>= 1)
    for (int q = 0; q < 4; ++q) v[q] = __dadd_rn(v[q], __shfl_xor(v[q], off));
  __shared__ double s_part[OR_TB / OR_WAVE][4];
  if ((threadIdx.x & (OR_WAVE - 1)) == 0)
    for (int q = 0; q < 4; ++q) s_part[threadIdx.x / OR_WAVE][q] = v[q];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < OR_TB / OR_WAVE; ++w)
      for (int q = 0; q < 4; ++q) v[q] = __dadd_rn(v[q], s_part[w][q]);
}

// R^T [x, y, 1] scaled to the unit sphere: Camera._xy_to_xyz (camera.py:1486-1492) and the normalisation of
// RotationMatchesXYZ.predicted (optimize.py:969): times 1 / norm, norm = sqrt((a^2 + b^2) + c^2).
__device__ __forceinline__ void or_ray(const double* __restrict__ R, double x, double y, double d[3]) {
  for (int k = 0; k < 3; ++k) d[k] = __dadd_rn(__dadd_rn(__dmul_rn(R[k], x), __dmul_rn(R[3 + k], y)), R[6 + k]);
  const double n2 = __dadd_rn(__dadd_rn(__dmul_rn(d[0], d[0]), __dmul_rn(d[1], d[1])), __dmul_rn(d[2], d[2]));
  const double inv = __ddiv_rn(1.0, __dsqrt_rn(n2));
  for (int k = 0; k < 3; ++k) d[k] = __dmul_rn(d[k], inv);
}

// np.sign: -1, 0, 1, NaN for NaN
__device__ __forceinline__ double or_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v)); }

__global__ void __launch_bounds__(OR_TB) k_orient_map(const OrChunk* __restrict__ chunks, const int32_t* __restrict__ pair_i,
                                                      const int32_t* __restrict__ pair_j, const double2* __restrict__ xy_i,
                                                      const double2* __restrict__ xy_j, const double* __restrict__ R,
                                                      const double* __restrict__ Rprime, double* __restrict__ partial) {
  const OrChunk c = chunks[blockIdx.x];
  const double* __restrict__ Ri = R + 9 * (size_t)pair_i[c.pair];
  const double* __restrict__ Rj = R + 9 * (size_t)pair_j[c.pair];
  const double* __restrict__ Rp = Rprime + 27 * (size_t)pair_i[c.pair];  // [r][w][k]
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int m = threadIdx.x; m < c.count; m += OR_TB) {
    const double2 a = xy_i[c.start + m], b = xy_j[c.start + m];
    double di[3], dj[3], s[3];
    or_ray(Ri, a.x, a.y, di);
    or_ray(Rj, b.x, b.y, dj);
    double e[3];
    for (int r = 0; r < 3; ++r) {
      const double d = __dsub_rn(di[r], dj[r]);
      e[r] = fabs(d);
      s[r] = or_sign(d);
    }
    acc[0] = __dadd_rn(acc[0], __dadd_rn(__dadd_rn(e[0], e[1]), e[2]));
    for (int w = 0; w < 3; ++w) {
      double t[3];  // dD/dw[r] = Rprime[r, w, :] . [x, y, 1], times sign[r]
      for (int r = 0; r < 3; ++r) {
        const double* q = Rp + 9 * r + 3 * w;
        t[r] = __dmul_rn(s[r], __dadd_rn(__dadd_rn(__dmul_rn(q[0], a.x), __dmul_rn(q[1], a.y)), q[2]));
      }
      acc[1 + w] = __dadd_rn(acc[1 + w], __dadd_rn(__dadd_rn(t[0], t[1]), t[2]));
    }
  }
  block_sum4(acc);
  if (threadIdx.x == 0)
    for (int q = 0; q < 4; ++q) partial[4 * (size_t)blockIdx.x + q] = acc[q];
}

// A pair's [4]: its chunks' partials in chunk order, from +0.
__device__ __forceinline__ void or_pair_sum(const double* __restrict__ partial, const int32_t* __restrict__ chunk_off, int p,
                                            double v[4]) {
  for (int q = 0; q < 4; ++q) v[q] = 0.0;
  for (int c = chunk_off[p]; c < chunk_off[p + 1]; ++c)
    for (int q = 0; q < 4; ++q) v[q] = __dadd_rn(v[q], partial[4 * (size_t)c + q]);
}

// grid: ceil(n_images / 256) workgroups for the images, then one for the objective.  out: gradient [n_images][3], objective.
__global__ void __launch_bounds__(OR_TB) k_orient_reduce(const double* __restrict__ partial, const int32_t* __restrict__ chunk_off,
                                                         const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc,
                                                         int n_images, int n_pairs, double* __restrict__ out) {
  if (blockIdx.x + 1 < gridDim.x) {
    const int img = blockIdx.x * OR_TB + threadIdx.x;
    if (img >= n_images) return;
    double g[3] = {0.0, 0.0, 0.0};
    for (int e = inc_off[img]; e < inc_off[img + 1]; ++e) {
      const int code = inc[e];  // the pair, or ~pair where the image is the pair's j
      double v[4];
      or_pair_sum(partial, chunk_off, code < 0 ? ~code : code, v);
      for (int w = 0; w < 3; ++w) g[w] = code < 0 ? __dsub_rn(g[w], v[1 + w]) : __dadd_rn(g[w], v[1 + w]);
    }
    for (int w = 0; w < 3; ++w) out[3 * (size_t)img + w] = g[w];
    return;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = threadIdx.x; p < n_pairs; p += OR_TB) {
    double v[4];
    or_pair_sum(partial, chunk_off, p, v);
    acc[0] = __dadd_rn(acc[0], v[0]);
  }
  block_sum4(acc);
  if (threadIdx.x == 0) out[3 * (size_t)n_images] = acc[0];
}

// Camera._uv_to_xy on explicit points: uv [n][2] -> xy [n][2]
__global__ void __launch_bounds__(OR_TB) k_uv_to_xy(const CamDev* __restrict__ cam, const double2* __restrict__ uv, int n,
                                                    double2* __restrict__ xy) {
  const int i = blockIdx.x * OR_TB + threadIdx.x;
  if (i >= n) return;
  const double2 p = uv[i];
  // (unproject's first lines, glh_math.h)
  double x = (p.x - cam->off[0]) * (1.0 / cam->f[0]);
  double y = (p.y - cam->off[1]) * (1.0 / cam->f[1]);
  undistort(*cam, cam_flags(*cam), x, y);
  xy[i] = make_double2(x, y);
}

}  // namespace
}  // namespace glh

struct glh_orient : glh::DeviceObject {
  int n_images = 0, n_pairs = 0, n_chunks = 0;
  glh::DevBuf chunks, pair_i, pair_j, xy_i, xy_j, chunk_off, inc_off, inc, rot, partial, out;
  glh::StageEvents<glh::OR_TIMES + 1> ev;
  std::vector<double> stage;  // host side of `rot` ([n][9] R, then [n][27] Rprime) and of `out`
};

namespace glh {

static int orient_fill(glh_orient* h, int n_images, int n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                       const int64_t* pair_offset, const double* xy_i, const double* xy_j) {
  h->n_images = n_images, h->n_pairs = n_pairs;
  std::vector<OrChunk> chunks;
  std::vector<int32_t> chunk_off(n_pairs + 1, 0), inc_off(n_images + 1, 0);
  for (int p = 0; p < n_pairs; ++p) {
    for (int64_t s = pair_offset[p]; s < pair_offset[p + 1]; s += OR_CHUNK) {
      const int64_t left = pair_offset[p + 1] - s;
      chunks.push_back(OrChunk{s, p, (int32_t)(left < OR_CHUNK ? left : OR_CHUNK)});
    }
    chunk_off[p + 1] = (int32_t)chunks.size();
    ++inc_off[pair_i[p] + 1];
    ++inc_off[pair_j[p] + 1];
  }
  for (int m = 0; m < n_images; ++m) inc_off[m + 1] += inc_off[m];
  std::vector<int32_t> inc(2 * (size_t)n_pairs), fill(inc_off.begin(), inc_off.end() - 1);
  for (int p = 0; p < n_pairs; ++p) {  // the reference adds to image i, then subtracts from image j
    inc[fill[pair_i[p]]++] = p;
    inc[fill[pair_j[p]]++] = ~p;
  }
  h->n_chunks = (int)chunks.size();
  const size_t N = (size_t)pair_offset[n_pairs];
  CHK(h->ev.create());
  if (chunks.empty()) chunks.push_back(OrChunk{0, 0, 0});  // (nothing is copied from a null pointer; n_chunks stays 0)
  const double none[2] = {0.0, 0.0};
  if (N == 0) xy_i = xy_j = none;
  if (n_pairs == 0) pair_i = pair_j = chunk_off.data(), inc.push_back(0);
  CHK(h->chunks.up(chunks.data(), chunks.size() * sizeof(OrChunk)));
  CHK(h->pair_i.up(pair_i, (n_pairs ? (size_t)n_pairs : 1) * 4));
  CHK(h->pair_j.up(pair_j, (n_pairs ? (size_t)n_pairs : 1) * 4));
  CHK(h->xy_i.up(xy_i, (N ? N : 1) * 16));
  CHK(h->xy_j.up(xy_j, (N ? N : 1) * 16));
  CHK(h->chunk_off.up(chunk_off.data(), chunk_off.size() * 4));
  CHK(h->inc_off.up(inc_off.data(), inc_off.size() * 4));
  CHK(h->inc.up(inc.data(), inc.size() * 4));
  CHK(h->rot.alloc((size_t)n_images * 36 * 8));
  CHK(h->partial.alloc(chunks.size() * 32));
  CHK(h->out.alloc(((size_t)n_images * 3 + 1) * 8));
  h->stage.resize((size_t)n_images * 36);
  return GLH_OK;
}

int orient_create(int device, int n_images, int n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                  const int64_t* pair_offset, const double* xy_i, const double* xy_j, glh_orient** out) {
  return create_object("orient", device, out, [&](glh_orient* h) {
    return orient_fill(h, n_images, n_pairs, pair_i, pair_j, pair_offset, xy_i, xy_j);
  });
}

int orient_eval(glh_orient* h, const double* R, const double* Rprime, double* objective, double* gradient,
                double* times_ms) {
  const size_t n = (size_t)h->n_images;
  CHK(h->use());
  hipStream_t s = h->stream;
  for (size_t k = 0; k < 9 * n; ++k) h->stage[k] = R[k];
  for (size_t k = 0; k < 27 * n; ++k) h->stage[9 * n + k] = Rprime[k];
  CHK(h->ev.record(0, s));
  HIPCHK(hipMemcpy(h->rot.p, h->stage.data(), n * 36 * 8, hipMemcpyHostToDevice));
  CHK(h->ev.record(1, s));
  if (h->n_chunks) {
    hipLaunchKernelGGL(k_orient_map, dim3((unsigned)h->n_chunks), dim3(OR_TB), 0, s, h->chunks.as<OrChunk>(),
                       h->pair_i.as<int32_t>(), h->pair_j.as<int32_t>(), h->xy_i.as<double2>(), h->xy_j.as<double2>(),
                       h->rot.as<double>(), h->rot.as<double>() + 9 * n, h->partial.as<double>());
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(2, s));
  hipLaunchKernelGGL(k_orient_reduce, dim3((unsigned)((n + OR_TB - 1) / OR_TB + 1)), dim3(OR_TB), 0, s,
                     h->partial.as<double>(), h->chunk_off.as<int32_t>(), h->inc_off.as<int32_t>(), h->inc.as<int32_t>(),
                     h->n_images, h->n_pairs, h->out.as<double>());
  HIPCHK(hipGetLastError());
  CHK(h->ev.record(3, s));
  CHK(h->out.down(h->stage.data(), (3 * n + 1) * 8));
  CHK(h->ev.record(4, s));
  HIPCHK(hipEventSynchronize(h->ev.e[4]));
  for (size_t k = 0; k < 3 * n; ++k) gradient[k] = h->stage[k];
  *objective = h->stage[3 * n];
  h->ev.report(times_ms, OR_TIMES, OR_TIMES);
  return GLH_OK;
}

void orient_destroy(glh_orient* h) { destroy_object(h); }

int uv_to_xy_run(int device, const CamDev& cam, const double* uv, int n, double* xy) {
  HIPCHK(hipSetDevice(device));
  DevBuf dc, du, dx;
  CHK(dc.up(&cam, sizeof cam));
  CHK(du.up(uv, (size_t)n * 16));
  CHK(dx.alloc((size_t)n * 16));
  hipLaunchKernelGGL(k_uv_to_xy, dim3((unsigned)((n + OR_TB - 1) / OR_TB)), dim3(OR_TB), 0, nullptr, dc.as<CamDev>(),
                     du.as<double2>(), n, dx.as<double2>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return dx.down(xy, (size_t)n * 16);
}

}  // namespace glh
