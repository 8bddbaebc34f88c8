// glh_match.hip -- the exact two nearest neighbours among descriptor sets (optimize.match_keypoints, optimize.py:2234-2309,
// with a brute-force matcher in the place of cv2.FlannBasedMatcher): the work behind glh_match_create / _put / _drop /
// _knn2 / _destroy (include/glimpse_hip.h; glimpse_hip.hip validates the arguments).
//
// The result, by definition: for query row q of set Q the two train rows of set T with the smallest keys (d2, index) in
// lexicographic order.  The order is total, so "the best two of a set of candidates" is associative and commutative: the
// result does not depend on the tile sizes, on how T is split over workgroups, or on the order in which partial results
// are merged.  Nothing here is an ordered reduction, and nothing needs an atomic.
//
//   put.  A set is uploaded once and prepared for its path.
//     u8  (D <= 256): k_match_prep_u8 makes int8 x - 128, zero-padded to DP = 32 KS bytes a row (KS in 1, 2, 4, 8), and
//         the int32 squared norm of every shifted row.  The shift cancels in q - t; the padding adds 0 to every product.
//     f32 (any D):    k_match_prep_f32 zero-pads the rows to a multiple of 32 floats (s + (0 - 0) * (0 - 0) == s bit for
//         bit, s being +0 or positive).
//
//   k_match_i8<KS>, 256 threads (4 waves) per 128 queries and one range of T tiles.  d2 = |q|^2 + |t|^2 - 2 q.t in int32,
//   exact (below 2^24).  Wave w owns queries 32 w .. 32 w + 31 of the workgroup as the B operand of
//   v_mfma_i32_32x32x32_i8: lane l keeps bytes 32 ks + 16 (l >> 5) .. + 15 of query l & 31 for every K step ks in 4 KS
//   registers during the whole sweep.  T is the A operand: tiles of 128 rows go through LDS (row pitch DP + 16 bytes; the
//   next tile is fetched into registers while this one is multiplied) and are shared by the four waves; lane l reads the
//   same bytes of train row l & 31 of a 32-row subtile.  Both operands take their K elements the same way, so whatever
//   the instruction's K order is, the products pair up.  The accumulator (C/D: column = lane & 31, row = (reg & 3) +
//   8 (reg >> 2) + 4 (lane >> 5)) gives a lane 16 train rows of its own query.  Each becomes one int32 key, d2 * 128 + the
//   row in the tile (d2 < 2^24, so the key is below 2^31 and orders as (d2, row) does); a lane keeps the two smallest keys
//   of a tile with a max and two mins per value, no branch, and pushes them into its running best two at the end of the
//   tile.  The two lane halves are combined once, at the end.
//
//   k_match_f32, 128 threads, one query each, T in tiles of 32 rows and 32 elements through LDS: d2 accumulated in
//   float32 in element order k = 0 .. D - 1 as s = s + (q_k - t_k) * (q_k - t_k), every operation rounded (explicit
//   round-to-nearest intrinsics; the library is built with -ffp-contract=off besides).  tests/matcher_restated.py
//   restates it in NumPy bit for bit.  The float32-input MFMA is not used: its summation order cannot be restated.
//
//   Both keep the running best two in four registers (mt_push), write them to idx / d2 when T is one range, and to a
//   partial [range][n_q] otherwise, which k_match_merge folds with the same mt_push.  The n_q x n_t distances never reach
//   memory.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <new>

#include "../../include/glimpse_hip.h"
#include "glh_match.h"
#include "glh_stage.h"

namespace glh {
namespace {

constexpr int MT_QB = 128;      // queries per workgroup, both paths
constexpr int MT_TI = 128;      // train rows per LDS tile, integer path
constexpr int MT_TF = 32;       // train rows per LDS tile, float path
constexpr int MT_KF = 32;       // elements per LDS tile, float path
constexpr int MT_KFP = MT_KF + 4;  // its row pitch in floats
constexpr int MT_WGS = 1024;    // workgroups wanted before T stops being split (4 per CU)
constexpr int MT_NONE = INT_MAX;  // the index of "no neighbour yet"; also the int32 key of "no row"
static_assert(MT_TI == 128, "k_match_i8 packs the row in the tile into the low 7 bits of a key");

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;

struct __attribute__((aligned(16))) Best2 {
  float d0, d1;
  int i0, i1;
};

__device__ __forceinline__ Best2 mt_empty() { return Best2{INFINITY, INFINITY, MT_NONE, MT_NONE}; }

// (d, i) before (bd, bi) in the key order
__device__ __forceinline__ bool mt_less(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// The best two of b and the candidate (d, i).  A NaN distance is never taken; (inf, MT_NONE) changes nothing.
__device__ __forceinline__ void mt_push(Best2& b, float d, int i) {
  if (!mt_less(d, i, b.d1, b.i1)) return;
  if (mt_less(d, i, b.d0, b.i0)) {
    b.d1 = b.d0, b.i1 = b.i0;
    b.d0 = d, b.i0 = i;
  } else {
    b.d1 = d, b.i1 = i;
  }
}

__device__ __forceinline__ void mt_write(const Best2& b, int q, int32_t* __restrict__ idx, float* __restrict__ d2) {
  idx[2 * (size_t)q] = b.i0 == MT_NONE ? -1 : b.i0;
  idx[2 * (size_t)q + 1] = b.i1 == MT_NONE ? -1 : b.i1;
  d2[2 * (size_t)q] = b.d0;
  d2[2 * (size_t)q + 1] = b.d1;
}

// One wave per row: x - 128 into the padded int8 row, and the row's squared norm.
__global__ void __launch_bounds__(64) k_match_prep_u8(const uint8_t* __restrict__ x, int n, int dim, int dp,
                                                      int8_t* __restrict__ y, int32_t* __restrict__ norm) {
  const int row = blockIdx.x;
  if (row >= n) return;
  int s = 0;
  for (int k = threadIdx.x; k < dp; k += 64) {
    const int v = k < dim ? (int)x[(size_t)row * dim + k] - 128 : 0;
    y[(size_t)row * dp + k] = (int8_t)v;
    s += v * v;
  }
  for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) norm[row] = s;
}

__global__ void __launch_bounds__(256) k_match_prep_f32(const float* __restrict__ x, int n, int dim, int dp,
                                                        float* __restrict__ y) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n * dp) return;
  const size_t row = i / dp;
  const int k = (int)(i % dp);
  y[i] = k < dim ? x[row * dim + k] : 0.f;
}

// grid (ceil(n_q / 128), ranges).  Range y takes T tiles y tiles_per_range .. of n_tiles.  partial == nullptr: one range,
// the result goes to idx / d2.
template <int KS>
__global__ void __launch_bounds__(256) k_match_i8(const int8_t* __restrict__ Q, const int32_t* __restrict__ qnorm, int n_q,
                                                  const int8_t* __restrict__ T, const int32_t* __restrict__ tnorm, int n_t,
                                                  int n_tiles, int tiles_per_range, Best2* __restrict__ partial,
                                                  int32_t* __restrict__ idx, float* __restrict__ d2) {
  constexpr int DP = 32 * KS, PITCH = DP + 16, CH = DP / 16;  // CH 16-byte pieces a row; 128 CH = 256 KS a tile
  __shared__ __attribute__((aligned(16))) int8_t s_t[MT_TI * PITCH];
  __shared__ __attribute__((aligned(16))) int32_t s_tk[MT_TI];  // |t|^2 * 128 + the row in the tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
  const int q = blockIdx.x * MT_QB + wave * 32 + c;
  const int qc = q < n_q ? q : n_q - 1;  // (a lane past the end works on the last query and writes nothing)
  i32x4 qf[KS];
  #pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const i32x4*>(Q + (size_t)qc * DP + 32 * ks + 16 * h);
  const int qn7 = qnorm[qc] << 7;
  const int tile0 = blockIdx.y * tiles_per_range;
  const int tile1 = tile0 + tiles_per_range < n_tiles ? tile0 + tiles_per_range : n_tiles;
  Best2 b = mt_empty();
  i32x4 pre[KS];
  int pre_n = 0;
  auto fetch = [&](int tile) {
    #pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int piece = tid + 256 * j, t = tile * MT_TI + piece / CH;
      pre[j] = t < n_t ? *reinterpret_cast<const i32x4*>(T + (size_t)t * DP + 16 * (piece % CH)) : i32x4{0, 0, 0, 0};
    }
    if (tid < MT_TI) pre_n = tile * MT_TI + tid < n_t ? tnorm[tile * MT_TI + tid] : 0;
  };
  if (tile0 < tile1) fetch(tile0);
  for (int tile = tile0; tile < tile1; ++tile) {
    __syncthreads();  // the tile before has been read
    #pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int piece = tid + 256 * j;
      *reinterpret_cast<i32x4*>(s_t + (piece / CH) * PITCH + 16 * (piece % CH)) = pre[j];
    }
    if (tid < MT_TI) s_tk[tid] = (pre_n << 7) | tid;
    __syncthreads();
    if (tile + 1 < tile1) fetch(tile + 1);
    int k0 = MT_NONE, k1 = MT_NONE;
    for (int sub = 0; sub < MT_TI / 32; ++sub) {
      const int t0 = tile * MT_TI + sub * 32;
      if (t0 >= n_t) break;
      i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const i32x4 a = *reinterpret_cast<const i32x4*>(s_t + (sub * 32 + c) * PITCH + 32 * ks + 16 * h);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[ks], acc, 0, 0, 0);
      }
      // key = d2 * 128 + the row in the tile, of the lane's 16 train rows: register 4 g + r is row 8 g + 4 h + r of the
      // subtile.  s_tk holds |t|^2 * 128 + row; -256 q.t is one 24-bit multiply-add (|q.t| <= 2^22).
      int key[16];
      #pragma unroll
      for (int g = 0; g < 4; ++g) {
        const i32x4 tk = *reinterpret_cast<const i32x4*>(s_tk + sub * 32 + 8 * g + 4 * h);
        #pragma unroll
        for (int r = 0; r < 4; ++r) key[4 * g + r] = __mul24(acc[4 * g + r], -256) + (tk[r] + qn7);
      }
      if (t0 + 32 > n_t)  // rows past the end of T
        #pragma unroll
        for (int g = 0; g < 4; ++g)
          #pragma unroll
          for (int r = 0; r < 4; ++r)
            if (t0 + 8 * g + 4 * h + r >= n_t) key[4 * g + r] = MT_NONE;
      #pragma unroll
      for (int r = 0; r < 16; ++r) {  // the tile's two smallest keys, k0 <= k1, without a branch
        const int up = key[r] > k0 ? key[r] : k0;
        k1 = up < k1 ? up : k1;
        k0 = key[r] < k0 ? key[r] : k0;
      }
    }
    // the tile's best two into the running best two (a later tile never wins a tie: its indices are higher)
    if (k0 != MT_NONE) mt_push(b, (float)(k0 >> 7), tile * MT_TI + (k0 & (MT_TI - 1)));
    if (k1 != MT_NONE) mt_push(b, (float)(k1 >> 7), tile * MT_TI + (k1 & (MT_TI - 1)));
  }
  Best2 o;  // the other lane half's best two of the same query
  o.d0 = __shfl_xor(b.d0, 32), o.d1 = __shfl_xor(b.d1, 32), o.i0 = __shfl_xor(b.i0, 32), o.i1 = __shfl_xor(b.i1, 32);
  mt_push(b, o.d0, o.i0);
  mt_push(b, o.d1, o.i1);
  if (h == 0 && q < n_q) {
    if (partial)
      partial[(size_t)blockIdx.y * n_q + q] = b;
    else
      mt_write(b, q, idx, d2);
  }
}

// grid (ceil(n_q / 128), ranges) as above; Q [n_q][dp], T [n_t][dp] floats, dp a multiple of 32.
__global__ void __launch_bounds__(MT_QB) k_match_f32(const float* __restrict__ Q, int n_q, const float* __restrict__ T,
                                                     int n_t, int dp, int n_tiles, int tiles_per_range,
                                                     Best2* __restrict__ partial, int32_t* __restrict__ idx,
                                                     float* __restrict__ d2) {
  __shared__ __attribute__((aligned(16))) float s_t[MT_TF * MT_KFP];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * MT_QB + tid;
  const int qc = q < n_q ? q : n_q - 1;
  const float* __restrict__ qrow = Q + (size_t)qc * dp;
  const int tile0 = blockIdx.y * tiles_per_range;
  const int tile1 = tile0 + tiles_per_range < n_tiles ? tile0 + tiles_per_range : n_tiles;
  Best2 b = mt_empty();
  for (int tile = tile0; tile < tile1; ++tile) {
    const int t0 = tile * MT_TF;
    float acc[MT_TF];
    #pragma unroll
    for (int t = 0; t < MT_TF; ++t) acc[t] = 0.f;
    for (int k0 = 0; k0 < dp; k0 += MT_KF) {
      __syncthreads();  // the piece before has been read
      for (int j = tid; j < MT_TF * MT_KF / 4; j += MT_QB) {
        const int row = j / (MT_KF / 4), c4 = j % (MT_KF / 4);
        const float4 v = t0 + row < n_t ? *reinterpret_cast<const float4*>(T + (size_t)(t0 + row) * dp + k0 + 4 * c4)
                                        : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(s_t + row * MT_KFP + 4 * c4) = v;
      }
      __syncthreads();
      #pragma unroll
      for (int k4 = 0; k4 < MT_KF / 4; ++k4) {
        const float4 qv = *reinterpret_cast<const float4*>(qrow + k0 + 4 * k4);
        #pragma unroll
        for (int t = 0; t < MT_TF; ++t) {
          const float4 tv = *reinterpret_cast<const float4*>(s_t + t * MT_KFP + 4 * k4);
          float s = acc[t], u;
          u = __fsub_rn(qv.x, tv.x), s = __fadd_rn(s, __fmul_rn(u, u));
          u = __fsub_rn(qv.y, tv.y), s = __fadd_rn(s, __fmul_rn(u, u));
          u = __fsub_rn(qv.z, tv.z), s = __fadd_rn(s, __fmul_rn(u, u));
          u = __fsub_rn(qv.w, tv.w), s = __fadd_rn(s, __fmul_rn(u, u));
          acc[t] = s;
        }
      }
    }
    #pragma unroll
    for (int t = 0; t < MT_TF; ++t)
      if (t0 + t < n_t) mt_push(b, acc[t], t0 + t);
  }
  if (q < n_q) {
    if (partial)
      partial[(size_t)blockIdx.y * n_q + q] = b;
    else
      mt_write(b, q, idx, d2);
  }
}

__global__ void __launch_bounds__(256) k_match_merge(const Best2* __restrict__ partial, int n_q, int ranges,
                                                     int32_t* __restrict__ idx, float* __restrict__ d2) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n_q) return;
  Best2 b = partial[q];
  for (int r = 1; r < ranges; ++r) {
    const Best2 o = partial[(size_t)r * n_q + q];
    mt_push(b, o.d0, o.i0);
    mt_push(b, o.d1, o.i1);
  }
  mt_write(b, q, idx, d2);
}

struct MatchSet {
  int kind = 0, n = 0, dim = 0, dp = 0;
  DevBuf data, norm;  // the prepared rows [n][dp]; u8: the squared norms [n]
  double upload_ms = 0.0, prepare_ms = 0.0;
};

}  // namespace
}  // namespace glh

struct glh_match : glh::DeviceObject {
  std::map<int, std::unique_ptr<glh::MatchSet>> sets;
  glh::GrowBuf partial, idx, d2;
  glh::StageEvents<4> ev;
};

namespace glh {

int match_create(int device, glh_match** out) {
  return create_object("match", device, out, [](glh_match* h) { return h->ev.create(); });
}

bool match_info(const glh_match* h, int slot, MatchSetInfo* info) {
  const auto it = h->sets.find(slot);
  if (it == h->sets.end()) return false;
  *info = MatchSetInfo{it->second->kind, it->second->n, it->second->dim};
  return true;
}

static int match_fill(glh_match* h, MatchSet* s, const void* data) {
  const size_t n = (size_t)s->n;
  DevBuf raw;
  hipStream_t st = h->stream;
  CHK(h->ev.record(0, st));
  CHK(raw.up(data, n * s->dim * (s->kind == GLH_MATCH_U8 ? 1 : 4)));
  CHK(h->ev.record(1, st));
  if (s->kind == GLH_MATCH_U8) {
    int ks = 1;
    while (32 * ks < s->dim) ks *= 2;
    s->dp = 32 * ks;
    CHK(s->data.alloc(n * s->dp));
    CHK(s->norm.alloc(n * 4));
    hipLaunchKernelGGL(k_match_prep_u8, dim3((unsigned)s->n), dim3(64), 0, st, raw.as<uint8_t>(), s->n, s->dim, s->dp,
                       s->data.as<int8_t>(), s->norm.as<int32_t>());
  } else {
    s->dp = (s->dim + MT_KF - 1) / MT_KF * MT_KF;
    CHK(s->data.alloc(n * s->dp * 4));
    hipLaunchKernelGGL(k_match_prep_f32, dim3((unsigned)((n * s->dp + 255) / 256)), dim3(256), 0, st, raw.as<float>(), s->n,
                       s->dim, s->dp, s->data.as<float>());
  }
  HIPCHK(hipGetLastError());
  CHK(h->ev.record(2, st));
  HIPCHK(hipEventSynchronize(h->ev.e[2]));  // (raw is freed with this scope)
  s->upload_ms = h->ev.ms(0, 1), s->prepare_ms = h->ev.ms(1, 2);
  return GLH_OK;
}

int match_put(glh_match* h, int slot, int kind, int n, int dim, const void* data) {
  CHK(h->use());
  std::unique_ptr<MatchSet> s(new (std::nothrow) MatchSet);
  if (!s) return fail(GLH_E_NOMEM, "match: no memory for a set");
  s->kind = kind, s->n = n, s->dim = dim;
  CHK(match_fill(h, s.get(), data));
  h->sets[slot] = std::move(s);  // (what the slot held before is freed)
  return GLH_OK;
}

void match_drop(glh_match* h, int slot) {
  (void)hipSetDevice(h->device);
  h->sets.erase(slot);
}

int match_knn2(glh_match* h, int slot_q, int slot_t, int32_t* idx, float* d2, double* times_ms) {
  const MatchSet& Q = *h->sets.at(slot_q);
  const MatchSet& T = *h->sets.at(slot_t);
  CHK(h->use());
  const bool u8 = Q.kind == GLH_MATCH_U8;
  const int tile_rows = u8 ? MT_TI : MT_TF;
  const int n_tiles = (T.n + tile_rows - 1) / tile_rows, q_blocks = (Q.n + MT_QB - 1) / MT_QB;
  int want = MT_WGS / q_blocks;
  want = want < 1 ? 1 : (want > n_tiles ? n_tiles : want);
  const int tiles_per_range = (n_tiles + want - 1) / want;
  const int ranges = (n_tiles + tiles_per_range - 1) / tiles_per_range;
  CHK(h->idx.reserve((size_t)Q.n * 8));
  CHK(h->d2.reserve((size_t)Q.n * 8));
  if (ranges > 1) CHK(h->partial.reserve((size_t)ranges * Q.n * sizeof(Best2)));
  Best2* partial = ranges > 1 ? h->partial.as<Best2>() : nullptr;
  int32_t* d_idx = h->idx.as<int32_t>();
  float* d_d2 = h->d2.as<float>();
  const dim3 grid((unsigned)q_blocks, (unsigned)ranges);
  hipStream_t st = h->stream;
  CHK(h->ev.record(0, st));
  if (u8) {
#define MT_LAUNCH(KS)                                                                                                \
  hipLaunchKernelGGL(k_match_i8<KS>, grid, dim3(256), 0, st, Q.data.as<int8_t>(), Q.norm.as<int32_t>(), Q.n,         \
                     T.data.as<int8_t>(), T.norm.as<int32_t>(), T.n, n_tiles, tiles_per_range, partial, d_idx, d_d2)
    switch (Q.dp / 32) {
      case 1: MT_LAUNCH(1); break;
      case 2: MT_LAUNCH(2); break;
      case 4: MT_LAUNCH(4); break;
      default: MT_LAUNCH(8); break;
    }
#undef MT_LAUNCH
  } else {
    hipLaunchKernelGGL(k_match_f32, grid, dim3(MT_QB), 0, st, Q.data.as<float>(), Q.n, T.data.as<float>(), T.n, Q.dp, n_tiles,
                       tiles_per_range, partial, d_idx, d_d2);
  }
  HIPCHK(hipGetLastError());
  CHK(h->ev.record(1, st));
  if (ranges > 1) {
    hipLaunchKernelGGL(k_match_merge, dim3((unsigned)((Q.n + 255) / 256)), dim3(256), 0, st, partial, Q.n, ranges, d_idx, d_d2);
    HIPCHK(hipGetLastError());
  }
  CHK(h->ev.record(2, st));
  CHK(h->idx.down(idx, (size_t)Q.n * 8));
  CHK(h->d2.down(d2, (size_t)Q.n * 8));
  CHK(h->ev.record(3, st));
  HIPCHK(hipEventSynchronize(h->ev.e[3]));
  if (times_ms) {
    times_ms[0] = Q.upload_ms + (slot_q == slot_t ? 0.0 : T.upload_ms);
    times_ms[1] = Q.prepare_ms + (slot_q == slot_t ? 0.0 : T.prepare_ms);
    for (int k = 0; k < 3; ++k) times_ms[2 + k] = h->ev.ms(k, k + 1);
    if (ranges == 1) times_ms[3] = 0.0;  // (no merge kernel ran: the span between two events is not its time)
  }
  return GLH_OK;
}

void match_destroy(glh_match* h) { destroy_object(h); }

}  // namespace glh
