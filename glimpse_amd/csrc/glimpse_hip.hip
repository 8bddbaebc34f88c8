// glimpse_hip.hip -- C ABI (include/glimpse_hip.h) over the kernels in glh_kernels.h.
// Host side: context, HBM residency, launches on one HIP stream, stage timers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/glimpse_hip.h"
#include "glh_comm.h"
#include "glh_host.h"
#include "glh_kernels.h"
#include "glh_point.h"
#include "glh_point_variants.h"
#include "glh_project_dem.h"
#include "glh_horizon.h"
#include "glh_calib.h"
#include "glh_ransac_draw.h"
#include "glh_ransac_plan.h"
#include "glh_match.h"
#include "glh_sift.h"
#include "glh_orient.h"
#include "glh_ortho.h"
#include "glh_raycast.h"
#include "glh_displace.h"
#include "glh_velocity.h"
#include "glh_velocity_plan.h"
#include "glh_regrid.h"
#include "glh_viewshed.h"
#include "glh_filters.h"
#include "glh_frame_ring.h"
#include "glh_clahe.h"
#include "glh_terrain.h"
#include "glh_stage.h"

using namespace glh;

// The fused kernel's instantiations live in their own translation units (glh_point_inst.hip, glh_point_variants.h).
namespace glh {
#define GLH_PT_DECL(TB, PPT, NOBS, S, F, C) const void* GLH_PT_NAME(TB, PPT, NOBS, S, F, C)();
#define GLH_PT_DECL_SHAPE(TB, PPT, NOBS) GLH_PT_CODES(GLH_PT_DECL, TB, PPT, NOBS)
GLH_PT_SHAPES(GLH_PT_DECL_SHAPE)
#undef GLH_PT_DECL_SHAPE
#undef GLH_PT_DECL
}  // namespace glh

static const void* pt_kernel(int tb, int ppt, int nobs, int surf, bool fast, bool con) {
#define GLH_PT_PICK(TB, PPT, NOBS, S, F, C) \
  if (tb == TB && ppt == PPT && nobs == NOBS && surf == S && fast == (bool)F && con == (bool)C) \
    return GLH_PT_NAME(TB, PPT, NOBS, S, F, C)();
#define GLH_PT_PICK_SHAPE(TB, PPT, NOBS) GLH_PT_CODES(GLH_PT_PICK, TB, PPT, NOBS)
  GLH_PT_SHAPES(GLH_PT_PICK_SHAPE)
#undef GLH_PT_PICK_SHAPE
#undef GLH_PT_PICK
  return nullptr;
}

// (every instantiation with its surface code: code 2 holds the raster windows in static LDS)
static std::vector<std::pair<const void*, int>> pt_all_kernels() {
  std::vector<std::pair<const void*, int>> v;
#define GLH_PT_PUSH(TB, PPT, NOBS, S, F, C) v.push_back({GLH_PT_NAME(TB, PPT, NOBS, S, F, C)(), S});
#define GLH_PT_PUSH_SHAPE(TB, PPT, NOBS) GLH_PT_CODES(GLH_PT_PUSH, TB, PPT, NOBS)
  GLH_PT_SHAPES(GLH_PT_PUSH_SHAPE)
#undef GLH_PT_PUSH_SHAPE
#undef GLH_PT_PUSH
  return v;
}

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int glh::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// ------------------------------------------------------------------------------------------
// stages (for the event timers)
// ------------------------------------------------------------------------------------------
enum Stage {
  ST_INIT = 0,
  ST_EVOLVE_PROJECT,
  ST_MOMENTS,
  ST_TEMPLATE,
  ST_TILEPREP,
  ST_SSD,
  ST_SPLINE_FIT,
  ST_WEIGHTS,
  ST_RESAMPLE,
  ST_POINT_STEP,
  ST_REPROJECT,  // (glh_stage_reproject: stateless, reports its own kernel time)
  ST_COUNT
};
static const char* kStageNames[ST_COUNT] = {"init_particles", "evolve_project", "moments",
                                            "template_init",  "tileprep",       "ssd",
                                            "spline_fit",     "weights",        "resample",
                                            "point_step",     "reproject"};

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct Observer {
  int n_images = 0, width = 0, height = 0, channels = 0;
  int bits = 8;  // bits per sample of the frames: 8 or 16 (unsigned integers), 32 (float32), 64 (float64): glh_observer_set_depth
  size_t frame_bytes() const { return (size_t)width * height * channels * (bits / 8); }
  double sigma = 0.3;
  DevArray<CamDev> cams;                // device [n_images]
  std::vector<CamDev> cams_host;        // same, for kernels that take the camera by value
  std::vector<const uint8_t*> frames;   // device pointers (owned or borrowed: a borrowed frame is never freed here)
  std::vector<DevArray<uint8_t>> owned; // owned allocations (same indexing; null if borrowed)
};

// Every member that holds device memory, pinned memory, a stream or an event owns it (glh_stage.h) and gives it back
// when the context is deleted.  Members go in reverse order of declaration: the streams come first, so they outlive
// every buffer and event that work enqueued on them uses.
struct glh_ctx {
  glh_config cfg{};
  Stream stream;
  Stream copy_stream;        // frame ingest; opened with upload_done on the first async or pinned upload (open_copy_stream)
  Stream extra_streams[3];   // streams 2 .. 4 of glh_track
  // frame ingest (glh_observer_upload_frame_async): the copy stream and a ring of pinned staging buffers
  static constexpr int NSTAGE = 4;
  PinnedBuf stage[NSTAGE];
  Event stage_done[NSTAGE];
  bool stage_busy[NSTAGE] = {false, false, false, false};
  int stage_next = 0;
  // uploads from caller-registered host memory (glh_observer_upload_frame_pinned): ticket t has event pin_ev[t % NPIN]
  static constexpr int NPIN = 64;
  Event pin_ev[NPIN];
  int64_t pin_next = 0, pin_completed = 0;  // tickets handed out; every ticket below pin_completed has finished
  Event upload_done;             // recorded on copy_stream after the latest upload
  bool uploads_pending = false;  // the compute stream has not yet been ordered after upload_done
  int P = 0, N = 0, tw = 0, th = 0, NB = 0;
  int cur = 0;  // current particle/weight buffer
  int frame = 0;
  bool have_mask = false, have_active = false, keep_sse = false, keep_idx = false, has_dem = false;
  int fused = 1;    // glh_step: 0 staged kernels, 1 fused per-point kernel, 2 fused with tiles forced to HBM (test)
  int pt_base = 0;  // global index of this context's point 0
  bool all_cartesian = true;  // every point is CartesianMotion (the common fused instantiation; else the general one)
  bool fast_math = false;     // GLH_MATH_FAST (glh_set_math)
  // A dem_sigma that the fast arithmetic's reciprocal cannot take (sigma_outside_fast_domain), noticed where it was set and
  // refused where fast arithmetic would use it (check_fast_domain): the constant of a point whose dem is a raster
  // (glh_set_motion; fast_bad_point -1: none), a node of the dem_sigma raster (glh_set_raster; 0: none) that a point uses
  int fast_bad_point = -1;
  double fast_bad_const = 0.0, fast_bad_node = 0.0;
  bool sigma_raster_used = false;
  int hp_rx = 2, hp_ry = 2;   // half sizes of the median high-pass window (glh_set_highpass; 5 x 5 by default)
  int tile_cap = 0, search_cap = 0, sse_cap = 0, ssd_blocks = 2;
  Observer obs[MAX_OBS];
  // device buffers
  DevArray<double> particles[2], weights[2];
  DevArray<double> motion, uv, bbox_part, normals, u;
  DevArray<double> mean6, moments;
  struct RasterBuf {
    DevArray<double> z, gx, gy;
    RasterDev dev{};
    std::vector<double> hgx, hgy;  // host copies of the coordinates (same_grid below)
  } rasters[3];  // GLH_RASTER_DEM, _DEM_SIGMA, _VIEWSHED
  bool same_grid = false;  // the dem and dem_sigma rasters have bit-identical coordinate arrays (Surfaces::same_grid)
  DevArray<double> covariances;  // [max_frames][P][36], allocated on first use
  DevArray<double> uj;           // [P][N] host-fed per-particle uniforms (stratified / choice)
  DevArray<double> extra_ll;     // [P][N] caller-computed log-likelihood term of the next glh_update_weights, or null
  bool have_extra = false;
  DevArray<uint8_t> obs_mask, active;
  DevArray<uint32_t> pt_status;
  DevArray<int32_t> pt_err_frame, box, idx;
  DevArray<int32_t> obs_status_all;  // [max_frames][O][P]: the per-(observer, point) status of every frame
  DevArray<int32_t> tmpl_box, tmpl_hist_n, tmpl_valid;
  DevArray<double> tmpl_duv, tmpl_tile64, tmpl_hist_v, tmpl_hist_q;
  DevArray<float> tmpl_tile32, search;
  DevArray<unsigned long long> stamps;  // phase stamps of the fused kernel (diagnostic)
  DevArray<uint16_t> uidx[2];  // [P][N] record of every particle in particles[b] / weights[b] when compact
  bool compact = false;  // particles[cur] / weights[cur] are run-length compact (left by the fused step)
  DevArray<int32_t> resid_draws;  // [P] uniforms consumed by the last residual resampling
  DevArray<uint32_t> bins16;    // [P][65535 * 3 + 1] key histograms of 16-bit frames (staged tile kernels), on first use
  DevArray<double> fwork;       // [P][2 D^2] tile workspace of float64 frames (staged tile kernels), on first use
  DevArray<double> tracks_tmp;  // means | sigmas in the caller's layout (glh_get_tracks), grown on use
  DevArray<uint16_t> ws_keys;   // raw-key workspace of the fused kernel for tiles that do not fit in LDS
  int keys_cap = 0;
  int plan_N = 0;  // the N the pairwise-sum plan on the device was made for (0: none)
  bool track_covariances = false;  // glh_track_covariances
  // glh_track on two streams (glh_set_track_streams): 0 = automatic (two when the batch is at least two rounds of
  // workgroups per half), 1 = always one, 2 = two whenever the fused step runs
  int track_streams = 0;
  Event ev_fork, ev_join[3];   // the extra streams start behind ev_fork; the context's stream ends behind ev_join
  int last_track_streams = 1;  // streams the last glh_track used
  int n_cus = 256;             // compute units of the device (hipDeviceProp: glh_create)
  // diagnostic (GLH_PT_STOP="stamp:frame", read by glh_create): the fused launches of that frame end at that phase stamp
  int stop_stamp = -1, stop_frame = -1;
  DevArray<double> sse, sse_copy, ll_dbg;
  DevArray<double> lu;
  DevArray<double> poly;
  DevArray<int64_t> lu_off;
  DevArray<double> spl_inv;  // explicit inverses of the collocation matrices, sides 4 .. GLH_SPL_DENSE_MAX
  DevArray<int32_t> leaf_off, leaf_len, sum_ops, level_off, roots;
  int nleaves = 0, nnodes = 0, nlevels = 0, nroots = 0;
  int moments_frame = -1;  // history slot already filled by the fused resample kernel
  int interp_k = 3;  // interpolation order of the surface sampling: 3 (bicubic, the default), 1 (bilinear), or 0: the
                     // general orders interp_kx (rows axis) / interp_ky (columns axis) (glh_set_interpolation)
  int interp_kx = 3, interp_ky = 3;
  DevArray<double> glu[2];       // general orders: spline_lu_general factors for degree kx / ky by size
  DevArray<int64_t> glu_off[2];  // [max_search_dim + 1]
  int32_t last_variant[4] = {0, 0, 0, 0};  // fused kernel instantiation of the last step: TB, PPT, NOBS, fast | general << 1
  // profiling: a timed launch takes its two events from the pool (StageTimer), leaves them in `pending`, and
  // drain_profile puts them back
  bool profiling = false;
  struct Ev {
    Event a, b;
    int stage;
  };
  std::vector<Ev> pending;
  std::vector<Event> pool;
  double ms[ST_COUNT] = {0};
  int64_t launches[ST_COUNT] = {0};
  std::vector<float> launch_ms[ST_COUNT];  // duration of every timed launch since the last reset (bounded)
  // GPU time a stage spans since the last reset: from the start of its first timed launch to the end of its last one,
  // on whichever stream (launches of glh_track's two streams overlap: their durations do not add up to it)
  Event span_a[ST_COUNT];
  float span_ms[ST_COUNT] = {0};
  // multi-GPU (glh_comm.h)
  Comm* comm = nullptr;
};

// status words [O][P] of the current frame
static int32_t* cur_status(const glh_ctx* c) {
  return c->obs_status_all + (size_t)c->frame * c->cfg.n_observers * c->P;
}

struct StageTimer {
  glh_ctx* c;
  int stage;
  Event a, b;
  hipStream_t s;
  StageTimer(glh_ctx* ctx, int st, hipStream_t on = nullptr) : c(ctx), stage(st), s(on ? on : ctx->stream.get()) {
    c->launches[st]++;
    if (!c->profiling) return;
    auto get = [&]() {
      Event e;
      if (!c->pool.empty()) {
        e = std::move(c->pool.back());
        c->pool.pop_back();
      } else {
        (void)e.create();
      }
      return e;
    };
    a = get();
    b = get();
    (void)hipEventRecord(a, s);
  }
  ~StageTimer() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    c->pending.push_back({std::move(a), std::move(b), stage});
  }
};

static int drain_profile(glh_ctx* c) {
  if (c->pending.empty()) return GLH_OK;
  HIPCHK(hipStreamSynchronize(c->stream));
  for (auto& e : c->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      c->ms[e.stage] += ms;
      if (c->launch_ms[e.stage].size() < (1u << 16)) c->launch_ms[e.stage].push_back(ms);
    }
    Event& first = c->span_a[e.stage];
    if (!first) first = std::move(e.a);  // (kept until the next reset)
    float t = 0.f;
    if (hipEventElapsedTime(&t, first, e.b) == hipSuccess && t > c->span_ms[e.stage]) c->span_ms[e.stage] = t;
    if (e.a) c->pool.push_back(std::move(e.a));
    if (e.b) c->pool.push_back(std::move(e.b));  // (null when the timer could not create it)
  }
  c->pending.clear();
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// library / context
// ------------------------------------------------------------------------------------------
extern "C" int glh_version(void) { return GLH_VERSION; }
extern "C" const char* glh_last_error(void) { return g_err.c_str(); }
extern "C" int glh_stage_count(void) { return ST_COUNT; }
extern "C" const char* glh_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }

extern "C" int glh_device_count(int* count) {
  if (!count) return fail(GLH_E_INVALID, "count is null");
  HIPCHK(hipGetDeviceCount(count));
  return GLH_OK;
}

extern "C" int glh_device_memory(int device_id, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!free_bytes || !total_bytes) return fail(GLH_E_INVALID, "null argument");
  HIPCHK(hipSetDevice(device_id));
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  *free_bytes = (uint64_t)f;
  *total_bytes = (uint64_t)t;
  return GLH_OK;
}

extern "C" int glh_device_compute_units(int device_id, int* count) {
  if (!count) return fail(GLH_E_INVALID, "count is null");
  HIPCHK(hipDeviceGetAttribute(count, hipDeviceAttributeMultiprocessorCount, device_id));
  return GLH_OK;
}

// What is left to say once the members free themselves: nothing may still run on the streams when they go.
extern "C" int glh_destroy(glh_ctx* c) {
  if (!c) return GLH_OK;
  (void)hipSetDevice(c->cfg.device_id);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  for (const Stream& s : c->extra_streams)
    if (s) (void)hipStreamSynchronize(s);
  if (c->comm) (void)glh_comm_destroy(c);
  delete c;
  return GLH_OK;
}
struct CtxDestroy {
  void operator()(glh_ctx* c) const { (void)glh_destroy(c); }
};

extern "C" int glh_create(const glh_config* cfg, glh_ctx** out) {
  if (!cfg || !out) return fail(GLH_E_INVALID, "null argument");
  *out = nullptr;
  glh_config k = *cfg;
  if (k.max_tile <= 0) k.max_tile = 31;
  if (k.max_search_dim <= 0) k.max_search_dim = 320;
  if (k.max_frames <= 0) k.max_frames = 128;
  if (k.max_points <= 0 || k.max_particles <= 0 || k.n_observers <= 0 || k.n_observers > MAX_OBS)
    return fail(GLH_E_INVALID, "max_points/max_particles must be > 0 and 1 <= n_observers <= %d", MAX_OBS);
  if (k.max_points > 65535)  // the staged kernels put the point index in gridDim.y
    return fail(GLH_E_UNSUPPORTED, "max_points %d exceeds 65535 points per context: shard the points", k.max_points);
  if (k.max_tile < 5 || k.max_tile > 127) return fail(GLH_E_INVALID, "max_tile must be in [5, 127]");
  if (k.max_search_dim < k.max_tile + 3 || k.max_search_dim > 2000)
    return fail(GLH_E_INVALID, "max_search_dim must be in [max_tile + 3, 2000]");
  if ((size_t)k.max_particles * 10 + 4096 > 150 * 1024)
    return fail(GLH_E_UNSUPPORTED, "max_particles %d exceeds the LDS-resident scan (<= 14900)", k.max_particles);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (k.device_id < 0 || k.device_id >= ndev)
    return fail(GLH_E_INVALID, "device_id %d out of range (%d devices)", k.device_id, ndev);
  HIPCHK(hipSetDevice(k.device_id));
  // (a return below destroys the context with what it has so far; glh_destroy leaves glh_last_error() alone)
  Owned<glh_ctx*, CtxDestroy> made(new (std::nothrow) glh_ctx());
  glh_ctx* c = made.get();
  if (!c) return fail(GLH_E_NOMEM, "out of host memory");
  c->cfg = k;
  {
    int cus = 0;  // (what decides whether a batch is two rounds of workgroups per half: glh_track's two streams)
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k.device_id) == hipSuccess && cus > 0) c->n_cus = cus;
  }
  if (const char* stop = getenv("GLH_PT_STOP")) {  // (tools/phase_counts.sh: one process per setting)
    int s = -1, f = -1;
    if (sscanf(stop, "%d:%d", &s, &f) == 2) {
      c->stop_stamp = s;
      c->stop_frame = f;
    }
  }
  const size_t P = k.max_points, N = k.max_particles, O = k.n_observers;
  c->tile_cap = k.max_tile * k.max_tile;
  c->search_cap = k.max_search_dim * (k.max_search_dim + 16);  // rows padded for the fused kernel
  c->keys_cap = pt_keys_count(k.max_search_dim, k.max_search_dim);  // with the reflected border
  c->sse_cap = c->search_cap;
  const size_t NBmax = (N + BLK - 1) / BLK;
  CHK(c->stream.create());
  for (int i = 0; i < 2; ++i) {
    CHK(c->particles[i].alloc(P * N * 6));
    CHK(c->weights[i].alloc(P * N));
  }
  CHK(c->motion.alloc(P * GLH_MOTION_FULL_LEN));
  CHK(c->uv.alloc(O * P * N * 2));
  CHK(c->bbox_part.alloc(O * P * NBmax * 5));
  CHK(c->u.alloc(P));
  CHK(c->mean6.alloc(P * 6));
  CHK(c->moments.alloc((size_t)k.max_frames * P * 12));
  CHK(c->obs_mask.alloc(P * O));
  CHK(c->active.alloc(P));
  CHK(c->pt_status.alloc(P));
  CHK(c->pt_err_frame.alloc(P));
  CHK(c->obs_status_all.alloc((size_t)k.max_frames * O * P));
  CHK(c->box.alloc(O * P * 4));
  CHK(c->tmpl_box.alloc(O * P * 4));
  CHK(c->tmpl_hist_n.alloc(O * P));
  CHK(c->tmpl_valid.alloc(O * P));
  CHK(c->tmpl_duv.alloc(O * P * 2));
  CHK(c->tmpl_tile64.alloc(O * P * c->tile_cap));
  CHK(c->tmpl_tile32.alloc(O * P * c->tile_cap));
  CHK(c->tmpl_hist_v.alloc(O * P * c->tile_cap));
  CHK(c->tmpl_hist_q.alloc(O * P * c->tile_cap));
  CHK(c->search.alloc(O * P * (size_t)c->search_cap));
  CHK(c->ws_keys.alloc(O * P * (size_t)c->keys_cap));
  CHK(c->sse.alloc(O * P * (size_t)c->sse_cap));
  {  // spline LU table for every surface side 4..max_search_dim
    const int maxn = k.max_search_dim;
    std::vector<int64_t> off(maxn + 1, 0);
    int64_t total = 0;
    for (int n = 4; n <= maxn; ++n) {
      off[n] = total;
      total += 5 * (int64_t)n;
    }
    std::vector<double> lu((size_t)total);
    for (int n = 4; n <= maxn; ++n) spline_lu(n, lu.data() + off[n]);
    CHK(c->lu.alloc((size_t)total));
    CHK(c->lu_off.alloc((size_t)maxn + 1));
    if (hipMemcpy(c->lu, lu.data(), total * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->lu_off, off.data(), (maxn + 1) * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
      return fail(GLH_E_HIP, "upload of the spline LU table failed");
  }
  {
    std::vector<double> inv((size_t)spline_inverse_off(GLH_SPL_DENSE_MAX + 1));
    for (int n = 4; n <= GLH_SPL_DENSE_MAX; ++n) spline_inverse(n, inv.data() + spline_inverse_off(n));
    CHK(c->spl_inv.alloc(inv.size()));
    if (hipMemcpy(c->spl_inv, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      return fail(GLH_E_HIP, "upload of the spline inverse table failed");
  }
  {
    std::vector<double> tab(16 * GLH_NPOLY);
    basis_poly_table(tab.data());
    CHK(c->poly.alloc(tab.size()));
    if (hipMemcpy(c->poly, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
      return fail(GLH_E_HIP, "upload of the spline basis table failed");
  }
  {
    // kernels that may use more than the default 64 KB of dynamic LDS
    hipError_t e1 = hipFuncSetAttribute((const void*)k_resample, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024);
    hipError_t e2 = hipFuncSetAttribute((const void*)k_ssd, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    hipError_t e3 = hipFuncSetAttribute((const void*)k_tileprep, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    hipError_t e4 = hipSuccess;
    for (const auto& f : pt_all_kernels()) {
      hipError_t e = hipFuncSetAttribute(f.first, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         PT_LDS_MAX - (f.second == 2 ? PT_PATCH_LDS : 0));
      if (e != hipSuccess) e4 = e;
    }
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess)
      return fail(GLH_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  }
  *out = made.release();
  return GLH_OK;
}

// Order the compute stream after the frame uploads enqueued so far (no host wait).
static int join_uploads(glh_ctx* c) {
  if (c->uploads_pending) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->upload_done, 0));
    c->uploads_pending = false;
  }
  return GLH_OK;
}

extern "C" int glh_sync(glh_ctx* c) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  CHK(join_uploads(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

extern "C" int glh_get_stream(glh_ctx* c, void** stream) {
  if (!c || !stream) return fail(GLH_E_INVALID, "null argument");
  *stream = (void*)c->stream;
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// observers
// ------------------------------------------------------------------------------------------
static int check_obs(glh_ctx* c, int o) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (o < 0 || o >= c->cfg.n_observers) return fail(GLH_E_INVALID, "observer %d out of range", o);
  return GLH_OK;
}

extern "C" int glh_observer_init(glh_ctx* c, int o, int n_images, int width, int height, int channels,
                                 double sigma) {
  CHK(check_obs(c, o));
  if (n_images <= 0 || width <= 0 || height <= 0) return fail(GLH_E_INVALID, "bad observer geometry");
  if (channels != 1 && channels != 3)
    return fail(GLH_E_UNSUPPORTED, "frames must be uint8 with 1 or 3 channels (got %d)", channels);
  if (!(sigma > 0.0)) return fail(GLH_E_INVALID, "sigma must be > 0");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  Observer& ob = c->obs[o];
  ob.cams.reset();
  ob.owned.clear();  // (frees the frames of an earlier init)
  ob.n_images = n_images;
  ob.width = width;
  ob.height = height;
  ob.channels = channels;
  ob.bits = 8;
  ob.sigma = sigma;
  ob.frames.assign(n_images, nullptr);
  ob.owned.resize(n_images);
  CHK(ob.cams.alloc((size_t)n_images));
  return GLH_OK;
}

extern "C" int glh_observer_set_depth(glh_ctx* c, int o, int bits) {
  CHK(check_obs(c, o));
  if (bits != 8 && bits != 16 && bits != 32 && bits != 64)
    return fail(GLH_E_UNSUPPORTED, "frames are 8 or 16 bits per sample (unsigned), 32 = float32 or 64 = float64 samples "
                                   "(got %d)", bits);
  Observer& ob = c->obs[o];
  if (ob.n_images <= 0) return fail(GLH_E_STATE, "glh_observer_init first");
  if (bits >= 32 && ob.channels != 1 && ob.channels != 3)
    return fail(GLH_E_UNSUPPORTED, "float frames have one or three channels (observer %d has %d)", o, ob.channels);
  for (auto& p : ob.owned)
    if (p) return fail(GLH_E_STATE, "observer %d: set the depth before uploading frames", o);
  // what the wider tile kernels are sized for (their LDS requests grow with the context's limits)
  if (bits == 16 && (size_t)(BAND_H + 6) * c->cfg.max_search_dim * 4 > 96 * 1024)
    return fail(GLH_E_UNSUPPORTED, "16-bit frames: max_search_dim %d exceeds %d (one median band must fit 96 KiB of LDS)",
                c->cfg.max_search_dim, (int)(96 * 1024 / ((BAND_H + 6) * 4)));
  if (bits >= 32 && (size_t)c->cfg.max_tile * c->cfg.max_tile * 12 > 64 * 1024)
    return fail(GLH_E_UNSUPPORTED, "float frames: max_tile %d exceeds 73 (template workspace of 64 KiB of LDS)",
                c->cfg.max_tile);
  ob.bits = bits;
  return GLH_OK;
}

extern "C" int glh_observer_set_cameras(glh_ctx* c, int o, int first, int n, const double* cams) {
  CHK(check_obs(c, o));
  Observer& ob = c->obs[o];
  if (!cams || first < 0 || n <= 0 || first + n > ob.n_images)
    return fail(GLH_E_INVALID, "camera range [%d, %d) outside the observer's %d images", first, first + n, ob.n_images);
  std::vector<CamDev> tmp(n);
  for (int i = 0; i < n; ++i) {
    expand_camera(cams + (size_t)i * GLH_CAM_LEN, &tmp[i]);
    if ((int)tmp[i].imgsz[0] != ob.width || (int)tmp[i].imgsz[1] != ob.height)
      return fail(GLH_E_INVALID, "camera imgsz (%g, %g) != frame size (%d, %d): resized reads are out of scope",
                  tmp[i].imgsz[0], tmp[i].imgsz[1], ob.width, ob.height);
  }
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if ((int)ob.cams_host.size() != ob.n_images) ob.cams_host.resize(ob.n_images);
  for (int i = 0; i < n; ++i) ob.cams_host[first + i] = tmp[i];
  HIPCHK(hipMemcpyAsync(ob.cams + first, tmp.data(), n * sizeof(CamDev), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

extern "C" int glh_observer_upload_frame(glh_ctx* c, int o, int image, const uint8_t* pixels) {
  CHK(check_obs(c, o));
  Observer& ob = c->obs[o];
  if (!pixels || image < 0 || image >= ob.n_images) return fail(GLH_E_INVALID, "bad frame index %d", image);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  size_t bytes = ob.frame_bytes();
  if (!ob.owned[image]) CHK(ob.owned[image].alloc(bytes));
  HIPCHK(hipMemcpyAsync(ob.owned[image], pixels, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  ob.frames[image] = ob.owned[image];
  return GLH_OK;
}

// The copy stream and the event that marks its latest upload come together, on the first async or pinned upload: a
// failure between the two leaves neither behind.
static int open_copy_stream(glh_ctx* c) {
  if (c->copy_stream) return GLH_OK;
  Stream s;
  Event done;
  CHK(s.create());
  CHK(done.create(hipEventDisableTiming));
  c->copy_stream = std::move(s);
  c->upload_done = std::move(done);
  return GLH_OK;
}

// The same upload without waiting for the device: `pixels` is copied into a pinned staging buffer before the call
// returns (the caller may reuse it at once), the host-to-device copy runs on a copy stream, and the next call that
// reads frames is ordered after it on the device.  A decoder pool can so keep the PCIe link busy while it decodes.
extern "C" int glh_observer_upload_frame_async(glh_ctx* c, int o, int image, const uint8_t* pixels) {
  CHK(check_obs(c, o));
  Observer& ob = c->obs[o];
  if (!pixels || image < 0 || image >= ob.n_images) return fail(GLH_E_INVALID, "bad frame index %d", image);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const size_t bytes = ob.frame_bytes();
  CHK(open_copy_stream(c));
  const int k = c->stage_next;
  c->stage_next = (k + 1) % glh_ctx::NSTAGE;
  if (c->stage_busy[k]) {  // the copy that last used this slot has to be over before it is overwritten
    HIPCHK(hipEventSynchronize(c->stage_done[k]));
    c->stage_busy[k] = false;
  }
  CHK(c->stage[k].reserve(bytes));
  if (!c->stage_done[k]) CHK(c->stage_done[k].create(hipEventDisableTiming));
  memcpy(c->stage[k].get(), pixels, bytes);
  if (!ob.owned[image]) CHK(ob.owned[image].alloc(bytes));
  HIPCHK(hipMemcpyAsync(ob.owned[image], c->stage[k].get(), bytes, hipMemcpyHostToDevice, c->copy_stream));
  HIPCHK(hipEventRecord(c->stage_done[k], c->copy_stream));
  HIPCHK(hipEventRecord(c->upload_done, c->copy_stream));
  c->stage_busy[k] = true;
  c->uploads_pending = true;
  ob.frames[image] = ob.owned[image];
  return GLH_OK;
}

extern "C" int glh_host_register(void* ptr, uint64_t bytes) {
  if (!ptr || bytes == 0) return fail(GLH_E_INVALID, "null buffer");
  HIPCHK(hipHostRegister(ptr, (size_t)bytes, hipHostRegisterPortable));  // (for every device of the process)
  return GLH_OK;
}

extern "C" int glh_host_unregister(void* ptr) {
  if (!ptr) return fail(GLH_E_INVALID, "null buffer");
  HIPCHK(hipHostUnregister(ptr));
  return GLH_OK;
}

// advance pin_completed over every ticket whose event has passed (in order: the copy stream runs them in order)
static int pin_poll(glh_ctx* c, int64_t wait_for) {
  while (c->pin_completed < c->pin_next) {
    hipEvent_t e = c->pin_ev[c->pin_completed % glh_ctx::NPIN];
    if (c->pin_completed <= wait_for) {
      HIPCHK(hipEventSynchronize(e));
    } else {
      const hipError_t q = hipEventQuery(e);
      if (q == hipErrorNotReady) break;
      HIPCHK(q);
    }
    ++c->pin_completed;
  }
  return GLH_OK;
}

extern "C" int glh_observer_upload_frame_pinned(glh_ctx* c, int o, int image, const uint8_t* pixels, int64_t* ticket) {
  CHK(check_obs(c, o));
  Observer& ob = c->obs[o];
  if (!pixels || !ticket || image < 0 || image >= ob.n_images) return fail(GLH_E_INVALID, "bad frame index %d", image);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const size_t bytes = ob.frame_bytes();
  CHK(open_copy_stream(c));
  const int64_t t = c->pin_next;
  if (t - c->pin_completed >= glh_ctx::NPIN) CHK(pin_poll(c, t - glh_ctx::NPIN));  // (its event is about to be reused)
  Event& e = c->pin_ev[t % glh_ctx::NPIN];
  if (!e) CHK(e.create(hipEventDisableTiming));
  if (!ob.owned[image]) CHK(ob.owned[image].alloc(bytes));
  HIPCHK(hipMemcpyAsync(ob.owned[image], pixels, bytes, hipMemcpyHostToDevice, c->copy_stream));
  HIPCHK(hipEventRecord(e, c->copy_stream));
  HIPCHK(hipEventRecord(c->upload_done, c->copy_stream));
  c->pin_next = t + 1;
  c->uploads_pending = true;
  ob.frames[image] = ob.owned[image];
  *ticket = t;
  return GLH_OK;
}

extern "C" int glh_upload_done(glh_ctx* c, int64_t ticket, int wait, int* done) {
  if (!c || !done) return fail(GLH_E_INVALID, "null argument");
  if (ticket < 0 || ticket >= c->pin_next) return fail(GLH_E_INVALID, "unknown upload ticket %lld", (long long)ticket);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  CHK(pin_poll(c, wait ? ticket : -1));
  *done = ticket < c->pin_completed ? 1 : 0;
  return GLH_OK;
}

extern "C" int glh_observer_set_frame_device(glh_ctx* c, int o, int image, const void* dev) {
  CHK(check_obs(c, o));
  Observer& ob = c->obs[o];
  if (!dev || image < 0 || image >= ob.n_images) return fail(GLH_E_INVALID, "bad frame index %d", image);
  ob.owned[image].reset();  // (the caller's memory is borrowed: `owned` stays null and nothing here frees it)
  ob.frames[image] = (const uint8_t*)dev;
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// sequence state
// ------------------------------------------------------------------------------------------
extern "C" int glh_begin_sequence(glh_ctx* c, int P, int N, int tw, int th) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (P <= 0 || P > c->cfg.max_points || N <= 0 || N > c->cfg.max_particles)
    return fail(GLH_E_INVALID, "n_points %d / n_particles %d exceed the context capacity (%d, %d)", P, N,
                c->cfg.max_points, c->cfg.max_particles);
  if (tw < 5 || th < 5 || tw > c->cfg.max_tile || th > c->cfg.max_tile)
    return fail(GLH_E_INVALID, "tile_size (%d, %d) must be in [5, max_tile=%d]", tw, th, c->cfg.max_tile);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  c->P = P;
  c->N = N;
  c->tw = tw;
  c->th = th;
  c->NB = (N + BLK - 1) / BLK;
  c->cur = 0;
  c->compact = false;
  c->frame = 0;
  c->have_mask = c->have_active = false;
  c->pt_base = 0;
  const size_t O = c->cfg.n_observers;
  HIPCHK(hipMemsetAsync(c->pt_status, 0, P * sizeof(uint32_t), c->stream));
  HIPCHK(hipMemsetAsync(c->pt_err_frame, 0x7f, P * sizeof(int32_t), c->stream));
  HIPCHK(hipMemsetAsync(c->tmpl_valid, 0, O * P * sizeof(int32_t), c->stream));
  // (the fused kernel fetches a template's CDF length before it knows the template is valid: never garbage)
  HIPCHK(hipMemsetAsync(c->tmpl_hist_n, 0, O * P * sizeof(int32_t), c->stream));
  {
    // GLH_OBS_SKIPPED everywhere, for every frame
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)c->obs_status_all, GLH_OBS_SKIPPED, (size_t)c->cfg.max_frames * O * P,
                             c->stream));
  }
  size_t nm = (size_t)c->cfg.max_frames * P * 12;
  hipLaunchKernelGGL(k_fill_f64, dim3(256), dim3(256), 0, c->stream, c->moments, nm, (double)NAN);
  HIPCHK(hipGetLastError());
  if (c->covariances) {  // a reused context must not return the previous sequence's covariances
    hipLaunchKernelGGL(k_fill_f64, dim3(256), dim3(256), 0, c->stream, c->covariances,
                       (size_t)c->cfg.max_frames * c->cfg.max_points * 36, (double)NAN);
    HIPCHK(hipGetLastError());
  }
  // NumPy pairwise-sum plan for this N (kept from the last sequence when N is the same: five frees, allocations and
  // blocking copies -- ~10 ms -- that a tracker reusing its context for the next run does not pay again)
  if (c->plan_N != N) {
    PairwisePlan pl;
    pairwise_plan(N, pl);
    c->plan_N = 0;  // (no plan while its arrays are replaced: a failure half way leaves none marked valid)
    CHK(c->leaf_off.alloc(pl.leaf_off.size()));
    CHK(c->leaf_len.alloc(pl.leaf_len.size()));
    CHK(c->sum_ops.alloc(pl.ops.size()));
    CHK(c->level_off.alloc(pl.level_off.size()));
    CHK(c->roots.alloc(pl.roots.size()));
    HIPCHK(hipMemcpy(c->leaf_off, pl.leaf_off.data(), pl.leaf_off.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->leaf_len, pl.leaf_len.data(), pl.leaf_len.size() * 4, hipMemcpyHostToDevice));
    if (!pl.ops.empty()) HIPCHK(hipMemcpy(c->sum_ops, pl.ops.data(), pl.ops.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->level_off, pl.level_off.data(), pl.level_off.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->roots, pl.roots.data(), pl.roots.size() * 4, hipMemcpyHostToDevice));
    c->nleaves = (int)pl.leaf_off.size();
    c->nnodes = pl.nnodes;
    c->nlevels = (int)pl.level_off.size() - 1;
    c->nroots = (int)pl.roots.size();
    c->plan_N = N;
  }
  c->moments_frame = -1;
  return GLH_OK;
}

extern "C" int glh_set_frame(glh_ctx* c, int frame) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (frame < 0 || frame >= c->cfg.max_frames) return fail(GLH_E_INVALID, "frame %d outside [0, max_frames)", frame);
  c->frame = frame;
  return GLH_OK;
}

static int need_seq(glh_ctx* c) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (c->P <= 0) return fail(GLH_E_STATE, "glh_begin_sequence has not been called");
  return GLH_OK;
}

// The fused step leaves the state run-length compact; everything else works on one record per particle.
static int ensure_expanded(glh_ctx* c) {
  if (!c->compact) return GLH_OK;
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const dim3 grid((c->N + BLK - 1) / BLK, c->P);
  hipLaunchKernelGGL(k_expand_state, grid, dim3(BLK), 0, c->stream, c->particles[c->cur], c->weights[c->cur],
                     c->uidx[c->cur], c->particles[c->cur ^ 1], c->weights[c->cur ^ 1], c->N);
  HIPCHK(hipGetLastError());
  c->cur ^= 1;
  c->compact = false;
  return GLH_OK;
}

#define UPLOAD(dst, src, count, type)                                                                 \
  do {                                                                                                \
    HIPCHK(hipSetDevice(c->cfg.device_id));                                                           \
    HIPCHK(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(type), hipMemcpyHostToDevice, c->stream)); \
    HIPCHK(hipStreamSynchronize(c->stream));                                                          \
  } while (0)
#define DOWNLOAD(dst, src, count, type)                                                               \
  do {                                                                                                \
    HIPCHK(hipSetDevice(c->cfg.device_id));                                                           \
    HIPCHK(hipMemcpyAsync((dst), (src), (size_t)(count) * sizeof(type), hipMemcpyDeviceToHost, c->stream)); \
    HIPCHK(hipStreamSynchronize(c->stream));                                                          \
  } while (0)

// Fast arithmetic (glh_set_math): every kernel has it.  In the general instantiation (gridded surfaces, the other motion
// models) it changes the projection, the sampling, the weights and the resampling, and (round 5) the surface lookups of
// the evolve step and of the DEM term (glh_math.h: raster_bilinear_fast) and the tangent models' step.
static bool use_fast(const glh_ctx* c) { return c->fast_math; }

static Surfaces surfaces(const glh_ctx* c) {
  Surfaces s{};
  s.dem = c->rasters[GLH_RASTER_DEM].dev;
  s.dem_sigma = c->rasters[GLH_RASTER_DEM_SIGMA].dev;
  s.viewshed = c->rasters[GLH_RASTER_VIEWSHED].dev;
  s.same_grid = c->same_grid ? 1 : 0;
  return s;
}

static int check_raster_args(int nx, int ny, const double* gx, const double* gy, int sx, int sy) {
  if (nx < 2 || ny < 2) return fail(GLH_E_UNSUPPORTED, "rasters need at least 2 x 2 cells (got %d x %d)", nx, ny);
  if (!gx || !gy || (sx != 1 && sx != -1) || (sy != 1 && sy != -1)) return fail(GLH_E_INVALID, "bad raster geometry");
  for (int i = 1; i < nx; ++i)
    if (!(gx[i] > gx[i - 1])) return fail(GLH_E_INVALID, "gx must be strictly ascending");
  for (int i = 1; i < ny; ++i)
    if (!(gy[i] > gy[i - 1])) return fail(GLH_E_INVALID, "gy must be strictly ascending");
  return GLH_OK;
}
// (the kernels find a sample's cell from the cell size: glh_math.h, raster_interval)
static int check_raster_uniform(int nx, int ny, const double* gx, const double* gy, double xmin, double xmax, double ymin,
                                double ymax) {
  if (!raster_coordinates_uniform(gx, nx, xmin, xmax) || !raster_coordinates_uniform(gy, ny, ymin, ymax))
    return fail(GLH_E_UNSUPPORTED, "raster coordinates must be the cell centres of a uniform grid over the outer limits "
                                   "(glimpse.Grid.x / .y); these are further than a quarter cell from it");
  return GLH_OK;
}

// Fast arithmetic scales the DEM term of a gridded point by rcp_nr(2 zs^2) (glh_kernels.h: dem_log_likelihood<true>), a
// reciprocal only where its argument is a normal double: for 2 zs^2 below 2^-1022 (|zs| < 1.06e-154, zs^2 may even
// round to 0) or infinite (|zs| > 9.4e153) it returns NaN -- every weight of the point NaN -- where the IEEE division of
// the exact arithmetic gives inf or 0 and the particle the floor weight (measured on the device: INPUTS.md, "Fast
// arithmetic: the primitives").  Such a sigma is refused on the host instead of tested for in the particle loops.
// (0 is "no term" and NaN is NaN in either arithmetic: neither is refused.)
static bool sigma_outside_fast_domain(double zs) {
  if (zs == 0.0 || zs != zs) return false;
  const double s = 2.0 * (zs * zs);
  return s < 0x1p-1022 || s > 0x1.fffffffffffffp1023;
}
static int check_fast_domain(const glh_ctx* c) {
  if (!c->fast_math) return GLH_OK;
  const char* why = "is outside the domain of fast arithmetic (GLH_MATH_FAST needs 1.06e-154 <= |dem_sigma| <= 9.4e153, or 0)";
  if (c->fast_bad_point >= 0)
    return fail(GLH_E_UNSUPPORTED, "point %d: dem_sigma = %g %s", c->fast_bad_point, c->fast_bad_const, why);
  if (c->sigma_raster_used && c->fast_bad_node != 0.0)
    return fail(GLH_E_UNSUPPORTED, "the dem_sigma raster holds %g, which %s", c->fast_bad_node, why);
  return GLH_OK;
}

extern "C" int glh_set_raster(glh_ctx* c, int which, const double* z, int nx, int ny, const double* gx,
                              const double* gy, int sx, int sy, double xmin, double xmax, double ymin,
                              double ymax) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (which < GLH_RASTER_DEM || which > GLH_RASTER_VIEWSHED) return fail(GLH_E_INVALID, "unknown raster slot %d", which);
  auto& r = c->rasters[which];
  if (!z && !r.z) return GLH_OK;  // (no raster before, none now: nothing to wait for -- the usual call of every run)
  HIPCHK(hipSetDevice(c->cfg.device_id));
  HIPCHK(hipStreamSynchronize(c->stream));
  r.z.reset(), r.gx.reset(), r.gy.reset();
  r.dev = RasterDev{};
  r.hgx.clear();
  r.hgy.clear();
  c->same_grid = false;
  if (which == GLH_RASTER_DEM_SIGMA) c->fast_bad_node = 0.0;
  if (!z) return GLH_OK;
  CHK(check_raster_args(nx, ny, gx, gy, sx, sy));
  CHK(check_raster_uniform(nx, ny, gx, gy, xmin, xmax, ymin, ymax));
  if (which == GLH_RASTER_DEM_SIGMA)
    for (size_t i = 0; i < (size_t)nx * ny && c->fast_bad_node == 0.0; ++i)
      if (sigma_outside_fast_domain(z[i])) c->fast_bad_node = z[i];
  CHK(r.z.alloc((size_t)nx * ny));
  CHK(r.gx.alloc((size_t)nx));
  CHK(r.gy.alloc((size_t)ny));
  HIPCHK(hipMemcpy(r.z, z, (size_t)nx * ny * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r.gx, gx, (size_t)nx * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r.gy, gy, (size_t)ny * sizeof(double), hipMemcpyHostToDevice));
  r.dev = raster_dev(r.z, r.gx, r.gy, nx, ny, sx, sy, xmin, xmax, ymin, ymax);
  r.hgx.assign(gx, gx + nx);
  r.hgy.assign(gy, gy + ny);
  // a DEM and its uncertainty on ONE grid share the cell and the weights of a sample (raster_sample_pair): only when the
  // coordinate arrays are the same numbers -- equal limits and sizes alone allow a quarter cell of difference
  const auto &d0 = c->rasters[GLH_RASTER_DEM], &d1 = c->rasters[GLH_RASTER_DEM_SIGMA];
  c->same_grid = d0.z && d1.z && d0.hgx == d1.hgx && d0.hgy == d1.hgy;
  return GLH_OK;
}

extern "C" int glh_set_motion(glh_ctx* c, const double* params) {
  CHK(need_seq(c));
  if (!params) return fail(GLH_E_INVALID, "params is null");
  c->has_dem = false;
  c->all_cartesian = true;
  c->fast_bad_point = -1;
  c->sigma_raster_used = false;
  for (int p = 0; p < c->P; ++p) {
    const double* m = params + (size_t)p * GLH_MOTION_FULL_LEN;
    const int kind = (int)m[18];
    if (m[18] != (double)kind || kind < GLH_MOTION_CARTESIAN || kind > GLH_MOTION_EXTERNAL)
      return fail(GLH_E_INVALID, "point %d: unknown motion kind %g", p, m[18]);
    if (kind != GLH_MOTION_CARTESIAN) c->all_cartesian = false;
    if (m[20] != 0.0 && !c->rasters[GLH_RASTER_DEM].z)
      return fail(GLH_E_STATE, "point %d uses a dem raster but glh_set_raster(GLH_RASTER_DEM) was not called", p);
    if (m[21] != 0.0 && !c->rasters[GLH_RASTER_DEM_SIGMA].z)
      return fail(GLH_E_STATE, "point %d uses a dem_sigma raster but glh_set_raster(GLH_RASTER_DEM_SIGMA) was not called", p);
    if (kind <= GLH_MOTION_CYLINDRICAL && (m[17] != 0.0 || m[21] != 0.0)) c->has_dem = true;
    // (a constant dem_sigma beside a constant dem is scaled by an IEEE division in either arithmetic: k_weights, the fused step)
    if (kind <= GLH_MOTION_CYLINDRICAL && m[21] != 0.0) c->sigma_raster_used = true;
    if (kind <= GLH_MOTION_CYLINDRICAL && m[20] != 0.0 && m[21] == 0.0 && c->fast_bad_point < 0 &&
        sigma_outside_fast_domain(m[17])) {
      c->fast_bad_point = p;
      c->fast_bad_const = m[17];
    }
  }
  UPLOAD(c->motion, params, (size_t)c->P * GLH_MOTION_FULL_LEN, double);
  return GLH_OK;
}

extern "C" int glh_set_motion_cartesian(glh_ctx* c, const double* params) {
  CHK(need_seq(c));
  if (!params) return fail(GLH_E_INVALID, "params is null");
  std::vector<double> full((size_t)c->P * GLH_MOTION_FULL_LEN, 0.0);
  for (int p = 0; p < c->P; ++p)
    std::copy(params + (size_t)p * GLH_MOTION_LEN, params + (size_t)(p + 1) * GLH_MOTION_LEN,
              full.begin() + (size_t)p * GLH_MOTION_FULL_LEN);
  return glh_set_motion(c, full.data());
}
extern "C" int glh_set_point_offset(glh_ctx* c, int offset) {
  CHK(need_seq(c));
  if (offset < 0) return fail(GLH_E_INVALID, "offset must be >= 0");
  c->pt_base = offset;
  return GLH_OK;
}
extern "C" int glh_set_observer_mask(glh_ctx* c, const uint8_t* mask) {
  CHK(need_seq(c));
  c->have_mask = mask != nullptr;
  if (mask) UPLOAD(c->obs_mask, mask, (size_t)c->P * c->cfg.n_observers, uint8_t);
  return GLH_OK;
}
extern "C" int glh_set_active(glh_ctx* c, const uint8_t* active) {
  CHK(need_seq(c));
  c->have_active = active != nullptr;
  if (active) UPLOAD(c->active, active, (size_t)c->P, uint8_t);
  return GLH_OK;
}
extern "C" int glh_set_extra_log_likelihoods(glh_ctx* c, const double* ll) {
  CHK(need_seq(c));
  c->have_extra = ll != nullptr;
  if (!ll) return GLH_OK;
  if (!c->extra_ll) CHK(c->extra_ll.alloc((size_t)c->cfg.max_points * c->cfg.max_particles));
  UPLOAD(c->extra_ll, ll, (size_t)c->P * c->N, double);
  return GLH_OK;
}
extern "C" int glh_set_particles(glh_ctx* c, const double* p) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  c->moments_frame = -1;
  if (!p) return fail(GLH_E_INVALID, "particles is null");
  UPLOAD(c->particles[c->cur], p, (size_t)c->P * c->N * 6, double);
  return GLH_OK;
}
extern "C" int glh_get_particles(glh_ctx* c, double* p) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  if (!p) return fail(GLH_E_INVALID, "particles is null");
  DOWNLOAD(p, c->particles[c->cur], (size_t)c->P * c->N * 6, double);
  return GLH_OK;
}
extern "C" int glh_set_weights(glh_ctx* c, const double* w) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  c->moments_frame = -1;
  if (!w) return fail(GLH_E_INVALID, "weights is null");
  UPLOAD(c->weights[c->cur], w, (size_t)c->P * c->N, double);
  return GLH_OK;
}
extern "C" int glh_get_weights(glh_ctx* c, double* w) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  if (!w) return fail(GLH_E_INVALID, "weights is null");
  DOWNLOAD(w, c->weights[c->cur], (size_t)c->P * c->N, double);
  return GLH_OK;
}
extern "C" int glh_get_point_status(glh_ctx* c, uint32_t* st) {
  CHK(need_seq(c));
  if (!st) return fail(GLH_E_INVALID, "status is null");
  DOWNLOAD(st, c->pt_status, (size_t)c->P, uint32_t);
  return GLH_OK;
}
extern "C" int glh_get_point_error_frame(glh_ctx* c, int32_t* fr) {
  CHK(need_seq(c));
  if (!fr) return fail(GLH_E_INVALID, "frames is null");
  DOWNLOAD(fr, c->pt_err_frame, (size_t)c->P, int32_t);
  return GLH_OK;
}
extern "C" int glh_get_observer_status(glh_ctx* c, int32_t* st) {
  CHK(need_seq(c));
  if (!st) return fail(GLH_E_INVALID, "status is null");
  DOWNLOAD(st, cur_status(c), (size_t)c->cfg.n_observers * c->P, int32_t);
  return GLH_OK;
}
extern "C" int glh_get_observer_status_frames(glh_ctx* c, int frame0, int n_frames, int32_t* st) {
  CHK(need_seq(c));
  if (!st || frame0 < 0 || n_frames <= 0 || frame0 + n_frames > c->cfg.max_frames)
    return fail(GLH_E_INVALID, "bad frame range");
  const size_t per = (size_t)c->cfg.n_observers * c->P;
  DOWNLOAD(st, c->obs_status_all + (size_t)frame0 * per, (size_t)n_frames * per, int32_t);
  return GLH_OK;
}
extern "C" int glh_get_point_state(glh_ctx* c, int point, double* particles, double* weights) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  if (point < 0 || point >= c->P) return fail(GLH_E_INVALID, "point %d out of range", point);
  if (particles) DOWNLOAD(particles, c->particles[c->cur] + (size_t)point * c->N * 6, (size_t)c->N * 6, double);
  if (weights) DOWNLOAD(weights, c->weights[c->cur] + (size_t)point * c->N, (size_t)c->N, double);
  return GLH_OK;
}
extern "C" int glh_get_log_likelihoods(glh_ctx* c, int o, double* ll) {
  CHK(need_seq(c));
  CHK(check_obs(c, o));
  if (!ll || !c->keep_sse || !c->ll_dbg) return fail(GLH_E_STATE, "log-likelihood capture is off (glh_set_debug)");
  DOWNLOAD(ll, c->ll_dbg + (size_t)o * c->P * c->N, (size_t)c->P * c->N, double);
  return GLH_OK;
}
extern "C" int glh_get_search_boxes(glh_ctx* c, int32_t* boxes) {
  CHK(need_seq(c));
  if (!boxes) return fail(GLH_E_INVALID, "boxes is null");
  DOWNLOAD(boxes, c->box, (size_t)c->cfg.n_observers * c->P * 4, int32_t);
  return GLH_OK;
}
extern "C" int glh_get_resample_indices(glh_ctx* c, int32_t* idx) {
  CHK(need_seq(c));
  if (!idx || !c->idx) return fail(GLH_E_STATE, "index capture is off (glh_set_debug)");
  DOWNLOAD(idx, c->idx, (size_t)c->P * c->N, int32_t);
  return GLH_OK;
}

extern "C" int glh_set_debug(glh_ctx* c, int keep) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if (keep < 0 || keep > 2) return fail(GLH_E_INVALID, "keep must be 0, 1 or 2");
  c->keep_sse = keep == 1;
  c->keep_idx = keep != 0;
  if (keep == 2 && !c->idx) CHK(c->idx.alloc((size_t)c->cfg.max_points * c->cfg.max_particles));
  if (keep == 1) {
    if (!c->sse_copy)
      CHK(c->sse_copy.alloc((size_t)c->cfg.n_observers * c->cfg.max_points * (size_t)c->sse_cap));
    if (!c->idx) CHK(c->idx.alloc((size_t)c->cfg.max_points * c->cfg.max_particles));
    if (!c->ll_dbg)
      CHK(c->ll_dbg.alloc((size_t)c->cfg.n_observers * c->cfg.max_points * c->cfg.max_particles));
  }
  return GLH_OK;
}

// staging of host-fed random numbers (parity mode)
static int stage_normals(glh_ctx* c, const double* host, size_t count) {
  CHK(c->normals.reserve(count));
  HIPCHK(hipMemcpyAsync(c->normals, host, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // the host buffer may be reused by the caller right away
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

// GLH_RNG_HOST: the caller's `count` normals (`shape` in the message) go to the device; anything else but the device's
// Philox draws is refused
static int stage_rng(glh_ctx* c, int rng_mode, const double* normals, size_t count, const char* shape) {
  if (rng_mode == GLH_RNG_HOST) {
    if (!normals) return fail(GLH_E_INVALID, "GLH_RNG_HOST needs normals %s", shape);
    return stage_normals(c, normals, count);
  }
  if (rng_mode != GLH_RNG_PHILOX) return fail(GLH_E_INVALID, "unknown rng_mode %d", rng_mode);
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// stages
// ------------------------------------------------------------------------------------------
extern "C" int glh_init_particles(glh_ctx* c, int rng_mode, const double* normals, uint64_t seed) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  CHK(stage_rng(c, rng_mode, normals, (size_t)c->P * c->N * 6, "[P][N][6]"));
  c->moments_frame = -1;
  InitArgs a{};
  a.particles = c->particles[c->cur];
  a.weights = c->weights[c->cur];
  a.motion = c->motion;
  a.active = c->have_active ? c->active : nullptr;
  a.normals = c->normals;
  a.seed = seed;
  a.rng_mode = rng_mode;
  a.N = c->N;
  a.pt_base = c->pt_base;
  a.frame = c->frame;
  a.pt_status = c->pt_status;
  a.pt_err_frame = c->pt_err_frame;
  a.surf = surfaces(c);
  {
    StageTimer t(c, ST_INIT);
    hipLaunchKernelGGL(k_init_particles, dim3(c->NB, c->P), dim3(BLK), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

static void fill_obs(glh_ctx* c, int o, int image, ObsFrame* f) {
  const Observer& ob = c->obs[o];
  f->on = image >= 0;
  f->cam = ob.cams + (image >= 0 ? image : 0);
  f->frame = image >= 0 ? ob.frames[image] : nullptr;
  f->width = ob.width;
  f->height = ob.height;
  f->channels = ob.channels;
  f->bits = ob.bits;
  f->bins = c->bins16;
  f->fwork = c->fwork;
  f->fwork_cap = 2 * (int64_t)c->cfg.max_search_dim * c->cfg.max_search_dim;
}

// 16-bit frames: the zeroed per-point key histograms the staged tile kernels of observer `o` count into
static int prepare_bins16(glh_ctx* c, int o, bool search_tiles = false) {
  if (c->obs[o].bits >= 16 && !c->fwork)  // 16-bit and float frames: two tile-sized arrays of doubles per point
    CHK(c->fwork.alloc((size_t)c->cfg.max_points * 2 * c->cfg.max_search_dim * c->cfg.max_search_dim));
  if (c->obs[o].bits != 16 || search_tiles) return GLH_OK;  // (search tiles are ranked; only templates count into bins)
  const size_t per = (size_t)(65535 * 3 + 1);
  if (!c->bins16) CHK(c->bins16.alloc((size_t)c->cfg.max_points * per));
  HIPCHK(hipMemsetAsync(c->bins16, 0, (size_t)c->P * (65535 * c->obs[o].channels + 1) * sizeof(uint32_t), c->stream));
  return GLH_OK;
}

static int check_images(glh_ctx* c, const int32_t* images) {
  if (!images) return fail(GLH_E_INVALID, "images is null");
  for (int o = 0; o < c->cfg.n_observers; ++o) {
    if (images[o] < 0) continue;
    const Observer& ob = c->obs[o];
    if (images[o] >= ob.n_images) return fail(GLH_E_INVALID, "observer %d: image %d out of range", o, images[o]);
    if (!ob.frames[images[o]]) return fail(GLH_E_STATE, "observer %d: image %d has not been uploaded", o, images[o]);
  }
  return join_uploads(c);  // the kernels that follow read the frames
}

// evolve (optional) + project into the given images + bbox partials
static int launch_evolve_project(glh_ctx* c, bool do_evolve, double tau, int rng_mode, uint64_t seed,
                                 uint64_t step, const int32_t* images, bool store = true) {
  CHK(ensure_expanded(c));
  if (do_evolve) c->moments_frame = -1;
  EvolveArgs a{};
  a.particles = c->particles[c->cur];
  a.store = store;
  a.surf = surfaces(c);
  a.motion = c->motion;
  a.active = c->have_active ? c->active : nullptr;
  a.obs_mask = c->have_mask ? c->obs_mask : nullptr;
  a.normals = c->normals;
  a.uv = c->uv;
  a.bbox_part = c->bbox_part;
  a.pt_status = c->pt_status;
  a.pt_err_frame = c->pt_err_frame;
  a.seed = seed;
  a.step = step;
  a.tau = tau;
  a.do_evolve = do_evolve;
  a.rng_mode = rng_mode;
  a.N = c->N;
  a.P = c->P;
  a.O = c->cfg.n_observers;
  a.NB = c->NB;
  a.frame = c->frame;
  a.pt_base = c->pt_base;
  a.fast = use_fast(c);
  for (int o = 0; o < a.O; ++o) fill_obs(c, o, images ? images[o] : -1, &a.obs[o]);
  {
    StageTimer t(c, ST_EVOLVE_PROJECT);
    hipLaunchKernelGGL(k_evolve_project, dim3(c->NB, c->P), dim3(BLK), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

extern "C" int glh_evolve(glh_ctx* c, double tau, int rng_mode, const double* normals, uint64_t seed,
                          uint64_t step) {
  CHK(need_seq(c));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  CHK(stage_rng(c, rng_mode, normals, (size_t)c->P * c->N * 3, "[P][N][3]"));
  return launch_evolve_project(c, true, tau, rng_mode, seed, step, nullptr);
}

static int launch_moments(glh_ctx* c, double* out, int ld, int with_sigma) {
  CHK(ensure_expanded(c));
  MomentsArgs a{};
  a.particles = c->particles[c->cur];
  a.weights = c->weights[c->cur];
  a.active = c->have_active ? c->active : nullptr;
  a.out = out;
  a.N = c->N;
  a.ld = ld;
  a.with_sigma = with_sigma;
  {
    StageTimer t(c, ST_MOMENTS);
    hipLaunchKernelGGL(k_moments, dim3(c->P), dim3(BLK), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

extern "C" int glh_init_templates(glh_ctx* c, int o, int image) {
  CHK(need_seq(c));
  CHK(check_obs(c, o));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const Observer& ob = c->obs[o];
  if (image < 0 || image >= ob.n_images || !ob.frames[image])
    return fail(GLH_E_STATE, "observer %d: image %d is not resident", o, image);
  CHK(join_uploads(c));
  CHK(launch_moments(c, c->mean6, 6, 0));  // particle_mean with the carried weights (tracker.py:548)
  TemplateArgs a{};
  a.mean6 = c->mean6;
  a.active = c->have_active ? c->active : nullptr;
  a.obs_mask = c->have_mask ? c->obs_mask : nullptr;
  fill_obs(c, o, image, &a.obs);
  a.o = o;
  a.O = c->cfg.n_observers;
  a.P = c->P;
  a.tw = c->tw;
  a.th = c->th;
  a.tile_cap = c->tile_cap;
  a.frame = c->frame;
  a.hp_rx = c->hp_rx;
  a.hp_ry = c->hp_ry;
  a.tmpl_box = c->tmpl_box;
  a.tmpl_duv = c->tmpl_duv;
  a.tmpl_tile64 = c->tmpl_tile64;
  a.tmpl_tile32 = c->tmpl_tile32;
  a.tmpl_hist_v = c->tmpl_hist_v;
  a.tmpl_hist_q = c->tmpl_hist_q;
  a.tmpl_hist_n = c->tmpl_hist_n;
  a.tmpl_valid = c->tmpl_valid;
  a.pt_status = c->pt_status;
  a.pt_err_frame = c->pt_err_frame;
  CHK(prepare_bins16(c, o));
  a.obs.bins = c->bins16;
  a.obs.fwork = c->fwork;
  {
    StageTimer t(c, ST_TEMPLATE);
    hipLaunchKernelGGL(k_template_init, dim3(c->P), dim3(BLK),
                       (size_t)c->tw * c->th * (ob.bits >= 32 ? 12 : (ob.bits == 16 ? 4 : 2)), c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

// search tile -> SSD surface -> spline coefficients of every observer with an image
static int launch_tile_stages(glh_ctx* c, const int32_t* images) {
  const int O = c->cfg.n_observers;
  for (int o = 0; o < O; ++o) {
    if (images[o] < 0) {
      // no image for this observer at this frame (tracker.py:577): the status must not keep the previous frame's
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(cur_status(c) + (size_t)o * c->P), GLH_OBS_SKIPPED, (size_t)c->P,
                               c->stream));
      continue;
    }
    TilePrepArgs tp{};
    tp.active = c->have_active ? c->active : nullptr;
    tp.obs_mask = c->have_mask ? c->obs_mask : nullptr;
    fill_obs(c, o, images[o], &tp.obs);
    tp.o = o;
    tp.O = O;
    tp.P = c->P;
    tp.NB = c->NB;
    tp.tw = c->tw;
    tp.th = c->th;
    tp.tile_cap = c->tile_cap;
    tp.search_cap = c->search_cap;
    tp.max_dim = c->cfg.max_search_dim;
    tp.hp_rx = c->hp_rx;
    tp.hp_ry = c->hp_ry;
    tp.kcols = c->interp_ky;  // ("ky" widens the columns, "kx" the rows: tracker.py:585-590)
    tp.krows = c->interp_kx;
    tp.bbox_part = c->bbox_part;
    tp.tmpl_valid = c->tmpl_valid;
    tp.tmpl_hist_v = c->tmpl_hist_v;
    tp.tmpl_hist_q = c->tmpl_hist_q;
    tp.tmpl_hist_n = c->tmpl_hist_n;
    tp.box = c->box;
    tp.obs_status = cur_status(c);
    tp.search = c->search;
    CHK(prepare_bins16(c, o, true));
    tp.obs.bins = c->bins16;
    tp.obs.fwork = c->fwork;
    {
      StageTimer t(c, ST_TILEPREP);
      size_t lds = (size_t)(BAND_H + 6) * c->cfg.max_search_dim * (c->obs[o].bits == 16 ? 4 : 2);  // (halo of up to 3 rows)
      // float frames: the template CDF (up to tw x th values and quantiles) is searched twice per pixel -- from LDS
      // ... and the float32 scratch of a typical tile's normalisation (2 n floats) is read by one thread -- from LDS
      if (c->obs[o].bits >= 16)
        lds = std::max({lds, (size_t)2 * c->tile_cap * sizeof(double),
                        std::min((size_t)8 * c->cfg.max_search_dim * c->cfg.max_search_dim, (size_t)40 * 1024)});
      tp.lds_bytes = (int32_t)lds;
      hipLaunchKernelGGL(k_tileprep, dim3(c->P), dim3(BLK), lds, c->stream, tp);
    }
    HIPCHK(hipGetLastError());
    SsdArgs sa{};
    sa.o = o;
    sa.P = c->P;
    sa.tw = c->tw;
    sa.th = c->th;
    sa.tile_cap = c->tile_cap;
    sa.search_cap = c->search_cap;
    sa.sse_cap = c->sse_cap;
    sa.box = c->box;
    sa.obs_status = cur_status(c);
    sa.search = c->search;
    sa.tmpl = c->tmpl_tile32;
    sa.sse = c->sse;
    {
      StageTimer t(c, ST_SSD);
      hipLaunchKernelGGL(k_ssd, dim3(c->ssd_blocks, c->P), dim3(BLK), ssd_lds_bytes(c->tw, c->th), c->stream, sa);
    }
    HIPCHK(hipGetLastError());
    SplineFitArgs sf{};
    sf.o = o;
    sf.P = c->P;
    sf.tw = c->tw;
    sf.th = c->th;
    sf.sse_cap = c->sse_cap;
    sf.max_n = c->cfg.max_search_dim;
    sf.box = c->box;
    sf.obs_status = cur_status(c);
    sf.lu = c->lu;
    sf.lu_off = c->lu_off;
    sf.inv = c->spl_inv;
    sf.sse = c->sse;
    sf.sse_copy = c->keep_sse ? c->sse_copy : nullptr;
    sf.linear = c->interp_k == 1;
    sf.kx = c->interp_kx;
    sf.ky = c->interp_ky;
    if (c->interp_k == 0) {
      sf.glu_v = c->glu[0];
      sf.glu_v_off = c->glu_off[0];
      sf.glu_u = c->glu[1];
      sf.glu_u_off = c->glu_off[1];
    }
    {
      StageTimer t(c, ST_SPLINE_FIT);
      hipLaunchKernelGGL(k_spline_fit, dim3(c->P), dim3(BLK), 0, c->stream, sf);
    }
    HIPCHK(hipGetLastError());
  }
  return GLH_OK;
}

// (a context with rasters runs the fused step's instantiations with the raster samples)
static bool has_rasters(const glh_ctx* c) { return c->rasters[0].z || c->rasters[1].z || c->rasters[2].z; }

// What the fused step's host plan (glh_point_plan.h: pt_plan) reads of the context.
static PtSetup pt_setup(const glh_ctx* c) {
  PtSetup s{};
  s.N = c->N, s.O = c->cfg.n_observers, s.tw = c->tw, s.th = c->th;
  s.max_search_dim = c->cfg.max_search_dim, s.interp_k = c->interp_k;
  for (int o = 0; o < s.O && o < PT_MAX_OBS; ++o) s.bits[o] = c->obs[o].bits, s.channels[o] = c->obs[o].channels;
  s.rasters = has_rasters(c);
  s.nleaves = c->nleaves, s.nnodes = c->nnodes, s.nlevels = c->nlevels, s.nroots = c->nroots;
  s.small_lds = c->fused == 2;
  return s;
}

// Does the fused kernel take the step?  `plan` is filled either way: the staged k_weights takes its cell cap from it.
static bool fused_takes_step(const glh_ctx* c, PtPlan* plan) {
  *plan = pt_plan(pt_setup(c));
  return c->fused && !c->have_active && !c->keep_sse && !c->have_extra && plan->accepted;
}

static int update_weights_impl(glh_ctx* c, const int32_t* images, bool projected, const PtPlan& plan) {
  CHK(ensure_expanded(c));
  const int O = c->cfg.n_observers;
  // uv + bbox of the (already evolved) particles in the matched images
  if (!projected) CHK(launch_evolve_project(c, false, 0.0, GLH_RNG_PHILOX, 0, 0, images));
  CHK(launch_tile_stages(c, images));
  c->moments_frame = -1;
  WeightArgs wa{};
  wa.particles = c->particles[c->cur];
  wa.weights = c->weights[c->cur];
  wa.motion = c->motion;
  wa.active = c->have_active ? c->active : nullptr;
  wa.uv = c->uv;
  wa.box = c->box;
  wa.obs_status = cur_status(c);
  wa.tmpl_duv = c->tmpl_duv;
  wa.coef = c->sse;
  wa.poly = c->poly;
  wa.ll_out = c->keep_sse ? c->ll_dbg : nullptr;
  wa.extra = c->have_extra ? c->extra_ll : nullptr;
  wa.pt_status = c->pt_status;
  wa.pt_err_frame = c->pt_err_frame;
  for (int o = 0; o < O; ++o) {
    wa.on[o] = images[o] >= 0;
    wa.inv2s2[o] = 1.0 / (2.0 * (c->obs[o].sigma * c->obs[o].sigma));  // 1 / (2 * sigma ** 2)
  }
  wa.N = c->N;
  wa.P = c->P;
  wa.O = O;
  wa.tw = c->tw;
  wa.th = c->th;
  wa.sse_cap = c->sse_cap;
  wa.frame = c->frame;
  wa.fast = use_fast(c);
  wa.cell_cap = plan.cell_cap;
  wa.linear = c->interp_k == 1;
  wa.general = c->interp_k == 0;
  wa.kx = c->interp_kx;
  wa.ky = c->interp_ky;
  wa.surf = surfaces(c);
  {
    StageTimer t(c, ST_WEIGHTS);
    hipLaunchKernelGGL(k_weights, dim3((c->NB + WEIGHTS_PER_THREAD - 1) / WEIGHTS_PER_THREAD, c->P), dim3(BLK), 0, c->stream, wa);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

extern "C" int glh_update_weights(glh_ctx* c, const int32_t* images) {
  CHK(need_seq(c));
  CHK(check_fast_domain(c));
  CHK(check_images(c, images));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  return update_weights_impl(c, images, false, pt_plan(pt_setup(c)));
}

extern "C" int glh_resample(glh_ctx* c, int rng_mode, const double* u, uint64_t seed, uint64_t step) {
  return glh_resample_method(c, GLH_RESAMPLE_SYSTEMATIC, rng_mode, u, seed, step);
}

extern "C" int glh_resample_method(glh_ctx* c, int method, int rng_mode, const double* u, uint64_t seed,
                                   uint64_t step) {
  CHK(need_seq(c));
  CHK(ensure_expanded(c));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if (method != GLH_RESAMPLE_SYSTEMATIC && method != GLH_RESAMPLE_STRATIFIED && method != GLH_RESAMPLE_CHOICE &&
      method != GLH_RESAMPLE_RESIDUAL)
    return fail(GLH_E_INVALID, "unknown resampling method %d", method);
  if (method == GLH_RESAMPLE_RESIDUAL && !c->resid_draws) CHK(c->resid_draws.alloc((size_t)c->cfg.max_points));
  const bool per_particle = method != GLH_RESAMPLE_SYSTEMATIC;
  if (rng_mode == GLH_RNG_HOST) {
    if (!u) return fail(GLH_E_INVALID, "GLH_RNG_HOST needs u (%s)", per_particle ? "[P][N]" : "[P]");
    if (per_particle) {
      if (!c->uj) CHK(c->uj.alloc((size_t)c->cfg.max_points * c->cfg.max_particles));
      HIPCHK(hipMemcpyAsync(c->uj, u, (size_t)c->P * c->N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    } else {
      HIPCHK(hipMemcpyAsync(c->u, u, (size_t)c->P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
  } else if (rng_mode != GLH_RNG_PHILOX) {
    return fail(GLH_E_INVALID, "unknown rng_mode %d", rng_mode);
  }
  ResampleArgs a{};
  a.method = method;
  a.particles_in = c->particles[c->cur];
  a.weights_in = c->weights[c->cur];
  a.particles_out = c->particles[c->cur ^ 1];
  a.weights_out = c->weights[c->cur ^ 1];
  a.active = c->have_active ? c->active : nullptr;
  a.u = per_particle ? c->uj : c->u;
  a.idx_out = c->keep_idx ? c->idx : nullptr;
  a.n_draws = method == GLH_RESAMPLE_RESIDUAL ? c->resid_draws : nullptr;
  a.pt_status = c->pt_status;
  a.pt_err_frame = c->pt_err_frame;
  a.moments = c->moments + (size_t)c->frame * c->P * 12;  // fused particle_mean / sigma of frame c->frame
  a.leaf_off = c->leaf_off;
  a.leaf_len = c->leaf_len;
  a.ops = c->sum_ops;
  a.level_off = c->level_off;
  a.roots = c->roots;
  a.seed = seed;
  a.step = step;
  a.N = c->N;
  a.nleaves = c->nleaves;
  a.nnodes = c->nnodes;
  a.nlevels = c->nlevels;
  a.nroots = c->nroots;
  a.rng_mode = rng_mode;
  a.frame = c->frame;
  a.pt_base = c->pt_base;
  a.fast = use_fast(c);
  if (c->have_active) {
    // inactive points keep their state: copy their rows across before swapping buffers
    HIPCHK(hipMemcpyAsync(c->particles[c->cur ^ 1], c->particles[c->cur], (size_t)c->P * c->N * 6 * sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->weights[c->cur ^ 1], c->weights[c->cur], (size_t)c->P * c->N * sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));
  }
  {
    StageTimer t(c, ST_RESAMPLE);
    // c[N] | tree nodes | indices [N] u16 | repetitions [N] u16 (residual)
    size_t lds = ((size_t)c->N + c->nnodes) * sizeof(double) +
                 (method == GLH_RESAMPLE_RESIDUAL ? 2 : 1) * (size_t)c->N * sizeof(uint16_t);
    if (lds > 156 * 1024) return fail(GLH_E_UNSUPPORTED, "residual resampling: %d particles exceed the LDS-resident scan", c->N);
    hipLaunchKernelGGL(k_resample, dim3(c->P), dim3(BLK), lds, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  c->cur ^= 1;
  // the fused moments cover every point only when no active mask was in force
  c->moments_frame = c->have_active ? -1 : c->frame;
  return GLH_OK;
}

extern "C" int glh_record_moments(glh_ctx* c, int frame) {
  CHK(need_seq(c));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if (frame < 0 || frame >= c->cfg.max_frames) return fail(GLH_E_INVALID, "frame %d outside [0, max_frames)", frame);
  if (c->moments_frame == frame && !c->have_active) return GLH_OK;  // written by the fused resample kernel
  return launch_moments(c, c->moments + (size_t)frame * c->P * 12, 12, 1);
}

// The fused frame step (glh_point.h): ONE launch, one workgroup per point.
// `pt0`, `npts`, `on`: the block of points this launch updates and the stream it is enqueued on (glh_track runs the two
// halves of a large batch on two streams); `flip`: the last launch of the frame -- the state buffers change roles.
static int fused_step(glh_ctx* c, int frame, double tau, const int32_t* images, int rng_mode, const double* u,
                      uint64_t seed, const PtPlan& plan, int pt0 = 0, int npts = -1, hipStream_t on = nullptr,
                      bool flip = true) {
  const int O = c->cfg.n_observers;
  if (npts < 0) npts = c->P;
  if (!on) on = c->stream;
  if (rng_mode == GLH_RNG_HOST) {
    if (!u) return fail(GLH_E_INVALID, "GLH_RNG_HOST needs u [P]");
    HIPCHK(hipMemcpyAsync(c->u, u, (size_t)c->P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  PointArgs a{};
  a.particles_in = c->particles[c->cur];
  a.particles_out = c->particles[c->cur ^ 1];
  a.weights_tmp = c->weights[c->cur];
  a.weights_out = c->weights[c->cur ^ 1];
  a.motion = c->motion;
  a.obs_mask = c->have_mask ? c->obs_mask : nullptr;
  a.normals = c->normals;
  a.u = c->u;
  a.uv = c->uv;
  a.box = c->box;
  a.obs_status = cur_status(c);
  a.tmpl_valid = c->tmpl_valid;
  a.tmpl_duv = c->tmpl_duv;
  a.tmpl_tile32 = c->tmpl_tile32;
  a.tmpl_hist_v = c->tmpl_hist_v;
  a.tmpl_hist_q = c->tmpl_hist_q;
  a.tmpl_hist_n = c->tmpl_hist_n;
  a.ws_search = c->search;
  a.ws_keys = c->ws_keys;
  a.ws_sse = c->sse;
  a.lu = c->lu;
  a.lu_off = c->lu_off;
  a.inv = c->spl_inv;
  a.poly = c->poly;
  a.idx_out = c->keep_idx ? c->idx : nullptr;
  for (int b = 0; b < 2; ++b)
    if (!c->uidx[b]) CHK(c->uidx[b].alloc((size_t)c->cfg.max_points * c->cfg.max_particles));
  a.uidx_in = c->compact ? c->uidx[c->cur] : nullptr;
  a.uidx_out = c->uidx[c->cur ^ 1];
  a.stamps = c->stamps ? c->stamps + (size_t)pt0 * PT_NSTAMP : nullptr;  // (indexed by the launch's own block index)
  a.pt0 = pt0;
  a.moments = c->moments + (size_t)frame * c->P * 12;
  a.pt_status = c->pt_status;
  a.pt_err_frame = c->pt_err_frame;
  a.leaf_off = c->leaf_off;
  a.leaf_len = c->leaf_len;
  a.ops = c->sum_ops;
  a.level_off = c->level_off;
  a.roots = c->roots;
  a.seed = seed;
  a.step = (uint64_t)frame;
  a.tau = tau;
  for (int o = 0; o < O; ++o) {
    if (c->obs[o].bits >= 32) CHK(prepare_bins16(c, o, true));  // (the float workspace, on first use)
    fill_obs(c, o, images[o], &a.obs[o]);
    if ((int)c->obs[o].cams_host.size() != c->obs[o].n_images)
      return fail(GLH_E_STATE, "observer %d: cameras have not been set", o);
    a.cam[o] = c->obs[o].cams_host[images[o] >= 0 ? images[o] : 0];
    a.cam_flags[o] = cam_flags(a.cam[o]);
    a.inv2s2[o] = 1.0 / (2.0 * (c->obs[o].sigma * c->obs[o].sigma));
  }
  a.N = c->N;
  a.P = c->P;
  a.O = O;
  a.tw = c->tw;
  a.th = c->th;
  a.tile_cap = c->tile_cap;
  a.search_cap = c->search_cap;
  a.keys_cap = c->keys_cap;
  a.sse_cap = c->sse_cap;
  a.max_dim = c->cfg.max_search_dim;
  a.frame = frame;
  a.rng_mode = rng_mode;
  a.has_dem = c->has_dem;
  a.r2_bytes = plan.r2_bytes;
  a.cell_cap = plan.cell_cap;
  a.hp_rx = c->hp_rx;
  a.hp_ry = c->hp_ry;
  a.interp_k = c->interp_k;
  a.pt_base = c->pt_base;
  a.stop_at = c->stop_frame == frame ? c->stop_stamp : -1;
  a.surf = surfaces(c);
  a.nleaves = c->nleaves;
  a.nnodes = c->nnodes;
  a.nlevels = c->nlevels;
  a.nroots = c->nroots;
  {
    StageTimer t(c, ST_POINT_STEP, on);
    // the instantiation: the plan's launch shape, the code from what this launch is given (glh_point_plan.h: pt_code)
    PtLaunch l{};
    l.fast = use_fast(c), l.philox = rng_mode == GLH_RNG_PHILOX, l.compact = c->compact, l.masked = c->have_mask;
    l.all_cartesian = c->all_cartesian;
    l.hp_rx = c->hp_rx, l.hp_ry = c->hp_ry, l.interp_k = c->interp_k;
    for (int o = 0; o < O; ++o) l.on[o] = a.obs[o].on, l.cam_flags[o] = a.cam_flags[o], l.bits[o] = c->obs[o].bits;
    const PtCode code = pt_code(l, O, has_rasters(c));
    c->last_variant[0] = plan.tb; c->last_variant[1] = plan.ppt; c->last_variant[2] = O;
    c->last_variant[3] = code.flags;
    const void* kern = pt_kernel(plan.tb, plan.ppt, O, code.surf, code.fast, code.con);
    if (!kern) return fail(GLH_E_STATE, "no instantiation of the fused kernel for <%d, %d, %d>", plan.tb, plan.ppt, O);
    void* kargs[] = {(void*)&a};
    HIPCHK(hipLaunchKernel(kern, dim3(npts), dim3(plan.tb), kargs, plan.lds_bytes, on));
  }
  HIPCHK(hipGetLastError());
  if (flip) {
    c->cur ^= 1;
    c->compact = true;
    c->moments_frame = frame;
  }
  return GLH_OK;
}

extern "C" int glh_get_residual_draws(glh_ctx* c, int32_t* draws) {
  CHK(need_seq(c));
  if (!draws) return fail(GLH_E_INVALID, "null argument");
  if (!c->resid_draws) return fail(GLH_E_STATE, "no residual resampling has run");
  DOWNLOAD(draws, c->resid_draws, (size_t)c->P, int32_t);
  return GLH_OK;
}

extern "C" int glh_record_covariances(glh_ctx* c, int frame) {
  CHK(need_seq(c));
  // (a run-length compact state -- what the fused step leaves -- is read through its record indices: expanding it first
  // would cost a pass over the state and send the next frame to the general instantiation)
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if (frame < 0 || frame >= c->cfg.max_frames) return fail(GLH_E_INVALID, "frame %d outside [0, max_frames)", frame);
  if (!c->covariances) {
    const size_t n = (size_t)c->cfg.max_frames * c->cfg.max_points * 36;
    CHK(c->covariances.alloc(n));
    hipLaunchKernelGGL(k_fill_f64, dim3(256), dim3(256), 0, c->stream, c->covariances, n, (double)NAN);
    HIPCHK(hipGetLastError());
  }
  CovArgs a{};
  a.particles = c->particles[c->cur];
  a.weights = c->weights[c->cur];
  a.uidx = c->compact ? c->uidx[c->cur] : nullptr;
  a.active = c->have_active ? c->active : nullptr;
  a.out = c->covariances + (size_t)frame * c->P * 36;
  a.N = c->N;
  {
    StageTimer t(c, ST_MOMENTS);
    hipLaunchKernelGGL(k_covariance, dim3(c->P), dim3(BLK), 0, c->stream, a);
  }
  HIPCHK(hipGetLastError());
  return GLH_OK;
}

extern "C" int glh_get_covariances(glh_ctx* c, int frame0, int n_frames, double* out) {
  CHK(need_seq(c));
  if (!out || frame0 < 0 || n_frames <= 0 || frame0 + n_frames > c->cfg.max_frames)
    return fail(GLH_E_INVALID, "bad frame range");
  if (!c->covariances) return fail(GLH_E_STATE, "glh_record_covariances has not been called");
  DOWNLOAD(out, c->covariances + (size_t)frame0 * c->P * 36, (size_t)n_frames * c->P * 36, double);
  return GLH_OK;
}

extern "C" int glh_step(glh_ctx* c, int frame, double tau, const int32_t* images, int rng_mode,
                        const double* normals, const double* u, uint64_t seed) {
  CHK(need_seq(c));
  CHK(check_fast_domain(c));
  CHK(glh_set_frame(c, frame));
  CHK(check_images(c, images));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  CHK(stage_rng(c, rng_mode, normals, (size_t)c->P * c->N * 3, "[P][N][3]"));
  PtPlan plan;
  if (fused_takes_step(c, &plan)) return fused_step(c, frame, tau, images, rng_mode, u, seed, plan);
  // one pass over the particle state: evolve, NaN test, project, bbox partials
  CHK(launch_evolve_project(c, true, tau, rng_mode, seed, (uint64_t)frame, images));
  CHK(update_weights_impl(c, images, true, plan));
  CHK(glh_resample(c, rng_mode, u, seed, (uint64_t)frame));
  return glh_record_moments(c, frame);
}

// The frame loop of every track (tracker.py:326-357) in one call: n_frames consecutive glh_step updates with the
// device RNG, enqueued back to back on the context's stream (no host synchronisation in between).
extern "C" int glh_track(glh_ctx* c, int n_frames, const int32_t* frames, const double* taus, const int32_t* images,
                         uint64_t seed) {
  CHK(need_seq(c));
  CHK(check_fast_domain(c));
  if (n_frames <= 0 || !frames || !taus || !images)
    return fail(GLH_E_INVALID, "n_frames must be > 0 and the arrays non-null");
  const int O = c->cfg.n_observers;
  for (int k = 0; k < n_frames; ++k) {
    if (frames[k] < 0 || frames[k] >= c->cfg.max_frames)
      return fail(GLH_E_INVALID, "frame %d outside [0, max_frames)", frames[k]);
    CHK(check_images(c, images + (size_t)k * O));
  }
  // Two streams (round 4).  A launch of the fused step is rounds of workgroups -- 512 (or 256 of 1 024 threads) at a
  // time -- and between two launches the chip drains and refills: at C3 t(P) = 0.059 ms + 0.107 us x P, the constant
  // is 12 % of a frame.  The points are independent, so the batch is cut in two halves whose frame loops run on two
  // streams: while one half's launch drains, the other half's launch fills the idle compute units (C3 -6 %, C4 shard
  // -4 %; four ways: worse).  Same kernel, same per-point arithmetic: results are bit for bit those of one stream.
  PtPlan plan;
  const bool fused_ok = fused_takes_step(c, &plan);
  // Automatic (round 5): two streams as soon as the batch has more points than the chip has compute units.  Round 4 asked
  // for two full rounds of workgroups per half; but a launch ends with its slowest point (their lifetimes spread by 30 %),
  // the halves' launches drift apart and fill each other's tails, and a batch of 1.5 rounds no longer runs a half-empty
  // second one: same box, one -> two streams, C3 x 320 points -10.7 %, x 512 -9.4 %, x 768 -26 %, C5's per-GPU share (512
  // points) -8.5 %, C4 x 384 -26 %, C2 x 512 -9 %; at one workgroup per CU or fewer (C2's 256 points: +2 %, C4 x 256: +-0)
  // one stream (profiles/ab_r05/r5j23_streams_small.txt, r5j24_streams_threshold.txt).  Three streams: the same; four: worse.
  int ns = 1;
  if (fused_ok && !c->track_covariances) {
    if (c->track_streams >= 2) ns = c->track_streams;
    else if (c->track_streams == 0 && c->P > c->n_cus) ns = 2;
    ns = std::min(ns, c->P);
  }
  c->last_track_streams = ns;
  if (ns == 1) {
    // frame by frame through glh_step (fused or staged), covariances recorded after every frame when asked
    int rc = GLH_OK;
    for (int k = 0; k < n_frames && rc == GLH_OK; ++k) {
      rc = glh_step(c, frames[k], taus[k], images + (size_t)k * O, GLH_RNG_PHILOX, nullptr, nullptr, seed);
      if (rc == GLH_OK && c->track_covariances) rc = glh_record_covariances(c, frames[k]);
    }
    return rc;
  }
  HIPCHK(hipSetDevice(c->cfg.device_id));
  if (!c->ev_fork) CHK(c->ev_fork.create(hipEventDisableTiming));
  hipStream_t on[4] = {c->stream, nullptr, nullptr, nullptr};
  for (int q = 1; q < ns; ++q) {
    if (!c->extra_streams[q - 1]) CHK(c->extra_streams[q - 1].create());
    if (!c->ev_join[q - 1]) CHK(c->ev_join[q - 1].create(hipEventDisableTiming));
    on[q] = c->extra_streams[q - 1];
  }
  // the other streams start behind everything enqueued so far, and the context's stream ends behind them
  HIPCHK(hipEventRecord(c->ev_fork, c->stream));
  for (int q = 1; q < ns; ++q) HIPCHK(hipStreamWaitEvent(on[q], c->ev_fork, 0));
  int rc = GLH_OK;
  for (int k = 0; k < n_frames && rc == GLH_OK; ++k) {
    rc = glh_set_frame(c, frames[k]);
    for (int q = 0; q < ns && rc == GLH_OK; ++q) {
      const int p0 = (int)((int64_t)c->P * q / ns), p1 = (int)((int64_t)c->P * (q + 1) / ns);
      rc = fused_step(c, frames[k], taus[k], images + (size_t)k * O, GLH_RNG_PHILOX, nullptr, seed, plan, p0,
                      p1 - p0, on[q], q == ns - 1);
    }
  }
  for (int q = 1; q < ns; ++q) {
    (void)hipEventRecord(c->ev_join[q - 1], on[q]);
    (void)hipStreamWaitEvent(c->stream, c->ev_join[q - 1], 0);
  }
  return rc;
}

// Streams of glh_track's frame loop: 0 automatic, 1 one stream, 2 two streams whenever the fused step runs.
extern "C" int glh_set_track_streams(glh_ctx* c, int n) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (n < 0 || n > 4) return fail(GLH_E_INVALID, "streams must be 0 (automatic) or 1 .. 4");
  c->track_streams = n;
  return GLH_OK;
}

extern "C" int glh_debug_last_track_streams(glh_ctx* c, int* n) {
  if (!c || !n) return fail(GLH_E_INVALID, "null argument");
  *n = c->last_track_streams;
  return GLH_OK;
}

// glh_track also records the particle covariances of every frame it runs (Tracker.track(return_covariances=True),
// tracker.py:307-308, :352): 0 (default) or 1.
extern "C" int glh_track_covariances(glh_ctx* c, int on) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  c->track_covariances = on != 0;
  return GLH_OK;
}

extern "C" int glh_measure_copy_bandwidth(glh_ctx* c, uint64_t bytes, int iters, double* gbps) {
  if (!c || !gbps || bytes == 0 || iters <= 0) return fail(GLH_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  DevArray<uint8_t> src, dst;
  CHK(src.alloc((size_t)bytes));
  CHK(dst.alloc((size_t)bytes));
  Event e0, e1;
  float ms = 0.0f;
  hipError_t err = hipMemsetAsync(src, 1, bytes, c->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream);  // warm-up
  // (the two empty owners are filled in place, not by Event::create: a failure stays in `err` and is reported below)
  if (err == hipSuccess) err = hipEventCreate(&e0.p);
  if (err == hipSuccess) err = hipEventCreate(&e1.p);
  if (err == hipSuccess) err = hipEventRecord(e0, c->stream);
  for (int k = 0; k < iters && err == hipSuccess; ++k)
    err = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream);
  if (err == hipSuccess) err = hipEventRecord(e1, c->stream);
  if (err == hipSuccess) err = hipEventSynchronize(e1);
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  if (err != hipSuccess) return fail(GLH_E_HIP, "copy bandwidth measurement failed: %s", hipGetErrorString(err));
  *gbps = 2.0 * (double)bytes * iters / ((double)ms * 1e-3) / 1e9;
  return GLH_OK;
}

extern "C" int glh_debug_last_variant(glh_ctx* c, int32_t* variant) {
  if (!c || !variant) return fail(GLH_E_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) variant[k] = c->last_variant[k];
  return GLH_OK;
}

extern "C" int glh_debug_draws(glh_ctx* c, int kind, uint64_t seed, uint64_t step, double* out) {
  CHK(need_seq(c));
  if (!out || kind < 0 || kind > 2) return fail(GLH_E_INVALID, "kind must be 0 (init), 1 (evolve) or 2 (resample offset)");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const size_t per = kind == 0 ? 6 : (kind == 1 ? 3 : 0);
  const size_t count = kind == 2 ? (size_t)c->P : (size_t)c->P * c->N * per;
  DevArray<double> buf;
  CHK(buf.alloc(count));
  DrawsArgs a{};
  a.out = buf;
  a.seed = seed;
  a.step = step;
  a.kind = kind;
  a.N = c->N;
  a.P = c->P;
  a.pt_base = c->pt_base;
  hipLaunchKernelGGL(k_debug_draws, dim3(kind == 2 ? 1 : (c->N + BLK - 1) / BLK, c->P), dim3(BLK), 0, c->stream, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, buf, count * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(GLH_E_HIP, "glh_debug_draws failed: %s", hipGetErrorString(e));
  return GLH_OK;
}

extern "C" int glh_debug_phase_stamps(glh_ctx* c, uint64_t* stamps) {
  CHK(need_seq(c));
  if (!stamps) return fail(GLH_E_INVALID, "null argument");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const size_t n = (size_t)c->P * PT_NSTAMP;
  if (!c->stamps) {
    // first call arms the stamps; the next fused steps record them
    CHK(c->stamps.alloc((size_t)c->cfg.max_points * PT_NSTAMP));
    HIPCHK(hipMemset(c->stamps, 0, (size_t)c->cfg.max_points * PT_NSTAMP * sizeof(unsigned long long)));
    memset(stamps, 0, n * sizeof(uint64_t));
    return GLH_OK;
  }
  DOWNLOAD(stamps, c->stamps, n, unsigned long long);
  return GLH_OK;
}

extern "C" int glh_set_highpass(glh_ctx* c, int size_x, int size_y) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (size_x < 1 || size_y < 1 || size_x > 7 || size_y > 7 || !(size_x & 1) || !(size_y & 1))
    return fail(GLH_E_UNSUPPORTED, "high-pass window %d x %d: sizes must be odd and at most 7", size_x, size_y);
  c->hp_rx = size_x / 2;
  c->hp_ry = size_y / 2 | (GLH_HP_MODE(c->hp_ry) << 4);  // (the boundary mode rides in the half height: glh_math.h)
  return GLH_OK;
}

extern "C" int glh_set_highpass_mode(glh_ctx* c, int mode) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (mode < GLH_HP_REFLECT || mode > GLH_HP_WRAP)
    return fail(GLH_E_UNSUPPORTED, "high-pass boundary mode %d: 0 reflect, 1 nearest, 2 mirror, 3 wrap", mode);
  c->hp_ry = GLH_HP_RY(c->hp_ry) | (mode << 4);
  return GLH_OK;
}

extern "C" int glh_set_interpolation(glh_ctx* c, int kx, int ky) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (kx < 1 || kx > GLH_SPL_KMAX || ky < 1 || ky > GLH_SPL_KMAX)
    return fail(GLH_E_UNSUPPORTED, "interpolation orders (%d, %d): each of 1 .. %d (RectBivariateSpline)", kx, ky,
                GLH_SPL_KMAX);
  HIPCHK(hipSetDevice(c->cfg.device_id));
  for (int q = 0; q < 2; ++q) {
    c->glu[q].reset();
    c->glu_off[q].reset();
  }
  c->interp_kx = kx;
  c->interp_ky = ky;
  c->interp_k = (kx == 3 && ky == 3) ? 3 : ((kx == 1 && ky == 1) ? 1 : 0);
  if (c->interp_k == 0) {
    // any other orders: banded factors of the degree-k collocation matrices for every surface side up to the workspace's
    const int maxn = c->cfg.max_search_dim;
    for (int q = 0; q < 2; ++q) {
      const int k = q == 0 ? kx : ky;
      std::vector<int64_t> off(maxn + 1, 0);
      int64_t total = 0;
      for (int n = k + 1; n <= maxn; ++n) {
        off[n] = total;
        total += (int64_t)(2 * k + 1) * n;
      }
      std::vector<double> lu((size_t)total);
      for (int n = k + 1; n <= maxn; ++n)
        if (!spline_lu_general(n, k, lu.data() + off[n]))
          return fail(GLH_E_STATE, "spline collocation matrix of size %d, degree %d has support outside its band", n, k);
      CHK(c->glu[q].alloc((size_t)total));
      CHK(c->glu_off[q].alloc((size_t)maxn + 1));
      HIPCHK(hipMemcpy(c->glu[q], lu.data(), (size_t)total * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c->glu_off[q], off.data(), (size_t)(maxn + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    }
  }
  return GLH_OK;
}

extern "C" int glh_set_math(glh_ctx* c, int mode) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (mode != GLH_MATH_EXACT && mode != GLH_MATH_FAST) return fail(GLH_E_INVALID, "mode must be GLH_MATH_EXACT or GLH_MATH_FAST");
  c->fast_math = mode == GLH_MATH_FAST;
  return GLH_OK;
}

extern "C" int glh_set_fused(glh_ctx* c, int on) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (on < 0 || on > 2) return fail(GLH_E_INVALID, "mode must be 0, 1 or 2");
  c->fused = on;
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// results
// ------------------------------------------------------------------------------------------
extern "C" int glh_get_moments(glh_ctx* c, int frame0, int n_frames, double* out) {
  CHK(need_seq(c));
  if (!out || frame0 < 0 || n_frames <= 0 || frame0 + n_frames > c->cfg.max_frames)
    return fail(GLH_E_INVALID, "bad frame range");
  DOWNLOAD(out, c->moments + (size_t)frame0 * c->P * 12, (size_t)n_frames * c->P * 12, double);
  return GLH_OK;
}

extern "C" int glh_get_tracks(glh_ctx* c, int frame0, int n_frames, double* means, double* sigmas) {
  CHK(need_seq(c));
  if (!means || !sigmas || frame0 < 0 || n_frames <= 0 || frame0 + n_frames > c->cfg.max_frames)
    return fail(GLH_E_INVALID, "bad frame range or null output");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  const size_t n = (size_t)n_frames * c->P * 6;
  CHK(c->tracks_tmp.reserve(2 * n));
  hipLaunchKernelGGL(k_tracks_layout, dim3((unsigned)((n + BLK - 1) / BLK)), dim3(BLK), 0, c->stream,
                     c->moments + (size_t)frame0 * c->P * 12, n_frames, c->P, c->tracks_tmp, c->tracks_tmp + n);
  HIPCHK(hipGetLastError());
  DOWNLOAD(means, c->tracks_tmp, n, double);
  DOWNLOAD(sigmas, c->tracks_tmp + n, n, double);
  return GLH_OK;
}

extern "C" int glh_get_moments_device(glh_ctx* c, void** p, uint64_t* bytes) {
  CHK(need_seq(c));
  if (!p || !bytes) return fail(GLH_E_INVALID, "null argument");
  *p = c->moments;
  *bytes = (uint64_t)c->cfg.max_frames * c->P * 12 * sizeof(double);
  return GLH_OK;
}

extern "C" int glh_get_template(glh_ctx* c, int o, int pt, int32_t* box, double* duv, double* tile,
                                double* hv, double* hq, int32_t* hn) {
  CHK(need_seq(c));
  CHK(check_obs(c, o));
  if (pt < 0 || pt >= c->P) return fail(GLH_E_INVALID, "point %d out of range", pt);
  const size_t slot = (size_t)o * c->P + pt;
  int32_t valid = 0;
  DOWNLOAD(&valid, c->tmpl_valid + slot, 1, int32_t);
  if (!valid) return fail(GLH_E_STATE, "no template for observer %d, point %d", o, pt);
  int32_t n = 0;
  DOWNLOAD(&n, c->tmpl_hist_n + slot, 1, int32_t);
  if (hn) *hn = n;
  if (box) DOWNLOAD(box, c->tmpl_box + slot * 4, 4, int32_t);
  if (duv) DOWNLOAD(duv, c->tmpl_duv + slot * 2, 2, double);
  if (tile) DOWNLOAD(tile, c->tmpl_tile64 + slot * c->tile_cap, (size_t)c->tw * c->th, double);
  if (hv) DOWNLOAD(hv, c->tmpl_hist_v + slot * c->tile_cap, (size_t)n, double);
  if (hq) DOWNLOAD(hq, c->tmpl_hist_q + slot * c->tile_cap, (size_t)n, double);
  return GLH_OK;
}

extern "C" int glh_get_likelihood_debug(glh_ctx* c, int o, int pt, double* uv, int32_t* box, float* search,
                                        double* sse) {
  CHK(need_seq(c));
  CHK(check_obs(c, o));
  if (pt < 0 || pt >= c->P) return fail(GLH_E_INVALID, "point %d out of range", pt);
  const size_t slot = (size_t)o * c->P + pt;
  int32_t st = 0;
  DOWNLOAD(&st, cur_status(c) + slot, 1, int32_t);
  if (uv) DOWNLOAD(uv, c->uv + slot * c->N * 2, (size_t)c->N * 2, double);
  if (st != GLH_OBS_OK) {
    if (box) box[0] = box[1] = box[2] = box[3] = -1;
    return GLH_OK;
  }
  int32_t b[4];
  DOWNLOAD(b, c->box + slot * 4, 4, int32_t);
  if (box) memcpy(box, b, sizeof b);
  const int ws = b[2] - b[0], hs = b[3] - b[1];
  if (search) DOWNLOAD(search, c->search + slot * (size_t)c->search_cap, (size_t)ws * hs, float);
  if (sse) {
    if (!c->keep_sse || !c->sse_copy) return fail(GLH_E_STATE, "SSE capture is off (glh_set_debug)");
    DOWNLOAD(sse, c->sse_copy + slot * (size_t)c->sse_cap, (size_t)(ws - c->tw + 1) * (hs - c->th + 1), double);
  }
  return GLH_OK;
}

extern "C" int glh_profile_enable(glh_ctx* c, int on) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  CHK(drain_profile(c));
  c->profiling = on != 0;
  return GLH_OK;
}
extern "C" int glh_profile_reset(glh_ctx* c) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  CHK(drain_profile(c));
  for (int i = 0; i < ST_COUNT; ++i) {
    c->ms[i] = 0;
    c->launches[i] = 0;
    c->launch_ms[i].clear();
    if (c->span_a[i]) c->pool.push_back(std::move(c->span_a[i]));  // (which leaves span_a[i] null)
    c->span_ms[i] = 0.f;
  }
  return GLH_OK;
}
extern "C" int glh_profile_get(glh_ctx* c, double* ms, int64_t* launches) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  CHK(drain_profile(c));
  for (int i = 0; i < ST_COUNT; ++i) {
    if (ms) ms[i] = c->ms[i];
    if (launches) launches[i] = c->launches[i];
  }
  return GLH_OK;
}

extern "C" int glh_profile_get_span(glh_ctx* c, int stage, double* ms) {
  if (!c || !ms || stage < 0 || stage >= ST_COUNT) return fail(GLH_E_INVALID, "bad argument");
  CHK(drain_profile(c));
  *ms = (double)c->span_ms[stage];
  return GLH_OK;
}

extern "C" int glh_profile_get_launches(glh_ctx* c, int stage, double* ms, int cap, int* n) {
  if (!c || !n || stage < 0 || stage >= ST_COUNT || cap < 0 || (cap > 0 && !ms))
    return fail(GLH_E_INVALID, "bad argument");
  CHK(drain_profile(c));
  const auto& v = c->launch_ms[stage];
  *n = (int)v.size();
  for (int i = 0; i < cap && i < (int)v.size(); ++i) ms[i] = (double)v[i];
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// multi-GPU: one process per GPU, one gather at the end of a sequence (glh_comm.h)
// ------------------------------------------------------------------------------------------
#define NCCLCHK(api, expr)                                                                         \
  do {                                                                                             \
    ncclResult_t r_ = (expr);                                                                      \
    if (r_ != ncclSuccess)                                                                         \
      return fail(GLH_E_COMM, "%s failed: %s (%s:%d)", #expr, (api)->GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

extern "C" int glh_comm_unique_id(char* id) {
  if (!id) return fail(GLH_E_INVALID, "id is null");
  RcclApi* api = rccl_api();
  if (!api) return fail(GLH_E_COMM, "%s", rccl_load_error());
  static_assert(GLH_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the id is RCCL's ncclUniqueId");
  ncclUniqueId u;
  NCCLCHK(api, api->GetUniqueId(&u));
  memcpy(id, u.internal, GLH_COMM_ID_BYTES);
  return GLH_OK;
}

static int comm_free(glh_ctx* c) {
  if (!c->comm) return GLH_OK;
  Comm* k = c->comm;
  c->comm = nullptr;
  (void)hipSetDevice(c->cfg.device_id);
  (void)hipStreamSynchronize(c->stream);
  RcclApi* api = rccl_api();
  if (k->comm && api) (void)api->CommDestroy(k->comm);
  delete k;  // (with its staging and scalar buffers)
  return GLH_OK;
}

extern "C" int glh_comm_destroy(glh_ctx* c) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  return comm_free(c);
}

extern "C" int glh_comm_init(glh_ctx* c, const char* id, int rank, int world) {
  if (!c || !id) return fail(GLH_E_INVALID, "null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(GLH_E_INVALID, "need 0 <= rank < world (got %d, %d)", rank, world);
  RcclApi* api = rccl_api();
  if (!api) return fail(GLH_E_COMM, "%s", rccl_load_error());
  CHK(comm_free(c));
  HIPCHK(hipSetDevice(c->cfg.device_id));
  Comm* k = new (std::nothrow) Comm();
  if (!k) return fail(GLH_E_NOMEM, "out of host memory");
  k->rank = rank;
  k->world = world;
  ncclUniqueId u;
  memcpy(u.internal, id, GLH_COMM_ID_BYTES);
  ncclResult_t r = api->CommInitRank(&k->comm, world, u, rank);
  if (r != ncclSuccess) {
    delete k;
    return fail(GLH_E_COMM, "ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, world, c->cfg.device_id,
                api->GetErrorString(r));
  }
  if (k->scalar.alloc(2) != GLH_OK) {
    (void)api->CommDestroy(k->comm);
    delete k;
    return GLH_E_NOMEM;
  }
  c->comm = k;
  return GLH_OK;
}

static int need_comm(glh_ctx* c) {
  if (!c) return fail(GLH_E_INVALID, "null context");
  if (!c->comm) return fail(GLH_E_STATE, "glh_comm_init has not been called");
  return GLH_OK;
}

// max over the ranks of one host double (the bench's max-over-ranks wall time); doubles as a barrier: it
// returns once every rank's stream has reached the reduction
extern "C" int glh_comm_max_f64(glh_ctx* c, double* value) {
  CHK(need_comm(c));
  if (!value) return fail(GLH_E_INVALID, "value is null");
  RcclApi* api = rccl_api();
  Comm* k = c->comm;
  HIPCHK(hipSetDevice(c->cfg.device_id));
  HIPCHK(hipMemcpyAsync(k->scalar, value, sizeof(double), hipMemcpyHostToDevice, c->stream));
  NCCLCHK(api, api->AllReduce(k->scalar, k->scalar + 1, 1, ncclDouble, ncclMax, k->comm, c->stream));
  HIPCHK(hipMemcpyAsync(value, k->scalar + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

extern "C" int glh_comm_barrier(glh_ctx* c) {
  double v = 0.0;
  CHK(join_uploads(c));
  return glh_comm_max_f64(c, &v);
}

// Gather of the posterior moments (and the per-point status words) to rank `root`:
//   every rank sends frames [frame0, frame0 + n_frames) of its moments history, a contiguous block of
//   n_frames * P_rank * 12 doubles, and its P_rank status words; the root receives the blocks rank after rank,
//   out = | rank 0: [n_frames][P_0][12] | rank 1: [n_frames][P_1][12] | ... (doubles), status = | P_0 | P_1 | ...
// One ncclGroup of sends / receives on the context's stream (the root's own block goes through the same
// send / receive pair); the root then downloads to the host buffers.  points_per_rank [world].
extern "C" int glh_gather_moments(glh_ctx* c, int root, int frame0, int n_frames, const int32_t* points_per_rank,
                                  double* out, uint32_t* status) {
  CHK(need_comm(c));
  CHK(need_seq(c));
  Comm* k = c->comm;
  RcclApi* api = rccl_api();
  if (root < 0 || root >= k->world || !points_per_rank) return fail(GLH_E_INVALID, "bad root / points_per_rank");
  if (frame0 < 0 || n_frames <= 0 || frame0 + n_frames > c->cfg.max_frames) return fail(GLH_E_INVALID, "bad frame range");
  if (points_per_rank[k->rank] != c->P)
    return fail(GLH_E_INVALID, "points_per_rank[%d] = %d, but this context tracks %d points", k->rank,
                points_per_rank[k->rank], c->P);
  const bool is_root = k->rank == root;
  HIPCHK(hipSetDevice(c->cfg.device_id));
  size_t total_pts = 0;
  for (int r = 0; r < k->world; ++r) {
    if (points_per_rank[r] < 0) return fail(GLH_E_INVALID, "points_per_rank[%d] < 0", r);
    total_pts += (size_t)points_per_rank[r];
  }
  const size_t mom_doubles = total_pts * (size_t)n_frames * 12;
  const size_t st_off = (mom_doubles * 8 + 15) & ~(size_t)15;  // bytes
  if (is_root) CHK(k->stage.reserve(st_off + total_pts * 4));
  const double* mine = c->moments + (size_t)frame0 * c->P * 12;
  NCCLCHK(api, api->GroupStart());
  ncclResult_t r1 = api->Send(mine, (size_t)n_frames * c->P * 12, ncclDouble, root, k->comm, c->stream);
  ncclResult_t r2 = api->Send(c->pt_status, (size_t)c->P, ncclUint32, root, k->comm, c->stream);
  ncclResult_t r3 = ncclSuccess;
  if (is_root) {
    double* dst = k->stage.as<double>();
    uint32_t* sdst = reinterpret_cast<uint32_t*>(k->stage.as<uint8_t>() + st_off);
    for (int r = 0; r < k->world && r3 == ncclSuccess; ++r) {
      const size_t pr = (size_t)points_per_rank[r];
      r3 = api->Recv(dst, pr * n_frames * 12, ncclDouble, r, k->comm, c->stream);
      if (r3 == ncclSuccess) r3 = api->Recv(sdst, pr, ncclUint32, r, k->comm, c->stream);
      dst += pr * n_frames * 12;
      sdst += pr;
    }
  }
  ncclResult_t r4 = api->GroupEnd();
  for (ncclResult_t r : {r1, r2, r3, r4})
    if (r != ncclSuccess) return fail(GLH_E_COMM, "moments gather failed: %s", api->GetErrorString(r));
  if (is_root) {
    k->gathered_doubles = mom_doubles;
    k->gathered_points = total_pts;
    k->gathered_status_off = st_off;
    if (out) HIPCHK(hipMemcpyAsync(out, k->stage.p, mom_doubles * 8, hipMemcpyDeviceToHost, c->stream));
    if (out && status)
      HIPCHK(hipMemcpyAsync(status, k->stage.as<uint8_t>() + st_off, total_pts * 4, hipMemcpyDeviceToHost,
                            c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

// Host copy of what the last glh_gather_moments left on the root's device (when it was called with out = NULL: the
// exchange itself is then all that a caller times).
extern "C" int glh_get_gathered(glh_ctx* c, double* out, uint32_t* status) {
  CHK(need_comm(c));
  Comm* k = c->comm;
  if (!k->stage.p || !k->gathered_doubles) return fail(GLH_E_STATE, "no gathered moments on this rank");
  if (!out) return fail(GLH_E_INVALID, "out is null");
  HIPCHK(hipSetDevice(c->cfg.device_id));
  HIPCHK(hipMemcpyAsync(out, k->stage.p, k->gathered_doubles * 8, hipMemcpyDeviceToHost, c->stream));
  if (status)
    HIPCHK(hipMemcpyAsync(status, k->stage.as<uint8_t>() + k->gathered_status_off, k->gathered_points * 4,
                          hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return GLH_OK;
}

// ------------------------------------------------------------------------------------------
// stateless stage hooks (parity tests): explicit inputs -> one kernel -> outputs
// ------------------------------------------------------------------------------------------
namespace {
int finish() {
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return GLH_OK;
}
}  // namespace

static int stage_project_impl(int dev, const double* cam, const double* xyz, int n, double* uv, int directions,
                              double* depth = nullptr) {
  if (!cam || !xyz || !uv || n <= 0) return fail(GLH_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(dev));
  CamDev cd;
  expand_camera(cam, &cd);
  DevBuf dc, dx, du, dd;
  CHK(dc.up(&cd, sizeof cd));
  CHK(dx.up(xyz, (size_t)n * 3 * sizeof(double)));
  CHK(du.alloc((size_t)n * 2 * sizeof(double)));
  if (depth) CHK(dd.alloc((size_t)n * sizeof(double)));
  hipLaunchKernelGGL(k_project_points, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, dc.as<CamDev>(),
                     dx.as<double>(), n, du.as<double>(), directions, depth ? dd.as<double>() : nullptr);
  CHK(finish());
  if (depth) CHK(dd.down(depth, (size_t)n * sizeof(double)));
  return du.down(uv, (size_t)n * 2 * sizeof(double));
}

extern "C" int glh_stage_project_depth(int dev, const double* cam, const double* xyz, int n, int directions,
                                       double* uv, double* depth) {
  if (!depth) return fail(GLH_E_INVALID, "bad argument");
  if (cam && cam[23] != 0.0) return fail(GLH_E_INVALID, "depth is a camera notion (not a raster grid)");
  return stage_project_impl(dev, cam, xyz, n, uv, directions ? 1 : 0, depth);
}

extern "C" int glh_stage_project(int dev, const double* cam, const double* xyz, int n, double* uv) {
  return stage_project_impl(dev, cam, xyz, n, uv, 0);
}

extern "C" int glh_stage_project_directions(int dev, const double* cam, const double* xyz, int n, double* uv) {
  if (cam && cam[23] != 0.0) return fail(GLH_E_INVALID, "ray directions are a camera notion (not a raster grid)");
  return stage_project_impl(dev, cam, xyz, n, uv, 1);
}

extern "C" int glh_stage_project_fast(int dev, const double* cam, const double* xyz, int n, int directions, int simple,
                                      double* uv) {
  if (!cam || !xyz || !uv || n <= 0) return fail(GLH_E_INVALID, "bad argument");
  if (directions && cam[23] != 0.0) return fail(GLH_E_INVALID, "ray directions are a camera notion (not a raster grid)");
  CamDev cd;
  expand_camera(cam, &cd);
  if (simple && ((cam_flags(cd) | (directions ? CAM_F_DIRECTIONS : 0u)) & CAM_F_NOT_SIMPLE))
    return fail(GLH_E_INVALID, "project_simple_fast does not cover this camera (CAM_F_NOT_SIMPLE)");
  HIPCHK(hipSetDevice(dev));
  DevBuf dc, dx, du;
  CHK(dc.up(&cd, sizeof cd));
  CHK(dx.up(xyz, (size_t)n * 3 * sizeof(double)));
  CHK(du.alloc((size_t)n * 2 * sizeof(double)));
  hipLaunchKernelGGL(k_project_points_fast, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, dc.as<CamDev>(), dx.as<double>(),
                     n, du.as<double>(), directions ? 1 : 0, simple ? 1 : 0);
  CHK(finish());
  return du.down(uv, (size_t)n * 2 * sizeof(double));
}

extern "C" int glh_stage_fast_math(int dev, int op, const double* args, int n, double* out) {
  if (!args || !out || n <= 0) return fail(GLH_E_INVALID, "bad argument");
  if (op < GLH_FM_RCP || op > GLH_FM_BILINEAR) return fail(GLH_E_INVALID, "op is not one of GLH_FM_*");
  HIPCHK(hipSetDevice(dev));
  DevBuf da, dout;
  CHK(da.up(args, (size_t)n * GLH_FM_ARGS * sizeof(double)));
  CHK(dout.alloc((size_t)n * sizeof(double)));
  hipLaunchKernelGGL(k_fast_math, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, op, da.as<double>(), n, dout.as<double>());
  CHK(finish());
  return dout.down(out, (size_t)n * sizeof(double));
}

extern "C" int glh_stage_unproject(int dev, const double* cam, const double* uv, int n, const double* depth,
                                   int n_depth, int directions, double* xyz) {
  if (!cam || !uv || !xyz || n <= 0) return fail(GLH_E_INVALID, "bad argument");
  if (cam[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "uv_to_xyz of a raster grid is not built");
  if (depth && n_depth != 1 && n_depth != n) return fail(GLH_E_INVALID, "depth must have 1 or n entries");
  HIPCHK(hipSetDevice(dev));
  CamDev cd;
  expand_camera(cam, &cd);
  DevBuf dc, du, dd, dx;
  CHK(dc.up(&cd, sizeof cd));
  CHK(du.up(uv, (size_t)n * 2 * sizeof(double)));
  if (depth) CHK(dd.up(depth, (size_t)n_depth * sizeof(double)));
  CHK(dx.alloc((size_t)n * 3 * sizeof(double)));
  hipLaunchKernelGGL(k_unproject_points, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, dc.as<CamDev>(),
                     du.as<double>(), n, depth ? dd.as<double>() : nullptr, n_depth, directions, dx.as<double>());
  CHK(finish());
  return dx.down(xyz, (size_t)n * 3 * sizeof(double));
}

// Image.project over a batch of frames, through the staging ring of glh_frame_ring.h: three slots and three streams, so
// that frame k + 1's upload and frame k - 1's download overlap frame k's kernel.
namespace {
template <typename T>
void launch_reproject(hipStream_t s, int channels, const CamDev* src_cam, const CamDev* dst_cam, const void* src, int sw,
                      int sh, int dw, int dh, int method, void* out) {
  const dim3 grid((dw + RPJ_BX - 1) / RPJ_BX, (dh + RPJ_BY - 1) / RPJ_BY), block(RPJ_BX, RPJ_BY);
  if (channels == 1)
    hipLaunchKernelGGL((k_reproject<T, 1>), grid, block, 0, s, src_cam, dst_cam, (const T*)src, sw, sh, dw, dh, method,
                       (T*)out);
  else
    hipLaunchKernelGGL((k_reproject<T, 3>), grid, block, 0, s, src_cam, dst_cam, (const T*)src, sw, sh, dw, dh, method,
                       (T*)out);
}
}  // namespace

extern "C" int glh_stage_reproject(int dev, const void* frames, int depth_bits, int is_float, int width, int height,
                                   int channels, int n_frames, const double* src_cams, const double* dst_cam,
                                   int dst_width, int dst_height, int method, void* out, double* kernel_ms) {
  if (!frames || !src_cams || !dst_cam || !out || n_frames < 1) return fail(GLH_E_INVALID, "bad argument");
  if (!((!is_float && (depth_bits == 8 || depth_bits == 16)) || (is_float && (depth_bits == 32 || depth_bits == 64))))
    return fail(GLH_E_UNSUPPORTED, "frames of %d bits (%s): uint8, uint16, float32 or float64", depth_bits,
                is_float ? "float" : "integer");
  if (channels != 1 && channels != 3) return fail(GLH_E_UNSUPPORTED, "1 or 3 channels");
  if (method != RPJ_LINEAR && method != RPJ_NEAREST) return fail(GLH_E_UNSUPPORTED, "method %d: 0 linear, 1 nearest", method);
  // (the interpolator needs two grid points on an axis; the pixel index arithmetic is 32-bit)
  if (width < 2 || height < 2 || dst_width < 1 || dst_height < 1 || width > 32768 || height > 32768 ||
      dst_width > 32768 || dst_height > 32768)
    return fail(GLH_E_INVALID, "frame %d x %d -> %d x %d: a source of at least 2 x 2, at most 32768 on a side", width,
                height, dst_width, dst_height);
  if (dst_cam[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "the target is a raster grid, not a camera");
  if ((int)dst_cam[6] != dst_width || (int)dst_cam[7] != dst_height)
    return fail(GLH_E_INVALID, "target camera imgsz (%g, %g) != target size (%d, %d)", dst_cam[6], dst_cam[7], dst_width,
                dst_height);
  std::vector<CamDev> cams(n_frames + 1);
  for (int i = 0; i < n_frames; ++i) {
    const double* v = src_cams + (size_t)i * GLH_CAM_LEN;
    if (v[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "frame %d is a raster grid, not a camera", i);
    if ((int)v[6] != width || (int)v[7] != height)
      return fail(GLH_E_INVALID, "camera %d imgsz (%g, %g) != frame size (%d, %d)", i, v[6], v[7], width, height);
    if (!(v[0] == dst_cam[0] && v[1] == dst_cam[1] && v[2] == dst_cam[2]))
      return fail(GLH_E_INVALID, "source camera %d and the target camera have different positions ('xyz')", i);
    expand_camera(v, &cams[i]);
  }
  expand_camera(dst_cam, &cams[n_frames]);
  HIPCHK(hipSetDevice(dev));
  const size_t px = (size_t)(depth_bits / 8) * channels;
  const size_t in_bytes = (size_t)width * height * px, out_bytes = (size_t)dst_width * dst_height * px;
  DevBuf dcams;
  CHK(dcams.up(cams.data(), cams.size() * sizeof(CamDev)));
  FrameRing r;
  CHK(r.open(n_frames, in_bytes, out_bytes, kernel_ms != nullptr));
  const CamDev* dc = dcams.as<CamDev>();
  auto launch = [&](int i, int k) {
    if (depth_bits == 8)
      launch_reproject<uint8_t>(r.run, channels, dc + i, dc + n_frames, r.dev_in[k], width, height, dst_width, dst_height,
                                method, r.dev_out[k]);
    else if (depth_bits == 16)
      launch_reproject<uint16_t>(r.run, channels, dc + i, dc + n_frames, r.dev_in[k], width, height, dst_width, dst_height,
                                 method, r.dev_out[k]);
    else if (depth_bits == 32)
      launch_reproject<float>(r.run, channels, dc + i, dc + n_frames, r.dev_in[k], width, height, dst_width, dst_height,
                              method, r.dev_out[k]);
    else
      launch_reproject<double>(r.run, channels, dc + i, dc + n_frames, r.dev_in[k], width, height, dst_width, dst_height,
                               method, r.dev_out[k]);
  };
  return r.process(frames, n_frames, out, launch, kernel_ms);
}

static int check_box(const int32_t* box, int width, int height) {
  if (!box || box[0] < 0 || box[1] < 0 || box[2] > width || box[3] > height || box[2] <= box[0] || box[3] <= box[1])
    return fail(GLH_E_INVALID, "box outside the frame");
  return GLH_OK;
}

static int check_highpass(int size_x, int size_y) {
  if (size_x < 1 || size_y < 1 || size_x > 7 || size_y > 7 || !(size_x & 1) || !(size_y & 1))
    return fail(GLH_E_UNSUPPORTED, "high-pass window %d x %d: sizes must be odd and at most 7", size_x, size_y);
  return GLH_OK;
}

extern "C" int glh_stage_template(int dev, const uint8_t* frame, int width, int height, int channels,
                                  const int32_t* box, double* tile, double* hv, double* hq, int32_t* hn) {
  return glh_stage_template_highpass(dev, frame, width, height, channels, box, 5, 5, GLH_HP_REFLECT, tile, hv, hq, hn);
}

extern "C" int glh_stage_template_highpass(int dev, const uint8_t* frame, int width, int height, int channels,
                                           const int32_t* box, int size_x, int size_y, int mode, double* tile, double* hv,
                                           double* hq, int32_t* hn) {
  if (!frame || !tile || !hv || !hq || !hn) return fail(GLH_E_INVALID, "null argument");
  CHK(check_highpass(size_x, size_y));
  if (mode < GLH_HP_REFLECT || mode > GLH_HP_WRAP) return fail(GLH_E_UNSUPPORTED, "high-pass boundary mode %d", mode);
  if (channels != 1 && channels != 3) return fail(GLH_E_UNSUPPORTED, "1 or 3 channels");
  CHK(check_box(box, width, height));
  HIPCHK(hipSetDevice(dev));
  const size_t n = (size_t)(box[2] - box[0]) * (box[3] - box[1]);
  if (n * 2 > 60000) return fail(GLH_E_INVALID, "template too large for the test hook");
  DevBuf df, t64, t32, dv, dq, dn;
  CHK(df.up(frame, (size_t)width * height * channels));
  CHK(t64.alloc(n * 8)); CHK(t32.alloc(n * 4)); CHK(dv.alloc(n * 8)); CHK(dq.alloc(n * 8)); CHK(dn.alloc(4));
  TemplateBoxArgs a{};
  a.frame = df.as<uint8_t>();
  a.width = width;
  a.channels = channels;
  for (int k = 0; k < 4; ++k) a.box[k] = box[k];
  a.out.tile64 = t64.as<double>();
  a.out.tile32 = t32.as<float>();
  a.out.hist_v = dv.as<double>();
  a.out.hist_q = dq.as<double>();
  a.out.hist_n = dn.as<int32_t>();
  a.hp_rx = size_x / 2;
  a.hp_ry = size_y / 2 | (mode << 4);
  hipLaunchKernelGGL(k_template_from_box, dim3(1), dim3(BLK), n * sizeof(uint16_t), 0, a);
  CHK(finish());
  CHK(dn.down(hn, 4));
  CHK(t64.down(tile, n * 8));
  CHK(dv.down(hv, (size_t)*hn * 8));
  return dq.down(hq, (size_t)*hn * 8);
}

extern "C" int glh_stage_search_tile(int dev, const uint8_t* frame, int width, int height, int channels,
                                     const int32_t* box, const double* hv, const double* hq, int hn, float* tile) {
  return glh_stage_search_tile_highpass(dev, frame, width, height, channels, box, hv, hq, hn, 5, 5, GLH_HP_REFLECT, tile);
}

extern "C" int glh_stage_search_tile_highpass(int dev, const uint8_t* frame, int width, int height, int channels,
                                              const int32_t* box, const double* hv, const double* hq, int hn,
                                              int size_x, int size_y, int mode, float* tile) {
  if (!frame || !tile || !hv || !hq || hn <= 0) return fail(GLH_E_INVALID, "bad argument");
  CHK(check_highpass(size_x, size_y));
  if (mode < GLH_HP_REFLECT || mode > GLH_HP_WRAP) return fail(GLH_E_UNSUPPORTED, "high-pass boundary mode %d", mode);
  if (channels != 1 && channels != 3) return fail(GLH_E_UNSUPPORTED, "1 or 3 channels");
  CHK(check_box(box, width, height));
  HIPCHK(hipSetDevice(dev));
  const int w = box[2] - box[0], h = box[3] - box[1];
  const size_t n = (size_t)w * h;
  if ((size_t)(BAND_H + 6) * w * 2 > 60000) return fail(GLH_E_INVALID, "tile too wide for the test hook");
  DevBuf df, dv, dq, dout;
  CHK(df.up(frame, (size_t)width * height * channels));
  CHK(dv.up(hv, (size_t)hn * 8));
  CHK(dq.up(hq, (size_t)hn * 8));
  CHK(dout.alloc(n * 4));
  SearchBoxArgs a{};
  a.frame = df.as<uint8_t>();
  a.width = width;
  a.channels = channels;
  for (int k = 0; k < 4; ++k) a.box[k] = box[k];
  a.hist_v = dv.as<double>();
  a.hist_q = dq.as<double>();
  a.hist_n = hn;
  a.hp_rx = size_x / 2;
  a.hp_ry = size_y / 2 | (mode << 4);
  a.out = dout.as<float>();
  hipLaunchKernelGGL(k_search_from_box, dim3(1), dim3(BLK), (size_t)(BAND_H + 6) * w * sizeof(uint16_t), 0, a);
  CHK(finish());
  return dout.down(tile, n * 4);
}

extern "C" int glh_stage_ssd(int dev, const float* search, int hs, int ws, const float* templ, int th, int tw,
                             float* sse) {
  if (!search || !templ || !sse || th <= 0 || tw <= 0 || hs < th || ws < tw) return fail(GLH_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(dev));
  const int ho = hs - th + 1, wo = ws - tw + 1;
  DevBuf ds, dt, dbox, dst, dout;
  CHK(ds.up(search, (size_t)hs * ws * 4));
  CHK(dt.up(templ, (size_t)th * tw * 4));
  int32_t box[4] = {0, 0, ws, hs};
  int32_t st = GLH_OBS_OK;
  CHK(dbox.up(box, sizeof box));
  CHK(dst.up(&st, sizeof st));
  CHK(dout.alloc((size_t)ho * wo * 8));
  SsdArgs a{};
  a.o = 0;
  a.P = 1;
  a.tw = tw;
  a.th = th;
  a.tile_cap = th * tw;
  a.search_cap = hs * ws;
  a.sse_cap = ho * wo;
  size_t lds = ssd_lds_bytes(tw, th);
  HIPCHK(hipFuncSetAttribute((const void*)k_ssd, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
  a.box = dbox.as<int32_t>();
  a.obs_status = dst.as<int32_t>();
  a.search = ds.as<float>();
  a.tmpl = dt.as<float>();
  a.sse = dout.as<double>();
  hipLaunchKernelGGL(k_ssd, dim3(4, 1), dim3(BLK), lds, 0, a);
  CHK(finish());
  std::vector<double> tmp((size_t)ho * wo);
  CHK(dout.down(tmp.data(), tmp.size() * 8));
  for (size_t i = 0; i < tmp.size(); ++i) sse[i] = (float)tmp[i];  // exact: values are float32 widened
  return GLH_OK;
}

static int stage_sample_impl(int dev, const float* sse, int ho, int wo, int kx, int ky, const double* box,
                             const double* uv, int n, double* values, uint8_t* outside);

extern "C" int glh_stage_sample(int dev, const float* sse, int ho, int wo, const double* box, const double* uv, int n,
                                double* values, uint8_t* outside) {
  return stage_sample_impl(dev, sse, ho, wo, 0, 0, box, uv, n, values, outside);
}

extern "C" int glh_stage_sample_orders(int dev, const float* sse, int ho, int wo, int kx, int ky, const double* box,
                                       const double* uv, int n, double* values, uint8_t* outside) {
  if (kx < 1 || kx > GLH_SPL_KMAX || ky < 1 || ky > GLH_SPL_KMAX)
    return fail(GLH_E_UNSUPPORTED, "interpolation orders (%d, %d): each of 1 .. %d", kx, ky, GLH_SPL_KMAX);
  return stage_sample_impl(dev, sse, ho, wo, kx, ky, box, uv, n, values, outside);
}

// kx = ky = 0: the bicubic default (k_spline_fit's own path + spline_eval); else the general orders
static int stage_sample_impl(int dev, const float* sse, int ho, int wo, int kx, int ky, const double* box,
                             const double* uv, int n, double* values, uint8_t* outside) {
  const int need_h = kx ? kx + 1 : 4, need_w = ky ? ky + 1 : 4;
  if (!sse || !box || !uv || !values || !outside || ho < need_h || wo < need_w || n <= 0)
    return fail(GLH_E_INVALID, "bad argument");
  HIPCHK(hipSetDevice(dev));
  if (kx) {
    std::vector<double> z((size_t)ho * wo);
    for (size_t i = 0; i < z.size(); ++i) z[i] = (double)sse[i];
    std::vector<double> fv((size_t)(2 * kx + 1) * ho), fu((size_t)(2 * ky + 1) * wo);
    if (!spline_lu_general(ho, kx, fv.data()) || !spline_lu_general(wo, ky, fu.data()))
      return fail(GLH_E_STATE, "spline collocation matrix has support outside its band");
    const int maxn = ho > wo ? ho : wo;
    std::vector<int64_t> zero(maxn + 1, 0);
    DevBuf dz, dfv, dfu, doff, dbox, dst, duv, dval, dout;
    CHK(dz.up(z.data(), z.size() * 8));
    CHK(dfv.up(fv.data(), fv.size() * 8));
    CHK(dfu.up(fu.data(), fu.size() * 8));
    CHK(doff.up(zero.data(), zero.size() * 8));
    int32_t ibox[4] = {0, 0, wo, ho};
    int32_t st = GLH_OBS_OK;
    CHK(dbox.up(ibox, sizeof ibox));
    CHK(dst.up(&st, sizeof st));
    SplineFitArgs sf{};
    sf.o = 0; sf.P = 1; sf.tw = 1; sf.th = 1; sf.sse_cap = ho * wo; sf.max_n = maxn;
    sf.box = dbox.as<int32_t>();
    sf.obs_status = dst.as<int32_t>();
    sf.sse = dz.as<double>();
    sf.kx = kx; sf.ky = ky;
    sf.glu_v = dfv.as<double>(); sf.glu_v_off = doff.as<int64_t>();
    sf.glu_u = dfu.as<double>(); sf.glu_u_off = doff.as<int64_t>();
    hipLaunchKernelGGL(k_spline_fit, dim3(1), dim3(BLK), 0, 0, sf);
    CHK(duv.up(uv, (size_t)n * 16));
    CHK(dval.alloc((size_t)n * 8));
    CHK(dout.alloc((size_t)n));
    SampleArgs sa{};
    sa.coef = dz.as<double>();
    sa.ho = ho; sa.wo = wo; sa.n = n; sa.kx = kx; sa.ky = ky;
    for (int k = 0; k < 4; ++k) sa.sb[k] = box[k];
    sa.uv = duv.as<double>();
    sa.values = dval.as<double>();
    sa.outside = dout.as<uint8_t>();
    hipLaunchKernelGGL(k_sample, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, sa);
    CHK(finish());
    CHK(dval.down(values, (size_t)n * 8));
    return dout.down(outside, (size_t)n);
  }
  const int maxn = ho > wo ? ho : wo;
  std::vector<int64_t> off(maxn + 1, 0);
  std::vector<double> lu;
  for (int m : {ho, wo}) {
    off[m] = (int64_t)lu.size();
    lu.resize(lu.size() + 5 * (size_t)m);
    spline_lu(m, lu.data() + off[m]);
  }
  std::vector<double> z((size_t)ho * wo);
  for (size_t i = 0; i < z.size(); ++i) z[i] = (double)sse[i];
  DevBuf dz, dlu, doff, dbox, dst, duv, dval, dout, dinv;
  {
    std::vector<double> inv((size_t)spline_inverse_off(GLH_SPL_DENSE_MAX + 1));
    for (int m = 4; m <= GLH_SPL_DENSE_MAX; ++m)
      if (m == ho || m == wo) spline_inverse(m, inv.data() + spline_inverse_off(m));
    CHK(dinv.up(inv.data(), inv.size() * 8));
  }
  CHK(dz.up(z.data(), z.size() * 8));
  CHK(dlu.up(lu.data(), lu.size() * 8));
  CHK(doff.up(off.data(), off.size() * 8));
  // k_spline_fit derives (wo, ho) from box and (tw, th): use tw = th = 1
  int32_t ibox[4] = {0, 0, wo, ho};
  int32_t st = GLH_OBS_OK;
  CHK(dbox.up(ibox, sizeof ibox));
  CHK(dst.up(&st, sizeof st));
  SplineFitArgs sf{};
  sf.o = 0; sf.P = 1; sf.tw = 1; sf.th = 1; sf.sse_cap = ho * wo; sf.max_n = maxn;
  sf.box = dbox.as<int32_t>();
  sf.obs_status = dst.as<int32_t>();
  sf.lu = dlu.as<double>();
  sf.lu_off = doff.as<int64_t>();
  sf.inv = dinv.as<double>();
  sf.sse = dz.as<double>();
  sf.sse_copy = nullptr;
  hipLaunchKernelGGL(k_spline_fit, dim3(1), dim3(BLK), 0, 0, sf);
  CHK(duv.up(uv, (size_t)n * 16));
  CHK(dval.alloc((size_t)n * 8));
  CHK(dout.alloc((size_t)n));
  SampleArgs sa{};
  sa.coef = dz.as<double>();
  sa.ho = ho; sa.wo = wo; sa.n = n;
  for (int k = 0; k < 4; ++k) sa.sb[k] = box[k];
  sa.uv = duv.as<double>();
  sa.values = dval.as<double>();
  sa.outside = dout.as<uint8_t>();
  hipLaunchKernelGGL(k_sample, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, sa);
  CHK(finish());
  CHK(dval.down(values, (size_t)n * 8));
  return dout.down(outside, (size_t)n);
}

extern "C" int glh_stage_raster_sample(int dev, const double* z, int nx, int ny, const double* gx, const double* gy,
                                       int sx, int sy, double xmin, double xmax, double ymin, double ymax,
                                       const double* xy, int n, int order, double* values, uint8_t* oob) {
  if (!z || !xy || !values || !oob || n <= 0 || (order != 0 && order != 1)) return fail(GLH_E_INVALID, "bad argument");
  CHK(check_raster_args(nx, ny, gx, gy, sx, sy));
  CHK(check_raster_uniform(nx, ny, gx, gy, xmin, xmax, ymin, ymax));
  HIPCHK(hipSetDevice(dev));
  DevBuf dz, dgx, dgy, dxy, dv, do_;
  CHK(dz.up(z, (size_t)nx * ny * 8));
  CHK(dgx.up(gx, (size_t)nx * 8));
  CHK(dgy.up(gy, (size_t)ny * 8));
  CHK(dxy.up(xy, (size_t)n * 16));
  CHK(dv.alloc((size_t)n * 8));
  CHK(do_.alloc((size_t)n));
  const RasterDev r = raster_dev(dz.as<double>(), dgx.as<double>(), dgy.as<double>(), nx, ny, sx, sy, xmin, xmax, ymin, ymax);
  hipLaunchKernelGGL(k_raster_sample, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, 0, r, dxy.as<double>(), n, order,
                     dv.as<double>(), do_.as<uint8_t>());
  CHK(finish());
  CHK(dv.down(values, (size_t)n * 8));
  return do_.down(oob, (size_t)n);
}

// What the stages below check alike, before a device is touched (`who` is the stage's name: every message begins with it).
static int check_grid(const char* who, int nx, int ny, int least) {
  if (nx < least || ny < least) return fail(GLH_E_INVALID, "%s: %d x %d cells: at least %d on each axis", who, nx, ny, least);
  if ((int64_t)nx * ny >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "%s: %d x %d cells: fewer than 2^31 are served (32-bit cell indices)", who, nx, ny);
  return GLH_OK;
}

// (GLH_VIEWSHED_*, GLH_PD_*, GLH_FILTER_* and GLH_TERRAIN_* number the two float types alike)
static_assert(GLH_VIEWSHED_F64 == 0 && GLH_PD_F64 == 0 && GLH_FILTER_F64 == 0 && GLH_TERRAIN_F64 == 0, "float64 is 0");
static_assert(GLH_VIEWSHED_F32 == 1 && GLH_PD_F32 == 1 && GLH_FILTER_F32 == 1 && GLH_TERRAIN_F32 == 1, "float32 is 1");
static int check_float_dtype(const char* who, const char* what, int dtype) {
  if (dtype != 0 && dtype != 1) return fail(GLH_E_UNSUPPORTED, "%s: %s %d: 0 float64, 1 float32", who, what, dtype);
  return GLH_OK;
}

static int check_origins(const char* who, const double* origins, int m) {
  for (int i = 0; i < 3 * m; ++i)
    if (!std::isfinite(origins[i])) return fail(GLH_E_INVALID, "%s: origin %d is not finite", who, i / 3);
  return GLH_OK;
}

static int check_correction(const char* who, int correction, double radius, double refraction) {
  if (correction && !(std::isfinite(radius) && radius != 0.0 && std::isfinite(refraction)))
    return fail(GLH_E_INVALID, "%s: correction with radius %g, refraction %g", who, radius, refraction);
  return GLH_OK;
}

// Raster.viewshed (raster.py:1293-1389): the arguments are checked here, before a device is touched; the kernels, the sort
// and the launches are glh_viewshed.hip's.
extern "C" int glh_stage_viewshed(int dev, const void* z, int z_dtype, int nx, int ny, const double* x, const double* y,
                                  double inv_cell, const double* origins, int m, int correction, double radius,
                                  double refraction, uint8_t* visible, double* times_ms) {
  if (!z || !x || !y || !origins || !visible) return fail(GLH_E_INVALID, "viewshed: null argument");
  if (m < 1) return fail(GLH_E_INVALID, "viewshed: %d origins: at least one", m);
  CHK(check_grid("viewshed", nx, ny, 1));
  CHK(check_float_dtype("viewshed", "z_dtype", z_dtype));
  if (!(std::isfinite(inv_cell) && inv_cell > 0.0)) return fail(GLH_E_INVALID, "viewshed: inverse cell size %g", inv_cell);
  for (int i = 0; i < nx; ++i)
    if (!std::isfinite(x[i])) return fail(GLH_E_INVALID, "viewshed: x[%d] is not finite", i);
  for (int i = 0; i < ny; ++i)
    if (!std::isfinite(y[i])) return fail(GLH_E_INVALID, "viewshed: y[%d] is not finite", i);
  CHK(check_origins("viewshed", origins, m));
  CHK(check_correction("viewshed", correction, radius, refraction));
  const ViewshedJob job{dev, z, z_dtype == GLH_VIEWSHED_F32, nx, ny, x, y, inv_cell, origins, m, correction != 0, radius,
                        refraction, visible, times_ms};
  for (int o = 0; o < m; ++o) {
    const double far = viewshed_farthest_cells(job, origins + 3 * o);
    if (!(far < (double)VS_MAX_RINGS))
      return fail(GLH_E_UNSUPPORTED, "viewshed: origin %d is %g cells from the DEM's farthest cell (fewer than %d are served)", o,
                  far, VS_MAX_RINGS);
  }
  return viewshed_run(job);
}

// Raster.horizon (raster.py:1391-1463): the arguments are checked here, before a device is touched; the kernel and the
// launch are glh_horizon.hip's.
extern "C" int glh_stage_horizon(int dev, const void* z, int z_dtype, int nx, int ny, double xlim0, double ylim0, double d0,
                                 double d1, const double* origins, const int32_t* starts, const int32_t* ends, int m, int n,
                                 int correction, double radius, double refraction, int32_t* cell, double* dz,
                                 double* times_ms) {
  if (!z || !origins || !starts || !ends || !cell || !dz) return fail(GLH_E_INVALID, "horizon: null argument");
  if (m < 1 || n < 1) return fail(GLH_E_INVALID, "horizon: %d origins, %d headings: at least one of each", m, n);
  CHK(check_grid("horizon", nx, ny, 1));
  if ((int64_t)m * n >= ((int64_t)1 << 24))  // (one workgroup of up to 256 lanes per line: a launch holds fewer than 2^32)
    return fail(GLH_E_INVALID, "horizon: %d origins x %d headings: fewer than 2^24 lines are served", m, n);
  CHK(check_float_dtype("horizon", "z_dtype", z_dtype));
  if (!(std::isfinite(xlim0) && std::isfinite(ylim0) && std::isfinite(d0) && std::isfinite(d1) && d0 != 0.0 && d1 != 0.0))
    return fail(GLH_E_INVALID, "horizon: corner (%g, %g), cell size (%g, %g)", xlim0, ylim0, d0, d1);
  CHK(check_origins("horizon", origins, m));
  CHK(check_correction("horizon", correction, radius, refraction));
  for (int o = 0; o < m; ++o)
    if (starts[2 * o] < 0 || starts[2 * o] >= nx || starts[2 * o + 1] < 0 || starts[2 * o + 1] >= ny)
      return fail(GLH_E_INVALID, "horizon: start cell (col %d, row %d) of origin %d is outside the %d x %d grid", starts[2 * o],
                  starts[2 * o + 1], o, nx, ny);
  for (int64_t i = 0; i < (int64_t)m * n; ++i)
    if (ends[2 * i] < 0 || ends[2 * i] >= nx || ends[2 * i + 1] < 0 || ends[2 * i + 1] >= ny)
      return fail(GLH_E_INVALID, "horizon: end cell (col %d, row %d) of origin %d, heading %d is outside the %d x %d grid",
                  ends[2 * i], ends[2 * i + 1], (int)(i / n), (int)(i % n), nx, ny);
  const HorizonJob job{dev, z, z_dtype == GLH_VIEWSHED_F32, nx, ny, xlim0, ylim0, d0, d1, origins, starts, ends, m, n,
                       correction != 0, radius, refraction, cell, dz, times_ms};
  return horizon_run(job);
}

// optimize.ObserverCameras.fit's objective and gradient (optimize.py:2047-2072) and Camera._uv_to_xy (camera.py:1510-1519):
// the arguments are checked here, before a device is touched; the kernels and the launches are glh_orient.hip's, and so is
// the handle: glh_orient, like glh_match, glh_sift and glh_calib below, is defined by its stage file.
extern "C" int glh_orient_create(int dev, int n_images, int n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                                 const int64_t* pair_offset, const double* xy_i, const double* xy_j, glh_orient** handle) {
  if (!handle) return fail(GLH_E_INVALID, "orient: null handle pointer");
  *handle = nullptr;
  if (n_images < 1 || n_pairs < 0) return fail(GLH_E_INVALID, "orient: %d images, %d pairs", n_images, n_pairs);
  if (n_images >= (1 << 24) || n_pairs >= (1 << 30))
    return fail(GLH_E_INVALID, "orient: %d images, %d pairs: fewer than 2^24 images and 2^30 pairs are served", n_images, n_pairs);
  if (!pair_offset || (n_pairs && (!pair_i || !pair_j))) return fail(GLH_E_INVALID, "orient: null pair arrays");
  if (pair_offset[0] != 0) return fail(GLH_E_INVALID, "orient: pair_offset[0] is %lld, not 0", (long long)pair_offset[0]);
  int64_t chunks = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (pair_offset[p + 1] < pair_offset[p])
      return fail(GLH_E_INVALID, "orient: pair_offset decreases at pair %d (%lld after %lld)", p, (long long)pair_offset[p + 1],
                  (long long)pair_offset[p]);
    if (pair_i[p] < 0 || pair_i[p] >= n_images || pair_j[p] < 0 || pair_j[p] >= n_images)
      return fail(GLH_E_INVALID, "orient: pair %d joins images %d and %d of %d", p, pair_i[p], pair_j[p], n_images);
    chunks += (pair_offset[p + 1] - pair_offset[p] + OR_CHUNK - 1) / OR_CHUNK;
  }
  if (chunks >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "orient: %lld matches: fewer than 2^31 chunks of %d are served", (long long)pair_offset[n_pairs],
                OR_CHUNK);
  if (pair_offset[n_pairs] > 0 && (!xy_i || !xy_j)) return fail(GLH_E_INVALID, "orient: null match coordinates");
  return orient_create(dev, n_images, n_pairs, pair_i, pair_j, pair_offset, xy_i, xy_j, handle);
}

extern "C" int glh_orient_eval(glh_orient* handle, const double* R, const double* Rprime, double* objective, double* gradient,
                               double* times_ms) {
  if (!handle) return fail(GLH_E_INVALID, "orient: null handle");
  if (!R || !Rprime || !objective || !gradient) return fail(GLH_E_INVALID, "orient: null argument");
  return orient_eval(handle, R, Rprime, objective, gradient, times_ms);
}

extern "C" int glh_orient_destroy(glh_orient* handle) {
  orient_destroy(handle);  // (nothing on null)
  return GLH_OK;
}

extern "C" int glh_stage_uv_to_xy(int dev, const double* cam, const double* uv, int n, double* xy) {
  if (!cam || !uv || !xy || n <= 0) return fail(GLH_E_INVALID, "uv_to_xy: bad argument");
  if (cam[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "uv_to_xy of a raster grid is not built");
  CamDev cd;
  expand_camera(cam, &cd);
  return uv_to_xy_run(dev, cd, uv, n, xy);
}

// optimize.match_keypoints' nearest-neighbour search (optimize.py:2234-2309): the arguments are checked here, before a
// device is touched; the kernels and the launches are glh_match.hip's.
extern "C" int glh_match_create(int dev, glh_match** handle) {
  if (!handle) return fail(GLH_E_INVALID, "match: null handle pointer");
  *handle = nullptr;
  if (dev < 0) return fail(GLH_E_INVALID, "match: device %d", dev);
  return match_create(dev, handle);
}

extern "C" int glh_match_put(glh_match* handle, int slot, int kind, int n, int dim, const void* data) {
  if (!handle) return fail(GLH_E_INVALID, "match: null handle");
  if (slot < 0) return fail(GLH_E_INVALID, "match: slot %d", slot);
  if (kind != GLH_MATCH_U8 && kind != GLH_MATCH_F32) return fail(GLH_E_INVALID, "match: unknown kind %d", kind);
  if (n == 0) return fail(GLH_E_INVALID, "match: a set of 0 rows (n == 0) cannot be searched");
  if (n < 0 || n > MT_MAX_ROWS) return fail(GLH_E_INVALID, "match: %d rows: 1 .. 2^30 are served", n);
  const int max_dim = kind == GLH_MATCH_U8 ? MT_U8_MAX_DIM : MT_MAX_DIM;
  if (dim < 1 || dim > max_dim)
    return fail(GLH_E_INVALID, "match: dim %d: 1 .. %d are served for %s", dim, max_dim, kind == GLH_MATCH_U8 ? "uint8" : "float32");
  if ((int64_t)n * ((dim + 31) / 32 * 32) > MT_MAX_ELEMS)
    return fail(GLH_E_INVALID, "match: %d rows of %d elements: at most 2^35 padded elements a set are served", n, dim);
  if (!data) return fail(GLH_E_INVALID, "match: null data");
  return match_put(handle, slot, kind, n, dim, data);
}

extern "C" int glh_match_drop(glh_match* handle, int slot) {
  if (!handle) return fail(GLH_E_INVALID, "match: null handle");
  MatchSetInfo s;
  if (!match_info(handle, slot, &s)) return fail(GLH_E_INVALID, "match: unknown slot %d", slot);
  match_drop(handle, slot);
  return GLH_OK;
}

extern "C" int glh_match_knn2(glh_match* handle, int slot_q, int slot_t, int32_t* idx, float* d2, double* times_ms) {
  if (!handle) return fail(GLH_E_INVALID, "match: null handle");
  if (!idx || !d2) return fail(GLH_E_INVALID, "match: null argument");
  MatchSetInfo q, t;
  if (!match_info(handle, slot_q, &q)) return fail(GLH_E_INVALID, "match: unknown slot %d", slot_q);
  if (!match_info(handle, slot_t, &t)) return fail(GLH_E_INVALID, "match: unknown slot %d", slot_t);
  if (q.kind != t.kind)
    return fail(GLH_E_INVALID, "match: mixed kinds: slot %d is %s, slot %d is %s", slot_q, q.kind == GLH_MATCH_U8 ? "uint8" : "float32",
                slot_t, t.kind == GLH_MATCH_U8 ? "uint8" : "float32");
  if (q.dim != t.dim) return fail(GLH_E_INVALID, "match: dim mismatch: slot %d has %d, slot %d has %d", slot_q, q.dim, slot_t, t.dim);
  return match_knn2(handle, slot_q, slot_t, idx, d2, times_ms);
}

extern "C" int glh_match_destroy(glh_match* handle) {
  match_destroy(handle);  // (nothing on null)
  return GLH_OK;
}

// optimize.SIFT (INPUTS.md, "SIFT: the rule"): the arguments are checked here, before a device is touched; the kernels and
// the launches are glh_sift.hip's.
extern "C" int glh_sift_create(int dev, glh_sift** handle) {
  if (!handle) return fail(GLH_E_INVALID, "sift: null handle pointer");
  *handle = nullptr;
  if (dev < 0) return fail(GLH_E_INVALID, "sift: device %d", dev);
  return sift_create(dev, handle);
}

extern "C" int glh_sift_detect(glh_sift* handle, const uint8_t* image, int w, int h, const double* params, int* n,
                               double* times_ms) {
  if (!handle) return fail(GLH_E_INVALID, "sift: null handle");
  if (!image || !params || !n) return fail(GLH_E_INVALID, "sift: null argument");
  if (w < 1 || h < 1 || w > SF_MAX_SIDE || h > SF_MAX_SIDE)
    return fail(GLH_E_INVALID, "sift: an image of %d x %d: sides of 1 .. 2^23 are served", w, h);
  if ((int64_t)(2 * (int64_t)w) * (2 * (int64_t)h) >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "sift: an image of %d x %d doubles to 2^31 cells or more", w, h);
  SiftParams p;
  if (!(params[0] >= 1.0 && params[0] <= (double)SF_MAX_LAYERS) || params[0] != floor(params[0]))
    return fail(GLH_E_INVALID, "sift: nOctaveLayers %g: 1 .. %d are served", params[0], SF_MAX_LAYERS);
  p.S = (int)params[0];
  p.contrast = params[1];
  p.edge = params[2];
  p.sigma = params[3];
  if (!(p.contrast >= 0.0 && p.contrast <= 1e6)) return fail(GLH_E_INVALID, "sift: contrastThreshold %g", p.contrast);
  if (!(p.edge > 0.0 && p.edge <= 1e6)) return fail(GLH_E_INVALID, "sift: edgeThreshold %g", p.edge);
  if (!(p.sigma > 0.0 && p.sigma <= SF_MAX_SIGMA)) return fail(GLH_E_INVALID, "sift: sigma %g: 0 < sigma <= %g is served", p.sigma, SF_MAX_SIGMA);
  const double* table = params + 4 + p.S + 3;
  for (int i = 0; i < p.S + 3; ++i) {
    const double r = params[4 + i];
    if (!(r >= 0.0 && r <= (double)SF_MAX_RADIUS) || r != floor(r))
      return fail(GLH_E_INVALID, "sift: the radius of table %d is %g: 0 .. %d are served", i, r, SF_MAX_RADIUS);
    p.radius[i] = (int)r;
    p.table[i] = table;
    table += 2 * p.radius[i] + 1;
  }
  return sift_detect(handle, image, w, h, p, n, times_ms);
}

extern "C" int glh_sift_read(glh_sift* handle, double* keypoints, uint8_t* descriptors) {
  if (!handle) return fail(GLH_E_INVALID, "sift: null handle");
  if (!keypoints || !descriptors) return fail(GLH_E_INVALID, "sift: null argument");
  return sift_read(handle, keypoints, descriptors);
}

extern "C" int glh_sift_counts(glh_sift* handle, int32_t* counts) {
  if (!handle) return fail(GLH_E_INVALID, "sift: null handle");
  if (!counts) return fail(GLH_E_INVALID, "sift: null argument");
  sift_counts(handle, counts);
  return GLH_OK;
}

extern "C" int glh_sift_layer(glh_sift* handle, int kind, int octave, int index, void* out) {
  if (!handle) return fail(GLH_E_INVALID, "sift: null handle");
  if (!out) return fail(GLH_E_INVALID, "sift: null argument");
  return sift_layer(handle, kind, octave, index, out);
}

extern "C" int glh_sift_destroy(glh_sift* handle) {
  sift_destroy(handle);  // (nothing on null)
  return GLH_OK;
}

// optimize.Cameras' predictions (optimize.py:1721-1764): the arguments are checked here, before a device is touched; the
// kernels and the launches are glh_calib.hip's.
extern "C" int glh_calib_create(int dev, int n_cams, int n_controls, const int32_t* kind, const int32_t* cam_a,
                                const int32_t* cam_b, const int32_t* directions, const int64_t* row_offset, const double* obs,
                                const double* src, glh_calib** handle) {
  if (!handle) return fail(GLH_E_INVALID, "calib: null handle pointer");
  *handle = nullptr;
  if (n_cams < 1 || n_controls < 0) return fail(GLH_E_INVALID, "calib: %d cameras, %d controls", n_cams, n_controls);
  if (n_cams >= (1 << 20) || n_controls >= (1 << 24))
    return fail(GLH_E_INVALID, "calib: %d cameras, %d controls: fewer than 2^20 cameras and 2^24 controls are served", n_cams,
                n_controls);
  if (!row_offset || (n_controls && (!kind || !cam_a || !cam_b || !directions)))
    return fail(GLH_E_INVALID, "calib: null control arrays");
  if (row_offset[0] != 0) return fail(GLH_E_INVALID, "calib: row_offset[0] is %lld, not 0", (long long)row_offset[0]);
  for (int c = 0; c < n_controls; ++c) {
    if (row_offset[c + 1] < row_offset[c])
      return fail(GLH_E_INVALID, "calib: row_offset decreases at control %d (%lld after %lld)", c, (long long)row_offset[c + 1],
                  (long long)row_offset[c]);
    if (kind[c] < GLH_CALIB_POINTS || kind[c] > GLH_CALIB_ROTATION_XY)
      return fail(GLH_E_INVALID, "calib: control %d is of unknown kind %d", c, kind[c]);
    const bool pair = kind[c] >= GLH_CALIB_MATCHES;
    if (cam_a[c] < 0 || cam_a[c] >= n_cams || (pair && (cam_b[c] < 0 || cam_b[c] >= n_cams)))
      return fail(GLH_E_INVALID, "calib: control %d names cameras %d and %d of %d", c, cam_a[c], cam_b[c], n_cams);
  }
  if (row_offset[n_controls] >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "calib: %lld rows: fewer than 2^31 are served", (long long)row_offset[n_controls]);
  if (row_offset[n_controls] > 0 && (!obs || !src)) return fail(GLH_E_INVALID, "calib: null coordinates");
  std::vector<int32_t> b(cam_b, cam_b + n_controls);
  for (int c = 0; c < n_controls; ++c)
    if (kind[c] < GLH_CALIB_MATCHES) b[c] = cam_a[c];  // (one camera: both names are it)
  const CalibControls cc{n_cams, n_controls, kind, cam_a, b.data(), directions, row_offset, obs, src};
  return calib_create(dev, cc, handle);
}

// The camera vectors of a calibration call, expanded for the device; a raster-grid camera is refused in `who`'s name.
static int calib_cameras(const char* who, const double* cams, size_t count, std::vector<CamDev>& out) {
  out.resize(count);
  for (size_t i = 0; i < count; ++i) {
    if (cams[i * GLH_CAM_LEN + 23] != 0.0) return fail(GLH_E_UNSUPPORTED, "%s: camera %zu is a raster grid", who, i);
    expand_camera(cams + i * GLH_CAM_LEN, &out[i]);
  }
  return GLH_OK;
}

extern "C" int glh_calib_eval(glh_calib* handle, int n_sets, const double* cams, const double* rot, int n_jobs,
                              const int32_t* job_control, const int32_t* job_set, const int32_t* job_side,
                              const int64_t* job_seg, const int64_t* seg_vertex, const int64_t* seg_count,
                              const double* seg_par, int64_t n_vertices, const double* vertex, double* predicted,
                              double* times_ms) {
  if (!handle) return fail(GLH_E_INVALID, "calib: null handle");
  const CalibTable table = calib_table(handle);  // (the controls it was made with)
  if (n_sets < 1 || n_jobs < 0 || n_vertices < 0) return fail(GLH_E_INVALID, "calib: %d sets, %d jobs", n_sets, n_jobs);
  if ((int64_t)n_sets * table.n_cams >= ((int64_t)1 << 24))
    return fail(GLH_E_INVALID, "calib: %d sets of %d cameras: fewer than 2^24 cameras in all are served", n_sets, table.n_cams);
  if (!cams || !rot || !job_seg || !seg_vertex || (n_jobs && (!job_control || !job_set || !job_side)))
    return fail(GLH_E_INVALID, "calib: null argument");
  if (job_seg[0] != 0 || seg_vertex[0] != 0) return fail(GLH_E_INVALID, "calib: the segment table does not start at 0");
  const int n_controls = table.n_controls;
  int64_t rows = 0, points = 0;
  for (int q = 0; q < n_jobs; ++q) {
    if (job_control[q] < 0 || job_control[q] >= n_controls || job_set[q] < 0 || job_set[q] >= n_sets || job_side[q] < 0 ||
        job_side[q] > 1)
      return fail(GLH_E_INVALID, "calib: job %d is control %d of %d, set %d of %d, side %d", q, job_control[q], n_controls,
                  job_set[q], n_sets, job_side[q]);
    const int64_t n_segs = job_seg[q + 1] - job_seg[q];
    const bool lines = table.kind[job_control[q]] == GLH_CALIB_LINES;
    if (n_segs < 0 || n_segs >= ((int64_t)1 << 31) || (lines ? n_segs < 1 : n_segs != 0))
      return fail(GLH_E_INVALID, "calib: job %d (%s) has %lld segments", q, lines ? "lines" : "not lines", (long long)n_segs);
    if (lines && job_side[q] != 0) return fail(GLH_E_INVALID, "calib: job %d (lines) has side %d", q, job_side[q]);
    if (n_segs && (!seg_count || !seg_par || !vertex)) return fail(GLH_E_INVALID, "calib: null segment table");
    int64_t job_points = 0;
    for (int64_t k = job_seg[q]; k < job_seg[q + 1]; ++k) {
      if (seg_vertex[k + 1] <= seg_vertex[k] || seg_vertex[k + 1] > n_vertices || seg_count[k] < 1 ||
          seg_count[k] >= ((int64_t)1 << 31))
        return fail(GLH_E_INVALID, "calib: segment %lld has vertices %lld .. %lld of %lld and %lld points", (long long)k,
                    (long long)seg_vertex[k], (long long)seg_vertex[k + 1], (long long)n_vertices, (long long)seg_count[k]);
      job_points += seg_count[k];
    }
    if (job_points >= ((int64_t)1 << 31)) return fail(GLH_E_INVALID, "calib: job %d has %lld points", q, (long long)job_points);
    rows += table.row_offset[job_control[q] + 1] - table.row_offset[job_control[q]];
    points += job_points;
  }
  if (rows >= ((int64_t)1 << 31) || points >= ((int64_t)1 << 31) || n_vertices >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "calib: %lld rows, %lld points, %lld vertices: fewer than 2^31 of each are served", (long long)rows,
                (long long)points, (long long)n_vertices);
  if (rows > 0 && !predicted) return fail(GLH_E_INVALID, "calib: null output");
  std::vector<CamDev> cd;
  CHK(calib_cameras("calib", cams, (size_t)n_sets * table.n_cams, cd));
  const CalibEval e{n_sets, cd.data(), rot, n_jobs, job_control, job_set, job_side, job_seg, seg_vertex, seg_count, seg_par,
                    vertex, predicted, times_ms};
  return calib_eval(handle, e);
}

// optimize.ransac(batched=True): every row set fitted, and scored, in one call.  Checked here, before a device is touched.
extern "C" int glh_calib_fit_sets(glh_calib* handle, const double* cams, int fit_cam, int p, const int32_t* slots,
                                  const double* x0, const double* lb, const double* ub, const double* x_scale,
                                  const double* weights, const double* observed, int n_sets, const int64_t* set_offset,
                                  const int64_t* set_rows,
                                  int max_nfev, double ftol, double xtol, double gtol, int score, double max_error, double* x,
                                  int32_t* status, double* mean_error, uint8_t* inlier, double* times_ms) {
  if (!handle) return fail(GLH_E_INVALID, "calib fit: null handle");
  const CalibTable table = calib_table(handle);
  CalibFit f{{p, slots, x0, lb, ub, x_scale, max_nfev, ftol, xtol, gtol}, nullptr, cams, fit_cam, weights, observed, n_sets,
             set_offset, set_rows, score, max_error, x, status, mean_error, inlier, times_ms};
  char why[400];
  if (!fs_check(table, f, why, sizeof(why))) return fail(GLH_E_INVALID, "%s", why);
  std::vector<CamDev> cd;
  CHK(calib_cameras("calib fit", cams, (size_t)table.n_cams, cd));
  f.cams = cd.data();
  return calib_fit_sets(handle, f);
}

// optimize.ransac_pairs: RANSAC over many groups (one match control, one fitted camera each) in one pass, served from the
// CalibRansac its entry point filled.  The checks are glh_ransac_plan.h's rg_check, made before a device is touched.
static int ransac_groups(glh_calib* handle, CalibRansac& r) {
  if (!handle) return fail(GLH_E_INVALID, "ransac groups: null handle");
  const CalibTable table = calib_table(handle);
  if (!r.vectors) return fail(GLH_E_INVALID, "ransac groups: null argument");
  char why[400];
  if (!rg_check(table, r, why, sizeof(why))) return fail(GLH_E_INVALID, "%s", why);
  std::vector<CamDev> cd;
  CHK(calib_cameras("ransac groups", r.vectors, (size_t)table.n_cams, cd));
  r.cams = cd.data();
  static const uint8_t none = 0;  // (no group: the flags still have an address, which is what says that the call draws)
  if (r.draws && !r.n_groups) r.drawn = &none;
  return calib_ransac_groups(handle, r);
}

extern "C" int glh_calib_ransac_groups(glh_calib* handle, const double* cams, int n_groups, const int32_t* group_control,
                                       const int32_t* group_cam, int p, const int32_t* slots, const double* x0, const double* lb,
                                       const double* ub, const double* x_scale, const double* weights, const double* observed,
                                       const int64_t* hyp_offset, int n, const int64_t* samples, int max_nfev, double ftol,
                                       double xtol, double gtol, double max_error, int64_t min_inliers, double* x, int32_t* status,
                                       int32_t* consensus, double* refit_x, int32_t* refit_status, double* mean_error,
                                       int32_t* winner, uint8_t* inlier, double* times_ms) {
  CalibRansac r{{p, slots, x0, lb, ub, x_scale, max_nfev, ftol, xtol, gtol}, nullptr, cams, n_groups, group_control, group_cam,
                weights, observed, hyp_offset, n, samples, max_error, min_inliers, x, status, consensus, refit_x, refit_status,
                mean_error, winner, inlier, times_ms};
  return ransac_groups(handle, r);
}

// The same with the samples of the groups it names drawn on the device (INPUTS.md, "Device samples: the rule").
extern "C" int glh_calib_ransac_groups_drawn(glh_calib* handle, const double* cams, int n_groups, const int32_t* group_control,
                                             const int32_t* group_cam, int p, const int32_t* slots, const double* x0,
                                             const double* lb, const double* ub, const double* x_scale, const double* weights,
                                             const double* observed, const int64_t* hyp_offset, int n, const int64_t* samples,
                                             int max_nfev, double ftol, double xtol, double gtol, double max_error,
                                             int64_t min_inliers, double* x, int32_t* status, int32_t* consensus, double* refit_x,
                                             int32_t* refit_status, double* mean_error, int32_t* winner, uint8_t* inlier,
                                             const int32_t* group_id, const uint8_t* drawn, uint32_t seed0, uint32_t seed1,
                                             int64_t* samples_out, double* times_ms) {
  CalibRansac r{{p, slots, x0, lb, ub, x_scale, max_nfev, ftol, xtol, gtol}, nullptr, cams, n_groups, group_control, group_cam,
                weights, observed, hyp_offset, n, samples, max_error, min_inliers, x, status, consensus, refit_x, refit_status,
                mean_error, winner, inlier, times_ms, true, group_id, drawn, seed0, seed1, samples_out};
  return ransac_groups(handle, r);
}

// What optimize.ransac_pairs(samples="device") gives each pair (glh_ransac_draw.h: rd_hypotheses).  Host arithmetic only.
extern "C" int glh_ransac_hypotheses(int n_groups, const int64_t* rows, int n, int64_t iterations, int64_t* hyps,
                                     uint8_t* enumerated) {
  if (n_groups < 0 || (n_groups && (!rows || !hyps || !enumerated)))
    return fail(GLH_E_INVALID, "ransac hypotheses: %d groups or a null argument", n_groups);
  if (n < 1 || iterations < 0 || iterations > RANSAC_DRAW_LIMIT)
    return fail(GLH_E_INVALID, "ransac hypotheses: samples of %d rows, %lld iterations: at least 1 row, 0 .. 2^31 - 1 iterations", n,
                (long long)iterations);
  for (int g = 0; g < n_groups; ++g)
    if (rows[g] < 0 || rows[g] > RANSAC_DRAW_LIMIT)
      return fail(GLH_E_INVALID, "ransac hypotheses: group %d has %lld rows: 0 .. 2^31 - 1", g, (long long)rows[g]);
  for (int g = 0; g < n_groups; ++g) {
    bool all = false;
    hyps[g] = rd_hypotheses(rows[g], n, iterations, &all);
    enumerated[g] = all ? 1 : 0;
  }
  return GLH_OK;
}

// The hypotheses of an enumerated pair (glh_ransac_draw.h: rd_enumerate).  Host arithmetic only.
extern "C" int glh_ransac_combinations(int64_t rows, int n, int64_t count, int64_t* samples) {
  if (n < 1 || rows < n || rows > RANSAC_DRAW_LIMIT || count < 0 || count > RANSAC_DRAW_LIMIT || (count && !samples))
    return fail(GLH_E_INVALID, "ransac combinations: %lld of %d of %lld rows, or a null argument", (long long)count, n, (long long)rows);
  if (count > rd_combinations(rows, n, count))
    return fail(GLH_E_INVALID, "ransac combinations: %lld of %d of %lld rows: there are fewer", (long long)count, n, (long long)rows);
  rd_enumerate(rows, n, count, samples);
  return GLH_OK;
}

// The draw alone, for tests and probes: every group drawn, rows counted within the group.
extern "C" int glh_stage_ransac_samples(int dev, int n_groups, const int64_t* rows, const int32_t* group_id,
                                        const int64_t* hyp_offset, int n, uint32_t seed0, uint32_t seed1, int64_t* samples,
                                        double* times_ms) {
  if (n_groups < 0 || n_groups >= (1 << 24) || !hyp_offset || (n_groups && (!rows || !group_id)))
    return fail(GLH_E_INVALID, "ransac samples: %d groups (fewer than 2^24 are served) or a null argument", n_groups);
  if (n < 1) return fail(GLH_E_INVALID, "ransac samples: samples of %d rows", n);
  if (hyp_offset[0] != 0) return fail(GLH_E_INVALID, "ransac samples: hyp_offset[0] is %lld, not 0", (long long)hyp_offset[0]);
  for (int g = 0; g < n_groups; ++g) {
    if (hyp_offset[g + 1] < hyp_offset[g] || hyp_offset[g + 1] > RANSAC_DRAW_LIMIT / n)
      return fail(GLH_E_INVALID, "ransac samples: group %d ends at hypothesis %lld after %lld: not decreasing, fewer than 2^31 rows "
                                 "in all", g, (long long)hyp_offset[g + 1], (long long)hyp_offset[g]);
    if (rows[g] <= n || rows[g] > RANSAC_DRAW_LIMIT)
      return fail(GLH_E_INVALID, "ransac samples: group %d has %lld rows: more than the sample's %d, at most 2^31 - 1", g,
                  (long long)rows[g], n);
    if (group_id[g] < 0) return fail(GLH_E_INVALID, "ransac samples: group %d has the id %d: ids are not negative", g, group_id[g]);
  }
  if (n_groups && hyp_offset[n_groups] && !samples) return fail(GLH_E_INVALID, "ransac samples: null output");
  if (!n_groups || !hyp_offset[n_groups]) {  // nothing to draw
    if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0.0;
    return GLH_OK;
  }
  return ransac_draw_samples(RansacDraw{dev, n_groups, rows, group_id, hyp_offset, n, seed0, seed1, samples, times_ms});
}

// How optimize.ransac_pairs cuts its pairs into calls (glh_ransac_plan.h: rg_chunks).  Host arithmetic only.
extern "C" int glh_ransac_chunks(int n_groups, const int64_t* rows, const int64_t* hyps, int64_t budget, int32_t* chunk_of,
                                 int32_t* n_chunks) {
  if (n_groups < 0 || !n_chunks || (n_groups && (!rows || !hyps || !chunk_of)))
    return fail(GLH_E_INVALID, "ransac chunks: %d groups or a null argument", n_groups);
  for (int g = 0; g < n_groups; ++g)
    if (rows[g] < 0 || hyps[g] < 0) return fail(GLH_E_INVALID, "ransac chunks: group %d has %lld rows and %lld hypotheses", g,
                                                 (long long)rows[g], (long long)hyps[g]);
  *n_chunks = rg_chunks(n_groups, rows, hyps, budget, chunk_of);
  return GLH_OK;
}

extern "C" int glh_calib_destroy(glh_calib* handle) {
  calib_destroy(handle);  // (nothing on null)
  return GLH_OK;
}

// Raster.sample(grid=True) / resample, Raster.resize and RasterInterpolant (raster.py:1042-1083, :1178-1187, :1673-1700):
// the arguments are checked here, before a device is touched; the factoring, the kernels and the launches are
// glh_regrid.hip's.
static int check_regrid_outputs(const char* who, const double* xo, int mx, const double* yo, int my) {
  if (!xo || !yo) return fail(GLH_E_INVALID, "%s: null output coordinates", who);
  if (mx < 1 || my < 1) return fail(GLH_E_INVALID, "%s: %d x %d output coordinates: at least one of each", who, mx, my);
  if ((int64_t)mx * my >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "%s: %d x %d output cells: fewer than 2^31 are served", who, mx, my);
  for (int i = 0; i < mx; ++i)
    if (!std::isfinite(xo[i]) || (i && xo[i] < xo[i - 1]))
      return fail(GLH_E_INVALID, "%s: output x %d is not finite or decreases: the vectors are sorted ascending", who, i);
  for (int i = 0; i < my; ++i)
    if (!std::isfinite(yo[i]) || (i && yo[i] < yo[i - 1]))
      return fail(GLH_E_INVALID, "%s: output y %d is not finite or decreases: the vectors are sorted ascending", who, i);
  return GLH_OK;
}

static int check_regrid_axis(const char* who, const char* axis, const double* g, int n, int k, double lo, double hi) {
  if (k < 1 || k > RG_MAX_K) return fail(GLH_E_INVALID, "%s: order %d along %s: 1 .. 5 are served", who, k, axis);
  if (n <= k) return fail(GLH_E_INVALID, "%s: %d cells along %s: order %d needs more than %d", who, n, axis, k, k);
  if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi)) return fail(GLH_E_INVALID, "%s: box (%g, %g) along %s", who, lo, hi, axis);
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(g[i]) || (i && !(g[i] > g[i - 1])))
      return fail(GLH_E_INVALID, "%s: cell centre %d along %s is not finite or not above the one before: the vectors are "
                                 "sorted strictly ascending", who, i, axis);
  if (g[0] < lo || g[n - 1] > hi)
    return fail(GLH_E_INVALID, "%s: the cell centres along %s (%g .. %g) leave the box (%g, %g)", who, axis, g[0], g[n - 1], lo, hi);
  return GLH_OK;
}

static int check_regrid_src(const char* who, const glh_regrid_src* s, bool order1_only, RegridSource& out) {
  if (!s || !s->z || !s->gx || !s->gy) return fail(GLH_E_INVALID, "%s: null argument", who);
  CHK(check_grid(who, s->nx, s->ny, 1));
  CHK(check_regrid_axis(who, "x", s->gx, s->nx, s->kx, s->xmin, s->xmax));
  CHK(check_regrid_axis(who, "y", s->gy, s->ny, s->ky, s->ymin, s->ymax));
  if (order1_only && (s->kx != 1 || s->ky != 1))
    return fail(GLH_E_UNSUPPORTED, "%s: orders (%d, %d): the interpolant regrids at order 1", who, s->kx, s->ky);
  if (s->nan_mask && (s->kx != 1 || s->ky != 1))
    return fail(GLH_E_UNSUPPORTED, "%s: a NaN mask with orders (%d, %d): NaN cells are served at order 1 only (above it one "
                                   "NaN cell reaches every sample of the global fit)", who, s->kx, s->ky);
  const size_t cells = (size_t)s->nx * s->ny;
  for (size_t i = 0; i < cells; ++i)
    if (!std::isfinite(s->z[i])) return fail(GLH_E_INVALID, "%s: cell %zu is not finite (NaN cells go into nan_mask)", who, i);
  out = RegridSource{s->z, s->nan_mask, s->nx, s->ny, s->gx, s->gy, s->xmin, s->xmax, s->ymin, s->ymax, s->kx, s->ky,
                     s->use_zmin != 0, s->zmin, s->flip_x != 0, s->flip_y != 0};
  return GLH_OK;
}

extern "C" int glh_stage_raster_regrid(int dev, const glh_regrid_src* src, const double* xo, int mx, const double* yo, int my,
                                       double* out, double* times_ms) {
  if (!out) return fail(GLH_E_INVALID, "raster_regrid: null argument");
  RegridSource s{};
  CHK(check_regrid_src("raster_regrid", src, false, s));
  CHK(check_regrid_outputs("raster_regrid", xo, mx, yo, my));
  return regrid_run(RegridJob{dev, s, xo, yo, mx, my, out, times_ms});
}

extern "C" int glh_stage_zoom_linear(int dev, const double* a, int nx, int ny, int mx, int my, double* out, double* times_ms) {
  if (!a || !out) return fail(GLH_E_INVALID, "zoom_linear: null argument");
  CHK(check_grid("zoom_linear", nx, ny, 1));
  CHK(check_grid("zoom_linear (output)", mx, my, 1));
  return zoom_run(ZoomJob{dev, a, nx, ny, mx, my, out, times_ms});
}

extern "C" int glh_stage_raster_interpolate(int dev, int nx, int ny, const double* m0, const double* m1,
                                            const glh_regrid_src* m1_src, const double* s0, const double* s1,
                                            const glh_regrid_src* s1_src, const double* xo, const double* yo, double scale,
                                            double scale2, double third, double ratio, double* z, double* sigma,
                                            double* times_ms) {
  if (!m0 || !z || (!m1 && !m1_src)) return fail(GLH_E_INVALID, "raster_interpolate: null argument");
  if (sigma && (!s0 || (!s1 && !s1_src))) return fail(GLH_E_INVALID, "raster_interpolate: sigma asked for without both inputs");
  CHK(check_grid("raster_interpolate", nx, ny, 1));
  RegridSource ms{}, ss{};
  const bool regrid_m = m1_src != nullptr, regrid_s = sigma && s1_src != nullptr;
  if (regrid_m) CHK(check_regrid_src("raster_interpolate (means)", m1_src, true, ms));
  if (regrid_s) CHK(check_regrid_src("raster_interpolate (sigmas)", s1_src, true, ss));
  if (regrid_m || regrid_s) CHK(check_regrid_outputs("raster_interpolate", xo, nx, yo, ny));
  const InterpolateJob job{dev, nx, ny, m0, regrid_m ? nullptr : m1, regrid_m ? &ms : nullptr, sigma ? s0 : nullptr,
                           regrid_s ? nullptr : s1, regrid_s ? &ss : nullptr, xo, yo, scale, scale2, third, ratio, z, sigma,
                           times_ms};
  return interpolate_run(job);
}

// Camera.project_dem (camera.py:967-1129) and Camera.rasterize (camera.py:858-883): the arguments are checked here, before
// a device is touched; the kernels, the sort and the launches are glh_project_dem.hip's.
static int check_pd_axis(const char* name, int n, const int32_t* start, const int32_t* end, int cells) {
  for (int k = 0; k < n; ++k) {
    if (start[k] < 0 || end[k] > cells || start[k] >= end[k])
      return fail(GLH_E_INVALID, "project_dem: %s slice %d is [%d, %d) of %d cells", name, k, start[k], end[k], cells);
    if (k && (start[k] < start[k - 1] || end[k] <= end[k - 1]))
      return fail(GLH_E_INVALID, "project_dem: %s slices %d and %d are not ascending", name, k - 1, k);
  }
  return GLH_OK;
}

extern "C" int glh_stage_project_dem(int dev, const double* cam, const void* z, int z_dtype, int nx, int ny,
                                     const uint8_t* mask, const void* values, int v_dtype, int layers, int n_tx,
                                     const int32_t* x_start, const int32_t* x_end, const double* x_coords, int n_ty,
                                     const int32_t* y_start, const int32_t* y_end, const double* y_coords, int return_depth,
                                     double* out, double* times_ms) {
  if (!cam || !z || !x_start || !x_end || !x_coords || !y_start || !y_end || !y_coords || !out)
    return fail(GLH_E_INVALID, "project_dem: null argument");
  if (nx < 1 || ny < 1 || n_tx < 1 || n_ty < 1)
    return fail(GLH_E_INVALID, "project_dem: %d x %d cells in %d x %d tiles: at least one of each", nx, ny, n_tx, n_ty);
  if (layers < 0 || (layers > 0) != (values != nullptr))
    return fail(GLH_E_INVALID, "project_dem: %d layers %s values", layers, values ? "with" : "without");
  if (layers == 0 && !return_depth) return fail(GLH_E_INVALID, "project_dem: neither values nor the depth asked for");
  CHK(check_float_dtype("project_dem", "z_dtype", z_dtype));
  if (layers && (v_dtype < GLH_PD_F64 || v_dtype > GLH_PD_U16))
    return fail(GLH_E_UNSUPPORTED, "project_dem: v_dtype %d: 0 float64, 1 float32, 2 uint8, 3 uint16", v_dtype);
  if (cam[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "project_dem: the camera is a raster grid");
  const double w = cam[6], h = cam[7];
  if (!(w >= 1.0 && h >= 1.0 && w == std::floor(w) && h == std::floor(h)))
    return fail(GLH_E_INVALID, "project_dem: imgsz (%g, %g) is not a positive integer size", w, h);
  CHK(check_pd_axis("column", n_tx, x_start, x_end, nx));
  CHK(check_pd_axis("row", n_ty, y_start, y_end, ny));
  CamDev cd;
  expand_camera(cam, &cd);
  const ProjectDemJob job{dev, &cd, (int)w, (int)h, z, z_dtype == GLH_PD_F32, nx, ny, mask, values, layers ? v_dtype : GLH_PD_F64,
                          layers, PdAxis{n_tx, x_start, x_end, x_coords}, PdAxis{n_ty, y_start, y_end, y_coords},
                          return_depth != 0, out, times_ms};
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)nx * ny >= lim || w * h >= (double)(lim - 1) || w * h * (layers + 1) >= 9e15 ||
      project_dem_memberships(job) >= lim)
    return fail(GLH_E_UNSUPPORTED, "project_dem: %d x %d cells (%lld with the tiles' overlap) into %g x %g pixels: fewer than "
                                   "2^31 of each are served (32-bit indices)", nx, ny, (long long)project_dem_memberships(job), w, h);
  return project_dem_run(job);
}

extern "C" int glh_stage_rasterize(int dev, const int32_t* keys, int n, const double* values, int layers, int n_pixels,
                                   double* out, double* times_ms) {
  if (!keys || !values || !out) return fail(GLH_E_INVALID, "rasterize: null argument");
  if (n < 1 || layers < 1 || n_pixels < 1)
    return fail(GLH_E_INVALID, "rasterize: %d points, %d layers, %d pixels: at least one of each", n, layers, n_pixels);
  for (int i = 0; i < n; ++i)
    if (keys[i] < 0 || keys[i] >= n_pixels)
      return fail(GLH_E_INVALID, "rasterize: key %d of point %d outside [0, %d)", keys[i], i, n_pixels);
  const RasterizeJob job{dev, keys, n, values, layers, n_pixels, out, times_ms};
  return rasterize_run(job);
}

// Image.orthorectify: the arguments are checked here, before a device is touched; the kernel and the launches are
// glh_ortho.hip's.
extern "C" int glh_stage_orthorectify(int dev, const void* frames, int depth_bits, int is_float, int width, int height,
                                      int channels, int n_frames, const double* cams, const void* z, int z_dtype, int nx,
                                      int ny, const double* x, const double* y, const uint8_t* seen, int n_seen,
                                      const int32_t* seen_of, int method, void* out, double* kernel_ms) {
  if (!frames || !cams || !z || !x || !y || !out || n_frames < 1) return fail(GLH_E_INVALID, "orthorectify: bad argument");
  if (!((!is_float && (depth_bits == 8 || depth_bits == 16)) || (is_float && (depth_bits == 32 || depth_bits == 64))))
    return fail(GLH_E_UNSUPPORTED, "orthorectify: frames of %d bits (%s): uint8, uint16, float32 or float64", depth_bits,
                is_float ? "float" : "integer");
  if (channels != 1 && channels != 3) return fail(GLH_E_UNSUPPORTED, "orthorectify: 1 or 3 channels");
  if (method != RPJ_LINEAR && method != RPJ_NEAREST)
    return fail(GLH_E_UNSUPPORTED, "orthorectify: method %d: 0 linear, 1 nearest", method);
  // (the interpolator needs two grid points on an axis; the pixel index arithmetic is 32-bit)
  if (width < 2 || height < 2 || width > 32768 || height > 32768)
    return fail(GLH_E_INVALID, "orthorectify: a frame of %d x %d: at least 2 x 2, at most 32768 on a side", width, height);
  CHK(check_grid("orthorectify", nx, ny, 1));
  CHK(check_float_dtype("orthorectify", "z_dtype", z_dtype));
  if (seen ? n_seen < 1 : seen_of != nullptr)
    return fail(GLH_E_INVALID, "orthorectify: %d masks %s", n_seen, seen ? "given" : "chosen from none");
  std::vector<CamDev> cd(n_frames);
  for (int i = 0; i < n_frames; ++i) {
    const double* v = cams + (size_t)i * GLH_CAM_LEN;
    if (v[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "orthorectify: frame %d is a raster grid, not a camera", i);
    if ((int)v[6] != width || (int)v[7] != height)
      return fail(GLH_E_INVALID, "orthorectify: camera %d imgsz (%g, %g) != frame size (%d, %d)", i, v[6], v[7], width, height);
    if (seen && seen_of && (seen_of[i] < 0 || seen_of[i] >= n_seen))
      return fail(GLH_E_INVALID, "orthorectify: frame %d takes mask %d of %d", i, seen_of[i], n_seen);
    expand_camera(v, &cd[i]);
  }
  const OrthoJob job{dev, frames, depth_bits, is_float, width, height, channels, n_frames, cd.data(), z, z_dtype == GLH_PD_F32,
                     nx, ny, x, y, seen, n_seen, seen_of, method, out, kernel_ms};
  return orthorectify_run(job);
}

// Raster.intersect_rays, Camera.uv_to_dem and Camera.xyz_map: the arguments are checked here, before a device is touched;
// the kernels and the launches are glh_raycast.hip's.
static int check_raycast_axis(const char* name, const double* g, int n, double d) {
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(g[k])) return fail(GLH_E_INVALID, "raycast: %s[%d] is not finite", name, k);
    if (!(std::fabs(g[k] - (g[0] + (double)k * d)) < 0.25 * std::fabs(d)))
      return fail(GLH_E_UNSUPPORTED, "raycast: %s[%d] = %g is not on the uniform grid %g + k * %g", name, k, g[k], g[0], d);
  }
  return GLH_OK;
}

extern "C" int glh_stage_raycast(int dev, const void* z, int z_dtype, int nx, int ny, const double* x, const double* y,
                                 double d0, double d1, int mode, const double* cam, const double* origins, int n_origins,
                                 const double* rays, int n, int step, int correction, double radius, double refraction,
                                 int block, double* t, double* xyz, int32_t* patch, uint8_t* status, double* times_ms) {
  if (!z || !x || !y || !t || !xyz || !patch || !status) return fail(GLH_E_INVALID, "raycast: null argument");
  if (nx < 1 || ny < 1 || n < 1) return fail(GLH_E_INVALID, "raycast: %d x %d cells, %d rays: at least one of each", nx, ny, n);
  if (mode != GLH_RAYCAST_DIRECTIONS && mode != GLH_RAYCAST_UV && mode != GLH_RAYCAST_GRID)
    return fail(GLH_E_UNSUPPORTED, "raycast: mode %d: 0 directions, 1 uv, 2 pixel grid", mode);
  if (mode == GLH_RAYCAST_DIRECTIONS ? (!origins || !rays) : (!cam || (mode == GLH_RAYCAST_UV && !rays)))
    return fail(GLH_E_INVALID, "raycast: null argument for mode %d", mode);
  if (mode == GLH_RAYCAST_DIRECTIONS && n_origins != 1 && n_origins != n)
    return fail(GLH_E_INVALID, "raycast: %d origins for %d rays: one, or one each", n_origins, n);
  if (nx < 2 || ny < 2)
    return fail(GLH_E_UNSUPPORTED, "raycast: a DEM of %d x %d cells has no patch between cell centres", nx, ny);
  if ((int64_t)nx * ny >= ((int64_t)1 << 31))
    return fail(GLH_E_UNSUPPORTED, "raycast: %d x %d cells: fewer than 2^31 are served (32-bit cell indices)", nx, ny);
  if (block < 0 || block > 32768 || (block & (block - 1)))
    return fail(GLH_E_UNSUPPORTED, "raycast: block %d: 0, or a power of two up to 32768", block);
  CHK(check_float_dtype("raycast", "z_dtype", z_dtype));
  if (!(std::isfinite(d0) && std::isfinite(d1) && d0 != 0.0 && d1 != 0.0))
    return fail(GLH_E_INVALID, "raycast: cell size (%g, %g)", d0, d1);
  CHK(check_raycast_axis("x", x, nx, d0));
  CHK(check_raycast_axis("y", y, ny, d1));
  CHK(check_correction("raycast", correction, radius, refraction));
  CamDev cd;
  int cols = 0, rows = 0;
  if (mode != GLH_RAYCAST_DIRECTIONS) {
    if (cam[23] != 0.0) return fail(GLH_E_UNSUPPORTED, "raycast: the camera is a raster grid, which has no position to see from");
    expand_camera(cam, &cd);
  }
  if (mode == GLH_RAYCAST_GRID) {
    const double w = cam[6], h = cam[7];
    if (step < 1) return fail(GLH_E_INVALID, "raycast: a pixel grid of step %d", step);
    if (!(w >= 1.0 && h >= 1.0 && w == std::floor(w) && h == std::floor(h) && w < 2147483648.0 && h < 2147483648.0))
      return fail(GLH_E_INVALID, "raycast: imgsz (%g, %g) is not a positive integer size", w, h);
    cols = (int)w / step, rows = (int)h / step;
    if ((int64_t)cols * rows >= ((int64_t)1 << 31))
      return fail(GLH_E_UNSUPPORTED, "raycast: %d x %d pixels: fewer than 2^31 rays are served", cols, rows);
    if ((int64_t)cols * rows != n)
      return fail(GLH_E_INVALID, "raycast: %d rays for a grid of %d x %d pixels", n, cols, rows);
  }
  const RaycastJob job{dev, z, z_dtype == GLH_PD_F32, nx, ny, x[0], y[0], d0, d1, mode,
                       mode == GLH_RAYCAST_DIRECTIONS ? nullptr : &cd, origins, mode == GLH_RAYCAST_DIRECTIONS ? n_origins : 1,
                       rays, n, step, cols, rows, correction != 0, radius, refraction, block, t, xyz, patch, status, times_ms};
  return raycast_run(job);
}

// glimpse_amd.displacements: the arguments are checked here, before a device is touched; the kernels and the launch are
// glh_displace.hip's.
extern "C" int glh_stage_displacements(int dev, const void* frames, int is_float, int width, int height, int n_frames,
                                       const int32_t* pairs, int n_pairs, const int32_t* corners, const uint8_t* valid, int n,
                                       const int32_t* guess, int guess_per_pair, int w, int h, int rx, int ry, int subpixel,
                                       double* duv, double* score, uint8_t* status, double* surface, double* times_ms) {
  if (!frames || !pairs || !corners || !valid || !duv || !score || !status)
    return fail(GLH_E_INVALID, "displacements: null argument");
  if (width < 1 || height < 1 || n_frames < 1 || n_pairs < 1 || n < 1)
    return fail(GLH_E_INVALID, "displacements: %d frames of %d x %d, %d pairs, %d points: at least one of each", n_frames,
                width, height, n_pairs, n);
  if (width > 32768 || height > 32768)
    return fail(GLH_E_UNSUPPORTED, "displacements: a frame of %d x %d: at most 32768 on a side", width, height);
  if (n_pairs > 65535) return fail(GLH_E_UNSUPPORTED, "displacements: %d pairs: up to 65535 in one call", n_pairs);
  if (w < DP_MIN_SIDE || w > DP_MAX_SIDE || h < DP_MIN_SIDE || h > DP_MAX_SIDE)
    return fail(GLH_E_UNSUPPORTED, "displacements: a template of %d x %d: sides of %d .. %d", w, h, DP_MIN_SIDE, DP_MAX_SIDE);
  if (rx < 1 || rx > DP_MAX_REACH || ry < 1 || ry > DP_MAX_REACH)
    return fail(GLH_E_UNSUPPORTED, "displacements: a reach of (%d, %d): 1 .. %d per axis", rx, ry, DP_MAX_REACH);
  for (int k = 0; k < 2 * n_pairs; ++k)
    if (pairs[k] < 0 || pairs[k] >= n_frames)
      return fail(GLH_E_INVALID, "displacements: pair %d names frame %d of %d", k / 2, pairs[k], n_frames);
  if (guess) {
    const size_t count = (size_t)(guess_per_pair ? n_pairs : 1) * n * 2;
    for (size_t k = 0; k < count; ++k)
      if (guess[k] < -(1 << 24) || guess[k] > (1 << 24))
        return fail(GLH_E_INVALID, "displacements: a guess of %d pixels: within +-2^24", guess[k]);
  }
  const DisplaceJob job{dev, frames, is_float != 0, width, height, n_frames, pairs, n_pairs, corners, valid, n, guess,
                        guess_per_pair != 0, w, h, rx, ry, subpixel != 0, duv, score, status, surface, times_ms};
  return displacements_run(job);
}

// glimpse_amd.velocity_field: the arguments are checked here, before a device is touched; the kernels and the launch are
// glh_velocity.hip's.
extern "C" int glh_stage_velocity_field(int dev, const double* duv, const double* score, const uint8_t* status, int n_pairs,
                                        int rows, int cols, int n, const double* dt, double scale_u, double scale_v,
                                        double min_score, int accept_edge, int radius, int min_neighbors, double threshold,
                                        double epsilon, int min_count, double* v, double* sigma, int32_t* count,
                                        uint8_t* kept, double* times_ms) {
  if (!duv || !score || !status || !dt || !v || !sigma || !count || !kept)
    return fail(GLH_E_INVALID, "velocity_field: null argument");
  if (n_pairs < 1 || rows < 1 || cols < 1 || n < 1 || (int64_t)rows * cols != n)
    return fail(GLH_E_INVALID, "velocity_field: %d pairs, %d nodes on a grid of %d x %d: at least one of each, rows * cols nodes",
                n_pairs, n, rows, cols);
  if (n_pairs > VF_MAX_PAIRS)
    return fail(GLH_E_UNSUPPORTED, "velocity_field: %d pairs: up to %d in one call", n_pairs, VF_MAX_PAIRS);
  if (n > VF_MAX_NODES) return fail(GLH_E_UNSUPPORTED, "velocity_field: %d nodes: up to %d in one call", n, VF_MAX_NODES);
  if (radius < 0 || radius > VF_MAX_RADIUS)
    return fail(GLH_E_UNSUPPORTED, "velocity_field: a radius of %d: 0 .. %d", radius, VF_MAX_RADIUS);
  if (radius > 0) {
    const int most = (2 * radius + 1) * (2 * radius + 1) - 1;
    if (min_neighbors < 1 || min_neighbors > most)
      return fail(GLH_E_INVALID, "velocity_field: min_neighbors %d: 1 .. %d at radius %d", min_neighbors, most, radius);
    if (!(std::isfinite(threshold) && threshold > 0.0 && std::isfinite(epsilon) && epsilon > 0.0))
      return fail(GLH_E_INVALID, "velocity_field: threshold %g, epsilon %g: finite and positive", threshold, epsilon);
  }
  if (min_count < 1) return fail(GLH_E_INVALID, "velocity_field: min_count %d: at least 1", min_count);
  if (!(std::isfinite(scale_u) && std::isfinite(scale_v)))
    return fail(GLH_E_INVALID, "velocity_field: a scale of (%g, %g) is not finite", scale_u, scale_v);
  for (int p = 0; p < n_pairs; ++p)
    if (!(std::isfinite(dt[p]) && dt[p] != 0.0))
      return fail(GLH_E_INVALID, "velocity_field: dt[%d] = %g: finite and not zero", p, dt[p]);
  const VelocityJob job{dev, duv, score, status, n_pairs, rows, cols, dt, {scale_u, scale_v}, min_score,
                        accept_edge ? GLH_DISPLACE_EDGE : GLH_DISPLACE_MATCHED, radius, min_neighbors, threshold, epsilon,
                        min_count, v, sigma, count, kept, times_ms};
  return velocity_field_run(job);
}

// helpers.maximum_filter, helpers.gaussian_filter (helpers.py:347-430) and Raster.fill_crevasses (raster.py:1266-1291): the
// arguments are checked here, before a device is touched; the kernels and the launches are glh_filters.hip's.
static int check_filter_array(const char* who, const void* a, int dtype, int nx, int ny, const void* out) {
  if (!a || !out) return fail(GLH_E_INVALID, "%s: null argument", who);
  CHK(check_grid(who, nx, ny, 1));
  return check_float_dtype(who, "dtype", dtype);
}

static int check_filter_window(const char* who, int size_y, int size_x, int mode) {
  if (size_y < 1 || size_x < 1) return fail(GLH_E_INVALID, "%s: a window of %d x %d cells", who, size_y, size_x);
  if (size_y > FL_MAX_WINDOW || size_x > FL_MAX_WINDOW)
    return fail(GLH_E_UNSUPPORTED, "%s: a window of %d x %d cells: up to %d a side are served", who, size_y, size_x, FL_MAX_WINDOW);
  if (mode < GLH_HP_REFLECT || mode > GLH_HP_WRAP) return fail(GLH_E_UNSUPPORTED, "%s: boundary mode %d of the maximum", who, mode);
  return GLH_OK;
}

static int check_filter_weights(const char* who, const double* w0, int r0, const double* w1, int r1, int mode) {
  const double* w[2] = {w0, w1};
  const int r[2] = {r0, r1};
  for (int ax = 0; ax < 2; ++ax) {
    if (!w[ax]) continue;
    if (r[ax] < 0) return fail(GLH_E_INVALID, "%s: radius %d along axis %d", who, r[ax], ax);
    if (r[ax] > FL_MAX_RADIUS)
      return fail(GLH_E_UNSUPPORTED, "%s: radius %d along axis %d: up to %d cells are served", who, r[ax], ax, FL_MAX_RADIUS);
    for (int k = 0; k <= 2 * r[ax]; ++k)
      if (!std::isfinite(w[ax][k])) return fail(GLH_E_INVALID, "%s: weight %d of axis %d is not finite", who, k, ax);
    for (int k = 0; k < r[ax]; ++k)
      if (w[ax][k] != w[ax][2 * r[ax] - k]) return fail(GLH_E_UNSUPPORTED, "%s: the weights of axis %d are not symmetric", who, ax);
  }
  if (mode < GLH_HP_REFLECT || mode > GLH_HP_WRAP) return fail(GLH_E_UNSUPPORTED, "%s: boundary mode %d of the Gaussian", who, mode);
  return GLH_OK;
}

extern "C" int glh_stage_max_filter(int dev, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                                    int size_y, int size_x, int mode, void* out, double* times_ms) {
  CHK(check_filter_array("max_filter", a, dtype, nx, ny, out));
  CHK(check_filter_window("max_filter", size_y, size_x, mode));
  return filters_run(FiltersJob{dev, a, dtype == GLH_FILTER_F32, nx, ny, mask, fill != 0, 1, size_y, size_x, mode, 0, nullptr, 0,
                                nullptr, 0, 0, out, times_ms});
}

extern "C" int glh_stage_gaussian_filter(int dev, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                                         const double* w0, int r0, const double* w1, int r1, int mode, void* out,
                                         double* times_ms) {
  CHK(check_filter_array("gaussian_filter", a, dtype, nx, ny, out));
  CHK(check_filter_weights("gaussian_filter", w0, r0, w1, r1, mode));
  return filters_run(FiltersJob{dev, a, dtype == GLH_FILTER_F32, nx, ny, mask, fill != 0, 0, 1, 1, 0, 1, w0, r0, w1, r1, mode, out,
                                times_ms});
}

extern "C" int glh_stage_fill_crevasses(int dev, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                                        int size_y, int size_x, int max_mode, const double* w0, int r0, const double* w1,
                                        int r1, int gauss_mode, void* out, double* times_ms) {
  CHK(check_filter_array("fill_crevasses", a, dtype, nx, ny, out));
  CHK(check_filter_window("fill_crevasses", size_y, size_x, max_mode));
  CHK(check_filter_weights("fill_crevasses", w0, r0, w1, r1, gauss_mode));
  return filters_run(FiltersJob{dev, a, dtype == GLH_FILTER_F32, nx, ny, mask, fill != 0, 1, size_y, size_x, max_mode, 1, w0, r0,
                                w1, r1, gauss_mode, out, times_ms});
}

// optimize.CLAHE (INPUTS.md, "CLAHE: the rule"): the arguments are checked here, before a device is touched; the kernels
// and the launches are glh_clahe.hip's.
extern "C" int glh_stage_clahe(int dev, const uint8_t* src, int w, int h, int channels, double clip_limit, int tiles_x,
                               int tiles_y, uint8_t* dst, uint8_t* luts, double* times_ms) {
  if (!src || !dst) return fail(GLH_E_INVALID, "clahe: null argument");
  if (w < 1 || h < 1 || (int64_t)w * h >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "clahe: %d x %d pixels: at least one, fewer than 2^31", w, h);
  if (channels < 1 || channels > 4) return fail(GLH_E_INVALID, "clahe: %d channels: 1 to 4 are served", channels);
  if (tiles_x < 1 || tiles_x > w || tiles_y < 1 || tiles_y > h)
    return fail(GLH_E_INVALID, "clahe: a grid of %d x %d tiles on %d x %d pixels: at least one tile and at most one per pixel "
                               "along each axis", tiles_x, tiles_y, w, h);
  if (!std::isfinite(clip_limit)) return fail(GLH_E_INVALID, "clahe: clipLimit %g is not finite", clip_limit);
  const ClaheGeometry geo = clahe_geometry(w, h, clip_limit, tiles_x, tiles_y);
  const int64_t lim31 = (int64_t)1 << 31;
  if (geo.ext_w >= lim31 || geo.ext_h >= lim31 || geo.area >= lim31)
    return fail(GLH_E_UNSUPPORTED, "clahe: the image extended to the grid is %lld x %lld pixels with %lld to a tile: fewer than "
                                   "2^31 of each are served (32-bit indices and counts)", (long long)geo.ext_w,
                (long long)geo.ext_h, (long long)geo.area);
  return clahe_run(ClaheJob{dev, src, w, h, channels, tiles_x, tiles_y, geo, dst, luts, times_ms});
}

// Raster.gradient, Raster.hillshade (raster.py:1465-1474, :1249-1264) and helpers.polygons_to_mask (helpers.py:1701-1768):
// the arguments are checked here, before a device is touched; the kernels and the launches are glh_terrain.hip's.
static int check_terrain_dem(const char* who, int nx, int ny, int dtype, double d0, double d1) {
  CHK(check_grid(who, nx, ny, 2));
  if (!std::isfinite(d0) || !std::isfinite(d1) || d0 == 0.0 || d1 == 0.0)
    return fail(GLH_E_INVALID, "%s: cell sizes (%g, %g): finite and not zero", who, d0, d1);
  return check_float_dtype(who, "dtype", dtype);
}

extern "C" int glh_stage_gradient(int dev, const void* z, int dtype, int nx, int ny, double d0, double d1, void* dzdx,
                                  void* dzdy, double* times_ms) {
  if (!z || !dzdx || !dzdy) return fail(GLH_E_INVALID, "gradient: null argument");
  CHK(check_terrain_dem("gradient", nx, ny, dtype, d0, d1));
  return gradient_run(GradientJob{dev, z, dtype == GLH_TERRAIN_F32, nx, ny, d0, d1, dzdx, dzdy, times_ms});
}

extern "C" int glh_stage_hillshade(int dev, const void* z, int dtype, int nx, int ny, double d0, double d1, double vert_exag,
                                   const double* direction, double fraction, double* out, double* times_ms) {
  if (!z || !direction || !out) return fail(GLH_E_INVALID, "hillshade: null argument");
  CHK(check_terrain_dem("hillshade", nx, ny, dtype, d0, d1));
  if (!std::isfinite(vert_exag) || !std::isfinite(fraction) || !std::isfinite(direction[0]) || !std::isfinite(direction[1]) ||
      !std::isfinite(direction[2]))
    return fail(GLH_E_INVALID, "hillshade: vert_exag %g, fraction %g, direction (%g, %g, %g): all finite", vert_exag, fraction,
                direction[0], direction[1], direction[2]);
  const HillshadeJob job{dev, z, dtype == GLH_TERRAIN_F32, nx, ny, d0, d1, vert_exag, {direction[0], direction[1], direction[2]},
                         fraction, out, times_ms};
  return hillshade_run(job);
}

extern "C" int glh_stage_polygon_mask(int dev, const double* xy, int n_vertices, const int32_t* ring_off, int n_polygons,
                                      int n_holes, int nx, int ny, uint8_t* out, double* times_ms) {
  if (!xy || !ring_off || !out) return fail(GLH_E_INVALID, "polygon_mask: null argument");
  CHK(check_grid("polygon_mask", nx, ny, 1));
  if (n_vertices < 1 || n_polygons < 1 || n_holes < 0 || (int64_t)n_polygons + n_holes >= ((int64_t)1 << 31))
    return fail(GLH_E_INVALID, "polygon_mask: %d vertices, %d polygon rings, %d hole rings", n_vertices, n_polygons, n_holes);
  const int rings = n_polygons + n_holes;
  if (ring_off[0] != 0 || ring_off[rings] != n_vertices)
    return fail(GLH_E_INVALID, "polygon_mask: the ring offsets run from %d to %d, not from 0 to %d", ring_off[0], ring_off[rings],
                n_vertices);
  for (int k = 0; k < rings; ++k)
    if ((int64_t)ring_off[k + 1] - ring_off[k] < 3 || ring_off[k + 1] > n_vertices)
      return fail(GLH_E_INVALID, "polygon_mask: ring %d has %lld vertices: at least three", k,
                  (long long)ring_off[k + 1] - ring_off[k]);
  for (int64_t i = 0; i < 2 * (int64_t)n_vertices; ++i)
    if (!std::isfinite(xy[i])) return fail(GLH_E_INVALID, "polygon_mask: vertex %lld is not finite", (long long)(i / 2));
  return polygon_mask_run(PolygonMaskJob{dev, xy, ring_off, n_polygons, n_holes, nx, ny, out, times_ms});
}

extern "C" int glh_stage_resample(int dev, const double* weights, int n, double u, int64_t* idx) {
  if (!weights || !idx || n <= 0) return fail(GLH_E_INVALID, "bad argument");
  if ((size_t)n * 10 + 4096 > 150 * 1024) return fail(GLH_E_UNSUPPORTED, "n too large for the LDS-resident scan");
  HIPCHK(hipSetDevice(dev));
  PairwisePlan pl;
  pairwise_plan(n, pl);
  std::vector<double> pin((size_t)n * 6, 0.0);
  DevBuf dw, dpi, dpo, dwo, du, didx, dst, def, doff, dlen, dops, dlev, droot;
  CHK(dw.up(weights, (size_t)n * 8));
  CHK(dpi.up(pin.data(), pin.size() * 8));
  CHK(dpo.alloc(pin.size() * 8));
  CHK(dwo.alloc((size_t)n * 8));
  CHK(du.up(&u, 8));
  CHK(didx.alloc((size_t)n * 4));
  uint32_t st0 = 0;
  int32_t ef = 0x7f7f7f7f;
  CHK(dst.up(&st0, 4));
  CHK(def.up(&ef, 4));
  CHK(doff.up(pl.leaf_off.data(), pl.leaf_off.size() * 4));
  CHK(dlen.up(pl.leaf_len.data(), pl.leaf_len.size() * 4));
  CHK(dops.up(pl.ops.data(), pl.ops.size() * 4));
  CHK(dlev.up(pl.level_off.data(), pl.level_off.size() * 4));
  CHK(droot.up(pl.roots.data(), pl.roots.size() * 4));
  ResampleArgs a{};
  a.particles_in = dpi.as<double>();
  a.weights_in = dw.as<double>();
  a.particles_out = dpo.as<double>();
  a.weights_out = dwo.as<double>();
  a.active = nullptr;
  a.u = du.as<double>();
  a.idx_out = didx.as<int32_t>();
  a.moments = nullptr;
  a.pt_status = dst.as<uint32_t>();
  a.pt_err_frame = def.as<int32_t>();
  a.leaf_off = doff.as<int32_t>();
  a.leaf_len = dlen.as<int32_t>();
  a.ops = dops.as<int32_t>();
  a.level_off = dlev.as<int32_t>();
  a.roots = droot.as<int32_t>();
  a.N = n;
  a.nleaves = (int)pl.leaf_off.size();
  a.nnodes = pl.nnodes;
  a.nlevels = (int)pl.level_off.size() - 1;
  a.nroots = (int)pl.roots.size();
  a.rng_mode = GLH_RNG_HOST;
  a.frame = 0;
  HIPCHK(hipFuncSetAttribute((const void*)k_resample, hipFuncAttributeMaxDynamicSharedMemorySize, 156 * 1024));
  hipLaunchKernelGGL(k_resample, dim3(1), dim3(BLK), ((size_t)n + pl.nnodes) * 8 + (size_t)n * 2, 0, a);
  CHK(finish());
  std::vector<int32_t> tmp(n);
  CHK(didx.down(tmp.data(), (size_t)n * 4));
  for (int i = 0; i < n; ++i) idx[i] = tmp[i];
  return GLH_OK;
}
