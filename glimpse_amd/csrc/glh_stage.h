// glh_stage.h -- the host scaffold of a device stage: what glimpse_hip.hip (the C ABI) and the stage files
// (glh_viewshed.hip, glh_horizon.hip, glh_regrid.hip, glh_project_dem.hip, glh_filters.hip, glh_terrain.hip, glh_orient.hip, glh_calib.hip, glh_match.hip, glh_sift.hip) share to
// report an error, to own device memory and to time their phases.  Host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/glimpse_hip.h"

namespace glh {

// Keeps the formatted message (cut to 512 bytes) for glh_last_error() of the calling thread and returns `code`.  Defined in
// glimpse_hip.hip.
int fail(int code, const char* fmt, ...);

}  // namespace glh

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(GLH_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                 \
  } while (0)

#define CHK(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_ != GLH_OK) return rc_; \
  } while (0)

namespace glh {

// A device allocation that is freed with its scope.
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
  int alloc(size_t bytes) {
    if (bytes == 0) bytes = 8;  // (an empty array still gets an address)
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // (the error is sticky: the next launch check would report it again)
      return fail(GLH_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return GLH_OK;
  }
  int up(const void* src, size_t bytes) {
    CHK(alloc(bytes));
    HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    return GLH_OK;
  }
  int down(void* dst, size_t bytes) {
    HIPCHK(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return GLH_OK;
  }
};

// The N events a stage records between its phases; times_ms of the C ABI is made of the spans between them.
template <int N>
struct StageEvents {
  hipEvent_t e[N] = {};
  ~StageEvents() {
    for (hipEvent_t v : e)
      if (v) (void)hipEventDestroy(v);
  }
  int create() {
    for (hipEvent_t& v : e) HIPCHK(hipEventCreate(&v));
    return GLH_OK;
  }
  int record(int k, hipStream_t stream) {
    HIPCHK(hipEventRecord(e[k], stream));
    return GLH_OK;
  }
  // milliseconds from event a to event b (both complete); 0 when the runtime cannot tell
  double ms(int a, int b) const {
    float f = 0.f;
    return hipEventElapsedTime(&f, e[a], e[b]) == hipSuccess ? (double)f : 0.0;
  }
  // times_ms[k] = ms(k, k + 1) for the first `intervals` of `slots` entries, 0 for the rest; nothing on null
  void report(double* times_ms, int intervals, int slots) const {
    if (!times_ms) return;
    for (int k = 0; k < slots; ++k) times_ms[k] = k < intervals ? ms(k, k + 1) : 0.0;
  }
};

}  // namespace glh
