// glh_stage.h -- the host scaffold of a device stage: what glimpse_hip.hip (the C ABI and its tracking context, glh_ctx)
// and the stage files (glh_viewshed.hip, glh_horizon.hip, glh_regrid.hip, glh_project_dem.hip, glh_ortho.hip,
// glh_raycast.hip, glh_filters.hip, glh_terrain.hip, glh_displace.hip, glh_velocity.hip, glh_orient.hip, glh_calib.hip,
// glh_match.hip, glh_sift.hip, glh_clahe.hip) share to report an error, to own device memory and to time their phases.
// Everything that has to be given back to HIP is a member that gives it back (glh_owned.h: Owned): device memory (DevBuf,
// GrowBuf, DevArray<T>), pinned host memory (PinnedBuf), a stream (Stream) and an event (Event).  The four handle-based
// objects (glh_orient, glh_calib, glh_match, glh_sift) also share what a handle is made of: a buffer that grows
// (GrowBuf), the device and the stream (DeviceObject) and how a handle comes and goes (create_object, destroy_object).
// The plain C++ of a staging buffer is glh_stage_layout.h's: where its arrays lie (StageLayout), each array named once
// (StagePlan, Stage).  Host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include <new>

#include "../../include/glimpse_hip.h"
#include "glh_owned.h"
#include "glh_stage_layout.h"

namespace glh {

// Keeps the formatted message (cut to 512 bytes) for glh_last_error() of the calling thread and returns `code`.  Defined in
// glimpse_hip.hip.
int fail(int code, const char* fmt, ...);

}  // namespace glh

// (HIPCHK_AT: the same report made on behalf of a caller, whose file and line it names)
#define HIPCHK_AT(call, expr, file, line)                                                            \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess)                                                                            \
      return fail(GLH_E_HIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e_), file, line);      \
  } while (0)

#define HIPCHK(expr) HIPCHK_AT(#expr, expr, __FILE__, __LINE__)

#define CHK(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_ != GLH_OK) return rc_; \
  } while (0)

namespace glh {

struct DeviceFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
struct HostFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
struct StreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct EventDestroy {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};

// A device allocation that is freed with its scope.
struct DevBuf : Owned<void*, DeviceFree> {
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
  // hipMalloc's one report: *out is the memory, or null with the bytes asked for in the message
  static int acquire(size_t bytes, void** out) {
    if (bytes == 0) bytes = 8;  // (an empty array still gets an address)
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) {
      *out = nullptr;
      (void)hipGetLastError();  // (the error is sticky: the next launch check would report it again)
      return fail(GLH_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return GLH_OK;
  }
  int alloc(size_t bytes) {  // (in place of what was held)
    reset();
    return acquire(bytes, &p);
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

// A device buffer that keeps its memory between calls and is replaced by a larger one when more is asked for.  After a
// reserve that succeeded p is never null (0 bytes get DevBuf::alloc's 8), so it can be handed to a library for which a
// null pointer means something else (rocprim's scratch argument).
struct GrowBuf : DevBuf {
  size_t cap = 0;  // the bytes last asked for
  int reserve(size_t bytes) {
    return grow(*this, cap, bytes, DevBuf::acquire);
  }
};

// A device array of T: a GrowBuf counted in elements, which reads as the T* it holds (a kernel argument, `if (!a)`).
// alloc(count) replaces what is held, reserve(count) only when it holds fewer; an array of 0 elements has room for one.
template <typename T>
struct DevArray : GrowBuf {
  T* get() const { return static_cast<T*>(p); }
  operator T*() const { return get(); }
  int alloc(size_t count) {
    cap = 0;
    CHK(DevBuf::alloc(bytes_of(count)));
    cap = bytes_of(count);  // (a reserve of no more keeps it)
    return GLH_OK;
  }
  int reserve(size_t count) { return GrowBuf::reserve(bytes_of(count)); }
  static size_t bytes_of(size_t count) { return (count ? count : 1) * sizeof(T); }
};

// Pinned host memory that grows like a GrowBuf.
struct PinnedBuf : Owned<void*, HostFree> {
  size_t cap = 0;  // the bytes last asked for
  int reserve(size_t bytes) {
    return grow(*this, cap, bytes, [](size_t n, void** out) {
      HIPCHK(hipHostMalloc(out, n, hipHostMallocDefault));
      return GLH_OK;
    });
  }
};

// A non-blocking stream and an event, made on first use by create() and destroyed with their owner.
struct Stream : Owned<hipStream_t, StreamDestroy> {
  operator hipStream_t() const { return p; }
  int create() {
    reset();
    HIPCHK(hipStreamCreateWithFlags(&p, hipStreamNonBlocking));
    return GLH_OK;
  }
};
struct Event : Owned<hipEvent_t, EventDestroy> {
  operator hipEvent_t() const { return p; }
  int create(unsigned flags = hipEventDefault) {
    reset();
    HIPCHK(hipEventCreateWithFlags(&p, flags));
    return GLH_OK;
  }
};

// What the handle of every device object starts with.
struct DeviceObject {
  int device = 0;
  // The null stream: every copy an object makes is ordered with its kernels.
  static constexpr hipStream_t stream = nullptr;
  // Makes the device current for the calling thread; a failure names the caller's line (a method of the object's file).
  int use(const char* file = __builtin_FILE(), int line = __builtin_LINE()) const {
    const hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) (void)hipGetLastError();  // (the error is sticky: the next launch check would report it again)
    HIPCHK_AT("hipSetDevice(device)", e, file, line);
    return GLH_OK;
  }
};

// X_create: a handle H (a DeviceObject) of `who` on `device`, made current and then filled by fill(h); *out gets it only
// when all of that succeeded.
template <typename H, typename Fill>
int create_object(const char* who, int device, H** out, Fill fill, const char* file = __builtin_FILE(),
                  int line = __builtin_LINE()) {
  H* h = new (std::nothrow) H;
  if (!h) return fail(GLH_E_NOMEM, "%s: no memory for a handle", who);
  h->device = device;
  int rc = h->use(file, line);
  if (rc == GLH_OK) rc = fill(h);
  if (rc != GLH_OK) {
    delete h;  // (with what a fill that failed half way had allocated)
    return rc;
  }
  *out = h;
  return GLH_OK;
}

// X_destroy: frees the handle's device memory on its device; nothing on null.
template <typename H>
void destroy_object(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

// The N events a stage records between its phases; times_ms of the C ABI is made of the spans between them.
template <int N>
struct StageEvents {
  Event e[N];
  int create() {
    for (Event& v : e) CHK(v.create());
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
