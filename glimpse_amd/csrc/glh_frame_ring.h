// glh_frame_ring.h -- the staging ring a batch of frames travels through (glh_stage_reproject, glh_stage_orthorectify):
// NSLOT slots, each a pinned input and output staging buffer and a device input and output buffer; three streams (upload,
// kernel, download) chained by events, so that frame k + 1's upload and frame k - 1's download overlap frame k's kernel
// -- the staging ring of glh_observer_upload_frame_async, in both directions.  Host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <vector>

#include "glh_stage.h"

namespace glh {

struct FrameRing {
  static constexpr int NSLOT = 3;
  hipStream_t up = nullptr, run = nullptr, down = nullptr;
  hipEvent_t uploaded[NSLOT] = {}, computed[NSLOT] = {}, downloaded[NSLOT] = {};
  std::vector<hipEvent_t> k0, k1;  // around every kernel (timing)
  uint8_t *pin_in[NSLOT] = {}, *pin_out[NSLOT] = {}, *dev_in[NSLOT] = {}, *dev_out[NSLOT] = {};
  int nslot = 0;
  size_t in_bytes = 0, out_bytes = 0;
  ~FrameRing() {
    for (hipStream_t s : {up, run, down})
      if (s) (void)hipStreamSynchronize(s);
    for (int k = 0; k < NSLOT; ++k) {
      for (hipEvent_t e : {uploaded[k], computed[k], downloaded[k]})
        if (e) (void)hipEventDestroy(e);
      if (pin_in[k]) (void)hipHostFree(pin_in[k]);
      if (pin_out[k]) (void)hipHostFree(pin_out[k]);
      if (dev_in[k]) (void)hipFree(dev_in[k]);
      if (dev_out[k]) (void)hipFree(dev_out[k]);
    }
    for (hipEvent_t e : k0) (void)hipEventDestroy(e);
    for (hipEvent_t e : k1) (void)hipEventDestroy(e);
    for (hipStream_t s : {up, run, down})
      if (s) (void)hipStreamDestroy(s);
  }
  // The streams, and min(n_frames, NSLOT) slots for frames of in_bytes that come back as out_bytes; `timed`: also a pair
  // of events around every frame's kernel.
  int open(int n_frames, size_t in_bytes_, size_t out_bytes_, bool timed) {
    nslot = n_frames < NSLOT ? n_frames : NSLOT;
    in_bytes = in_bytes_, out_bytes = out_bytes_;
    HIPCHK(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&run, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    for (int k = 0; k < nslot; ++k) {
      HIPCHK(hipEventCreateWithFlags(&uploaded[k], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&computed[k], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&downloaded[k], hipEventDisableTiming));
      HIPCHK(hipHostMalloc((void**)&pin_in[k], in_bytes, hipHostMallocDefault));
      HIPCHK(hipHostMalloc((void**)&pin_out[k], out_bytes, hipHostMallocDefault));
      HIPCHK(hipMalloc((void**)&dev_in[k], in_bytes));
      HIPCHK(hipMalloc((void**)&dev_out[k], out_bytes));
    }
    if (timed) {
      k0.resize(n_frames, nullptr);
      k1.resize(n_frames, nullptr);
      for (int i = 0; i < n_frames; ++i) {
        HIPCHK(hipEventCreate(&k0[i]));
        HIPCHK(hipEventCreate(&k1[i]));
      }
    }
    return GLH_OK;
  }
  // Frames `frames` [n_frames][in_bytes] -> `out` [n_frames][out_bytes]: launch(i, slot) enqueues frame i's kernel on `run`,
  // from dev_in[slot] into dev_out[slot].  kernel_ms (with open(timed)): the sum of the kernels' durations.
  template <typename Launch>
  int process(const void* frames, int n_frames, void* out, Launch launch, double* kernel_ms) {
    const uint8_t* in = static_cast<const uint8_t*>(frames);
    uint8_t* res = static_cast<uint8_t*>(out);
    const bool timed = !k0.empty();
    auto collect = [&](int frame) {  // the finished frame of this slot, from its pinned buffer to the caller's array
      const int k = frame % nslot;
      HIPCHK(hipEventSynchronize(downloaded[k]));
      memcpy(res + (size_t)frame * out_bytes, pin_out[k], out_bytes);
      return (int)GLH_OK;
    };
    for (int i = 0; i < n_frames; ++i) {
      const int k = i % nslot;
      if (i >= nslot) CHK(collect(i - nslot));  // (its download is over, so its kernel and upload are: the slot is free)
      memcpy(pin_in[k], in + (size_t)i * in_bytes, in_bytes);
      HIPCHK(hipMemcpyAsync(dev_in[k], pin_in[k], in_bytes, hipMemcpyHostToDevice, up));
      HIPCHK(hipEventRecord(uploaded[k], up));
      HIPCHK(hipStreamWaitEvent(run, uploaded[k], 0));
      if (timed) HIPCHK(hipEventRecord(k0[i], run));
      launch(i, k);
      HIPCHK(hipGetLastError());
      if (timed) HIPCHK(hipEventRecord(k1[i], run));
      HIPCHK(hipEventRecord(computed[k], run));
      HIPCHK(hipStreamWaitEvent(down, computed[k], 0));
      HIPCHK(hipMemcpyAsync(pin_out[k], dev_out[k], out_bytes, hipMemcpyDeviceToHost, down));
      HIPCHK(hipEventRecord(downloaded[k], down));
    }
    for (int i = n_frames > nslot ? n_frames - nslot : 0; i < n_frames; ++i) CHK(collect(i));
    if (timed && kernel_ms) {
      double total = 0.0;
      for (int i = 0; i < n_frames; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, k0[i], k1[i]));
        total += ms;
      }
      *kernel_ms = total;
    }
    return GLH_OK;
  }
};

}  // namespace glh
