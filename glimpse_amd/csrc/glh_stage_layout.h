// glh_stage_layout.h -- the plain part of a staging buffer (glh_stage.h includes it): where its arrays lie, and the host
// bytes of a buffer that names each array once with its element type and count.  No HIP header and no HIP call (the one
// upload and the downloads stay with DevBuf / GrowBuf): tests/hostcheck/stage_hostcheck.cpp compiles it for the CPU.
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

namespace glh {

// Where the arrays of a staging buffer lie, one after another: place(bytes) is the next one's offset, a multiple of 16,
// and `size` what the buffer holds after it.
struct StageLayout {
  size_t size = 0;
  size_t place(size_t bytes) {
    const size_t at = size;
    size = (at + bytes + 15) & ~(size_t)15;
    return at;
  }
};

template <typename T>
struct StageArray {  // `count` elements of T at byte `at` of a staging buffer
  size_t at = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
};

// The typed layout: place<T>(count) is the next array, on(base, array) its address in the device buffer at `base`.
// Enough for a buffer that only the device writes and whose arrays are downloaded one by one.
struct StagePlan {
  StageLayout lay;
  template <typename T>
  StageArray<T> place(size_t count) {
    return StageArray<T>{lay.place(count * sizeof(T)), count};
  }
  // what is uploaded or downloaded: every array placed so far, `least` bytes for a buffer without any
  size_t bytes(size_t least = 16) const { return lay.size ? lay.size : least; }
  template <typename T>
  static T* on(void* base, StageArray<T> a) {
    return reinterpret_cast<T*>(static_cast<char*>(base) + a.at);
  }
};

// The plan with its host bytes, in the caller's vector, which only grows: put<T>(src, count) places the next array and
// copies it in, room<T>(count) places one that the caller builds at host(array); hold() .. bytes() is the one upload.
// After a download into hold(), take(dst, array) copies an array out.  A pointer from host() or hold() holds until the
// next put, room or hold.
struct Stage : StagePlan {
  std::vector<char>& mem;
  explicit Stage(std::vector<char>& memory) : mem(memory) {}
  char* hold() {  // host memory for all that is placed so far
    if (mem.size() < bytes()) mem.resize(bytes());
    return mem.data();
  }
  template <typename T>
  StageArray<T> room(size_t count) {
    const StageArray<T> a = place<T>(count);
    hold();
    return a;
  }
  template <typename T>
  StageArray<T> put(const void* src, size_t count) {
    const StageArray<T> a = room<T>(count);
    if (count) memcpy(mem.data() + a.at, src, a.bytes());
    return a;
  }
  template <typename T>
  T* host(StageArray<T> a) {
    return reinterpret_cast<T*>(mem.data() + a.at);
  }
  template <typename T>
  void take(void* dst, StageArray<T> a) const {
    if (a.count) memcpy(dst, mem.data() + a.at, a.bytes());
  }
};

}  // namespace glh
