// glh_owned.h -- who frees what: the move-only owner of one resource that glh_stage.h builds its device buffers, pinned
// buffers, streams and events on, and the grow-only step of a buffer with a capacity.  No HIP header and no HIP call: the
// release is a type parameter, and tests/hostcheck/owner_cases.h runs both on the CPU with a release that counts.
#pragma once
#include <stddef.h>

namespace glh {

// Holds p and gives it to Release{}(p) exactly once: when the owner goes, on reset(), or when another owner is moved
// over it.  A null p is never released, and an owner that was moved from holds null.
template <typename T, typename Release>
struct Owned {
  T p{};
  Owned() = default;
  explicit Owned(T held) : p(held) {}
  Owned(Owned&& o) noexcept : p(o.release()) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  T get() const { return p; }
  T release() {  // hands p to the caller, who frees it from now on
    T held = p;
    p = T{};
    return held;
  }
  void reset(T next = T{}) {
    if (p) Release{}(p);
    p = next;
  }
};

// The grow-only step of an owner `o` that holds `cap` units: nothing when n units are held already; else the old value
// is released first (the two never exist side by side), acquire(n, &value) gives the new value and returns 0, o holds
// it and cap becomes n.  When acquire fails its code is returned and o holds nothing, with cap 0.
template <typename O, typename Acquire>
int grow(O& o, size_t& cap, size_t n, Acquire acquire) {
  if (n <= cap && o.p) return 0;
  o.reset();
  cap = 0;
  decltype(o.p) next{};
  const int rc = acquire(n, &next);
  if (rc != 0) return rc;
  o.reset(next);
  cap = n;
  return 0;
}

}  // namespace glh
