// owner_cases.h -- TEST-ONLY: the move-only owner and the grow-only step of glimpse_amd/csrc/glh_owned.h (what every
// device buffer, pinned buffer, stream and event of the library is freed by) with a release that counts instead of
// freeing.  The values are heap blocks, so a release that is missed or made twice is also AddressSanitizer's to report.
// Shared by stage_hostcheck.cpp (tests/test_stage_host.py) and sanitize_main.cpp (tests/test_hostcheck.py).
#pragma once
#include <utility>
#include <vector>

#include "../../glimpse_amd/csrc/glh_owned.h"

namespace glh {

struct CountingFree {
  static std::vector<int*>& freed() {  // every value released so far, in order
    static std::vector<int*> v;
    return v;
  }
  void operator()(int* p) const {
    freed().push_back(p);
    delete p;
  }
};
using CountedInt = Owned<int*, CountingFree>;

// Returns the number of conditions that do not hold.
inline int owner_cases() {
  std::vector<int*>& freed = CountingFree::freed();
  int bad = 0;
  freed.clear();
  // destruction releases exactly once; an owner that never held a value releases nothing
  int* a = new int(1);
  {
    CountedInt o(a), none;
    bad += o.get() != a || none.get() != nullptr || !freed.empty();
  }
  bad += freed != std::vector<int*>{a};
  // reset() followed by destruction releases once; reset() of a null value releases nothing
  freed.clear();
  int* b = new int(2);
  {
    CountedInt o(b);
    o.reset();
    bad += o.get() != nullptr || freed != std::vector<int*>{b};
    o.reset();
  }
  bad += freed.size() != 1;
  // reset(next) releases the old value and holds the new one; release() hands the value over without releasing it
  freed.clear();
  int *c = new int(3), *d = new int(4);
  {
    CountedInt o(c);
    o.reset(d);
    bad += o.get() != d || freed != std::vector<int*>{c};
    int* mine = o.release();
    bad += mine != d || o.get() != nullptr;
    delete mine;
  }
  bad += freed.size() != 1;
  // move construction: the moved-from owner holds null and never releases, the new one releases once
  freed.clear();
  int* e = new int(5);
  {
    CountedInt from(e);
    {
      CountedInt to(std::move(from));
      bad += from.get() != nullptr || to.get() != e || !freed.empty();
    }
    bad += freed != std::vector<int*>{e};
  }
  bad += freed.size() != 1;
  // move-assignment over a held value releases the overwritten value once, at once, and the moved-from value never;
  // over an empty owner it releases nothing; onto itself it keeps the value
  freed.clear();
  int *f = new int(6), *g = new int(7);
  {
    CountedInt to(f), from(g), empty;
    to = std::move(from);
    bad += freed != std::vector<int*>{f} || to.get() != g || from.get() != nullptr;
    empty = std::move(to);
    bad += freed.size() != 1 || empty.get() != g || to.get() != nullptr;
    CountedInt& self = empty;
    empty = std::move(self);
    bad += freed.size() != 1 || empty.get() != g;
  }
  bad += freed != std::vector<int*>{f, g};
  // owners in a vector that grows (what an observer keeps its frames in) move and release each value once
  freed.clear();
  {
    std::vector<CountedInt> v(1);
    v[0].reset(new int(8));
    v.resize(64);
    bad += !freed.empty() || !v[0].get() || v[63].get();
    v.clear();
    bad += freed.size() != 1;
  }
  bad += freed.size() != 1;
  // the grow-only step: the first reserve acquires; one that fits keeps the value and does not acquire; a larger one
  // releases exactly the one old value before it acquires; a failed acquire leaves nothing held and a capacity of 0
  freed.clear();
  {
    CountedInt o;
    size_t cap = 0;
    int acquired = 0, fail_with = 0;
    size_t released_before_acquire = 0;
    auto acquire = [&](size_t n, int** out) {
      released_before_acquire = freed.size();
      if (fail_with) return fail_with;
      ++acquired;
      *out = new int((int)n);
      return 0;
    };
    bad += grow(o, cap, 10, acquire) != 0 || cap != 10 || acquired != 1 || !freed.empty();
    int* first = o.get();
    bad += grow(o, cap, 10, acquire) != 0 || grow(o, cap, 3, acquire) != 0 || grow(o, cap, 0, acquire) != 0;
    bad += o.get() != first || cap != 10 || acquired != 1 || !freed.empty();
    bad += grow(o, cap, 11, acquire) != 0 || cap != 11 || acquired != 2 || *o.get() != 11;
    bad += freed != std::vector<int*>{first} || released_before_acquire != 1;
    int* second = o.get();
    fail_with = -3;
    bad += grow(o, cap, 12, acquire) != -3 || o.get() != nullptr || cap != 0 || acquired != 2;
    bad += freed != std::vector<int*>{first, second};
    fail_with = 0;  // (and an owner that lost its value acquires again, whatever is asked for)
    bad += grow(o, cap, 1, acquire) != 0 || cap != 1 || acquired != 3 || freed.size() != 2;
  }
  bad += freed.size() != 3;
  return bad;
}

}  // namespace glh
