// The joint extrema reduction of the fused step's phase A (glh_math.h: wave_max4_joint) on a scalar model of the wave:
// the very schedule the kernel runs, with the lane operations restated on arrays of 64 doubles.  Test-only
// (tests/test_extrema_host.py).
#include <utility>

#include "../../glimpse_amd/csrc/glh_math.h"

namespace {

struct Lanes {
  double v[64];
};

// v_permlane32_swap / v_permlane16_swap and the DPP row exchanges, lane for lane
struct ModelLanes {
  static void swap32(Lanes& a, Lanes& b) {
    for (int i = 0; i < 32; ++i) std::swap(a.v[32 + i], b.v[i]);
  }
  static void swap16(Lanes& a, Lanes& b) {
    for (int r = 0; r < 2; ++r)
      for (int i = 0; i < 16; ++i) std::swap(a.v[(2 * r + 1) * 16 + i], b.v[2 * r * 16 + i]);
  }
  template <typename F>
  static Lanes from(const Lanes& v, F src) {
    Lanes r;
    for (int i = 0; i < 64; ++i) r.v[i] = v.v[src(i)];
    return r;
  }
  static Lanes xor1(const Lanes& v) { return from(v, [](int i) { return i ^ 1; }); }
  static Lanes xor2(const Lanes& v) { return from(v, [](int i) { return i ^ 2; }); }
  static Lanes half_mirror(const Lanes& v) { return from(v, [](int i) { return (i & ~7) | (7 - (i & 7)); }); }
  static Lanes mirror(const Lanes& v) { return from(v, [](int i) { return (i & ~15) | (15 - (i & 15)); }); }
  static Lanes max(const Lanes& a, const Lanes& b) {
    Lanes r;
    for (int i = 0; i < 64; ++i) r.v[i] = glh::max_nn(a.v[i], b.v[i]);
    return r;
  }
};

}  // namespace

// in: [4][64] = min u, min v, max u, max v per lane (what a lane holds after phase A's loop); out: [64], the wave after the
// butterfly exactly as the kernel leaves it (minima still negated in rows 0 and 1)
extern "C" void hc_extrema4(const double* in, double* out) {
  Lanes q[4];
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < 64; ++i) q[k].v[i] = k < 2 ? -in[k * 64 + i] : in[k * 64 + i];
  const Lanes r = glh::wave_max4_joint(q[0], q[1], q[2], q[3], ModelLanes{});
  for (int i = 0; i < 64; ++i) out[i] = r.v[i];
}
