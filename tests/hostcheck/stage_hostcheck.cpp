// stage_hostcheck.cpp -- the plain part of a staging buffer (csrc/glh_stage_layout.h: StagePlan, Stage) on the CPU: a
// stand-alone program, built with AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_stage_host.py and run
// directly.  Arrays of 0 and 1 elements and of 15, 16 and 17 bytes, of two element types, in every order of three: the
// offsets are those of a sequence of StageLayout::place calls, multiples of 16; put reads exactly count * sizeof(T) from
// a source that is a heap block of just that size (the sanitizer's red zones lie either side of it) and writes exactly
// those bytes; an empty array has an offset and copies nothing; the total is StageLayout::size.  Then the owner that frees
// every buffer, stream and event of the library (csrc/glh_owned.h), with a release that counts: owner_cases.h.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../glimpse_amd/csrc/glh_stage_layout.h"
#include "owner_cases.h"

using namespace glh;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct Wide {  // 17 bytes
  uint8_t b[17];
};
static_assert(sizeof(Wide) == 17, "an element of 17 bytes");

// One array of the sequence: `count` elements of `width` bytes (1: uint8_t, 4: int32_t, 17: Wide).
struct Spec {
  size_t width, count;
};
// 0, 1, 15, 16 and 17 bytes of uint8_t; 0, 1 and 4 elements (16 bytes) of int32_t; 0 and 1 elements of 17 bytes
static const Spec SPECS[] = {{1, 0}, {1, 1}, {1, 15}, {1, 16}, {1, 17}, {4, 0}, {4, 1}, {4, 4}, {4, 5}, {17, 0}, {17, 1}};
static const int N_SPECS = (int)(sizeof(SPECS) / sizeof(SPECS[0]));

// (a heap block of exactly `bytes` bytes; none for 0, which put must not read)
static std::unique_ptr<uint8_t[]> source(size_t bytes, uint8_t first) {
  if (!bytes) return nullptr;
  std::unique_ptr<uint8_t[]> s(new uint8_t[bytes]);
  for (size_t k = 0; k < bytes; ++k) s[k] = (uint8_t)(first + k);
  return s;
}

static size_t put(Stage& st, const Spec& s, const void* src) {
  if (s.width == 1) {
    const StageArray<const uint8_t> a = st.put<const uint8_t>(src, s.count);
    EXPECT(a.count == s.count && a.bytes() == s.count);
    return a.at;
  }
  if (s.width == 4) {
    const StageArray<const int32_t> a = st.put<const int32_t>(src, s.count);
    EXPECT(a.count == s.count && a.bytes() == 4 * s.count);
    return a.at;
  }
  const StageArray<const Wide> a = st.put<const Wide>(src, s.count);
  EXPECT(a.count == s.count && a.bytes() == 17 * s.count);
  return a.at;
}

static void check_sequences() {
  for (int i = 0; i < N_SPECS; ++i)
    for (int j = 0; j < N_SPECS; ++j)
      for (int k = 0; k < N_SPECS; ++k) {
        const Spec seq[3] = {SPECS[i], SPECS[j], SPECS[k]};
        StageLayout want;
        std::vector<char> mem;
        Stage st(mem);
        size_t at[3], bytes[3];
        std::unique_ptr<uint8_t[]> src[3];
        for (int q = 0; q < 3; ++q) {
          bytes[q] = seq[q].width * seq[q].count;
          src[q] = source(bytes[q], (uint8_t)(1 + 60 * q));
          const size_t expected = want.place(bytes[q]);
          const size_t before = mem.size();
          at[q] = put(st, seq[q], src[q].get());
          EXPECT(at[q] == expected && at[q] % 16 == 0 && st.lay.size == want.size && st.lay.size % 16 == 0);
          EXPECT(mem.size() >= st.bytes() && mem.size() >= before && st.hold() == mem.data());
        }
        EXPECT(st.bytes() == (want.size ? want.size : 16) && st.bytes(0) == want.size);
        // every array holds its source, and a later put has not touched an earlier array
        for (int q = 0; q < 3; ++q)
          EXPECT(bytes[q] == 0 || std::memcmp(mem.data() + at[q], src[q].get(), bytes[q]) == 0);
      }
}

// put writes count * sizeof(T) bytes and no more: the padding after the array and the arrays either side keep what they held.
static void check_neighbours() {
  for (const Spec& s : SPECS) {
    const size_t bytes = s.width * s.count;
    std::vector<char> mem(256, (char)0x5A);
    Stage st(mem);
    const std::unique_ptr<uint8_t[]> left = source(16, 200), mid = source(bytes, 1), right = source(17, 100);
    const size_t a = put(st, Spec{1, 16}, left.get());
    const size_t b = put(st, s, mid.get());
    EXPECT(a == 0 && b == 16);
    // (the bytes from the array's end to the end of the memory are still the fill)
    for (size_t k = b + bytes; k < mem.size(); ++k) EXPECT(mem[k] == (char)0x5A);
    const size_t c = put(st, Spec{1, 17}, right.get());
    EXPECT(c == 16 + ((bytes + 15) & ~(size_t)15) && mem.size() == 256);
    EXPECT(std::memcmp(mem.data(), left.get(), 16) == 0 && std::memcmp(mem.data() + c, right.get(), 17) == 0);
    EXPECT(bytes == 0 || std::memcmp(mem.data() + b, mid.get(), bytes) == 0);
    for (size_t k = b + bytes; k < c; ++k) EXPECT(mem[k] == (char)0x5A);
    for (size_t k = c + 17; k < mem.size(); ++k) EXPECT(mem[k] == (char)0x5A);
    // take copies the same bytes out, into a block of exactly that size
    const std::unique_ptr<uint8_t[]> out = source(bytes, 0);
    if (s.width == 4)
      st.take(out.get(), StageArray<const int32_t>{b, s.count});
    else if (s.width == 17)
      st.take(out.get(), StageArray<const Wide>{b, s.count});
    else
      st.take(out.get(), StageArray<const uint8_t>{b, s.count});
    EXPECT(bytes == 0 || std::memcmp(out.get(), mid.get(), bytes) == 0);
  }
}

// room, host, on and place: typed addresses at the array's offset; a plan without arrays still has bytes to move.
static void check_rooms() {
  std::vector<char> mem;
  Stage st(mem);
  EXPECT(st.bytes() == 16 && st.bytes(0) == 0);
  const auto none = st.room<int32_t>(0);
  EXPECT(none.at == 0 && none.count == 0 && st.lay.size == 0 && mem.size() >= 16);
  const auto five = st.room<int32_t>(5);
  int32_t* host = st.host(five);
  for (int k = 0; k < 5; ++k) host[k] = 7 * k;
  const auto one = st.room<double>(1);
  *st.host(one) = 2.5;
  EXPECT(five.at == 0 && one.at == 32 && st.lay.size == 48 && mem.size() == 48);
  EXPECT((char*)st.host(five) == mem.data() && (char*)st.host(one) == mem.data() + 32 && st.host(five)[4] == 28);
  alignas(16) char device[64];
  EXPECT((char*)Stage::on(device, one) == device + 32 && (char*)StagePlan::on(device, five) == device);
  StagePlan out;
  const auto x = out.place<double>(3);
  const auto flags = out.place<uint8_t>(0);
  const auto status = out.place<int32_t>(3);
  EXPECT(x.at == 0 && flags.at == 32 && status.at == 32 && out.lay.size == 48 && out.bytes() == 48);
  // hold: memory for a plan that was only placed (an output buffer), which keeps what it has when it is large enough
  Stage back(mem);
  back.place<double>(2);
  EXPECT(back.hold() == mem.data() && mem.size() == 48);
  back.place<double>(9);
  EXPECT(back.hold() == mem.data() && mem.size() == 16 + 80);
}

int main() {
  check_sequences();
  check_neighbours();
  check_rooms();
  EXPECT(owner_cases() == 0);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
