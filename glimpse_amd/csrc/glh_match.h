// glh_match.h -- what glimpse_hip.hip (the C ABI: glh_match_create / _put / _drop / _knn2 / _destroy) hands to
// glh_match.hip (the exact two nearest neighbours of optimize.match_keypoints, optimize.py:2234-2309).  Host-only
// declarations.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct glh_match;  // the C ABI's handle: the resident descriptor sets of one device (glh_match.hip)

namespace glh {

constexpr int MT_TIMES = 5;       // entries of times_ms (include/glimpse_hip.h)
constexpr int MT_U8_MAX_DIM = 256; // the integer path holds a query's whole descriptor in registers
constexpr int MT_MAX_ROWS = 1 << 30;
constexpr int MT_MAX_DIM = 1 << 16;
constexpr int64_t MT_MAX_ELEMS = (int64_t)1 << 35;  // rows x padded elements of one set: the preparation grid stays below 2^32

struct MatchSetInfo {  // of a resident set
  int kind, n, dim;
};

// The arguments have been checked (glimpse_hip.hip).  A GLH_* status, with the message left for glh_last_error() on
// failure (glh_stage.h: fail).
int match_create(int device, glh_match** out);
bool match_info(const glh_match* h, int slot, MatchSetInfo* info);  // false: nothing in that slot
int match_put(glh_match* h, int slot, int kind, int n, int dim, const void* data);
void match_drop(glh_match* h, int slot);
int match_knn2(glh_match* h, int slot_q, int slot_t, int32_t* idx, float* d2, double* times_ms);
void match_destroy(glh_match* h);

}  // namespace glh
