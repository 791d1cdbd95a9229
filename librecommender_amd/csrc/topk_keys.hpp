// Order-preserving (score, id) keys and the wave-level selection over lists of them, shared by the full-catalogue scan
// (score_topk.hip) and the inverted-file scan (ivf.hip).  A key is (score bits made monotone << 32) | ~id: larger key = larger
// score, then smaller id — a total order, so a result does not depend on the tiling that produced its candidates.  0 is never a
// key of a finite or infinite score and marks an empty slot.
#pragma once
#include "common.hpp"

namespace lr {

__device__ __forceinline__ uint32_t fkey(float s) {
  const uint32_t b = __float_as_uint(s + 0.0f);  // -0 -> +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ uint64_t make_key(float s, uint32_t id) {
  return (static_cast<uint64_t>(fkey(s)) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - id);
}

// exact k-th largest key of L[0..cnt) (cnt >= k), wave-cooperative; returns it on all lanes.
__device__ __forceinline__ uint64_t wave_select_kth(const uint64_t* L, int cnt, int k, int lane) {
  uint64_t T = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const uint64_t trial = T | (1ull << bit);
    int c = 0;
    for (int j0 = 0; j0 < cnt; j0 += kWave) {
      const int j = j0 + lane;
      const bool ge = (j < cnt) && (L[j] >= trial);
      c += __popcll(__ballot(ge));
    }
    if (c >= k) T = trial;
  }
  return T;
}

// keep the entries >= T (exactly k of them when cnt >= k), in place, stable.  Returns new cnt.
__device__ __forceinline__ int wave_compact(uint64_t* L, int cnt, uint64_t T, int lane) {
  int base = 0;
  for (int j0 = 0; j0 < cnt; j0 += kWave) {
    const int j = j0 + lane;
    const uint64_t e = (j < cnt) ? L[j] : 0ull;
    const bool keep = (j < cnt) && (e >= T);
    const uint64_t mask = __ballot(keep);
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    if (keep) L[base + pre] = e;  // base+pre <= j: never overtakes unread data of this wave
    base += __popcll(mask);
  }
  return base;
}

__device__ __forceinline__ bool is_consumed(const int32_t* __restrict__ ci, int64_t lo, int64_t hi,
                                            int32_t id) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t v = ci[mid];
    if (v == id) return true;
    if (v < id) lo = mid + 1; else hi = mid;
  }
  return false;
}

__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ ci, int64_t lo,
                                                   int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(ci[mid]) < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace lr
