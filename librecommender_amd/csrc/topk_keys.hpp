// Order-preserving (score, id) keys, the wave-level selection over lists of them and the workgroup's final sort and write-out,
// shared by the full-catalogue scan (score_topk.hip) and the inverted-file search (ivf_common.hpp, ivf.hip, ivf_sq8.hip).  A
// key is (score bits made monotone << 32) | ~id: larger key = larger score, then smaller id — a total order, so a result does
// not depend on the tiling that produced its candidates.  0 is never a key of a finite or infinite score and marks an empty
// slot.
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

// bitonic sort of a[0..K2) in LDS, descending, by the whole workgroup (K2 a power of two; empty slots, 0, end up last).  The
// caller's barrier after filling `a` comes before the call; the sort ends with one.
__device__ __forceinline__ void block_sort_keys_desc(uint64_t* a, int K2, int tid, int nthreads) {
  for (int size = 2; size <= K2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < K2 / 2; t += nthreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint64_t x = a[lo], y = a[hi];
        if (desc ? (x < y) : (x > y)) {
          a[lo] = y;
          a[hi] = x;
        }
      }
      __syncthreads();
    }
  }
}

// out_scores / out_ids [row * k ..): the first k of the sorted keys a[0..avail) as (score, id_base + id); -inf / -1 where the
// slot is empty or beyond `avail`
__device__ __forceinline__ void emit_topk(const uint64_t* a, int avail, int k, int64_t row, int64_t id_base,
                                          float* __restrict__ out_scores, int64_t* __restrict__ out_ids, int tid, int nthreads) {
  for (int r = tid; r < k; r += nthreads) {
    const uint64_t e = r < avail ? a[r] : 0ull;
    if (e == 0ull) {
      out_scores[row * k + r] = -INFINITY;
      out_ids[row * k + r] = -1;
    } else {
      out_scores[row * k + r] = fkey_inv(static_cast<uint32_t>(e >> 32));
      out_ids[row * k + r] = id_base + static_cast<int64_t>(0xFFFFFFFFu - static_cast<uint32_t>(e));
    }
  }
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
