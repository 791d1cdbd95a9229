// The two-pass, tile-by-tile CSR build shared by the similarity kernel (cf_sim.hip) and Swing's user-pair table
// (swing.hip).  Work items are (row, column tile) pairs that persistent workgroups claim one at a time; a workgroup
// accumulates its tile in LDS and then emits the kept columns in ascending order: pass 0 writes the item's count, pass 1
// writes columns and values at the item's offset (an exclusive scan of the counts, ops._two_pass_csr).  Nothing here
// computes a value: what is kept, and with which value, is the caller's callable, defined in the caller's file below its
// `#pragma clang fp contract(off)`, so include this header above that pragma.
#pragma once
#include "common.hpp"

namespace lr {

// first position in a[lo, hi) (ascending) whose value is not below v
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(a[mid]) < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename Kern>
int set_lds(Kern kern, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}

// The workgroup takes the next slot of the work list: one atomic per item, the same slot in every thread.  The second
// barrier keeps the next claim from overwriting *sItem (LDS) before every thread has read it.
__device__ __forceinline__ int64_t claim_item(int* counter, int64_t* sItem) {
  if (threadIdx.x == 0) *sItem = atomicAdd(counter, 1);
  __syncthreads();
  const int64_t slot = *sItem;
  __syncthreads();
  return slot;
}

// Emit the kept columns of the tile [c0, c1) in ascending order.  Wave w owns the contiguous columns
// [c0 + w * span, c0 + (w + 1) * span), 64 per round; a ballot keeps the order inside a round, the per-wave totals
// (sWave, LDS, one per wave) order the waves.  `entry(c, idx, v)` says whether column c (idx = c - c0) is kept; v is null
// where only that is asked (the counting rounds of both passes) and otherwise takes the column's value.  The tile's LDS
// state must be complete (a barrier behind it) on entry; ends in a barrier, after which it may be overwritten.
template <int PASS, int THREADS, int TILE, typename Entry>
__device__ __forceinline__ void emit_tile(int64_t c0, int64_t c1, int64_t* sWave, int64_t* item_nnz,
                                          const int64_t* item_off, int64_t item, int32_t* out_col, float* out_val,
                                          Entry entry) {
  constexpr int waves = THREADS / kWave, span = TILE / waves;
  static_assert(THREADS % kWave == 0 && TILE % (waves * kWave) == 0, "a wave's span is whole rounds of 64 columns");
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t wb = c0 + static_cast<int64_t>(wave) * span;
  int64_t kept = 0;
  for (int r = 0; r < span; r += kWave) {
    const int64_t c = wb + r + lane;
    bool keep = false;
    if (c < c1) keep = entry(c, static_cast<int>(c - c0), static_cast<float*>(nullptr));
    kept += __popcll(__ballot(keep));
  }
  if (lane == 0) sWave[wave] = kept;
  __syncthreads();
  if (PASS == 0) {
    if (tid == 0) {
      int64_t t = 0;
      for (int w = 0; w < waves; ++w) t += sWave[w];
      item_nnz[item] = t;
    }
  } else {
    int64_t base = item_off[item];
    for (int w = 0; w < wave; ++w) base += sWave[w];
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
    for (int r = 0; r < span; r += kWave) {
      const int64_t c = wb + r + lane;
      bool keep = false;
      float v = 0.0f;
      if (c < c1) keep = entry(c, static_cast<int>(c - c0), &v);
      const uint64_t m = __ballot(keep);
      if (keep) {
        const int64_t pos = base + __popcll(m & below);
        out_col[pos] = static_cast<int32_t>(c);
        out_val[pos] = v;
      }
      base += __popcll(m);
    }
  }
  __syncthreads();
}

// The same emit for a caller that keeps more than one value per column (the pair state of cf_sim.hip): `keep(c, idx)`
// says whether column c is kept, and in pass 1 `write(pos, c, idx)` stores it at position pos of the output, the item's
// offset plus the number of kept columns below c.  Same conditions on entry and exit as emit_tile.
template <int PASS, int THREADS, int TILE, typename Keep, typename Write>
__device__ __forceinline__ void emit_tile_to(int64_t c0, int64_t c1, int64_t* sWave, int64_t* item_nnz,
                                             const int64_t* item_off, int64_t item, Keep keep, Write write) {
  constexpr int waves = THREADS / kWave, span = TILE / waves;
  static_assert(THREADS % kWave == 0 && TILE % (waves * kWave) == 0, "a wave's span is whole rounds of 64 columns");
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t wb = c0 + static_cast<int64_t>(wave) * span;
  int64_t kept = 0;
  for (int r = 0; r < span; r += kWave) {
    const int64_t c = wb + r + lane;
    kept += __popcll(__ballot(c < c1 && keep(c, static_cast<int>(c - c0))));
  }
  if (lane == 0) sWave[wave] = kept;
  __syncthreads();
  if (PASS == 0) {
    if (tid == 0) {
      int64_t t = 0;
      for (int w = 0; w < waves; ++w) t += sWave[w];
      item_nnz[item] = t;
    }
  } else {
    int64_t base = item_off[item];
    for (int w = 0; w < wave; ++w) base += sWave[w];
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
    for (int r = 0; r < span; r += kWave) {
      const int64_t c = wb + r + lane;
      const bool k = c < c1 && keep(c, static_cast<int>(c - c0));
      const uint64_t m = __ballot(k);
      if (k) write(base + __popcll(m & below), c, static_cast<int>(c - c0));
      base += __popcll(m);
    }
  }
  __syncthreads();
}

}  // namespace lr
