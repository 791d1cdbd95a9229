// Sub-wave row groups of BPR (bpr.hip) and SVD / SVD++ (svd.hip): G lanes hold one row of up to G * R floats, R per lane.
// Not shared on purpose: the staged gathers (bpr_fetch_block, the loop of svdpp_pool_kernel, hist_accum), which cost
// the update kernels 6 - 16 VGPRs as a shared helper, and the long-run workspace of svd.hip against embed_scatter.hip,
// which is on the timed path of the benchmark.
#pragma once
#include "common.hpp"

namespace lr {

// all-reduce over the G lanes of a group; every lane of the wave takes part
template <int G>
__device__ __forceinline__ float group_sum(float x) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// this thread's group among all groups of a grid of kBlock-thread workgroups, and the number of those groups
template <int G>
__device__ __forceinline__ int64_t group_index() {
  return (static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x) / G;
}
template <int G>
__device__ __forceinline__ int64_t group_stride() {
  return static_cast<int64_t>(gridDim.x) * (kBlock / G);
}

}  // namespace lr

// group size G and dwords per lane R for a row of D <= 256 floats: returns CALL(G, R)
#define LR_ROW_GROUP_DISPATCH_256(D, CALL) \
  do {                                     \
    if ((D) <= 16) return CALL(16, 1);     \
    if ((D) <= 32) return CALL(16, 2);     \
    if ((D) <= 64) return CALL(32, 2);     \
    if ((D) <= 128) return CALL(64, 2);    \
    return CALL(64, 4);                    \
  } while (0)
