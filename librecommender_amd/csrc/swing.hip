// Swing item-to-item scores (replaces rust/src/graph.rs:143-233, compute_single_swing / compute_swing_scores, of the
// reference's kNN engine):
//     s[i][j] = sum over user pairs u < v, both in U_i and U_j, of  w_u * w_v * 1 / (alpha + |I_u ^ I_v| - 1),  j != i,
// with w_u = 1 / sqrt(|I_u|).  The reference walks every user pair of every item and scatters the pair's term over the
// pair's common items; here every entry is owned by one wave, so no floating-point atomic is needed.
//
// Two stages:
//   1. swing_pairs_kernel: the user-pair table F, an upper (v > u) user x user CSR with f_uv = w_u * w_v / (alpha + c_uv - 1)
//      for every pair that shares an item.  Work items are (user u, 8,192-column tile) pairs, claimed and emitted by
//      tile_csr.hpp; a workgroup counts c_uv for its tile in LDS with integer atomics (the count does not depend on the
//      order), pass 0 writes the nnz of every work item, pass 1 recomputes and writes columns ascending and values at the
//      scanned offsets.
//   2. swing_scores_kernel: the score pattern is the set of item pairs with at least two common users (the item x item
//      co-occurrence of cf_sim.hip with min_common = 2, which counts, scans and fills it).  A wave takes an entry (i, j > i),
//      intersects U_i with U_j into a sorted list T (LDS, or a global slot when the shorter list exceeds the LDS budget),
//      and sums f_uv over the pairs of T: lane l takes the pairs l, l + 64, ... of the row-major upper triangle of T x T
//      in that order, f_uv is found by binary search in row u of F (or by its offset when the row holds every v > u),
//      and the 64 partial sums are reduced by a fixed butterfly.  The order depends on |T| alone, so two runs give the same bits; the value is written to (i, j) and to
//      its mirror (j, i), so the matrix is symmetric bit for bit.
// Every term is built from correctly rounded f32 sqrt, divisions and unfused products, as the reference builds it.
#include "tile_csr.hpp"

#pragma clang fp contract(off)

namespace lr {
namespace {

constexpr int kPairThreads = 256;
constexpr int kPairWaves = kPairThreads / kWave;
constexpr int kPairTile = 8192;                       // columns per LDS tile: one int32 count each
constexpr int kScoreThreads = 256;
constexpr int kScoreWaves = kScoreThreads / kWave;
constexpr int kScoreTCap = 2048;                      // users of one intersection kept in LDS, per wave
constexpr int kScoreChunk = 8;                        // entries claimed per atomic
constexpr int kScoreBlocksPerCU = 5;                  // 32 KB of LDS each
constexpr int kScoreGrid = kNumCU * kScoreBlocksPerCU;
constexpr size_t kCounterBytes = 256;

// w_u = 1 / sqrt(|I_u|) (graph.rs:210-213)
__device__ __forceinline__ float user_weight(int64_t deg) { return __fdiv_rn(1.0f, sqrtf(static_cast<float>(deg))); }

// w_u * w_v * (alpha + (c - 1)).recip() (graph.rs:185-186)
__device__ __forceinline__ float pair_term(float wu, float wv, float alpha, int c) {
  const float wuv = wu * wv;
  const float r = __fdiv_rn(1.0f, alpha + static_cast<float>(c - 1));
  return wuv * r;
}

struct PairArgs {
  const int64_t* u_ptr;    // user x item CSR
  const int32_t* u_col;
  const int64_t* i_ptr;    // item x user CSR
  const int32_t* i_col;
  int64_t n_users;
  float alpha;
  const int32_t* item_row;
  const int32_t* item_tile;
  const int32_t* order;
  int64_t n_items;
  int64_t* item_nnz;
  const int64_t* item_off;
  int32_t* out_col;
  float* out_val;
  int* counter;
};

template <int PASS>
__global__ __launch_bounds__(kPairThreads) void swing_pairs_kernel(PairArgs a) {
  __shared__ int sC[kPairTile];
  __shared__ int64_t sWave[kPairWaves];
  __shared__ int64_t sItem;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;

  for (;;) {
    const int64_t slot = claim_item(a.counter, &sItem);
    if (slot >= a.n_items) break;
    const int64_t item = a.order[slot];
    const int64_t u = a.item_row[item];
    const int64_t c0 = static_cast<int64_t>(a.item_tile[item]) * kPairTile;
    const int64_t c1 = (c0 + kPairTile < a.n_users) ? c0 + kPairTile : a.n_users;
    const int64_t first = (u + 1 > c0) ? u + 1 : c0;      // upper triangle only
    for (int j = tid; j < kPairTile; j += kPairThreads) sC[j] = 0;
    __syncthreads();
    const int64_t ub = a.u_ptr[u], ue = a.u_ptr[u + 1];
    for (int64_t k = ub + wave; k < ue; k += kPairWaves) {
      const int64_t y = a.u_col[k];
      const int64_t hi = a.i_ptr[y + 1];
      const int64_t lo = lower_bound_i32(a.i_col, a.i_ptr[y], hi, first);
      for (int64_t e = lo + lane; e < hi; e += kWave) {
        const int64_t c = a.i_col[e];
        if (c >= c1) break;
        atomicAdd(&sC[static_cast<int>(c - c0)], 1);
      }
    }
    __syncthreads();

    // The count pass asks only whether the pair shares an item: the term (two square roots, two divisions) is pass 1's.
    const float wu = PASS == 1 ? user_weight(ue - ub) : 0.0f;
    emit_tile<PASS, kPairThreads, kPairTile>(
        c0, c1, sWave, a.item_nnz, a.item_off, item, a.out_col, a.out_val, [&](int64_t c, int idx, float* v) {
          const int cnt = sC[idx];
          if (v != nullptr && cnt > 0) *v = pair_term(wu, user_weight(a.u_ptr[c + 1] - a.u_ptr[c]), a.alpha, cnt);
          return cnt > 0;
        });
  }
}

struct ScoreArgs {
  const int64_t* i_ptr;    // item x user CSR
  const int32_t* i_col;
  const int64_t* p_ptr;    // the pair table
  const int32_t* p_col;
  const float* p_val;
  const int64_t* s_ptr;    // the score pattern: symmetric, columns ascending
  const int32_t* s_col;
  const int32_t* s_row;    // row of every entry
  int64_t nnz;
  float* s_val;
  int64_t n_users;
  int32_t* slots;          // kScoreGrid * kScoreWaves slots of slot_len users
  int64_t slot_len;
  int* counter;
};

// A slot in global memory is written and then read by other lanes of the same wave: the reads go to L2.
template <bool IN_LDS>
__device__ __forceinline__ int t_load(const int32_t* T, int64_t k) {
  if (IN_LDS) return T[k];
  return __hip_atomic_load(T + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// U_i ^ U_j into T (ascending): the lanes take 64 users of the shorter list and look each up in the longer one.
__device__ __forceinline__ int intersect(const int32_t* __restrict__ A, int la, const int32_t* __restrict__ B, int lb,
                                         int32_t* T, int lane) {
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
  int t = 0;
  for (int b0 = 0; b0 < la; b0 += kWave) {
    const int k = b0 + lane;
    bool found = false;
    int32_t x = 0;
    if (k < la) {
      x = A[k];
      const int64_t pos = lower_bound_i32(B, 0, lb, x);
      found = pos < lb && B[pos] == x;
    }
    const uint64_t m = __ballot(found);
    if (found) T[t + __popcll(m & below)] = x;
    t += __popcll(m);
  }
  return t;
}

// The sum of f over the pairs of T: lane l takes the pairs l, l + 64, ... of the row-major upper triangle.
template <bool IN_LDS>
__device__ __forceinline__ float sum_pairs(const ScoreArgs& s, const int32_t* T, int t, int lane) {
  float acc = 0.0f;
  int a = 0, cur = -1;
  int64_t r = lane, lo = 0, hi = 0, u = 0;
  bool full = false;       // row u of F holds every v > u: column v sits at lo + (v - u - 1), no search
  for (;;) {
    while (a < t - 1 && r >= t - 1 - a) {
      r -= t - 1 - a;
      ++a;
    }
    if (a >= t - 1) break;
    if (a != cur) {
      u = t_load<IN_LDS>(T, a);
      lo = s.p_ptr[u];
      hi = s.p_ptr[u + 1];
      full = hi - lo == s.n_users - 1 - u;
      cur = a;
    }
    const int32_t v = t_load<IN_LDS>(T, a + 1 + r);
    if (full) {
      acc = acc + s.p_val[lo + (v - u - 1)];
    } else {
      const int64_t pos = lower_bound_i32(s.p_col, lo, hi, v);
      if (pos < hi && s.p_col[pos] == v) acc = acc + s.p_val[pos];
    }
    r += kWave;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
  return acc;
}

__global__ __launch_bounds__(kScoreThreads) void swing_scores_kernel(ScoreArgs s) {
  __shared__ int32_t sT[kScoreWaves][kScoreTCap];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int32_t* const lds_t = sT[wave];
  int32_t* const slot = s.slots + (static_cast<int64_t>(blockIdx.x) * kScoreWaves + wave) * s.slot_len;

  for (;;) {
    int64_t e0 = 0;
    if (lane == 0) e0 = static_cast<int64_t>(atomicAdd(s.counter, 1)) * kScoreChunk;
    e0 = __shfl(e0, 0);
    if (e0 >= s.nnz) break;
    const int64_t e1 = (e0 + kScoreChunk < s.nnz) ? e0 + kScoreChunk : s.nnz;
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t i = s.s_row[e], j = s.s_col[e];
      if (j <= i) continue;                               // written by the mirror entry
      const int64_t ib = s.i_ptr[i], jb = s.i_ptr[j];
      int la = static_cast<int>(s.i_ptr[i + 1] - ib), lb = static_cast<int>(s.i_ptr[j + 1] - jb);
      const int32_t* A = s.i_col + ib;
      const int32_t* B = s.i_col + jb;
      if (la > lb) {
        const int32_t* p = A; A = B; B = p;
        const int l = la; la = lb; lb = l;
      }
      float v = 0.0f;
      if (la <= kScoreTCap) {
        const int t = intersect(A, la, B, lb, lds_t, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        v = sum_pairs<true>(s, lds_t, t, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      } else if (la <= s.slot_len) {
        const int t = intersect(A, la, B, lb, slot, lane);
        __threadfence();
        v = sum_pairs<false>(s, slot, t, lane);
        __threadfence();
      }
      if (lane == 0) {
        s.s_val[e] = v;
        const int64_t mb = s.s_ptr[j], me = s.s_ptr[j + 1];
        const int64_t m = lower_bound_i32(s.s_col, mb, me, i);
        if (m < me && s.s_col[m] == i) s.s_val[m] = v;
      }
    }
  }
}

}  // namespace
}  // namespace lr

using namespace lr;

extern "C" int lr_swing_tile_cols(void) { return kPairTile; }

extern "C" int lr_swing_lds_users(void) { return kScoreTCap; }

extern "C" size_t lr_swing_pairs_ws_bytes(void) { return kCounterBytes; }

extern "C" int lr_swing_pairs_f32(const int64_t* u_ptr, const int32_t* u_col, const int64_t* i_ptr, const int32_t* i_col,
                                  int64_t n_users, float alpha, const int32_t* item_row, const int32_t* item_tile,
                                  const int32_t* order, int64_t n_items, int pass, int64_t* item_nnz,
                                  const int64_t* item_off, int32_t* out_col, float* out_val, void* ws, size_t ws_bytes,
                                  lr_stream_t stream) {
  if (n_users < 0 || n_users > INT32_MAX || n_items < 0 || (pass != 0 && pass != 1)) return LR_EINVAL;
  if (n_items == 0) return LR_OK;
  if (!u_ptr || !u_col || !i_ptr || !i_col || !item_row || !item_tile || !order) return LR_EINVAL;
  if ((pass == 0 && !item_nnz) || (pass == 1 && (!item_off || !out_col || !out_val))) return LR_EINVAL;
  if (ws == nullptr || ws_bytes < lr_swing_pairs_ws_bytes()) return LR_EWORKSPACE;
  PairArgs a{u_ptr, u_col, i_ptr, i_col, n_users, alpha, item_row, item_tile, order, n_items, item_nnz, item_off,
             out_col, out_val, static_cast<int*>(ws)};
  hipStream_t s = as_stream(stream);
  zero_words_async(ws, 1, s);
  const int grid = static_cast<int>(n_items < 4 * kNumCU ? n_items : 4 * kNumCU);
  if (pass == 0) hipLaunchKernelGGL(swing_pairs_kernel<0>, dim3(grid), dim3(kPairThreads), 0, s, a);
  else hipLaunchKernelGGL(swing_pairs_kernel<1>, dim3(grid), dim3(kPairThreads), 0, s, a);
  return launch_status();
}

extern "C" size_t lr_swing_scores_ws_bytes(int64_t max_item_users) {
  const int64_t slot = max_item_users > kScoreTCap ? max_item_users : 0;
  return kCounterBytes + static_cast<size_t>(kScoreGrid) * kScoreWaves * static_cast<size_t>(slot) * sizeof(int32_t);
}

extern "C" int lr_swing_scores_f32(const int64_t* i_ptr, const int32_t* i_col, int64_t max_item_users, int64_t n_users,
                                   const int64_t* p_ptr, const int32_t* p_col, const float* p_val, const int64_t* s_ptr,
                                   const int32_t* s_col, const int32_t* s_row, int64_t nnz, float* s_val, void* ws,
                                   size_t ws_bytes, lr_stream_t stream) {
  if (nnz < 0 || max_item_users < 0 || max_item_users > INT32_MAX || n_users < 0) return LR_EINVAL;
  if (nnz == 0) return LR_OK;
  if (!i_ptr || !i_col || !p_ptr || !p_col || !p_val || !s_ptr || !s_col || !s_row || !s_val) return LR_EINVAL;
  if (ws == nullptr || ws_bytes < lr_swing_scores_ws_bytes(max_item_users)) return LR_EWORKSPACE;
  ScoreArgs a{i_ptr, i_col, p_ptr, p_col, p_val, s_ptr, s_col, s_row, nnz, s_val, n_users,
              reinterpret_cast<int32_t*>(static_cast<unsigned char*>(ws) + kCounterBytes),
              max_item_users > kScoreTCap ? max_item_users : 0, static_cast<int*>(ws)};
  hipStream_t s = as_stream(stream);
  zero_words_async(ws, 1, s);
  const int64_t waves = ceil_div(nnz, kScoreChunk);
  const int grid = grid_for(waves, kScoreWaves, kScoreGrid);
  hipLaunchKernelGGL(swing_scores_kernel, dim3(grid), dim3(kScoreThreads), 0, s, a);
  return launch_status();
}
