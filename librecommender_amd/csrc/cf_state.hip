// RsUserCF / RsItemCF: what the incremental neighbourhood models keep and refresh on the device, next to the pair state of
// cf_sim.hip (rust/src/similarities.rs, incremental.rs, item_cf.rs, user_cf.rs, inference.rs).
//
//   sums of squares   one wave per row: 64 squares are loaded at once and folded by lane order into one sequential f32
//                     chain, the reference's `fold(0.0, |ss, d| ss + d * d)` over the row in ascending column order.
//   merge and refresh the row-wise union of the old state CSR and the delta CSR (both with ascending columns).  Work is
//                     assigned by entries, not by rows, so a row of any length is spread over as many workgroups as it
//                     needs: a workgroup takes kMgChunk consecutive entries of one side, finds the rows of its first and
//                     last entry by binary search over the rowptr, and every thread finds its entry's row between the two
//                     (no step at all inside a long row) and its entry's rank in the other side's row by binary search.
//                     Pass 0 flags the delta entries that the old state does not hold; their running count (`rank`, an
//                     exclusive scan with the total behind it, made by the caller) places every entry in pass 1: an old
//                     entry e goes to e + rank[j], j its lower bound in the delta row, and a new delta entry j to
//                     i + rank[j], i its lower bound in the old row.  A pair of the delta gets prod = old + delta (one f32
//                     add), cnt = old + delta and a fresh cosine from the sums of squares; every other pair is copied bit
//                     for bit, also where a sum of squares of its rows has changed (the reference's scheme).
//   predict           one wave per pair: the top-k list of the similarity row, cut to k, is intersected with the
//                     interaction row by binary search, and the hits are summed in list order.
// Nothing here uses a floating-point atomic: every value is computed by one thread from fixed operands.
#include "tile_csr.hpp"

// The reference rounds every product and every sum to f32 (no contraction into an FMA).
#pragma clang fp contract(off)

namespace lr {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

// ---- sums of squares -----------------------------------------------------------------------------------------------
constexpr int kSqThreads = 256;

__global__ __launch_bounds__(kSqThreads) void cf_sumsq_kernel(const int64_t* __restrict__ ptr,
                                                              const float* __restrict__ val, int64_t n_rows,
                                                              int accumulate, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kSqThreads / kWave);
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * (kSqThreads / kWave) + threadIdx.x / kWave; r < n_rows;
       r += waves) {
    const int64_t b = ptr[r], e = ptr[r + 1];
    float s = 0.0f;
    for (int64_t k0 = b; k0 < e; k0 += kWave) {
      float sq = 0.0f;
      if (k0 + lane < e) {
        const float d = val[k0 + lane];
        sq = mul_rn(d, d);
      }
      const int nb = static_cast<int>((e - k0) < kWave ? (e - k0) : kWave);
      for (int l = 0; l < nb; ++l) s = add_rn(s, __shfl(sq, l));   // lane order: ascending column
    }
    if (lane == 0) out[r] = accumulate ? add_rn(out[r], s) : s;
  }
}

// ---- merge and refresh ---------------------------------------------------------------------------------------------
constexpr int kMgThreads = 256;
constexpr int kMgChunk = 2048;       // entries of one side per workgroup pass

// the row of entry e: the last r of [lo, hi] with ptr[r] <= e (ptr ascending, ptr[lo] <= e; empty rows are skipped)
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t e) {
  int64_t end = hi + 1;
  while (end - lo > 1) {
    const int64_t mid = lo + ((end - lo) >> 1);
    if (ptr[mid] <= e) lo = mid;
    else end = mid;
  }
  return lo;
}

// `compute_cosine` (similarities.rs:22-29) / `accumulate_cosine` (incremental.rs:104-110).  sqrtf, not __fsqrt_rn: in
// this toolchain's headers the latter is the native 1-ulp square root, the former the correctly rounded one.
__device__ __forceinline__ float cosine(float prod, float s1, float s2) {
  if (prod == 0.0f || s1 == 0.0f || s2 == 0.0f) return 0.0f;
  return __fdiv_rn(prod, mul_rn(sqrtf(s1), sqrtf(s2)));
}

struct MergeArgs {
  const int64_t* o_ptr;
  const int32_t* o_col;
  const float* o_prod;
  const int32_t* o_cnt;
  const float* o_sim;
  int64_t o_nnz;
  const int64_t* d_ptr;
  const int32_t* d_col;
  const float* d_prod;
  const int32_t* d_cnt;
  int64_t d_nnz;
  int64_t n_x;
  const float* sumsq;
  uint8_t* is_new;         // pass 0
  const int64_t* rank;     // pass 1: [d_nnz + 1]
  int32_t* out_col;
  float* out_prod;
  int32_t* out_cnt;
  float* out_sim;
};

// Calls body(e, row) for every entry e of the CSR side `ptr` (nnz entries, n_x rows), kMgChunk entries per workgroup pass.
template <typename Body>
__device__ __forceinline__ void for_entries(const int64_t* __restrict__ ptr, int64_t nnz, int64_t n_x, Body body) {
  __shared__ int64_t sRow[2];
  for (int64_t e0 = static_cast<int64_t>(blockIdx.x) * kMgChunk; e0 < nnz;
       e0 += static_cast<int64_t>(gridDim.x) * kMgChunk) {
    const int64_t e1 = (e0 + kMgChunk < nnz) ? e0 + kMgChunk : nnz;
    if (threadIdx.x < 2) sRow[threadIdx.x] = row_of(ptr, 0, n_x - 1, threadIdx.x == 0 ? e0 : e1 - 1);
    __syncthreads();
    const int64_t r_lo = sRow[0], r_hi = sRow[1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += kMgThreads) body(e, row_of(ptr, r_lo, r_hi, e));
    __syncthreads();   // sRow is rewritten by the next chunk
  }
}

// pass 0: is_new[j] = 1 where the old row does not hold the delta entry's column
__global__ __launch_bounds__(kMgThreads) void cf_merge_flag_kernel(MergeArgs a) {
  for_entries(a.d_ptr, a.d_nnz, a.n_x, [&](int64_t j, int64_t r) {
    const int32_t c = a.d_col[j];
    const int64_t oe = a.o_ptr[r + 1];
    const int64_t i = lower_bound_i32(a.o_col, a.o_ptr[r], oe, c);
    a.is_new[j] = (i < oe && a.o_col[i] == c) ? 0 : 1;
  });
}

// pass 1, the old side: every old entry, merged with its delta entry where there is one
__global__ __launch_bounds__(kMgThreads) void cf_merge_old_kernel(MergeArgs a) {
  for_entries(a.o_ptr, a.o_nnz, a.n_x, [&](int64_t e, int64_t r) {
    const int32_t c = a.o_col[e];
    const int64_t de = a.d_ptr[r + 1];
    const int64_t j = lower_bound_i32(a.d_col, a.d_ptr[r], de, c);
    const int64_t pos = e + a.rank[j];
    float prod = a.o_prod[e], sim = a.o_sim[e];
    int32_t cnt = a.o_cnt[e];
    if (j < de && a.d_col[j] == c) {
      prod = add_rn(prod, a.d_prod[j]);
      cnt += a.d_cnt[j];
      sim = cosine(prod, a.sumsq[r], a.sumsq[c]);
    }
    a.out_col[pos] = c;
    a.out_prod[pos] = prod;
    a.out_cnt[pos] = cnt;
    a.out_sim[pos] = sim;
  });
}

// pass 1, the delta side: the entries that the old state does not hold
__global__ __launch_bounds__(kMgThreads) void cf_merge_new_kernel(MergeArgs a) {
  for_entries(a.d_ptr, a.d_nnz, a.n_x, [&](int64_t j, int64_t r) {
    const int64_t before = a.rank[j];
    if (a.rank[j + 1] == before) return;
    const int32_t c = a.d_col[j];
    const int64_t pos = lower_bound_i32(a.o_col, a.o_ptr[r], a.o_ptr[r + 1], c) + before;
    const float prod = a.d_prod[j];
    a.out_col[pos] = c;
    a.out_prod[pos] = prod;
    a.out_cnt[pos] = a.d_cnt[j];
    a.out_sim[pos] = cosine(prod, a.sumsq[r], a.sumsq[c]);
  });
}

// ---- prediction ----------------------------------------------------------------------------------------------------
constexpr int kPredThreads = 256;

// One wave per pair (item_cf.rs:118-153, user_cf.rs:113-148, inference.rs:11-71): the first min(k, len) entries of the
// top-k list of row srow[q] that the interaction row irow[q] holds, whatever their label; ranking S / n with S the
// sequential sum of the hit sims in list order, rating the sequential sum of (label * sim) / S; nothing is clipped.
__global__ __launch_bounds__(kPredThreads) void cf_predict_topk_kernel(
    const int32_t* __restrict__ srow, const int32_t* __restrict__ irow, int64_t n, const int32_t* __restrict__ tk_ids,
    const float* __restrict__ tk_sims, const int32_t* __restrict__ tk_len, int64_t tk_k, int64_t k,
    const int64_t* __restrict__ i_ptr, const int32_t* __restrict__ i_col, const float* __restrict__ i_val, int rating,
    float default_pred, float* __restrict__ pred, int32_t* __restrict__ none) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kPredThreads / kWave);
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * (kPredThreads / kWave) + threadIdx.x / kWave; q < n;
       q += waves) {
    const int64_t sr = srow[q], ir = irow[q];
    const int64_t have = tk_len[sr] < tk_k ? tk_len[sr] : tk_k;
    const int64_t len = have < k ? have : k;
    const int64_t ib = i_ptr[ir], ie = i_ptr[ir + 1];
    float S = 0.0f, out = 0.0f;
    int cnt = 0;
    for (int round = 0; round < (rating ? 2 : 1); ++round) {   // rating: S first, then the weighted labels
      for (int64_t t0 = 0; t0 < len; t0 += kWave) {
        const int64_t t = t0 + lane;
        bool hit = false;
        float s = 0.0f, l = 0.0f;
        if (t < len) {
          const int32_t c = tk_ids[sr * tk_k + t];
          const int64_t p = lower_bound_i32(i_col, ib, ie, c);
          if (p < ie && i_col[p] == c) {
            hit = true;
            s = tk_sims[sr * tk_k + t];
            l = i_val[p];
          }
        }
        for (uint64_t m = __ballot(hit); m != 0; m &= m - 1) {   // list order; the same in every lane
          const int b = __ffsll(static_cast<unsigned long long>(m)) - 1;
          const float sb = __shfl(s, b), lb = __shfl(l, b);
          if (round == 0) {
            S = add_rn(S, sb);
            cnt += 1;
          } else {
            out = add_rn(out, __fdiv_rn(mul_rn(lb, sb), S));
          }
        }
      }
      if (cnt == 0) break;
    }
    if (!rating && cnt > 0) out = __fdiv_rn(S, static_cast<float>(cnt));
    if (lane == 0) {
      pred[q] = cnt > 0 ? out : default_pred;
      none[q] = cnt > 0 ? 0 : 1;
    }
  }
}

}  // namespace
}  // namespace lr

using namespace lr;

extern "C" int lr_cf_sumsq_f32(const int64_t* ptr, const float* val, int64_t n_rows, int accumulate, float* out,
                               lr_stream_t stream) {
  if (n_rows < 0) return LR_EINVAL;
  if (n_rows == 0) return LR_OK;
  if (!ptr || !out) return LR_EINVAL;
  const int grid = grid_for(n_rows, kSqThreads / kWave);
  hipLaunchKernelGGL(cf_sumsq_kernel, dim3(grid), dim3(kSqThreads), 0, as_stream(stream), ptr, val, n_rows,
                     accumulate ? 1 : 0, out);
  return launch_status();
}

extern "C" int lr_cf_state_merge_f32(const int64_t* o_ptr, const int32_t* o_col, const float* o_prod,
                                     const int32_t* o_cnt, const float* o_sim, int64_t o_nnz, const int64_t* d_ptr,
                                     const int32_t* d_col, const float* d_prod, const int32_t* d_cnt, int64_t d_nnz,
                                     int64_t n_x, const float* sumsq, int pass, uint8_t* is_new, const int64_t* rank,
                                     int32_t* out_col, float* out_prod, int32_t* out_cnt, float* out_sim,
                                     lr_stream_t stream) {
  if (n_x < 0 || n_x > INT32_MAX || o_nnz < 0 || d_nnz < 0 || (pass != 0 && pass != 1)) return LR_EINVAL;
  if (n_x == 0 || (o_nnz == 0 && d_nnz == 0)) return LR_OK;
  if (!o_ptr || !d_ptr) return LR_EINVAL;
  if (o_nnz > 0 && (!o_col || !o_prod || !o_cnt || !o_sim)) return LR_EINVAL;
  if (d_nnz > 0 && (!d_col || !d_prod || !d_cnt)) return LR_EINVAL;
  if (pass == 0 && d_nnz > 0 && !is_new) return LR_EINVAL;
  if (pass == 1 && (!rank || !sumsq || !out_col || !out_prod || !out_cnt || !out_sim)) return LR_EINVAL;
  MergeArgs a{o_ptr, o_col, o_prod, o_cnt, o_sim, o_nnz, d_ptr, d_col, d_prod, d_cnt, d_nnz, n_x, sumsq,
              is_new, rank, out_col, out_prod, out_cnt, out_sim};
  hipStream_t s = as_stream(stream);
  if (pass == 0) {
    if (d_nnz > 0)
      hipLaunchKernelGGL(cf_merge_flag_kernel, dim3(grid_for(d_nnz, kMgChunk)), dim3(kMgThreads), 0, s, a);
  } else {
    if (o_nnz > 0)
      hipLaunchKernelGGL(cf_merge_old_kernel, dim3(grid_for(o_nnz, kMgChunk)), dim3(kMgThreads), 0, s, a);
    if (d_nnz > 0)
      hipLaunchKernelGGL(cf_merge_new_kernel, dim3(grid_for(d_nnz, kMgChunk)), dim3(kMgThreads), 0, s, a);
  }
  return launch_status();
}

extern "C" int lr_cf_predict_topk_f32(const int32_t* srow, const int32_t* irow, int64_t n, const int32_t* tk_ids,
                                      const float* tk_sims, const int32_t* tk_len, int64_t tk_k, int64_t k,
                                      const int64_t* i_ptr, const int32_t* i_col, const float* i_val, int rating,
                                      float default_pred, float* pred, int32_t* none, lr_stream_t stream) {
  if (n < 0 || k < 0 || tk_k < 1) return LR_EINVAL;
  if (n == 0) return LR_OK;
  if (!srow || !irow || !tk_ids || !tk_sims || !tk_len || !i_ptr || !pred || !none) return LR_EINVAL;
  const int grid = grid_for(n, kPredThreads / kWave);
  hipLaunchKernelGGL(cf_predict_topk_kernel, dim3(grid), dim3(kPredThreads), 0, as_stream(stream), srow, irow, n,
                     tk_ids, tk_sims, tk_len, tk_k, k, i_ptr, i_col, i_val, rating ? 1 : 0, default_pred, pred, none);
  return launch_status();
}
