// UserCF / ItemCF ranking: the per-row top-k of the similarity matrix (libreco/bases/cf_base.py:340-355), the
// recommendation scoring of both models (algorithms/item_cf.py:117-149, user_cf.py:117-147, cf_base.py:310-338) and the
// neighbourhood prediction (item_cf.py:70-115, user_cf.py:70-115, cf_base.py:212-250).
//
// Selection is exact and deterministic: every candidate becomes a unique 64-bit key (value descending, then id
// ascending), a radix select over 8-bit digits (LDS integer histograms) finds the key of rank `need`, the keys up to it
// are gathered into LDS and sorted by a bitonic network, and the rounds repeat in slices of kSelMax for any k.
#include "common.hpp"

// The reference rounds every product and every sum to f32 (no contraction into an FMA).  HIP's __fmul_rn / __fadd_rn are
// plain operators in a header compiled with contraction on, so the two would still fuse; these are not contracted.
#pragma clang fp contract(off)

namespace lr {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kSelThreads = 256;
constexpr int kSelMax = 2048;          // keys sorted per round in LDS (16 KiB)

__device__ __forceinline__ uint64_t make_key(float v, int32_t id) {
  const uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);     // -0 ties with +0, as in Python's sort
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (static_cast<uint64_t>(~asc) << 32) | static_cast<uint32_t>(id);
}
__device__ __forceinline__ float key_value(uint64_t k) {
  const uint32_t asc = ~static_cast<uint32_t>(k >> 32);
  return __uint_as_float((asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc);
}
__device__ __forceinline__ int32_t key_id(uint64_t k) { return static_cast<int32_t>(static_cast<uint32_t>(k)); }

struct SelShared {
  uint64_t keys[kSelMax];
  int hist[256];
  int64_t red[kSelThreads / kWave];
  uint64_t thr;
  int64_t rem;
  int fill;
  int done;
};

__device__ int64_t block_sum_i64(int64_t v, SelShared& S) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) S.red[threadIdx.x / kWave] = v;
  __syncthreads();
  int64_t t = 0;
  for (int w = 0; w < kSelThreads / kWave; ++w) t += S.red[w];
  __syncthreads();
  return t;
}

// Writes the `m` = min(k, valid) smallest keys of src (src.get(e, key) -> valid) in ascending order through out(pos, key);
// returns the number of valid entries.
template <typename Src, typename Out>
__device__ int64_t select_sorted(const Src& src, int64_t n, int64_t k, SelShared& S, Out out) {
  const int tid = threadIdx.x;
  int64_t nv = 0;
  for (int64_t e = tid; e < n; e += kSelThreads) {
    uint64_t key;
    nv += src.get(e, key) ? 1 : 0;
  }
  const int64_t total = block_sum_i64(nv, S);
  const int64_t m = k < total ? k : total;
  bool has_prev = false;
  uint64_t prev = 0;
  for (int64_t written = 0; written < m;) {
    const int64_t need = (m - written) < kSelMax ? (m - written) : kSelMax;
    const int64_t remaining = total - written;
    uint64_t thr = ~0ull;
    if (remaining > kSelMax) {   // radix select of the key of rank `need` among the keys above prev
      uint64_t prefix = 0, mask = 0;
      if (tid == 0) {
        S.rem = need;
        S.done = 0;
      }
      for (int shift = 56; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += kSelThreads) S.hist[b] = 0;
        __syncthreads();
        for (int64_t e = tid; e < n; e += kSelThreads) {
          uint64_t key;
          if (src.get(e, key) && (!has_prev || key > prev) && (key & mask) == prefix)
            atomicAdd(&S.hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
          int64_t cum = 0, r = S.rem;
          int sel = 255;
          for (int b = 0; b < 256; ++b) {
            if (cum + S.hist[b] >= r) {
              sel = b;
              break;
            }
            cum += S.hist[b];
          }
          r -= cum;
          S.rem = r;
          S.done = (S.hist[sel] == r) ? 1 : 0;
          S.thr = static_cast<uint64_t>(sel);
        }
        __syncthreads();
        prefix |= S.thr << shift;
        mask |= 255ull << shift;
        const int done = S.done;
        __syncthreads();
        if (done) break;
      }
      thr = prefix | ~mask;
    }
    // gather (prev, thr] and sort
    if (tid == 0) S.fill = 0;
    __syncthreads();
    for (int64_t e = tid; e < n; e += kSelThreads) {
      uint64_t key;
      if (src.get(e, key) && (!has_prev || key > prev) && key <= thr) {
        const int p = atomicAdd(&S.fill, 1);
        if (p < kSelMax) S.keys[p] = key;
      }
    }
    __syncthreads();
    const int got = S.fill < kSelMax ? S.fill : kSelMax;
    int P = 1;
    while (P < got) P <<= 1;
    for (int i = got + tid; i < P; i += kSelThreads) S.keys[i] = ~0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < P; i += kSelThreads) {
          const int j = i ^ stride;
          if (j > i) {
            const bool up = (i & size) == 0;
            const uint64_t ki = S.keys[i], kj = S.keys[j];
            if ((ki > kj) == up) {
              S.keys[i] = kj;
              S.keys[j] = ki;
            }
          }
        }
        __syncthreads();
      }
    }
    for (int i = tid; i < need; i += kSelThreads) out(written + i, S.keys[i]);
    prev = S.keys[need - 1];
    has_prev = true;
    written += need;
    __syncthreads();
  }
  return total;
}

// ---- top-k of every similarity row ---------------------------------------------------------------------------------
struct CsrRowSrc {
  const int32_t* col;
  const float* val;
  int64_t base;
  __device__ bool get(int64_t e, uint64_t& key) const {
    key = make_key(val[base + e], col[base + e]);
    return true;
  }
};

__global__ __launch_bounds__(kSelThreads) void cf_topk_kernel(const int64_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ col,
                                                              const float* __restrict__ val, int64_t n_rows, int64_t k,
                                                              int32_t* __restrict__ out_ids,
                                                              float* __restrict__ out_sims,
                                                              int32_t* __restrict__ out_len) {
  __shared__ SelShared S;
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int64_t b = rowptr[r], n = rowptr[r + 1] - b;
    CsrRowSrc src{col, val, b};
    int32_t* ids = out_ids + r * k;
    float* sims = out_sims + r * k;
    const int64_t total = select_sorted(src, n, k, S, [&](int64_t pos, uint64_t key) {
      ids[pos] = key_id(key);
      sims[pos] = key_value(key);
    });
    if (threadIdx.x == 0) out_len[r] = static_cast<int32_t>(total < k ? total : k);
    __syncthreads();
  }
}

// ---- recommendation scoring --------------------------------------------------------------------------------------
struct ScoreSrc {
  const float* score;
  const uint8_t* flag;
  __device__ bool get(int64_t e, uint64_t& key) const {
    if (flag[e] != 1) return false;
    key = make_key(score[e], static_cast<int32_t>(e));
    return true;
  }
};

// flag[] per item of the user's scratch row: 0 untouched, 1 candidate, 2 touched but consumed (filtered out).
__global__ __launch_bounds__(kSelThreads) void cf_recommend_kernel(
    const int32_t* __restrict__ users, int64_t B, int user_cf, const int64_t* __restrict__ ui_ptr,
    const int32_t* __restrict__ ui_col, const float* __restrict__ ui_val, const int32_t* __restrict__ tk_ids,
    const float* __restrict__ tk_sims, const int32_t* __restrict__ tk_len, int64_t tk_k, int64_t n_items,
    const int64_t* __restrict__ cons_ptr, const int32_t* __restrict__ cons_idx, int filter_consumed, int64_t n_rec,
    float* __restrict__ score_ws, uint8_t* __restrict__ flag_ws, int32_t* __restrict__ out_ids,
    float* __restrict__ out_scores, int32_t* __restrict__ out_len, int64_t* __restrict__ out_ncand,
    int32_t* __restrict__ out_fallback) {
  __shared__ SelShared S;
  __shared__ int sTouched;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  const int64_t u = users[b];
  float* score = score_ws + b * n_items;
  uint8_t* flag = flag_ws + b * n_items;
  for (int64_t j = tid; j < n_items; j += kSelThreads) {
    score[j] = 0.0f;
    flag[j] = 0;
  }
  if (tid == 0) sTouched = 0;
  __syncthreads();
  int touched = 0;
  if (!user_cf) {
    // item_cf.py:117-140: the user's items in ascending id, each item's top-k list in top-k order
    for (int64_t p = ui_ptr[u]; p < ui_ptr[u + 1]; ++p) {
      const int64_t i = ui_col[p];
      const float label = ui_val[p];
      const int len = tk_len[i];
      for (int t = tid; t < len; t += kSelThreads) {
        const int32_t j = tk_ids[i * tk_k + t];
        score[j] = add_rn(score[j], mul_rn(tk_sims[i * tk_k + t], label));
        flag[j] = 1;
        touched = 1;
      }
      __syncthreads();
    }
  } else {
    // user_cf.py:117-135: the user's top-k similar users in top-k order, each one's items in ascending id
    const int len = tk_len[u];
    for (int t = 0; t < len; ++t) {
      const int64_t v = tk_ids[u * tk_k + t];
      const float sim = tk_sims[u * tk_k + t];
      for (int64_t p = ui_ptr[v] + tid; p < ui_ptr[v + 1]; p += kSelThreads) {
        const int32_t j = ui_col[p];
        score[j] = add_rn(score[j], mul_rn(sim, ui_val[p]));
        flag[j] = 1;
        touched = 1;
      }
      __syncthreads();
    }
  }
  if (touched) sTouched = 1;
  __syncthreads();
  if (filter_consumed) {
    for (int64_t p = cons_ptr[b] + tid; p < cons_ptr[b + 1]; p += kSelThreads) {
      const int32_t j = cons_idx[p];
      if (flag[j] == 1) flag[j] = 2;
    }
  }
  __syncthreads();
  ScoreSrc src{score, flag};
  int32_t* ids = out_ids + b * n_rec;
  float* sc = out_scores + b * n_rec;
  const int64_t total = select_sorted(src, n_items, n_rec, S, [&](int64_t pos, uint64_t key) {
    ids[pos] = key_id(key);
    sc[pos] = key_value(key);
  });
  if (tid == 0) {
    out_len[b] = static_cast<int32_t>(total < n_rec ? total : n_rec);
    out_ncand[b] = total;
    out_fallback[b] = sTouched == 0 ? 1 : (total == 0 ? 2 : 0);
  }
}

// ---- prediction ---------------------------------------------------------------------------------------------------
constexpr int kPredThreads = 256;

__device__ __forceinline__ float wave_sum_f(float v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v = add_rn(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// One wave per pair: the first k entries of the similarity row (column order) that are in the interaction row and
// positive; rating: sum(l * s / S) / sum(s / S) clipped, ranking: the mean of s (cf_base.py:212-250).
__global__ __launch_bounds__(kPredThreads) void cf_predict_kernel(
    const int32_t* __restrict__ srow, const int32_t* __restrict__ irow, int64_t n, const int64_t* __restrict__ s_ptr,
    const int32_t* __restrict__ s_col, const float* __restrict__ s_val, const int64_t* __restrict__ i_ptr,
    const int32_t* __restrict__ i_col, const float* __restrict__ i_val, int64_t k, int rating, float lower,
    float upper, float default_pred, float* __restrict__ pred, int32_t* __restrict__ none) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t waves = static_cast<int64_t>(gridDim.x) * (kPredThreads / kWave);
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * (kPredThreads / kWave) + threadIdx.x / kWave; q < n;
       q += waves) {
    const int64_t sr = srow[q], ir = irow[q];
    const int64_t sb = s_ptr[sr], sl = s_ptr[sr + 1] - sb;
    const int64_t m = sl < k ? sl : k;
    const int64_t ib = i_ptr[ir], ie = i_ptr[ir + 1];
    float S = 0.0f;
    int cnt = 0;
    for (int64_t e = lane; e < m; e += kWave) {
      const float s = s_val[sb + e];
      if (s > 0.0f) {
        const int32_t c = s_col[sb + e];
        int64_t lo = ib, hi = ie;
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (i_col[mid] < c) lo = mid + 1;
          else hi = mid;
        }
        if (lo < ie && i_col[lo] == c) {
          S = add_rn(S, s);
          cnt += 1;
        }
      }
    }
    S = wave_sum_f(S);
    cnt = wave_sum_i(cnt);
    float out = default_pred;
    if (cnt > 0) {
      if (!rating) {
        out = __fdiv_rn(S, static_cast<float>(cnt));
      } else {
        float num = 0.0f, den = 0.0f;
        for (int64_t e = lane; e < m; e += kWave) {
          const float s = s_val[sb + e];
          if (s > 0.0f) {
            const int32_t c = s_col[sb + e];
            int64_t lo = ib, hi = ie;
            while (lo < hi) {
              const int64_t mid = lo + ((hi - lo) >> 1);
              if (i_col[mid] < c) lo = mid + 1;
              else hi = mid;
            }
            if (lo < ie && i_col[lo] == c) {
              const float w = __fdiv_rn(s, S);
              num = add_rn(num, mul_rn(i_val[lo], w));
              den = add_rn(den, w);
            }
          }
        }
        num = wave_sum_f(num);
        den = wave_sum_f(den);
        out = __fdiv_rn(num, den);
        out = out < lower ? lower : (out > upper ? upper : out);
      }
    }
    if (lane == 0) {
      pred[q] = out;
      none[q] = cnt > 0 ? 0 : 1;
    }
  }
}

}  // namespace
}  // namespace lr

using namespace lr;

extern "C" int lr_cf_select_max(void) { return kSelMax; }

extern "C" int lr_cf_topk_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows, int64_t k,
                              int32_t* out_ids, float* out_sims, int32_t* out_len, lr_stream_t stream) {
  if (n_rows < 0 || k < 1 || k > INT32_MAX) return LR_EINVAL;
  if (n_rows == 0) return LR_OK;
  if (!rowptr || !out_ids || !out_sims || !out_len) return LR_EINVAL;
  const int grid = grid_for(n_rows, 1);
  hipLaunchKernelGGL(cf_topk_kernel, dim3(grid), dim3(kSelThreads), 0, as_stream(stream), rowptr, col, val, n_rows, k,
                     out_ids, out_sims, out_len);
  return launch_status();
}

extern "C" size_t lr_cf_recommend_ws_bytes(int64_t B, int64_t n_items) {
  if (B < 0 || n_items < 0) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(n_items) * (sizeof(float) + sizeof(uint8_t)) + 256;
}

extern "C" int lr_cf_recommend_f32(const int32_t* users, int64_t B, int user_cf, const int64_t* ui_ptr,
                                   const int32_t* ui_col, const float* ui_val, const int32_t* tk_ids,
                                   const float* tk_sims, const int32_t* tk_len, int64_t tk_k, int64_t n_items,
                                   const int64_t* cons_ptr, const int32_t* cons_idx, int filter_consumed,
                                   int64_t n_rec, int32_t* out_ids, float* out_scores, int32_t* out_len,
                                   int64_t* out_ncand, int32_t* out_fallback, void* ws, size_t ws_bytes,
                                   lr_stream_t stream) {
  if (B < 0 || n_items < 1 || n_items > INT32_MAX || n_rec < 1 || tk_k < 1) return LR_EINVAL;
  if (B == 0) return LR_OK;
  if (!users || !ui_ptr || !tk_ids || !tk_sims || !tk_len || !out_ids || !out_scores || !out_len || !out_ncand ||
      !out_fallback || (filter_consumed && (!cons_ptr || !cons_idx)))
    return LR_EINVAL;
  if (B > INT32_MAX) return LR_ESHAPE;
  if (ws == nullptr || ws_bytes < lr_cf_recommend_ws_bytes(B, n_items)) return LR_EWORKSPACE;
  float* score = static_cast<float*>(ws);
  uint8_t* flag = reinterpret_cast<uint8_t*>(score + B * n_items);
  hipLaunchKernelGGL(cf_recommend_kernel, dim3(static_cast<unsigned>(B)), dim3(kSelThreads), 0, as_stream(stream),
                     users, B, user_cf ? 1 : 0, ui_ptr, ui_col, ui_val, tk_ids, tk_sims, tk_len, tk_k, n_items,
                     cons_ptr, cons_idx, filter_consumed ? 1 : 0, n_rec, score, flag, out_ids, out_scores, out_len,
                     out_ncand, out_fallback);
  return launch_status();
}

extern "C" int lr_cf_predict_f32(const int32_t* srow, const int32_t* irow, int64_t n, const int64_t* s_ptr,
                                 const int32_t* s_col, const float* s_val, const int64_t* i_ptr, const int32_t* i_col,
                                 const float* i_val, int64_t k, int rating, float lower, float upper,
                                 float default_pred, float* pred, int32_t* none, lr_stream_t stream) {
  if (n < 0 || k < 0) return LR_EINVAL;
  if (n == 0) return LR_OK;
  if (!srow || !irow || !s_ptr || !i_ptr || !pred || !none) return LR_EINVAL;
  const int grid = grid_for(n, kPredThreads / kWave);
  hipLaunchKernelGGL(cf_predict_kernel, dim3(grid), dim3(kPredThreads), 0, as_stream(stream), srow, irow, n, s_ptr,
                     s_col, s_val, i_ptr, i_col, i_val, k, rating ? 1 : 0, lower, upper, default_pred, pred, none);
  return launch_status();
}
