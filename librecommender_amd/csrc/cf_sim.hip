// UserCF / ItemCF similarity (replaces libreco/utils/_similarities.pyx:17-533): the symmetric sparse co-occurrence
// product of the forward CSR X (n_x rows over y) with its inverted index Y (the transpose), with the per-pair count, the
// `min_common` threshold and the cosine / pearson / jaccard normalisation, written straight into the full symmetric CSR.
//
// Work items are (row x1, column tile) pairs.  A workgroup keeps an f32 product sum and an int32 count per column of its
// tile in LDS, walks x1's y-list in ascending y and, for every y, adds the products of the entries of Y[y] that fall into
// the tile (found by binary search when the row spans more than one tile).  The entries of one Y[y] have distinct
// columns, and a barrier separates consecutive y, so every column is accumulated in ascending y with an unfused multiply
// and add: the reference's f32 order, with no atomics.  (x1, x2) and (x2, x1) get the same bits because the product is
// commutative.  The count pass writes the nnz of every work item; the fill pass recomputes and writes the columns in
// ascending order at the item's offset (an exclusive scan of the counts): the claim and the emit of tile_csr.hpp.
//
// The pair state of RsUserCF / RsItemCF (rust/src/similarities.rs:120-180, incremental.rs:24-73) is the same accumulation
// with another epilogue (STATE): every column with a count above 0 is emitted with its product sum and its count, whatever
// the sum is, and nothing is normalised.
#include "tile_csr.hpp"

// The reference rounds every product and every sum to f32 (no contraction into an FMA).  HIP's __fmul_rn / __fadd_rn are
// plain operators in a header compiled with contraction on, so the two would still fuse; these are not contracted.
#pragma clang fp contract(off)

namespace lr {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }

constexpr int kSimThreads = 512;
constexpr int kSimWaves = kSimThreads / kWave;
constexpr int kSimTile = 8192;                        // columns per LDS tile: 8 B each
constexpr int kSimBatch = kSimThreads;                // y metadata staged per batch
constexpr int kSimGroup = 8;                          // y whose first chunk is loaded before the LDS updates

constexpr size_t kSimLds = static_cast<size_t>(kSimTile) * (sizeof(float) + sizeof(int)) +
                           static_cast<size_t>(kSimBatch) * (sizeof(int64_t) + sizeof(int) + sizeof(float)) +
                           static_cast<size_t>(kSimWaves + 1) * sizeof(int64_t) + 64;

struct SimArgs {
  const int64_t* x_ptr;
  const int32_t* x_col;
  const float* x_val;
  const int64_t* y_ptr;
  const int32_t* y_col;
  const float* y_val;
  int64_t n_x;
  const float* norm;
  const int32_t* cnt;
  int jaccard;
  int min_common;
  const int32_t* item_row;
  const int32_t* item_tile;
  const int32_t* order;
  int64_t n_items;
  int64_t* item_nnz;
  const int64_t* item_off;
  int32_t* out_col;
  float* out_val;
  int32_t* out_cnt;      // STATE only
  int* counter;
};

// The similarity of (x1, x2) from the accumulated product sum and count, 0 when the pair is not kept
// (_similarities.pyx:125-133 cosine, :232-240 pearson, :330-334 jaccard).
__device__ __forceinline__ float pair_value(const SimArgs& a, int64_t x1, int64_t x2, float prods, int count) {
  if (count < a.min_common) return 0.0f;
  if (a.jaccard) {
    const float inter = static_cast<float>(count);
    const float uni = sub_rn(static_cast<float>(a.cnt[x1] + a.cnt[x2]), inter);
    return __fdiv_rn(inter, uni);
  }
  const float n1 = a.norm[x1], n2 = a.norm[x2];
  if (prods == 0.0f || n1 == 0.0f || n2 == 0.0f) return 0.0f;
  return __fdiv_rn(prods, mul_rn(n1, n2));
}

template <int PASS, bool STATE>
__global__ __launch_bounds__(kSimThreads) void cf_sim_kernel(SimArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  float* sP = reinterpret_cast<float*>(lds);
  int* sC = reinterpret_cast<int*>(sP + kSimTile);
  int64_t* sLo = reinterpret_cast<int64_t*>(sC + kSimTile);
  int* sLen = reinterpret_cast<int*>(sLo + kSimBatch);
  float* sA = reinterpret_cast<float*>(sLen + kSimBatch);
  int64_t* sWave = reinterpret_cast<int64_t*>(sA + kSimBatch);   // [kSimWaves + 1]
  __shared__ int64_t sItem;

  const int tid = threadIdx.x;
  const int64_t n_tiles = ceil_div(a.n_x, kSimTile);

  for (;;) {
    const int64_t slot = claim_item(a.counter, &sItem);
    if (slot >= a.n_items) break;
    const int64_t item = a.order[slot];
    const int64_t x1 = a.item_row[item];
    const int64_t c0 = static_cast<int64_t>(a.item_tile[item]) * kSimTile;
    const int64_t c1 = (c0 + kSimTile < a.n_x) ? c0 + kSimTile : a.n_x;
    const bool whole = n_tiles == 1;

    for (int j = tid; j < kSimTile; j += kSimThreads) {
      sP[j] = 0.0f;
      sC[j] = 0;
    }
    const int64_t xb = a.x_ptr[x1], xe = a.x_ptr[x1 + 1];
    for (int64_t k0 = xb; k0 < xe; k0 += kSimBatch) {
      const int nb = static_cast<int>((xe - k0) < kSimBatch ? (xe - k0) : kSimBatch);
      __syncthreads();   // the previous batch's metadata is no longer read
      if (tid < nb) {
        const int64_t y = a.x_col[k0 + tid];
        int64_t lo = a.y_ptr[y], hi = a.y_ptr[y + 1];
        if (!whole) {
          lo = lower_bound_i32(a.y_col, lo, hi, c0);
          hi = lower_bound_i32(a.y_col, lo, hi, c1);
        }
        sLo[tid] = lo;
        sLen[tid] = static_cast<int>(hi - lo);
        sA[tid] = a.jaccard ? 0.0f : a.x_val[k0 + tid];
      }
      __syncthreads();
      for (int g0 = 0; g0 < nb; g0 += kSimGroup) {
        int cc[kSimGroup];
        float bb[kSimGroup];
#pragma unroll
        for (int g = 0; g < kSimGroup; ++g) {
          cc[g] = -1;
          bb[g] = 0.0f;
          const int j = g0 + g;
          if (j < nb && tid < sLen[j]) {
            cc[g] = a.y_col[sLo[j] + tid];
            if (!a.jaccard) bb[g] = a.y_val[sLo[j] + tid];
          }
        }
#pragma unroll
        for (int g = 0; g < kSimGroup; ++g) {
          const int j = g0 + g;
          if (j < nb) {   // uniform over the workgroup
            const float av = sA[j];
            if (cc[g] >= 0 && cc[g] != x1) {
              const int idx = static_cast<int>(cc[g] - c0);
              if (!a.jaccard) sP[idx] = add_rn(sP[idx], mul_rn(av, bb[g]));
              sC[idx] += 1;
            }
            const int len = sLen[j];
            for (int k = tid + kSimThreads; k < len; k += kSimThreads) {
              const int64_t e = sLo[j] + k;
              const int c = a.y_col[e];
              if (c != x1) {
                const int idx = static_cast<int>(c - c0);
                if (!a.jaccard) sP[idx] = add_rn(sP[idx], mul_rn(av, a.y_val[e]));
                sC[idx] += 1;
              }
            }
            __syncthreads();
          }
        }
      }
    }
    __syncthreads();

    if constexpr (STATE) {
      emit_tile_to<PASS, kSimThreads, kSimTile>(c0, c1, sWave, a.item_nnz, a.item_off, item,
                                                [&](int64_t, int idx) { return sC[idx] > 0; },
                                                [&](int64_t pos, int64_t c, int idx) {
                                                  a.out_col[pos] = static_cast<int32_t>(c);
                                                  a.out_val[pos] = sP[idx];
                                                  a.out_cnt[pos] = sC[idx];
                                                });
    } else {
      emit_tile<PASS, kSimThreads, kSimTile>(c0, c1, sWave, a.item_nnz, a.item_off, item, a.out_col, a.out_val,
                                             [&](int64_t c, int idx, float* v) {
                                               const float sim = pair_value(a, x1, c, sP[idx], sC[idx]);
                                               if (v != nullptr) *v = sim;
                                               return sim != 0.0f;
                                             });
    }
  }
}

}  // namespace
}  // namespace lr

using namespace lr;

template <bool STATE>
static int launch_sim(const SimArgs& a, int pass, lr_stream_t stream) {
  hipStream_t s = as_stream(stream);
  zero_words_async(a.counter, 1, s);
  const int grid = static_cast<int>(a.n_items < 2 * kNumCU ? a.n_items : 2 * kNumCU);
  int rc;
  if (pass == 0) {
    if ((rc = set_lds(cf_sim_kernel<0, STATE>, kSimLds)) != LR_OK) return rc;
    hipLaunchKernelGGL((cf_sim_kernel<0, STATE>), dim3(grid), dim3(kSimThreads), kSimLds, s, a);
  } else {
    if ((rc = set_lds(cf_sim_kernel<1, STATE>, kSimLds)) != LR_OK) return rc;
    hipLaunchKernelGGL((cf_sim_kernel<1, STATE>), dim3(grid), dim3(kSimThreads), kSimLds, s, a);
  }
  return launch_status();
}

extern "C" int lr_cf_sim_tile_cols(void) { return kSimTile; }

extern "C" size_t lr_cf_sim_ws_bytes(void) { return 256; }

extern "C" int lr_cf_sim_f32(const int64_t* x_ptr, const int32_t* x_col, const float* x_val, const int64_t* y_ptr,
                             const int32_t* y_col, const float* y_val, int64_t n_x, const float* norm,
                             const int32_t* cnt, int sim_type, int min_common, const int32_t* item_row,
                             const int32_t* item_tile, const int32_t* order, int64_t n_items, int pass,
                             int64_t* item_nnz, const int64_t* item_off, int32_t* out_col, float* out_val, void* ws,
                             size_t ws_bytes, lr_stream_t stream) {
  if (n_x < 0 || n_x > INT32_MAX || n_items < 0 || sim_type < 0 || sim_type > 2 || (pass != 0 && pass != 1))
    return LR_EINVAL;
  if (n_items == 0) return LR_OK;
  const bool jac = sim_type == 2;
  if (!x_ptr || !x_col || !y_ptr || !y_col || !item_row || !item_tile || !order) return LR_EINVAL;
  if ((!jac && (!x_val || !y_val || !norm)) || (jac && !cnt)) return LR_EINVAL;
  if ((pass == 0 && !item_nnz) || (pass == 1 && (!item_off || !out_col || !out_val))) return LR_EINVAL;
  if (ws == nullptr || ws_bytes < lr_cf_sim_ws_bytes()) return LR_EWORKSPACE;
  SimArgs a{x_ptr, x_col, x_val, y_ptr, y_col, y_val, n_x, norm, cnt, jac ? 1 : 0, min_common < 1 ? 1 : min_common,
            item_row, item_tile, order, n_items, item_nnz, item_off, out_col, out_val, nullptr, static_cast<int*>(ws)};
  return launch_sim<false>(a, pass, stream);
}

extern "C" int lr_cf_pair_state_f32(const int64_t* x_ptr, const int32_t* x_col, const float* x_val, const int64_t* y_ptr,
                                    const int32_t* y_col, const float* y_val, int64_t n_x, const int32_t* item_row,
                                    const int32_t* item_tile, const int32_t* order, int64_t n_items, int pass,
                                    int64_t* item_nnz, const int64_t* item_off, int32_t* out_col, float* out_prod,
                                    int32_t* out_cnt, void* ws, size_t ws_bytes, lr_stream_t stream) {
  if (n_x < 0 || n_x > INT32_MAX || n_items < 0 || (pass != 0 && pass != 1)) return LR_EINVAL;
  if (n_items == 0) return LR_OK;
  if (!x_ptr || !x_col || !x_val || !y_ptr || !y_col || !y_val || !item_row || !item_tile || !order) return LR_EINVAL;
  if ((pass == 0 && !item_nnz) || (pass == 1 && (!item_off || !out_col || !out_prod || !out_cnt))) return LR_EINVAL;
  if (ws == nullptr || ws_bytes < lr_cf_sim_ws_bytes()) return LR_EWORKSPACE;
  SimArgs a{x_ptr, x_col, x_val, y_ptr, y_col, y_val, n_x, nullptr, nullptr, 0, 1,
            item_row, item_tile, order, n_items, item_nnz, item_off, out_col, out_prod, out_cnt, static_cast<int*>(ws)};
  return launch_sim<true>(a, pass, stream);
}
