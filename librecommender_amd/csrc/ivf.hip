// Inverted-file (IVF-Flat) index over f32 rows, inner-product metric: deterministic k-means (assignment + per-list means), the
// list build, and the search (coarse top-nprobe over the centroids, then a scan of the probed lists with fused filter and top-k).
//
// Decomposition
//   assign    : ivf_assign_kernel.  A workgroup keeps 16 R rows in registers (16 lanes per row, each lane NCH 16-byte chunks; R rows
//               per lane group) and streams ALL centroids through LDS in tiles of 32 KB; per (row, centroid) the 16 partial
//               dot products are reduced with four DPP adds, and every lane of the group tracks the same (best score, lowest id).
//               This is the VALU form (f32 fma per lane): the f32 MFMA form of the same loop is future work (profiles/ivf.md).
//   lists     : stable radix sort of (list id, row id) pairs (rocPRIM, integer work only) gives list_ids ascending within a list;
//               list_ptr is a lower bound of every list id in the sorted keys.  The row permutation is lr_embed_gather_f32.
//   centroids : the entry stream (rows in list order) is cut into chunks of kIvfCH entries, one wave per chunk, so one huge list
//               spreads over the chip.  A list that lies inside one chunk is summed and divided there; a list that crosses chunk
//               borders leaves one partial sum per chunk and a second kernel adds them in chunk order (four interleaved slices,
//               combined in slice order).  No floating-point atomics: the order of every sum is fixed by the shapes alone.
//   search    : the driver, the plan, the wave's running top-k and the scan kernel are ivf_common.hpp's (ivf_search: coarse =
//               lr_score_topk_f32(queries, centroids, k = nprobe); plan; ivf_scan_kernel<Scorer>; merge).  This file supplies
//               (1) FlatScorer<NCH>, the scan's row scorer: the query sits in registers, list rows stream as float4 per lane (16
//               lanes per row, four rows per load, NCH chunks per lane), DPP reduce; (2) ivf_plan_kernel: every (query, probed
//               list) becomes ceil(len / CL) work items and the counts are scanned (one workgroup); (3) ivf_merge_kernel: one
//               workgroup per query streams its work items' keys through the scan's threshold / append / select scheme (one
//               list per wave, then wave 0 folds the four) and sorts the k winners (topk_keys.hpp).  Order (score desc, id asc)
//               is total, so the result does not depend on CL or on the grid.  The plan and merge kernels work on 64-bit keys
//               only and serve every list format through ivf_launch_plan / ivf_launch_merge.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "ivf_common.hpp"
#include "topk_keys.hpp"

namespace lr {

constexpr int kIvfCH = 1024;               // entries per chunk of the centroid sums
constexpr int kIvfTileBytes = 32 * 1024;   // centroid tile of the assignment in LDS

// ---- assignment ---------------------------------------------------------------------------------------------------------------
template <int NCH, int R>
__global__ __launch_bounds__(kBlock) void ivf_assign_kernel(const float* __restrict__ rows, int64_t n,
                                                            const float* __restrict__ cent, int nlist, int D, int TC,
                                                            int32_t* __restrict__ list_of, float* __restrict__ best_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* s_c = reinterpret_cast<float4*>(smem);      // [TC][NCH * 16] chunks, zero beyond D
  constexpr int W = NCH * 16;
  const int tid = threadIdx.x, j = tid & 15, grp = tid >> 4;
  const int D4 = D >> 2;
  constexpr int ROWS = 16 * R;
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * ROWS; t0 < n; t0 += static_cast<int64_t>(gridDim.x) * ROWS) {
    float4 x[R][NCH];
    float best[R];
    int bi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = t0 + grp * R + r;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ch = j + 16 * c;
        x[r][c] = (row < n && ch < D4) ? ld4(rows + row * D + ch * 4) : f4_zero();
      }
      best[r] = -INFINITY;
      bi[r] = 0;
    }
    for (int c0 = 0; c0 < nlist; c0 += TC) {
      const int tc = nlist - c0 < TC ? nlist - c0 : TC;
      __syncthreads();      // the previous tile has been read
      for (int q = tid; q < tc * W; q += kBlock) {
        const int cc = q / W, ch = q - cc * W;
        s_c[q] = ch < D4 ? ld4(cent + static_cast<int64_t>(c0 + cc) * D + ch * 4) : f4_zero();
      }
      __syncthreads();
      for (int cc = 0; cc < tc; ++cc) {
        float4 cv[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) cv[c] = s_c[cc * W + j + 16 * c];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float p = 0.f;
#pragma unroll
          for (int c = 0; c < NCH; ++c) p = dot4(x[r][c], cv[c], p);
          p = row16_sum(p);
          if (p > best[r]) {      // strict: ties stay with the lowest list id
            best[r] = p;
            bi[r] = c0 + cc;
          }
        }
      }
    }
    if (j == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int64_t row = t0 + grp * R + r;
        if (row < n) {
          list_of[row] = bi[r];
          if (best_out != nullptr) best_out[row] = best[r];
        }
      }
    }
  }
}

// ---- list build ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ivf_list_ptr_kernel(const int32_t* __restrict__ sorted, int64_t n, int nlist,
                                                              int64_t* __restrict__ list_ptr) {
  for (int l = blockIdx.x * kBlock + threadIdx.x; l <= nlist; l += gridDim.x * kBlock)
    list_ptr[l] = lower_bound_i32(sorted, 0, n, l);
}

// ---- centroid means -----------------------------------------------------------------------------------------------------------
// part[(c * 2 + 0) * D ..]: chunk c's sum of the list that began before the chunk; [(c * 2 + 1) * D ..]: of the list that begins
// inside it and runs on past its end.
__global__ __launch_bounds__(kBlock) void ivf_centroid_chunk_kernel(const float* __restrict__ rows, int D,
                                                                    const int64_t* __restrict__ list_ptr,
                                                                    const int32_t* __restrict__ list_ids, int64_t n, int nlist,
                                                                    int64_t n_rows, float* __restrict__ cent,
                                                                    float* __restrict__ part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int D4 = D >> 2;
  const int64_t nchunk = ceil_div(n, kIvfCH);
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (kBlock / kWave);
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x >> 6); c < nchunk; c += nwaves) {
    const int64_t p0 = c * kIvfCH, p1 = p0 + kIvfCH < n ? p0 + kIvfCH : n;
    int lo = 0, hi = nlist - 1;      // the list of entry p0: the first l with list_ptr[l + 1] > p0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (list_ptr[mid + 1] > p0) hi = mid; else lo = mid + 1;
    }
    int l = lo;
    int64_t p = p0;
    while (p < p1 && l < nlist) {
      const int64_t ls = list_ptr[l], le = list_ptr[l + 1];
      if (le <= p) {      // an empty list
        ++l;
        continue;
      }
      const int64_t e = le < p1 ? le : p1;
      float4 acc = f4_zero();
#pragma unroll 4
      for (int64_t q = p; q < e; ++q) {
        const int64_t id = list_ids[q];
        if (lane < D4 && id >= 0 && id < n_rows) acc = f4_add(acc, ld4(rows + id * D + lane * 4));
      }
      const bool before = ls < p0, after = le > p1;
      if (lane < D4) {
        if (!before && !after) {
          const float cnt = static_cast<float>(le - ls);
          st4(cent + static_cast<int64_t>(l) * D + lane * 4, make_float4(acc.x / cnt, acc.y / cnt, acc.z / cnt, acc.w / cnt));
        } else {
          st4(part + (c * 2 + (before ? 0 : 1)) * D + lane * 4, acc);
        }
      }
      p = e;
    }
  }
}

__global__ __launch_bounds__(kBlock) void ivf_centroid_fold_kernel(int D, const int64_t* __restrict__ list_ptr, int nlist,
                                                                   float* __restrict__ cent, const float* __restrict__ part) {
  __shared__ float4 s_red[4][kWave];
  const int col = threadIdx.x & (kWave - 1), slice = threadIdx.x >> 6;
  const int D4 = D >> 2;
  for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
    const int64_t ls = list_ptr[l], le = list_ptr[l + 1];
    if (le <= ls) continue;
    const int64_t c0 = ls / kIvfCH, c1 = (le - 1) / kIvfCH;
    if (c0 == c1) continue;      // summed and divided by the chunk kernel
    float4 acc = f4_zero();
    if (col < D4)
      for (int64_t i = slice; i <= c1 - c0; i += 4)
        acc = f4_add(acc, ld4(part + ((c0 + i) * 2 + (i == 0 ? 1 : 0)) * D + col * 4));
    s_red[slice][col] = acc;
    __syncthreads();
    if (slice == 0 && col < D4) {
      const float4 t = f4_add(f4_add(f4_add(s_red[0][col], s_red[1][col]), s_red[2][col]), s_red[3][col]);
      const float cnt = static_cast<float>(le - ls);
      st4(cent + static_cast<int64_t>(l) * D + col * 4, make_float4(t.x / cnt, t.y / cnt, t.z / cnt, t.w / cnt));
    }
    __syncthreads();
  }
}

// ---- search -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ivf_chunks_of(int64_t l, const int64_t* __restrict__ list_ptr, int nlist, int CL) {
  if (l < 0 || l >= nlist) return 0;
  return static_cast<int>((list_ptr[l + 1] - list_ptr[l] + CL - 1) / CL);
}

// pref[i] = work items before pair i, pref[P] = their total.  One workgroup: thread t takes a contiguous span of pairs.
__global__ __launch_bounds__(1024) void ivf_plan_kernel(const int64_t* __restrict__ coarse_ids, int64_t P,
                                                        const int64_t* __restrict__ list_ptr, int nlist, int CL,
                                                        int32_t* __restrict__ pref) {
  __shared__ int s_sum[1024];
  const int tid = threadIdx.x;
  const int64_t per = ceil_div(P, 1024);
  const int64_t a = tid * per < P ? tid * per : P, b = a + per < P ? a + per : P;
  int sum = 0;
  for (int64_t i = a; i < b; ++i) sum += ivf_chunks_of(coarse_ids[i], list_ptr, nlist, CL);
  s_sum[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? s_sum[tid - off] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  int base = s_sum[tid] - sum;
  for (int64_t i = a; i < b; ++i) {
    pref[i] = base;
    base += ivf_chunks_of(coarse_ids[i], list_ptr, nlist, CL);
  }
  if (tid == 1023) pref[P] = s_sum[1023];
}

// The f32 row scorer of the scan (ivf_common.hpp): 16 lanes per row, lane j holds the 16-byte chunks j + 16 c, c < NCH.
template <int NCH>
struct FlatScorer {
  static constexpr int RPW = 4;
  static constexpr int PUSHES = 4;      // at most 16 keys a trip: one look at the room per trip (profiles/ivf_search_refactor.md)
  const float* list_rows;
  int D;
  struct Query {
    float4 v[NCH];
  };
  __device__ __forceinline__ Query load_query(const float* __restrict__ queries, int64_t q, int j) const {
    Query qv;
#pragma unroll
    for (int c = 0; c < NCH; ++c) qv.v[c] = (j + 16 * c) < (D >> 2) ? ld4(queries + q * D + (j + 16 * c) * 4) : f4_zero();
    return qv;
  }
  __device__ __forceinline__ float score(const Query& qv, int64_t row, bool in_range, int j) const {
    float p = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ch = j + 16 * c;
      const float4 v = (in_range && ch < (D >> 2)) ? ld4(list_rows + row * D + ch * 4) : f4_zero();
      p = dot4(v, qv.v[c], p);
    }
    return row16_sum(p);
  }
};

__global__ __launch_bounds__(kBlock) void ivf_merge_kernel(const int32_t* __restrict__ pref, int nprobe,
                                                           const uint64_t* __restrict__ part_keys,
                                                           const int32_t* __restrict__ part_cnt, int k, int C, int K2, int64_t Wmax,
                                                           float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* s_keys = reinterpret_cast<uint64_t*>(smem);                       // [4][C]
  int* s_cnt = reinterpret_cast<int*>(s_keys + static_cast<size_t>(4) * C);   // [4]
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
  const int64_t u = blockIdx.x;
  const int64_t w0 = pref[u * nprobe], w1 = pref[(u + 1) * nprobe] < Wmax ? pref[(u + 1) * nprobe] : Wmax;
  WaveTopk tk;
  tk.L = s_keys + static_cast<size_t>(wid) * C;
  tk.k = k;
  tk.C = C;
  tk.lane = lane;
  tk.cnt = 0;
  tk.T = 0ull;
  for (int64_t w = w0 + wid; w < w1; w += 4) {
    const int n = part_cnt[w];
    for (int i0 = 0; i0 < n; i0 += kWave) {
      const int i = i0 + lane;
      const uint64_t key = i < n ? part_keys[w * k + i] : 0ull;
      tk.push(i < n && key > tk.T, key);
      if (tk.cnt + kWave > C) tk.shrink();
    }
  }
  if (tk.cnt > k) tk.shrink();
  if (lane == 0) s_cnt[wid] = tk.cnt;
  __syncthreads();
  if (wid == 0) {
    for (int o = 1; o < 4; ++o) {
      const int n = s_cnt[o];
      const uint64_t* src = s_keys + static_cast<size_t>(o) * C;
      for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        const uint64_t key = i < n ? src[i] : 0ull;
        tk.push(i < n && key > tk.T, key);
        if (tk.cnt + kWave > C) tk.shrink();
      }
    }
    if (tk.cnt > k) tk.shrink();
    for (int i = tk.cnt + lane; i < K2; i += kWave) tk.L[i] = 0ull;
  }
  __syncthreads();
  block_sort_keys_desc(s_keys, K2, tid, kBlock);
  emit_topk(s_keys, K2, k, u, 0, out_scores, out_ids, tid, kBlock);
}

void ivf_launch_plan(const IvfPlan& p, const int64_t* coarse_ids, const int64_t* list_ptr, int nlist, int32_t* pref, hipStream_t s) {
  hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(1024), 0, s, coarse_ids, p.P, list_ptr, nlist, p.CL, pref);
}

void ivf_launch_merge(const IvfPlan& p, int64_t B, int nprobe, int k, const int32_t* pref, const uint64_t* part_keys,
                      const int32_t* part_cnt, float* out_scores, int64_t* out_ids, hipStream_t s) {
  hipLaunchKernelGGL(ivf_merge_kernel, dim3(static_cast<unsigned>(B)), dim3(kBlock), ivf_scan_lds(p) + 64, s, pref, nprobe, part_keys,
                     part_cnt, k, p.C, p.K2, p.Wmax, out_scores, out_ids);
}

static inline bool ivf_row_shape_ok(int D) { return D >= 4 && D <= 256 && (D % 4) == 0; }
static inline int ivf_key_bits(int nlist) {
  int bits = 1;
  while (bits < 31 && (int64_t(1) << bits) < nlist) ++bits;
  return bits;
}
static inline size_t ivf_sort_scratch(int64_t n) { return ivf_al(static_cast<size_t>(n) * 8) * 2 + (size_t(8) << 20); }

}  // namespace lr

using namespace lr;

extern "C" int lr_ivf_supported(int64_t B, int64_t N, int D, int k, int nprobe, int nlist) {
  return ivf_plan(B, N, D, k, nprobe, nlist).ok ? 1 : 0;
}

extern "C" size_t lr_ivf_search_ws_bytes(int64_t B, int64_t N, int D, int k, int nprobe, int nlist) {
  const IvfPlan p = ivf_plan(B, N, D, k, nprobe, nlist);
  return p.ok ? p.total : 0;
}

extern "C" int lr_ivf_assign_f32(const float* rows, int64_t n, const float* centroids, int nlist, int D, int32_t* list_of,
                                 float* best_score, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && nlist >= 1);
  if (!ivf_row_shape_ok(D) || nlist > 65536 || n >= (int64_t(1) << 31)) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(rows && centroids && list_of);
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(rows) % 16 == 0 && reinterpret_cast<uintptr_t>(centroids) % 16 == 0);
  hipStream_t s = as_stream(stream);
  const int nch = D <= 64 ? 1 : D <= 128 ? 2 : 4;
  const int TC = kIvfTileBytes / (nch * 256);
  const int rows_per_block = nch == 4 ? 64 : 128;
  const dim3 grid(grid_for(n, rows_per_block)), block(kBlock);
  if (nch == 1)
    hipLaunchKernelGGL((ivf_assign_kernel<1, 8>), grid, block, kIvfTileBytes, s, rows, n, centroids, nlist, D, TC, list_of, best_score);
  else if (nch == 2)
    hipLaunchKernelGGL((ivf_assign_kernel<2, 8>), grid, block, kIvfTileBytes, s, rows, n, centroids, nlist, D, TC, list_of, best_score);
  else
    hipLaunchKernelGGL((ivf_assign_kernel<4, 4>), grid, block, kIvfTileBytes, s, rows, n, centroids, nlist, D, TC, list_of, best_score);
  return launch_status();
}

extern "C" size_t lr_ivf_build_ws_bytes(int64_t n, int nlist) {
  (void)nlist;
  if (n < 0) n = 0;
  return ivf_al(static_cast<size_t>(n) * 4) + ivf_sort_scratch(n);
}

extern "C" int lr_ivf_build_lists(const int32_t* list_of, int64_t n, int nlist, int64_t* list_ptr, int32_t* list_ids, void* ws,
                                  size_t ws_bytes, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && nlist >= 1 && list_ptr);
  if (nlist > 65536 || n >= (int64_t(1) << 31)) return LR_ESHAPE;
  hipStream_t s = as_stream(stream);
  if (n > 0) {
    LR_CHECK_ARG(list_of && list_ids && ws && reinterpret_cast<uintptr_t>(ws) % 256 == 0);
    if (ws_bytes < lr_ivf_build_ws_bytes(n, nlist)) return LR_EWORKSPACE;
    int32_t* sorted = static_cast<int32_t*>(ws);
    char* prim = static_cast<char*>(ws) + ivf_al(static_cast<size_t>(n) * 4);
    const size_t prim_bytes = ws_bytes - ivf_al(static_cast<size_t>(n) * 4);
    rocprim::counting_iterator<int32_t> iota(0);
    const unsigned bits = static_cast<unsigned>(ivf_key_bits(nlist));
    size_t need = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, need, list_of, sorted, iota, list_ids, static_cast<size_t>(n), 0u, bits, s);
    if (e != hipSuccess) return static_cast<int>(e);
    if (need > prim_bytes) return LR_EWORKSPACE;
    e = rocprim::radix_sort_pairs(prim, need, list_of, sorted, iota, list_ids, static_cast<size_t>(n), 0u, bits, s);
    if (e != hipSuccess) return static_cast<int>(e);
    hipLaunchKernelGGL(ivf_list_ptr_kernel, dim3(grid_for(nlist + 1, kBlock)), dim3(kBlock), 0, s, sorted, n, nlist, list_ptr);
  } else {
    hipLaunchKernelGGL(ivf_list_ptr_kernel, dim3(grid_for(nlist + 1, kBlock)), dim3(kBlock), 0, s,
                       static_cast<const int32_t*>(nullptr), int64_t(0), nlist, list_ptr);
  }
  return launch_status();
}

extern "C" size_t lr_ivf_centroids_ws_bytes(int64_t n, int D) {
  if (n < 0 || D < 1) return 0;
  return ivf_al(static_cast<size_t>(ceil_div(n, kIvfCH)) * 2 * D * sizeof(float)) + 256;
}

extern "C" int lr_ivf_centroids_f32(const float* rows, int64_t n_rows, int D, const int64_t* list_ptr, const int32_t* list_ids,
                                    int64_t n, int nlist, float* centroids, void* ws, size_t ws_bytes, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && n_rows >= 0 && nlist >= 1);
  if (!ivf_row_shape_ok(D) || nlist > 65536 || n >= (int64_t(1) << 31)) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(rows && list_ptr && list_ids && centroids && ws);
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(rows) % 16 == 0 && reinterpret_cast<uintptr_t>(centroids) % 16 == 0 &&
               reinterpret_cast<uintptr_t>(ws) % 16 == 0);
  if (ws_bytes < lr_ivf_centroids_ws_bytes(n, D)) return LR_EWORKSPACE;
  hipStream_t s = as_stream(stream);
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(ivf_centroid_chunk_kernel, dim3(grid_for(ceil_div(n, kIvfCH), kBlock / kWave)), dim3(kBlock), 0, s, rows, D,
                     list_ptr, list_ids, n, nlist, n_rows, centroids, part);
  hipLaunchKernelGGL(ivf_centroid_fold_kernel, dim3(grid_for(nlist, 1)), dim3(kBlock), 0, s, D, list_ptr, nlist, centroids, part);
  return launch_status();
}

extern "C" int lr_ivf_search_f32(const float* queries, int64_t B, const float* centroids, int nlist, const int64_t* list_ptr,
                                 const int32_t* list_ids, const float* list_rows, int64_t N, int D,
                                 const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag, int k,
                                 int nprobe, float* out_scores, int64_t* out_ids, void* ws, size_t ws_bytes,
                                 lr_stream_t stream) {
  return ivf_search(queries, B, centroids, nlist, list_ptr, list_ids, N, D, consumed_ptr, consumed_idx, filter_flag, k, nprobe,
                    out_scores, out_ids, ws, ws_bytes, stream, true, ivf_rows_ptr_ok(list_rows), [&](auto launch) {
                      if (D <= 64) launch(FlatScorer<1>{list_rows, D});
                      else if (D <= 128) launch(FlatScorer<2>{list_rows, D});
                      else launch(FlatScorer<4>{list_rows, D});
                    });
}
