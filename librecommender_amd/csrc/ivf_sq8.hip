// Inverted-file index with scalar-quantised lists (IVF-SQ8), inner-product metric: the list-ordered copy of the catalogue is int8
// codes with one f32 scale per row instead of f32 rows, and a short candidate list is re-scored exactly from the f32 catalogue
// the caller holds anyway.  Training and the lists are ivf.hip's; this file holds the encoder, the scan and the re-rank.
//
// Decomposition
//   encode : ivf_sq8_encode_kernel.  16 lanes per row, lane j holds columns [16 j, 16 j + 16) in registers (the row is read once,
//            gathered through list_ids): a = max |x| over the 16 lanes, scale = a / 127, code = clamp(rint(x / scale), -127, 127),
//            division and rounding by intrinsics so that nothing contracts.  A lane writes its 16 codes with one 16-byte store;
//            columns from D up to the stored stride are code 0.  a == 0 gives scale 0 and codes 0.
//   search : the whole search but the scoring of a row is ivf_common.hpp's (ivf_search, ivf_scan_kernel<Scorer>).  Sq8Scorer<LPR>
//            scores code rows: a row is `stride` bytes (D rounded up to 16), LPR = next_pow2(stride / 16) lanes share a row and
//            each loads 16 codes with one 16-byte load, so a wave-load covers 64 / LPR rows; the f32 query slice of the lane sits in
//            registers; dot = 16 fmas in column order, then log2(LPR) DPP pair sums; score = scale * dot, one rounded multiply.
//   rerank : ivf_rerank_kernel.  One workgroup per query: every 16-lane group gathers a candidate's f32 row by global id and
//            takes the f32 inner product (fma chains, DPP sum), ids of -1 are skipped; the keys are sorted in LDS and the k best
//            written, -1 / -inf beyond them (topk_keys.hpp).
// No floating-point atomics: two calls give the same bits.
#include "common.hpp"
#include "ivf_common.hpp"
#include "topk_keys.hpp"

namespace lr {

constexpr int kSq8MaxRefine = 64;

// ---- encode -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sq8_code(float x, float scale) {
  if (!(scale > 0.f)) return 0;
  const float r = rintf(__fdiv_rn(x, scale));      // half to even
  return static_cast<int>(fminf(fmaxf(r, -127.f), 127.f));
}
__device__ __forceinline__ uint32_t sq8_pack(float4 x, float scale) {
  return (static_cast<uint32_t>(sq8_code(x.x, scale)) & 0xffu) | ((static_cast<uint32_t>(sq8_code(x.y, scale)) & 0xffu) << 8) |
         ((static_cast<uint32_t>(sq8_code(x.z, scale)) & 0xffu) << 16) | (static_cast<uint32_t>(sq8_code(x.w, scale)) << 24);
}

__global__ __launch_bounds__(kBlock) void ivf_sq8_encode_kernel(const float* __restrict__ rows, int64_t n_rows, int D,
                                                                const int32_t* __restrict__ list_ids, int64_t n,
                                                                int8_t* __restrict__ codes, int stride,
                                                                float* __restrict__ scales) {
  const int j = threadIdx.x & 15, grp = threadIdx.x >> 4;
  for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * 16; r0 < n; r0 += static_cast<int64_t>(gridDim.x) * 16) {
    const int64_t r = r0 + grp;
    const int64_t src = r < n ? (list_ids != nullptr ? static_cast<int64_t>(list_ids[r]) : r) : -1;
    const bool live = src >= 0 && src < n_rows;      // an id outside the catalogue encodes as a zero row
    float4 x[4];
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int col = 16 * j + 4 * c;
      x[c] = (live && col < D) ? ld4(rows + src * D + col) : f4_zero();
      a = fmaxf(fmaxf(a, fmaxf(fabsf(x[c].x), fabsf(x[c].y))), fmaxf(fabsf(x[c].z), fabsf(x[c].w)));
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) a = fmaxf(a, __shfl_xor(a, m, 16));
    const float scale = __fdiv_rn(a, 127.f);
    if (r < n && 16 * j < stride) {
      const uint4 w = make_uint4(sq8_pack(x[0], scale), sq8_pack(x[1], scale), sq8_pack(x[2], scale), sq8_pack(x[3], scale));
      *reinterpret_cast<uint4*>(codes + r * stride + 16 * j) = w;
    }
    if (r < n && j == 0) scales[r] = scale;
  }
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------
// sum over the LPR lanes that share a row: the first log2(LPR) steps of row16_sum
template <int LPR>
__device__ __forceinline__ float sq8_lanes_sum(float v) {
  if (LPR >= 2) v = ivf_dpp_add<0xB1>(v);     // quad_perm [1,0,3,2]
  if (LPR >= 4) v = ivf_dpp_add<0x4E>(v);     // quad_perm [2,3,0,1]
  if (LPR >= 8) v = ivf_dpp_add<0x141>(v);    // row_half_mirror
  if (LPR >= 16) v = ivf_dpp_add<0x140>(v);   // row_mirror
  return v;
}
// p + sum of four codes (the bytes of w, lowest first) times q
__device__ __forceinline__ float sq8_dot4(uint32_t w, float4 q, float p) {
  p = fmaf(static_cast<float>(static_cast<int32_t>(w << 24) >> 24), q.x, p);
  p = fmaf(static_cast<float>(static_cast<int32_t>(w << 16) >> 24), q.y, p);
  p = fmaf(static_cast<float>(static_cast<int32_t>(w << 8) >> 24), q.z, p);
  return fmaf(static_cast<float>(static_cast<int32_t>(w) >> 24), q.w, p);
}

// The code row scorer of the scan (ivf_common.hpp): LPR lanes per row, lane j holds columns [16 j, 16 j + 16) as one 16-byte load.
template <int LPR>
struct Sq8Scorer {
  static constexpr int RPW = kWave / LPR;
  static constexpr int PUSHES = 1;      // up to 64 keys per wave-load
  const int8_t* codes;
  int stride;
  const float* scales;
  int D;
  struct Query {
    float4 v[4];
  };
  __device__ __forceinline__ Query load_query(const float* __restrict__ queries, int64_t q, int j) const {
    Query qv;
#pragma unroll
    for (int c = 0; c < 4; ++c) qv.v[c] = (16 * j + 4 * c) < D ? ld4(queries + q * D + 16 * j + 4 * c) : f4_zero();
    return qv;
  }
  __device__ __forceinline__ float score(const Query& qv, int64_t row, bool in_range, int j) const {
    const bool mine = 16 * j < stride;      // LPR is a power of two: the lanes past the row's last chunk load nothing
    const uint4 v = (in_range && mine) ? *reinterpret_cast<const uint4*>(codes + row * stride + 16 * j) : make_uint4(0u, 0u, 0u, 0u);
    const float scale = (in_range && j == 0) ? scales[row] : 0.f;
    float p = sq8_dot4(v.x, qv.v[0], 0.f);
    p = sq8_dot4(v.y, qv.v[1], p);
    p = sq8_dot4(v.z, qv.v[2], p);
    p = sq8_dot4(v.w, qv.v[3], p);
    return __fmul_rn(scale, sq8_lanes_sum<LPR>(p));
  }
};

// ---- re-rank ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ivf_rerank_kernel(const float* __restrict__ queries, const float* __restrict__ rows,
                                                            int64_t N, int D, const int64_t* __restrict__ cand_ids, int kk, int k,
                                                            int K2, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  __shared__ uint64_t a[1024];
  const int tid = threadIdx.x, j = tid & 15, grp = tid >> 4;
  const int D4 = D >> 2;
  const int64_t u = blockIdx.x;
  float4 qv[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) qv[c] = (j + 16 * c) < D4 ? ld4(queries + u * D + (j + 16 * c) * 4) : f4_zero();
  for (int c0 = 0; c0 < K2; c0 += 16) {      // K2 is a multiple of 16 or below it: every lane of a group takes the same trips
    const int ci = c0 + grp;
    const int64_t id = ci < kk ? cand_ids[u * kk + ci] : -1;
    const bool live = id >= 0 && id < N;
    float p = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ch = j + 16 * c;
      const float4 v = (live && ch < D4) ? ld4(rows + id * D + ch * 4) : f4_zero();
      p = dot4(v, qv[c], p);
    }
    p = row16_sum(p);
    if (j == 0 && ci < K2) a[ci] = (live && p == p) ? make_key(p, static_cast<uint32_t>(id)) : 0ull;
  }
  __syncthreads();
  block_sort_keys_desc(a, K2, tid, kBlock);
  emit_topk(a, K2, k, u, 0, out_scores, out_ids, tid, kBlock);
}

static inline bool sq8_stride_ok(int D, int stride) { return stride >= D && stride <= 256 && (stride % 16) == 0; }

}  // namespace lr

using namespace lr;

extern "C" int lr_ivf_sq8_supported(int64_t B, int64_t N, int D, int k, int nprobe, int nlist, int refine) {
  if (refine < 0 || refine > kSq8MaxRefine || k < 1 || k > 1024) return 0;
  const int64_t kk = refine == 0 ? k : (static_cast<int64_t>(k) * refine < 1024 ? static_cast<int64_t>(k) * refine : 1024);
  return ivf_plan(B, N, D, static_cast<int>(kk), nprobe, nlist).ok ? 1 : 0;
}

extern "C" size_t lr_ivf_sq8_search_ws_bytes(int64_t B, int64_t N, int D, int kk, int nprobe, int nlist) {
  const IvfPlan p = ivf_plan(B, N, D, kk, nprobe, nlist);
  return p.ok ? p.total : 0;
}

extern "C" int lr_ivf_sq8_encode_f32(const float* rows, int64_t n_rows, int D, const int32_t* list_ids, int64_t n, int8_t* codes,
                                     int code_stride, float* scales, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && n_rows >= 0);
  if (D < 4 || D > 256 || (D % 4) != 0 || !sq8_stride_ok(D, code_stride) || n >= (int64_t(1) << 31) || n_rows >= (int64_t(1) << 31))
    return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(rows && codes && scales);
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(rows) % 16 == 0 && reinterpret_cast<uintptr_t>(codes) % 16 == 0);
  hipLaunchKernelGGL(ivf_sq8_encode_kernel, dim3(grid_for(n, 16)), dim3(kBlock), 0, as_stream(stream), rows, n_rows, D, list_ids, n,
                     codes, code_stride, scales);
  return launch_status();
}

extern "C" int lr_ivf_sq8_search_f32(const float* queries, int64_t B, const float* centroids, int nlist, const int64_t* list_ptr,
                                     const int32_t* list_ids, const int8_t* codes, int code_stride, const float* scales, int64_t N,
                                     int D, const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag,
                                     int kk, int nprobe, float* out_scores, int64_t* out_ids, void* ws, size_t ws_bytes,
                                     lr_stream_t stream) {
  const int chunks = code_stride / 16;
  return ivf_search(queries, B, centroids, nlist, list_ptr, list_ids, N, D, consumed_ptr, consumed_idx, filter_flag, kk, nprobe,
                    out_scores, out_ids, ws, ws_bytes, stream, sq8_stride_ok(D, code_stride), ivf_rows_ptr_ok(codes) && scales,
                    [&](auto launch) {
                      if (chunks == 1) launch(Sq8Scorer<1>{codes, code_stride, scales, D});
                      else if (chunks == 2) launch(Sq8Scorer<2>{codes, code_stride, scales, D});
                      else if (chunks <= 4) launch(Sq8Scorer<4>{codes, code_stride, scales, D});
                      else if (chunks <= 8) launch(Sq8Scorer<8>{codes, code_stride, scales, D});
                      else launch(Sq8Scorer<16>{codes, code_stride, scales, D});
                    });
}

extern "C" int lr_ivf_rerank_f32(const float* queries, int64_t B, const float* rows, int64_t N, int D, const int64_t* cand_ids,
                                 int kk, int k, float* out_scores, int64_t* out_ids, lr_stream_t stream) {
  LR_CHECK_ARG(B >= 0);
  if (B == 0) return LR_OK;
  if (N < 1 || N >= (int64_t(1) << 31) || D < 4 || D > 256 || (D % 4) != 0 || kk < 1 || kk > 1024 || k < 1 || k > 1024 ||
      B >= (int64_t(1) << 31))
    return LR_ESHAPE;
  LR_CHECK_ARG(queries && rows && cand_ids && out_scores && out_ids);
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(queries) % 16 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0);
  hipLaunchKernelGGL(ivf_rerank_kernel, dim3(static_cast<unsigned>(B)), dim3(kBlock), 0, as_stream(stream), queries, rows, N, D,
                     cand_ids, kk, k, ivf_pow2(kk), out_scores, out_ids);
  return launch_status();
}
