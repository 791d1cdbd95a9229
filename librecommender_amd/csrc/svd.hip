// SVD and SVD++ (`libreco/algorithms/svd.py:103-144`, `libreco/algorithms/svdpp.py:102-135,196-214`): the ragged
// history pool z_u = p_u + |N(u)|^-1/2 sum_{j in N(u)} y_j, the score s = bu[u] + bi[i] + <x_u, q_i> with its loss and
// dL/ds, and the update of the y rows from the per-user gradient sums.
//   svdpp_pool_kernel      one sub-wave group per listed user walks that user's history; the gathers of kAhead rows are
//                          issued before the first add, so the latency of divergent rows overlaps (the kChainBlock idea of
//                          bpr.hip).  A history of any length is one loop: no launch per length class.
//   mf_score_kernel        one group per sample gathers the user-side row (a table row, or the sample's slot of the pooled
//                          block) and q_i, reduces the dot inside the group, and writes score, loss, g = dL/ds and, in the
//                          gradient mode, the rows g q and g x.
//   svdpp_hist_*_kernel    the y side.  An entry of the concatenated histories of the batch's distinct users is (y row,
//                          user slot); lr_segments_build groups the entries by y row.  One group per touched row adds
//                          |N(u_e)|^-1/2 G[slot_e, :] over its run in run order, reading the gradient THROUGH the slot: no
//                          [entries, K] buffer exists.  Runs longer than kSvdLongRun are cut into chunks of kSvdChunk
//                          entries summed by separate groups; a run's partials are then added in chunk order.  The sum is
//                          either applied (TF1 Adam on the touched rows) or written out per run.
// Rows are 1 - 512 floats and the tables are cache resident, so a group is sized to the row.  No float atomics: two
// runs give the same bits.  Ids outside a table are dropped, never dereferenced.
#include <math.h>

#include "row_group.hpp"

namespace lr {

constexpr int kSvdMaxK = 512;
constexpr int kAhead = 8;          // rows whose gathers are in flight before the first add
constexpr int kSvdLongRun = 64;    // runs longer than this are summed chunk by chunk
constexpr int kSvdChunk = 64;

// ---- history pool ------------------------------------------------------------------------
template <int G, int R>
__global__ __launch_bounds__(kBlock) void svdpp_pool_kernel(
    const float* __restrict__ P, const float* __restrict__ Y, int64_t nU, int64_t nY, int K,
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_idx, int64_t nnz,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ n_rows_dev, int64_t n_rows, float* __restrict__ out,
    float* __restrict__ scale_out) {
  const int lane = threadIdx.x % G;
  int64_t nr = n_rows;
  if (n_rows_dev != nullptr) {
    const int64_t d = *n_rows_dev;
    nr = d < 0 ? 0 : (d < nr ? d : nr);
  }
  const int64_t stride = group_stride<G>();
  for (int64_t r = group_index<G>(); r < nr; r += stride) {
    const int64_t u = rows != nullptr ? static_cast<int64_t>(rows[r]) : r;
    const bool ok = u >= 0 && u < nU;
    int64_t b = 0, e = 0;
    if (ok) {
      b = hist_ptr[u];
      e = hist_ptr[u + 1];
    }
    if (b < 0) b = 0;
    if (e > nnz) e = nnz;
    if (e < b) e = b;
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.f;
    for (int64_t i0 = b; i0 < e; i0 += kAhead) {
      int32_t id[kAhead];
#pragma unroll
      for (int t = 0; t < kAhead; ++t) id[t] = hist_idx[i0 + t < e ? i0 + t : e - 1];
      float y[kAhead][R];
#pragma unroll
      for (int t = 0; t < kAhead; ++t) {
        const bool v = i0 + t < e && id[t] >= 0 && id[t] < nY;
        const int64_t base = (v ? static_cast<int64_t>(id[t]) : 0) * K;      // always a valid address
#pragma unroll
        for (int q = 0; q < R; ++q) {
          const float x = Y[base + min(lane + q * G, K - 1)];
          y[t][q] = v ? x : 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < kAhead; ++t)                      // history order
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] += y[t][q];
    }
    const int64_t n = e - b;
    const float sc = n > 0 ? 1.f / sqrtf(static_cast<float>(n)) : 0.f;
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int j = lane + q * G;
      if (j < K) {
        const float p = (P != nullptr && ok) ? P[u * K + j] : 0.f;
        out[r * K + j] = n > 0 ? p + sc * acc[q] : p;       // an empty history returns p's bits
      }
    }
    if (lane == 0 && scale_out != nullptr) scale_out[r] = sc;
  }
}

// ---- score, loss and dL/ds ---------------------------------------------------------------
template <int G, int R>
__global__ __launch_bounds__(kBlock) void mf_score_kernel(
    const float* __restrict__ X, int64_t nX, const int32_t* __restrict__ xidx, const float* __restrict__ Q, int64_t nI,
    const float* __restrict__ bu, int64_t nU, const float* __restrict__ bi, int K, const int32_t* __restrict__ users,
    const int32_t* __restrict__ items, const float* __restrict__ labels, int64_t B, int loss_kind, int mode, float gscale,
    float* __restrict__ score, float* __restrict__ loss_out, float* __restrict__ g_out, float* __restrict__ gx,
    float* __restrict__ gq) {
  const int lane = threadIdx.x % G;
  const int64_t s = group_index<G>();
  const bool in = s < B;
  int32_t u = -1, i = -1;
  int64_t xr = -1;
  float y = 0.f;
  if (in) {
    u = users[s];
    i = items[s];
    xr = xidx != nullptr ? static_cast<int64_t>(xidx[s]) : static_cast<int64_t>(u);
    y = labels[s];
  }
  const bool ok = in && u >= 0 && u < nU && i >= 0 && i < nI && xr >= 0 && xr < nX;
  float xx[R], qq[R];
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + r * G;
    xx[r] = 0.f;
    qq[r] = 0.f;
    if (ok && j < K) {
      xx[r] = X[xr * K + j];
      qq[r] = Q[static_cast<int64_t>(i) * K + j];
    }
    acc = fmaf(xx[r], qq[r], acc);
  }
  float sc = group_sum<G>(acc);       // every lane of the wave takes part: no early exit above
  if (ok) sc += (bu != nullptr ? bu[u] : 0.f) + (bi != nullptr ? bi[i] : 0.f);
  float loss, gs;
  if (loss_kind == LR_MF_MSE) {                            // tfops/loss.py:5-8
    const float d = sc - y;
    loss = d * d;
    gs = 2.f * d;
  } else {
    // e in (0, 1]: p = sigmoid(s) and 1 - p without cancellation, bce = max(s, 0) - s y + log1p(exp(-|s|)) finite
    const float e = expf(-fabsf(sc));
    const float inv = 1.f / (1.f + e);
    const float p = sc >= 0.f ? inv : e * inv;
    const float q1 = sc >= 0.f ? e * inv : inv;
    const float bce = fmaxf(sc, 0.f) - sc * y + log1pf(e);
    const float pmy = (1.f - y) * p - y * q1;              // p - y
    if (loss_kind == LR_MF_CROSS_ENTROPY) {                // tfops/loss.py:10-17
      loss = bce;
      gs = pmy;
    } else {                                               // focal, tfops/loss.py:56-62 (alpha 0.25, gamma 2)
      const float w = y * 0.25f + (1.f - y) * 0.75f;
      const float a = y * q1 + (1.f - y) * p;              // 1 - p_t
      const float da = -(2.f * y - 1.f) * (p * q1);
      loss = w * a * a * bce;
      gs = w * (2.f * a * da * bce + a * a * pmy);
    }
  }
  float g = gs * gscale;
  if (!ok) {                              // a sample with an id outside its table takes no part in any update
    sc = 0.f;
    loss = 0.f;
    g = 0.f;
  }
  if (!in) return;
  if (lane == 0) {
    score[s] = sc;
    loss_out[s] = loss;
    g_out[s] = g;
  }
  if (mode == LR_MF_GRAD) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      if (j < K) {
        gx[s * K + j] = g * qq[r];
        gq[s * K + j] = g * xx[r];
      }
    }
  }
}

// ---- the y side --------------------------------------------------------------------------
// Workspace of the long runs (lr_svdpp_hist_grad_ws_bytes):
//   int32 long_count | int32 chunk_count | pad to 256 B | long_seg[NL] | long_base[NL] | chunk_slot[NC] | partial[NC][K]
struct SvdLongWs {
  int32_t* counts;
  int32_t* long_seg;
  int32_t* long_base;
  int32_t* chunk_slot;
  float* partial;
  int n_long_max, n_chunk_max;
};

struct SvdHist {
  const float* Gm;            // [n_slots, K] per-user gradient sums
  const float* scale;         // [n_slots] |N(u)|^-1/2
  int64_t n_slots;
  const int32_t* ent_slot;    // [n] user slot of every entry
  const int32_t* seg_pos;
  const int32_t* seg_rows;
  const int32_t* seg_start;
  const int32_t* n_seg;
  int64_t n;
  int K;
};

// acc += sum over seg_pos[p0 .. p1) of scale[slot] * G[slot, :], in that order.  p0 < p1.  Three stages of loads
// (position -> slot -> scale and row), each at clamped, always valid addresses, kAhead entries at a time.
template <int G, int R>
__device__ __forceinline__ void hist_accum(const SvdHist& h, int p0, int p1, int lane, float (&acc)[R]) {
  for (int i0 = p0; i0 < p1; i0 += kAhead) {
    int32_t pp[kAhead], sl[kAhead];
#pragma unroll
    for (int t = 0; t < kAhead; ++t) pp[t] = h.seg_pos[min(i0 + t, p1 - 1)];
#pragma unroll
    for (int t = 0; t < kAhead; ++t) {
      const bool v = i0 + t < p1 && pp[t] >= 0 && pp[t] < h.n;
      const int32_t s = h.ent_slot[v ? pp[t] : 0];
      sl[t] = v ? s : -1;
    }
    float sc[kAhead], gv[kAhead][R];
#pragma unroll
    for (int t = 0; t < kAhead; ++t) {
      const bool v = sl[t] >= 0 && sl[t] < h.n_slots;
      const int64_t s = v ? sl[t] : 0;
      const float c = h.scale[s];
      sc[t] = v ? c : 0.f;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const float x = h.Gm[s * h.K + min(lane + q * G, h.K - 1)];
        gv[t][q] = v ? x : 0.f;
      }
    }
#pragma unroll
    for (int t = 0; t < kAhead; ++t)
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q] = fmaf(sc[t], gv[t][q], acc[q]);
  }
}

template <int MODE, int G, int R>
__device__ __forceinline__ void hist_apply(float* __restrict__ Y, float* __restrict__ m, float* __restrict__ v, int64_t nY,
                                           int K, int64_t run, int64_t row, int lane, const float (&acc)[R],
                                           float* __restrict__ grows, const AdamCoef& coef) {
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int j = lane + q * G;
    if (j >= K) continue;
    if (MODE == LR_SVD_HIST_ROWS) {
      grows[run * K + j] = acc[q];
    } else if (row >= 0 && row < nY) {
      const int64_t off = row * K + j;
      float mm = m[off], vv = v[off];
      Y[off] = adam_elem(Y[off], acc[q], mm, vv, coef);
      m[off] = mm;
      v[off] = vv;
    }
  }
}

__global__ __launch_bounds__(kBlock) void svdpp_hist_classify_kernel(const int32_t* __restrict__ seg_start,
                                                                     const int32_t* __restrict__ n_seg_ptr, int64_t n,
                                                                     SvdLongWs w) {
  int64_t n_seg = *n_seg_ptr;
  if (n_seg > n) n_seg = n;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; s < n_seg; s += stride) {
    const int len = seg_start[s + 1] - seg_start[s];
    if (len <= kSvdLongRun) continue;
    const int nch = (len + kSvdChunk - 1) / kSvdChunk;
    const int slot = atomicAdd(&w.counts[0], 1);            // integer bookkeeping only: which slot a run gets does not
    const int base = atomicAdd(&w.counts[1], nch);          // enter any sum
    if (slot >= w.n_long_max || base + nch > w.n_chunk_max) continue;
    w.long_seg[slot] = static_cast<int32_t>(s);
    w.long_base[slot] = base;
    for (int j = 0; j < nch; ++j) w.chunk_slot[base + j] = slot;
  }
}

template <int MODE, int G, int R>
__global__ __launch_bounds__(kBlock) void svdpp_hist_kernel(float* __restrict__ Y, float* __restrict__ m,
                                                            float* __restrict__ v, int64_t nY, SvdHist h,
                                                            float* __restrict__ grows, AdamCoef coef, int skip_long) {
  const int lane = threadIdx.x % G;
  int64_t n_seg = *h.n_seg;
  if (n_seg > h.n) n_seg = h.n;
  const int64_t stride = group_stride<G>();
  for (int64_t run = group_index<G>(); run < n_seg; run += stride) {
    int p0 = h.seg_start[run], p1 = h.seg_start[run + 1];
    if (p0 < 0) p0 = 0;
    if (p1 > h.n) p1 = static_cast<int>(h.n);
    if (skip_long && p1 - p0 > kSvdLongRun) continue;       // summed chunk by chunk below
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.f;
    if (p0 < p1) hist_accum<G, R>(h, p0, p1, lane, acc);
    hist_apply<MODE, G, R>(Y, m, v, nY, h.K, run, h.seg_rows[run], lane, acc, grows, coef);
  }
}

template <int G, int R>
__global__ __launch_bounds__(kBlock) void svdpp_hist_chunk_kernel(SvdHist h, SvdLongWs w) {
  const int lane = threadIdx.x % G;
  int n_chunks = w.counts[1];
  if (n_chunks > w.n_chunk_max) n_chunks = w.n_chunk_max;
  const int64_t stride = group_stride<G>();
  for (int64_t c = group_index<G>(); c < n_chunks; c += stride) {
    const int slot = w.chunk_slot[c];
    if (slot < 0 || slot >= w.n_long_max) continue;
    const int s = w.long_seg[slot];
    if (s < 0 || s >= h.n) continue;
    const int j = static_cast<int>(c) - w.long_base[slot];
    int pe = h.seg_start[s + 1];
    if (pe > h.n) pe = static_cast<int>(h.n);
    const int p0 = h.seg_start[s] + j * kSvdChunk;
    const int p1 = p0 + kSvdChunk < pe ? p0 + kSvdChunk : pe;
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.f;
    if (p0 >= 0 && p0 < p1) hist_accum<G, R>(h, p0, p1, lane, acc);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const int col = lane + q * G;
      if (col < h.K) w.partial[c * h.K + col] = acc[q];
    }
  }
}

template <int MODE, int G, int R>
__global__ __launch_bounds__(kBlock) void svdpp_hist_finish_kernel(float* __restrict__ Y, float* __restrict__ m,
                                                                   float* __restrict__ v, int64_t nY, SvdHist h,
                                                                   float* __restrict__ grows, AdamCoef coef, SvdLongWs w) {
  const int lane = threadIdx.x % G;
  int n_long = w.counts[0];
  if (n_long > w.n_long_max) n_long = w.n_long_max;
  const int64_t stride = group_stride<G>();
  for (int64_t q0 = group_index<G>(); q0 < n_long; q0 += stride) {
    const int s = w.long_seg[q0];
    if (s < 0 || s >= h.n) continue;
    const int64_t base = w.long_base[q0];
    int nch = (h.seg_start[s + 1] - h.seg_start[s] + kSvdChunk - 1) / kSvdChunk;
    if (base < 0 || base + nch > w.n_chunk_max) nch = 0;
    float acc[R];
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0.f;
    for (int j = 0; j < nch; ++j)                           // chunk order
#pragma unroll
      for (int q = 0; q < R; ++q) acc[q] += w.partial[(base + j) * h.K + min(lane + q * G, h.K - 1)];
    hist_apply<MODE, G, R>(Y, m, v, nY, h.K, s, h.seg_rows[s], lane, acc, grows, coef);
  }
}

static inline size_t svd_align(size_t x) { return (x + 255) / 256 * 256; }
static inline int svd_long_max(int64_t n) { return static_cast<int>(n / kSvdLongRun + 1); }
static inline int svd_chunk_max(int64_t n) { return static_cast<int>(n / kSvdChunk + n / kSvdLongRun + 2); }
static SvdLongWs svd_make_ws(void* ws, int64_t n) {
  SvdLongWs w;
  char* p = static_cast<char*>(ws);
  w.n_long_max = svd_long_max(n);
  w.n_chunk_max = svd_chunk_max(n);
  w.counts = reinterpret_cast<int32_t*>(p);
  p += 256;
  w.long_seg = reinterpret_cast<int32_t*>(p);
  p += svd_align(static_cast<size_t>(w.n_long_max) * 4);
  w.long_base = reinterpret_cast<int32_t*>(p);
  p += svd_align(static_cast<size_t>(w.n_long_max) * 4);
  w.chunk_slot = reinterpret_cast<int32_t*>(p);
  p += svd_align(static_cast<size_t>(w.n_chunk_max) * 4);
  w.partial = reinterpret_cast<float*>(p);
  return w;
}

template <int G, int R>
static int pool_launch(hipStream_t st, const float* P, const float* Y, int64_t nU, int64_t nY, int K, const int64_t* hist_ptr,
                       const int32_t* hist_idx, int64_t nnz, const int32_t* rows, const int32_t* n_rows_dev, int64_t n_rows,
                       float* out, float* scale_out) {
  hipLaunchKernelGGL((svdpp_pool_kernel<G, R>), dim3(grid_for(n_rows, kBlock / G)), dim3(kBlock), 0, st, P, Y, nU, nY, K,
                     hist_ptr, hist_idx, nnz, rows, n_rows_dev, n_rows, out, scale_out);
  return launch_status();
}

template <int G, int R>
static int score_launch(hipStream_t st, const float* X, int64_t nX, const int32_t* xidx, const float* Q, int64_t nI,
                        const float* bu, int64_t nU, const float* bi, int K, const int32_t* users, const int32_t* items,
                        const float* labels, int64_t B, int loss_kind, int mode, float gscale, float* score, float* loss,
                        float* g, float* gx, float* gq) {
  const int64_t blocks = ceil_div(B, kBlock / G);
  hipLaunchKernelGGL((mf_score_kernel<G, R>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, X, nX, xidx, Q, nI, bu,
                     nU, bi, K, users, items, labels, B, loss_kind, mode, gscale, score, loss, g, gx, gq);
  return launch_status();
}

template <int MODE, int G, int R>
static int hist_launch(hipStream_t st, float* Y, float* m, float* v, int64_t nY, SvdHist h, float* grows, AdamCoef coef,
                       void* ws) {
  const bool use_long = ws != nullptr && h.n > kSvdLongRun;
  SvdLongWs w{};
  if (use_long) {
    w = svd_make_ws(ws, h.n);
    zero_words_async(w.counts, 2, st);
    hipLaunchKernelGGL(svdpp_hist_classify_kernel, dim3(grid_for(h.n, kBlock, kNumCU * 2)), dim3(kBlock), 0, st, h.seg_start,
                       h.n_seg, h.n, w);
  }
  hipLaunchKernelGGL((svdpp_hist_kernel<MODE, G, R>), dim3(grid_for(h.n, kBlock / G)), dim3(kBlock), 0, st, Y, m, v, nY, h,
                     grows, coef, use_long ? 1 : 0);
  if (use_long) {
    hipLaunchKernelGGL((svdpp_hist_chunk_kernel<G, R>), dim3(grid_for(w.n_chunk_max, kBlock / G)), dim3(kBlock), 0, st, h, w);
    hipLaunchKernelGGL((svdpp_hist_finish_kernel<MODE, G, R>), dim3(grid_for(w.n_long_max, kBlock / G)), dim3(kBlock), 0, st,
                       Y, m, v, nY, h, grows, coef, w);
  }
  return launch_status();
}

// rows of 257 - 512 floats take eight dwords per lane; the narrower ones share BPR's groups
template <int MODE>
static int hist_dispatch(hipStream_t st, float* Y, float* m, float* v, int64_t nY, SvdHist h, float* grows, AdamCoef coef,
                         void* ws) {
#define LR_SVD_HIST(G, R) hist_launch<MODE, G, R>(st, Y, m, v, nY, h, grows, coef, ws)
  if (h.K > 256) return LR_SVD_HIST(64, 8);
  LR_ROW_GROUP_DISPATCH_256(h.K, LR_SVD_HIST);
#undef LR_SVD_HIST
}

}  // namespace lr

using namespace lr;

extern "C" int lr_svd_supported(int K) { return K >= 1 && K <= kSvdMaxK ? 1 : 0; }

extern "C" int lr_svdpp_pool_f32(const float* P, const float* Y, int64_t n_users, int64_t n_items, int K,
                                 const int64_t* hist_ptr, const int32_t* hist_idx, int64_t nnz, const int32_t* rows,
                                 const int32_t* n_rows_dev, int64_t n_rows, float* out, float* scale_out,
                                 lr_stream_t stream) {
  LR_CHECK_ARG(n_rows >= 0 && n_users >= 1 && n_items >= 1 && nnz >= 0);
  if (!lr_svd_supported(K)) return LR_ESHAPE;
  if (n_rows == 0) return LR_OK;
  LR_CHECK_ARG(Y && hist_ptr && out && (hist_idx || nnz == 0));
  LR_CHECK_ARG(rows != nullptr || (n_rows_dev == nullptr && n_rows <= n_users));
  hipStream_t st = as_stream(stream);
#define LR_SVD_POOL(G, R) \
  pool_launch<G, R>(st, P, Y, n_users, n_items, K, hist_ptr, hist_idx, nnz, rows, n_rows_dev, n_rows, out, scale_out)
  if (K > 256) return LR_SVD_POOL(64, 8);
  LR_ROW_GROUP_DISPATCH_256(K, LR_SVD_POOL);
#undef LR_SVD_POOL
}

extern "C" int lr_mf_score_f32(const float* X, int64_t nX, const int32_t* xidx, const float* Q, int64_t n_items,
                               const float* bu, int64_t n_users, const float* bi, int K, const int32_t* users,
                               const int32_t* items, const float* labels, int64_t B, int loss_kind, int mode, float gscale,
                               float* score, float* loss, float* g, float* gx, float* gq, lr_stream_t stream) {
  LR_CHECK_ARG(B >= 0 && nX >= 1 && n_items >= 1 && n_users >= 1);
  if (!lr_svd_supported(K)) return LR_ESHAPE;
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(B < (int64_t{1} << 30));
  LR_CHECK_ARG(X && Q && users && items && labels && score && loss && g);
  LR_CHECK_ARG(loss_kind == LR_MF_MSE || loss_kind == LR_MF_CROSS_ENTROPY || loss_kind == LR_MF_FOCAL);
  LR_CHECK_ARG(mode == LR_MF_SCORE || (mode == LR_MF_GRAD && gx && gq));
  hipStream_t st = as_stream(stream);
#define LR_SVD_SCORE(G, R)                                                                                              \
  score_launch<G, R>(st, X, nX, xidx, Q, n_items, bu, n_users, bi, K, users, items, labels, B, loss_kind, mode, gscale, \
                     score, loss, g, gx, gq)
  if (K > 256) return LR_SVD_SCORE(64, 8);
  LR_ROW_GROUP_DISPATCH_256(K, LR_SVD_SCORE);
#undef LR_SVD_SCORE
}

extern "C" size_t lr_svdpp_hist_grad_ws_bytes(int64_t n_max, int K) {
  if (n_max < 0 || K < 1) return 0;
  return 256 + 2 * svd_align(static_cast<size_t>(svd_long_max(n_max)) * 4) +
         svd_align(static_cast<size_t>(svd_chunk_max(n_max)) * 4) +
         svd_align(static_cast<size_t>(svd_chunk_max(n_max)) * K * 4);
}

extern "C" int lr_svdpp_hist_grad_f32(int mode, float* Y, float* m, float* v, int64_t n_items, int K, const float* G,
                                      const float* scale, int64_t n_slots, const int32_t* ent_slot, const int32_t* seg_pos,
                                      const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg, int64_t n,
                                      float* grows, lr_adam_hp hp, void* ws, size_t ws_bytes, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && n_items >= 1 && n_slots >= 0);
  if (!lr_svd_supported(K)) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(n < (int64_t{1} << 31) && n_slots >= 1);
  LR_CHECK_ARG(G && scale && ent_slot && seg_pos && seg_rows && seg_start && n_seg);
  LR_CHECK_ARG((mode == LR_SVD_HIST_ADAM && Y && m && v && hp.step >= 1) || (mode == LR_SVD_HIST_ROWS && grows));
  if (ws != nullptr && ws_bytes < lr_svdpp_hist_grad_ws_bytes(n, K)) return LR_EWORKSPACE;
  SvdHist h{G, scale, n_slots, ent_slot, seg_pos, seg_rows, seg_start, n_seg, n, K};
  hipStream_t st = as_stream(stream);
  if (mode == LR_SVD_HIST_ADAM) return hist_dispatch<LR_SVD_HIST_ADAM>(st, Y, m, v, n_items, h, grows, make_adam_coef(hp), ws);
  AdamCoef none{};
  return hist_dispatch<LR_SVD_HIST_ROWS>(st, Y, m, v, n_items, h, grows, none, ws);
}
