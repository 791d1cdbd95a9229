// BPR (`libreco/algorithms/_bpr.pyx:116-399`, `libreco/algorithms/bpr.py:161-204`): score a window of
// (user, positive, negative) triples, then update every touched row in ascending sample order.
//
// The reference walks the samples one after the other.  Here an epoch is cut into windows: every
// c = 1 / (1 + exp(d)) and every gradient of a window is formed from the tables as they stood when the window began,
// and each touched row then takes the reference's per-sample optimiser step once per occurrence, in sample order.
//   bpr_score_kernel   one sub-wave group per sample gathers the three rows, reduces d inside the group and writes c and
//                      -log sigmoid(d); it also stashes p - q per sample (engine) or writes the per-position gradient rows
//                      of the mini-batch mode.
//   bpr_update_kernel  one sub-wave group per touched row (a run of lr_segments_build) keeps the row and its optimiser
//                      state in registers and walks the run.  Item rows go first and read the user rows straight from
//                      the (still untouched) user table; the user pass reads only the stash and c.
// Rows are 2 - 256 floats and the tables are cache resident, so a group is sized to the row (16 lanes at K = 16), not a
// whole wave.  No atomics, no inter-workgroup wait: the chain loop is bounded by the run length read from the segments.
#include <math.h>

#include "row_group.hpp"

namespace lr {

constexpr int kBprMaxD = 256;
constexpr int kChainBlock = 8;   // occurrences of a row whose operands are fetched together (ordered row update)

// ---- triple score ------------------------------------------------------------------------
template <int G, int R>
__global__ __launch_bounds__(kBlock) void bpr_score_kernel(
    const float* __restrict__ U, int64_t nU, int ldu, const float* __restrict__ I, int64_t nI, int ldi,
    const float* __restrict__ ibias, int D, const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
    const int32_t* __restrict__ neg, int64_t W, int mode, float gscale, float* __restrict__ c_out,
    float* __restrict__ loss_out, float* __restrict__ gu, float* __restrict__ gi, float* __restrict__ gb) {
  const int lane = threadIdx.x % G;
  const int64_t s = group_index<G>();
  const bool in = s < W;
  int32_t u = -1, p = -1, q = -1;
  if (in) {
    u = users[s];
    p = pos[s];
    q = neg[s];
  }
  const bool ok = in && u >= 0 && u < nU && p >= 0 && p < nI && q >= 0 && q < nI;
  float uu[R], dd[R];
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + r * G;
    uu[r] = 0.f;
    dd[r] = 0.f;
    if (ok && j < D) {
      uu[r] = U[static_cast<int64_t>(u) * ldu + j];
      dd[r] = I[static_cast<int64_t>(p) * ldi + j] - I[static_cast<int64_t>(q) * ldi + j];
    }
    acc = fmaf(uu[r], dd[r], acc);
  }
  float d = group_sum<G>(acc);          // every lane of the wave takes part: no early exit above
  if (ok && ibias != nullptr) d += ibias[p] - ibias[q];
  // c in [0, 1] for every d (exp overflows to inf -> c = 0); -log sigmoid(d) = max(-d, 0) + log1p(exp(-|d|)) stays finite
  float c = 1.f / (1.f + expf(d));
  float loss = fmaxf(-d, 0.f) + log1pf(expf(-fabsf(d)));
  if (!ok) {                            // a triple with an id outside its table takes no part in the update (c < 0)
    c = -1.f;
    loss = 0.f;
  }
  if (!in) return;
  if (lane == 0) {
    c_out[s] = c;
    if (loss_out != nullptr) loss_out[s] = loss;
  }
  if (mode == LR_BPR_STASH) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      if (j < D) gu[s * D + j] = dd[r];
    }
  } else if (mode == LR_BPR_GRAD) {     // gradient of mean(-log sigmoid(d)): -(c / B) is the whole backward
    const float a = ok ? c * gscale : 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      if (j < D) {
        gu[s * D + j] = -a * dd[r];
        gi[(2 * s) * D + j] = -a * uu[r];
        gi[(2 * s + 1) * D + j] = a * uu[r];
      }
    }
    if (lane == 0 && gb != nullptr) {
      gb[2 * s] = -a;
      gb[2 * s + 1] = a;
    }
  }
}

// ---- ordered row update ------------------------------------------------------------------
struct BprCoef {
  float lr, reg, mom, b1, b2, omb1, omb2, bc1, bc2;
};

template <int OPT>
__device__ __forceinline__ void bpr_step(float& x, float& s1, float& s2, float g, const BprCoef& k) {
  if (OPT == LR_BPR_SGD) {                                   // _bpr.pyx:181-190
    x += k.lr * g;
  } else if (OPT == LR_BPR_MOMENTUM) {                       // _bpr.pyx:273-280
    s1 = k.mom * s1 + k.lr * g;
    x += s1;
  } else {                                                   // _bpr.pyx:376-399: bias correction by the epoch
    s1 = k.b1 * s1 + k.omb1 * g;
    s2 = k.b2 * s2 + k.omb2 * (g * g);
    x += k.lr * (s1 / k.bc1) / (sqrtf(s2 / k.bc2) + 1e-8f);
  }
}

// A block of kChainBlock occurrences of a row, i0 .. i0 + kChainBlock - 1 of seg_pos (those at or beyond `e` and those of a
// skipped sample get cs < 0): the window-start c of each one's sample times the other factor of its gradient (the user row
// for an item occurrence, p - q for a user occurrence).  Three stages of loads, each at clamped, always valid addresses
// and without a branch between them, so that the loads of one stage are in flight together.
template <int G, int R>
__device__ __forceinline__ void bpr_fetch_block(int i0, int e, int lane, int Dw, int D, const int32_t* __restrict__ seg_pos,
                                                const float* __restrict__ c, int64_t W, const float* __restrict__ other,
                                                int64_t other_rows, const int32_t* __restrict__ other_ids,
                                                float (&cs)[kChainBlock], float (&o)[kChainBlock][R]) {
  const bool item = other_ids != nullptr;
  int pp[kChainBlock];
#pragma unroll
  for (int t = 0; t < kChainBlock; ++t) pp[t] = seg_pos[min(i0 + t, e - 1)];
  float cv[kChainBlock];
  int64_t orow[kChainBlock];
  bool ok[kChainBlock];
#pragma unroll
  for (int t = 0; t < kChainBlock; ++t) {
    int64_t s = item ? (pp[t] >> 1) : pp[t];
    ok[t] = i0 + t < e && pp[t] >= 0 && s < W;
    s = ok[t] ? s : 0;
    cv[t] = c[s];
    orow[t] = item ? other_ids[s] : s;
  }
#pragma unroll
  for (int t = 0; t < kChainBlock; ++t) {
    ok[t] = ok[t] && cv[t] >= 0.f && orow[t] >= 0 && orow[t] < other_rows;
    const int64_t base = (ok[t] ? orow[t] : 0) * D;
    const float sc = (item && (pp[t] & 1)) ? -cv[t] : cv[t];      // the negative's gradient is -c u - reg q
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      o[t][r] = sc * other[base + min(j, D - 1)];
    }
    cs[t] = ok[t] ? 1.f : -1.f;
  }
}

template <int OPT, int G, int R>
__global__ __launch_bounds__(kBlock) void bpr_update_kernel(
    float* __restrict__ table, float* __restrict__ st1, float* __restrict__ st2, int64_t V, int D, int Dw,
    const int32_t* __restrict__ seg_pos, const int32_t* __restrict__ seg_rows, const int32_t* __restrict__ seg_start,
    const int32_t* __restrict__ n_seg, int64_t n, const float* __restrict__ c, int64_t W,
    const float* __restrict__ other, int64_t other_rows, const int32_t* __restrict__ other_ids, BprCoef k) {
  const int lane = threadIdx.x % G;
  int64_t nseg = *n_seg;
  if (nseg > n) nseg = n;
  const int64_t stride = group_stride<G>();
  for (int64_t run = group_index<G>(); run < nseg; run += stride) {
    const int64_t row = seg_rows[run];
    int b = seg_start[run], e = seg_start[run + 1];
    if (row < 0 || row >= V || b < 0) continue;
    if (e > n) e = static_cast<int>(n);
    float x[R], x0[R], s1[R], s2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      x[r] = s1[r] = s2[r] = 0.f;
      if (j < Dw) {
        x[r] = table[row * D + j];
        if (OPT != LR_BPR_SGD) s1[r] = st1[row * D + j];
        if (OPT == LR_BPR_ADAM) s2[r] = st2[row * D + j];
      }
      x0[r] = k.reg * x[r];                                  // the reg term too is the window-start one
    }
    // The chain is sequential by definition, but an occurrence's operands (position -> sample -> c, user id -> row:
    // dependent loads) do not depend on it: they are fetched kChainBlock occurrences at a time and then applied one
    // after the other in run order.
    for (int i0 = b; i0 < e; i0 += kChainBlock) {
      float cs[kChainBlock], o[kChainBlock][R];
      bpr_fetch_block<G, R>(i0, e, lane, Dw, D, seg_pos, c, W, other, other_rows, other_ids, cs, o);
#pragma unroll
      for (int t = 0; t < kChainBlock; ++t) {
        if (cs[t] < 0.f) continue;
#pragma unroll
        for (int r = 0; r < R; ++r) bpr_step<OPT>(x[r], s1[r], s2[r], o[t][r] - x0[r], k);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      if (j < Dw) {
        table[row * D + j] = x[r];
        if (OPT != LR_BPR_SGD) st1[row * D + j] = s1[r];
        if (OPT == LR_BPR_ADAM) st2[row * D + j] = s2[r];
      }
    }
  }
}

template <int G, int R>
static int score_launch(hipStream_t st, const float* U, int64_t nU, int ldu, const float* I, int64_t nI, int ldi,
                        const float* ibias, int D, const int32_t* users, const int32_t* pos, const int32_t* neg, int64_t W,
                        int mode, float gscale, float* c, float* loss, float* gu, float* gi, float* gb) {
  const int64_t blocks = ceil_div(W, kBlock / G);
  hipLaunchKernelGGL((bpr_score_kernel<G, R>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, U, nU, ldu, I, nI,
                     ldi, ibias, D, users, pos, neg, W, mode, gscale, c, loss, gu, gi, gb);
  return launch_status();
}

template <int OPT, int G, int R>
static int update_launch(hipStream_t st, float* table, float* s1, float* s2, int64_t V, int D, int Dw, const int32_t* seg_pos,
                         const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg, int64_t n, const float* c,
                         int64_t W, const float* other, int64_t other_rows, const int32_t* other_ids, BprCoef k) {
  hipLaunchKernelGGL((bpr_update_kernel<OPT, G, R>), dim3(grid_for(n, kBlock / G)), dim3(kBlock), 0, st, table, s1, s2, V, D,
                     Dw, seg_pos, seg_rows, seg_start, n_seg, n, c, W, other, other_rows, other_ids, k);
  return launch_status();
}

template <int OPT>
static int update_dispatch(hipStream_t st, float* table, float* s1, float* s2, int64_t V, int D, int Dw, const int32_t* seg_pos,
                           const int32_t* seg_rows, const int32_t* seg_start, const int32_t* n_seg, int64_t n, const float* c,
                           int64_t W, const float* other, int64_t other_rows, const int32_t* other_ids, BprCoef k) {
#define LR_BPR_UPD(G, R) \
  update_launch<OPT, G, R>(st, table, s1, s2, V, D, Dw, seg_pos, seg_rows, seg_start, n_seg, n, c, W, other, other_rows, other_ids, k)
  LR_ROW_GROUP_DISPATCH_256(D, LR_BPR_UPD);
#undef LR_BPR_UPD
}

}  // namespace lr

using namespace lr;

extern "C" int lr_bpr_supported(int D) { return D >= 1 && D <= kBprMaxD ? 1 : 0; }

extern "C" int lr_bpr_triple_score_f32(const float* U, int64_t nU, int ldu, const float* I, int64_t nI, int ldi,
                                       const float* ibias, int D, const int32_t* users, const int32_t* pos,
                                       const int32_t* neg, int64_t W, int mode, float gscale, float* c, float* loss,
                                       float* gu, float* gi, float* gb, lr_stream_t stream) {
  LR_CHECK_ARG(W >= 0 && nU >= 1 && nI >= 1);
  if (!lr_bpr_supported(D) || ldu < D || ldi < D) return LR_ESHAPE;
  if (W == 0) return LR_OK;
  LR_CHECK_ARG(W < (int64_t{1} << 30));
  LR_CHECK_ARG(U && I && users && pos && neg && c);
  LR_CHECK_ARG(mode == LR_BPR_SCORE || mode == LR_BPR_STASH || mode == LR_BPR_GRAD);
  LR_CHECK_ARG(mode == LR_BPR_SCORE || gu != nullptr);
  LR_CHECK_ARG(mode != LR_BPR_GRAD || gi != nullptr);
  hipStream_t st = as_stream(stream);
#define LR_BPR_SCORE_CALL(G, R) \
  score_launch<G, R>(st, U, nU, ldu, I, nI, ldi, ibias, D, users, pos, neg, W, mode, gscale, c, loss, gu, gi, gb)
  LR_ROW_GROUP_DISPATCH_256(D, LR_BPR_SCORE_CALL);
#undef LR_BPR_SCORE_CALL
}

extern "C" int lr_bpr_row_update_f32(int optimizer, float* table, float* state1, float* state2, int64_t V, int D, int Dw,
                                     const int32_t* seg_pos, const int32_t* seg_rows, const int32_t* seg_start,
                                     const int32_t* n_seg, int64_t n, const float* c, int64_t W, const float* other,
                                     int64_t other_rows, const int32_t* other_ids, double lr, double reg, int epoch,
                                     lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && W >= 0 && V >= 1 && epoch >= 1);
  if (!lr_bpr_supported(D) || Dw < 1 || Dw > D) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(n < (int64_t{1} << 31) && n == (other_ids != nullptr ? 2 * W : W));
  LR_CHECK_ARG(table && seg_pos && seg_rows && seg_start && n_seg && c && other && other_rows >= 1);
  LR_CHECK_ARG(optimizer == LR_BPR_SGD || (optimizer == LR_BPR_MOMENTUM && state1) ||
               (optimizer == LR_BPR_ADAM && state1 && state2));
  BprCoef k;
  k.lr = static_cast<float>(lr);
  k.reg = static_cast<float>(reg);
  k.mom = 0.9f;
  k.b1 = 0.9f;
  k.b2 = 0.999f;
  k.omb1 = static_cast<float>(1.0 - 0.9);
  k.omb2 = static_cast<float>(1.0 - 0.999);
  k.bc1 = static_cast<float>(1.0 - pow(0.9, static_cast<double>(epoch)));
  k.bc2 = static_cast<float>(1.0 - pow(0.999, static_cast<double>(epoch)));
  hipStream_t st = as_stream(stream);
  if (optimizer == LR_BPR_SGD)
    return update_dispatch<LR_BPR_SGD>(st, table, state1, state2, V, D, Dw, seg_pos, seg_rows, seg_start, n_seg, n, c, W, other,
                                       other_rows, other_ids, k);
  if (optimizer == LR_BPR_MOMENTUM)
    return update_dispatch<LR_BPR_MOMENTUM>(st, table, state1, state2, V, D, Dw, seg_pos, seg_rows, seg_start, n_seg, n, c, W,
                                            other, other_rows, other_ids, k);
  return update_dispatch<LR_BPR_ADAM>(st, table, state1, state2, V, D, Dw, seg_pos, seg_rows, seg_start, n_seg, n, c, W, other,
                                      other_rows, other_ids, k);
}
