// Skip-gram word2vec in windows: the training of Item2Vec (negative sampling) and DeepWalk (negative
// sampling and hierarchical softmax), which the reference hands to gensim's CPU threads.
//
// word2vec walks the (input, predicted) pairs one after the other.  Here an epoch's pairs are cut into windows: every
// f = syn0[in] . syn1[t] and every g = (label - sigmoid(f)) * alpha of a window comes from the tables as they stood when
// the window began, and each touched row then takes its sum in ascending sample order.  No float atomics.
//   w2v_walks_kernel        one thread per random walk over the successor CSR
//   w2v_keep_kernel         frequent-word subsampling flags
//   w2v_pairs_kernel        count / emit of the (input, predicted, centre position) pairs of the compacted corpus
//   w2v_targets_kernel      count / fill of a pair's target list: the predicted word, 5 negatives, the Huffman path
//   w2v_score_kernel        one sub-wave group per pair: g per target, the pair's sum of g * syn1[t] (the stash), its loss
//   w2v_update_kernel       one sub-wave group per touched row (a run of lr_segments_build): the row stays in registers
//                           while the run is walked in ascending position.  Output rows add g * syn0[in] (syn0 still
//                           untouched); input rows add their pairs' stash rows.
// Every draw is mix64 of (seed, stream, a, b): a pure function of the position, bit-exact against tests/w2v_oracle.py.
#include <math.h>

#include "mix64.hpp"
#include "row_group.hpp"

namespace lr {

constexpr int kW2vMaxD = 256;
constexpr int kW2vChainFloats = 32;   // row floats per lane fetched together in the ordered row update: 32 / R occurrences
constexpr uint64_t kW2vGold = 0x9e3779b97f4a7c15ull;
enum : uint64_t { kW2vWalk = 1, kW2vKeep = 2, kW2vShrink = 3, kW2vNeg = 4 };

__host__ __device__ inline uint64_t w2v_hash(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b) {
  uint64_t z = mix64(seed + kW2vGold * stream);
  z = mix64(z + kW2vGold * (a + 1));
  return mix64(z + kW2vGold * (b + 1));
}

// ---- corpus ------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void w2v_walks_kernel(
    const int32_t* __restrict__ starts, int64_t n_walks, int L, const int64_t* __restrict__ sptr,
    const int32_t* __restrict__ sidx, int64_t n_items, int64_t n_edges, uint64_t seed, uint64_t pass,
    int32_t* __restrict__ walks, int32_t* __restrict__ lens) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; w < n_walks; w += stride) {
    int32_t node = starts[w];
    bool ok = node >= 0 && node < n_items;
    int len = 0;
    for (int s = 0; s < L; ++s) {
      walks[w * L + s] = ok ? node : -1;
      if (!ok) continue;
      ++len;
      if (s + 1 == L) break;
      const int64_t lo = sptr[node], hi = sptr[node + 1];
      if (lo < 0 || hi > n_edges || hi <= lo) {             // a node without successors ends the walk
        ok = false;
        continue;
      }
      const uint64_t h = w2v_hash(seed, kW2vWalk, pass, static_cast<uint64_t>(w) * L + s);
      const uint64_t pick = ((h >> 32) * static_cast<uint64_t>(hi - lo)) >> 32;
      node = sidx[lo + static_cast<int64_t>(pick)];
      ok = node >= 0 && node < n_items;
    }
    lens[w] = len;
  }
}

__global__ __launch_bounds__(kBlock) void w2v_keep_kernel(const int32_t* __restrict__ tokens, int64_t n,
                                                         const int64_t* __restrict__ thr, int64_t n_items, uint64_t seed,
                                                         uint64_t epoch, uint8_t* __restrict__ keep) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const int32_t w = tokens[i];
    uint8_t k = 0;
    if (w >= 0 && w < n_items) {
      const uint64_t h = w2v_hash(seed, kW2vKeep, epoch, static_cast<uint64_t>(i));
      k = static_cast<int64_t>(h >> 32) < thr[w] ? 1 : 0;
    }
    keep[i] = k;
  }
}

// The context of compacted position i: [lo, hi] without i itself, cut at the sentence's ends.
__device__ __forceinline__ void w2v_context(int64_t i, const int32_t* __restrict__ craw, const int32_t* __restrict__ csent,
                                            const int64_t* __restrict__ cptr, int64_t nc, int64_t n_sent, int window,
                                            uint64_t seed, uint64_t epoch, int64_t& lo, int64_t& hi) {
  lo = 0;
  hi = -1;
  const int32_t s = csent[i];
  if (s < 0 || s >= n_sent) return;
  int64_t sb = cptr[s], se = cptr[s + 1];
  if (sb < 0) sb = 0;
  if (se > nc) se = nc;
  if (i < sb || i >= se) return;
  const uint64_t h = w2v_hash(seed, kW2vShrink, epoch, static_cast<uint64_t>(static_cast<uint32_t>(craw[i])));
  const int64_t r = window - static_cast<int64_t>(h % static_cast<uint64_t>(window));
  lo = i - r < sb ? sb : i - r;
  hi = i + r > se - 1 ? se - 1 : i + r;
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void w2v_pairs_kernel(
    const int32_t* __restrict__ ctok, const int32_t* __restrict__ craw, const int32_t* __restrict__ csent,
    const int64_t* __restrict__ cptr, int64_t nc, int64_t n_sent, int window, uint64_t seed, uint64_t epoch,
    int32_t* __restrict__ counts, const int64_t* __restrict__ offs, int64_t n_pairs, int32_t* __restrict__ in_ids,
    int32_t* __restrict__ pred, int32_t* __restrict__ centre) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < nc; i += stride) {
    int64_t lo, hi;
    w2v_context(i, craw, csent, cptr, nc, n_sent, window, seed, epoch, lo, hi);
    if (!EMIT) {
      counts[i] = hi >= lo ? static_cast<int32_t>(hi - lo) : 0;
    } else {
      int64_t o = offs[i];
      const int32_t me = ctok[i], raw = craw[i];
      for (int64_t j = lo; j <= hi; ++j) {
        if (j == i) continue;
        if (o >= 0 && o < n_pairs) {
          in_ids[o] = ctok[j];
          pred[o] = me;
          centre[o] = raw;
        }
        ++o;
      }
    }
  }
}

// ---- targets -----------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(kBlock) void w2v_targets_kernel(
    const int32_t* __restrict__ in_ids, const int32_t* __restrict__ pred, int64_t W, int64_t pair_base, int64_t n_items,
    const int64_t* __restrict__ cum, const int32_t* __restrict__ hs_ptr, const int32_t* __restrict__ hs_nodes,
    const int32_t* __restrict__ hs_codes, int64_t hs_len, uint64_t seed, uint64_t epoch, const int64_t* __restrict__ offs,
    int32_t* __restrict__ lens, int64_t n_slots, int32_t* __restrict__ rows, int32_t* __restrict__ labels,
    int32_t* __restrict__ slot_in) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; p < W; p += stride) {
    const int32_t pd = pred[p];
    const bool valid = pd >= 0 && pd < n_items;
    int64_t hb = 0, plen = 0;
    if (valid && hs_ptr != nullptr) {
      hb = hs_ptr[pd];
      plen = hs_ptr[pd + 1] - hb;
      if (hb < 0 || plen < 0 || hb + plen > hs_len) plen = 0;
    }
    if (!FILL) {
      lens[p] = static_cast<int32_t>(1 + LR_W2V_NEGATIVES + plen);
      continue;
    }
    const int64_t o = offs[p];
    if (o < 0 || offs[p + 1] - o != 1 + LR_W2V_NEGATIVES + plen || o + 1 + LR_W2V_NEGATIVES + plen > n_slots) continue;
    const int32_t in = in_ids[p];
    rows[o] = valid ? pd : -1;
    labels[o] = 1;
    slot_in[o] = in;
    for (int k = 0; k < LR_W2V_NEGATIVES; ++k) {
      const uint64_t h = w2v_hash(seed, kW2vNeg, epoch, static_cast<uint64_t>(pair_base + p) * LR_W2V_NEGATIVES + k);
      const int64_t r = static_cast<int64_t>(h >> 32);
      int64_t a = 0, b = n_items;                           // the first word whose cumulative weight exceeds r
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (cum[mid] > r) b = mid; else a = mid + 1;
      }
      // a draw equal to the predicted word is masked, not redrawn (word2vec)
      rows[o + 1 + k] = (valid && a < n_items && a != pd) ? static_cast<int32_t>(a) : -1;
      labels[o + 1 + k] = 0;
      slot_in[o + 1 + k] = in;
    }
    for (int64_t t = 0; t < plen; ++t) {
      rows[o + 1 + LR_W2V_NEGATIVES + t] = hs_nodes[hb + t];
      labels[o + 1 + LR_W2V_NEGATIVES + t] = 1 - hs_codes[hb + t];
      slot_in[o + 1 + LR_W2V_NEGATIVES + t] = in;
    }
  }
}

// ---- score -------------------------------------------------------------------------------
__device__ __forceinline__ int wave_max_int(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = max(x, __shfl_xor(x, o));
  return x;
}

template <int G, int R>
struct W2vTarget {
  float w[R];
  int lab;
  bool act, live;
};

template <int G, int R>
__device__ __forceinline__ W2vTarget<G, R> w2v_load_target(int t, int cnt, int64_t o, bool ok, int lane, int D,
                                                           const float* __restrict__ syn1, int64_t V1,
                                                           const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ labels) {
  W2vTarget<G, R> x;
  x.act = t < cnt;
  const int32_t row = x.act ? rows[o + t] : -1;
  x.lab = x.act ? labels[o + t] : 0;
  x.live = ok && row >= 0 && row < V1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + r * G;
    x.w[r] = (x.live && j < D) ? syn1[static_cast<int64_t>(row) * D + j] : 0.f;
  }
  return x;
}

template <int G, int R>
__global__ __launch_bounds__(kBlock) void w2v_score_kernel(
    const float* __restrict__ syn0, int64_t n_items, const float* __restrict__ syn1, int64_t V1, int D,
    const int32_t* __restrict__ in_ids, const int32_t* __restrict__ centre, int64_t W, const int64_t* __restrict__ offs,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ labels, int64_t n_slots, double pos0, double inv_total,
    float* __restrict__ g_out, float* __restrict__ stash, float* __restrict__ loss_out) {
  const int lane = threadIdx.x % G;
  const int64_t p = group_index<G>();
  const bool in = p < W;
  int32_t id = -1;
  int64_t o = 0;
  int cnt = 0;
  float alpha = 0.f;
  if (in) {
    id = in_ids[p];
    o = offs[p];
    const int64_t e = offs[p + 1];
    if (o >= 0 && e >= o && e <= n_slots && e - o < (1 << 20)) cnt = static_cast<int>(e - o);
    const double progress = (pos0 + static_cast<double>(centre[p])) * inv_total;
    const double a = 0.025 - (0.025 - 1e-4) * progress;
    alpha = static_cast<float>(a < 1e-4 ? 1e-4 : a);
  }
  const bool ok = in && id >= 0 && id < n_items;   // a pair whose input id is outside the table takes no part (g = 0)
  const int nmax = wave_max_int(cnt);              // every lane of the wave walks the wave's longest list: no lane leaves
                                                   // before a group reduction
  float v[R], acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + r * G;
    v[r] = (ok && j < D) ? syn0[static_cast<int64_t>(id) * D + j] : 0.f;
    acc[r] = 0.f;
  }
  float loss = 0.f;
  W2vTarget<G, R> cur = w2v_load_target<G, R>(0, cnt, o, ok, lane, D, syn1, V1, rows, labels);
  for (int t = 0; t < nmax; ++t) {
    // the next target's row is requested before this one's reduction
    const W2vTarget<G, R> nxt = w2v_load_target<G, R>(t + 1, cnt, o, ok, lane, D, syn1, V1, rows, labels);
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) dot = fmaf(v[r], cur.w[r], dot);
    const float f = group_sum<G>(dot);
    float g = 0.f;
    if (cur.live) {
      if (fabsf(f) < 6.f) g = (static_cast<float>(cur.lab) - 1.f / (1.f + expf(-f))) * alpha;   // word2vec skips |f| >= 6
      const float x = cur.lab ? f : -f;                                                         // -log sigmoid(x)
      loss += fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fmaf(g, cur.w[r], acc[r]);
    if (cur.act && lane == 0) g_out[o + t] = g;
    cur = nxt;
  }
  if (!in) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int j = lane + r * G;
    if (j < D) stash[p * D + j] = acc[r];
  }
  if (lane == 0 && loss_out != nullptr) loss_out[p] = loss;
}

// ---- ordered row update ------------------------------------------------------------------
// slot_in != nullptr: output rows; occurrence at flat target slot q adds g[q] * other[slot_in[q]] (other = syn0).
// slot_in == nullptr: input rows; occurrence at pair q adds other[q] (other = the stash).

// The coefficient and the source row of CH occurrences of a run, i0 .. i0 + CH - 1 of seg_pos (position -> g, input id: two
// stages of dependent loads at clamped, always valid addresses).  An occurrence at or beyond `e`, with g = 0 (a masked or
// skipped target) or with an id outside `other` gets the coefficient 0 and takes no part.
template <int CH>
__device__ __forceinline__ void w2v_fetch_meta(int i0, int e, int64_t n, const int32_t* __restrict__ seg_pos,
                                               const float* __restrict__ g, const int32_t* __restrict__ slot_in,
                                               int64_t other_rows, float (&gv)[CH], int (&src)[CH]) {
  int pp[CH];
#pragma unroll
  for (int t = 0; t < CH; ++t) pp[t] = seg_pos[min(i0 + t, e - 1)];
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const bool in = i0 + t < e && pp[t] >= 0 && pp[t] < n;
    const int q = in ? pp[t] : 0;
    const float gg = slot_in != nullptr ? g[q] : 1.f;
    const int sr = slot_in != nullptr ? slot_in[q] : q;
    const bool ok = in && sr >= 0 && sr < other_rows;
    gv[t] = ok ? gg : 0.f;
    src[t] = ok ? sr : 0;
  }
}

template <int G, int R>
__global__ __launch_bounds__(kBlock) void w2v_update_kernel(
    float* __restrict__ table, int64_t V, int D, const int32_t* __restrict__ seg_pos, const int32_t* __restrict__ seg_rows,
    const int32_t* __restrict__ seg_start, const int32_t* __restrict__ n_seg, int64_t n, const float* __restrict__ g,
    const int32_t* __restrict__ slot_in, const float* __restrict__ other, int64_t other_rows) {
  constexpr int CH = kW2vChainFloats / R;          // occurrences of a row whose operands are fetched together
  const int lane = threadIdx.x % G;
  int64_t nseg = *n_seg;
  if (nseg > n) nseg = n;
  const int64_t stride = group_stride<G>();
  for (int64_t run = group_index<G>(); run < nseg; run += stride) {
    const int64_t row = seg_rows[run];
    int b = seg_start[run], e = seg_start[run + 1];
    if (row < 0 || row >= V || b < 0) continue;
    if (e > n) e = static_cast<int>(n);
    if (e <= b) continue;
    float x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      x[r] = j < D ? table[row * D + j] : 0.f;
    }
    // The sum is sequential by definition, but an occurrence's operands (position -> g, input id -> row: three stages of
    // dependent loads) do not depend on it.  They are fetched CH occurrences at a time; the first two stages of the next
    // block are in flight while this block's rows arrive and are added one after the other in run order.  A frequent row's
    // run is thousands of occurrences long, and without this its walk is one chain of load latencies.
    float gv[CH];
    int src[CH];
    w2v_fetch_meta<CH>(b, e, n, seg_pos, g, slot_in, other_rows, gv, src);
    for (int i0 = b; i0 < e; i0 += CH) {
      float o[CH][R];
#pragma unroll
      for (int t = 0; t < CH; ++t) {
        const int64_t base = static_cast<int64_t>(src[t]) * D;
#pragma unroll
        for (int r = 0; r < R; ++r) o[t][r] = other[base + min(lane + r * G, D - 1)];
      }
      float gn[CH];
      int sn[CH];
      w2v_fetch_meta<CH>(i0 + CH, e, n, seg_pos, g, slot_in, other_rows, gn, sn);
#pragma unroll
      for (int t = 0; t < CH; ++t) {
        if (gv[t] != 0.f) {
#pragma unroll
          for (int r = 0; r < R; ++r) x[r] = fmaf(gv[t], o[t][r], x[r]);
        }
        gv[t] = gn[t];
        src[t] = sn[t];
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = lane + r * G;
      if (j < D) table[row * D + j] = x[r];
    }
  }
}

template <int G, int R>
static int w2v_score_launch(hipStream_t st, const float* syn0, int64_t n_items, const float* syn1, int64_t V1, int D,
                            const int32_t* in_ids, const int32_t* centre, int64_t W, const int64_t* offs, const int32_t* rows,
                            const int32_t* labels, int64_t n_slots, double pos0, double inv_total, float* g, float* stash,
                            float* loss) {
  const int64_t blocks = ceil_div(W, kBlock / G);
  hipLaunchKernelGGL((w2v_score_kernel<G, R>), dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, syn0, n_items, syn1,
                     V1, D, in_ids, centre, W, offs, rows, labels, n_slots, pos0, inv_total, g, stash, loss);
  return launch_status();
}

template <int G, int R>
static int w2v_update_launch(hipStream_t st, float* table, int64_t V, int D, const int32_t* seg_pos, const int32_t* seg_rows,
                             const int32_t* seg_start, const int32_t* n_seg, int64_t n, const float* g,
                             const int32_t* slot_in, const float* other, int64_t other_rows) {
  hipLaunchKernelGGL((w2v_update_kernel<G, R>), dim3(grid_for(n, kBlock / G)), dim3(kBlock), 0, st, table, V, D, seg_pos,
                     seg_rows, seg_start, n_seg, n, g, slot_in, other, other_rows);
  return launch_status();
}

}  // namespace lr

using namespace lr;

extern "C" int lr_w2v_supported(int D) { return D >= 1 && D <= kW2vMaxD ? 1 : 0; }

extern "C" int lr_w2v_walks_i32(const int32_t* starts, int64_t n_walks, int walk_length, const int64_t* succ_ptr,
                                const int32_t* succ_idx, int64_t n_items, int64_t n_edges, uint64_t seed, int64_t pass,
                                int32_t* walks, int32_t* lens, lr_stream_t stream) {
  LR_CHECK_ARG(n_walks >= 0 && walk_length >= 1 && n_items >= 1 && n_edges >= 0 && pass >= 0);
  if (n_walks == 0) return LR_OK;
  LR_CHECK_ARG(n_walks * walk_length < (int64_t{1} << 31));
  LR_CHECK_ARG(starts && succ_ptr && walks && lens && (succ_idx || n_edges == 0));
  hipLaunchKernelGGL(w2v_walks_kernel, dim3(grid_for(n_walks, kBlock)), dim3(kBlock), 0, as_stream(stream), starts, n_walks,
                     walk_length, succ_ptr, succ_idx, n_items, n_edges, seed, static_cast<uint64_t>(pass), walks, lens);
  return launch_status();
}

extern "C" int lr_w2v_keep_u8(const int32_t* tokens, int64_t n, const int64_t* keep_thr, int64_t n_items, uint64_t seed,
                              int64_t epoch, uint8_t* keep, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && n_items >= 1 && epoch >= 0);
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(n < (int64_t{1} << 31) && tokens && keep_thr && keep);
  hipLaunchKernelGGL(w2v_keep_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, as_stream(stream), tokens, n, keep_thr,
                     n_items, seed, static_cast<uint64_t>(epoch), keep);
  return launch_status();
}

extern "C" int lr_w2v_pairs_count_i32(const int32_t* craw, const int32_t* csent, const int64_t* cptr, int64_t nc,
                                      int64_t n_sent, int window, uint64_t seed, int64_t epoch, int32_t* counts,
                                      lr_stream_t stream) {
  LR_CHECK_ARG(nc >= 0 && n_sent >= 0 && window >= 1 && epoch >= 0);
  if (nc == 0) return LR_OK;
  LR_CHECK_ARG(nc < (int64_t{1} << 31) && craw && csent && cptr && counts);
  hipLaunchKernelGGL((w2v_pairs_kernel<false>), dim3(grid_for(nc, kBlock)), dim3(kBlock), 0, as_stream(stream), nullptr, craw,
                     csent, cptr, nc, n_sent, window, seed, static_cast<uint64_t>(epoch), counts, nullptr, 0, nullptr, nullptr,
                     nullptr);
  return launch_status();
}

extern "C" int lr_w2v_pairs_emit_i32(const int32_t* ctok, const int32_t* craw, const int32_t* csent, const int64_t* cptr,
                                     int64_t nc, int64_t n_sent, int window, uint64_t seed, int64_t epoch, const int64_t* offs,
                                     int64_t n_pairs, int32_t* in_ids, int32_t* pred, int32_t* centre, lr_stream_t stream) {
  LR_CHECK_ARG(nc >= 0 && n_sent >= 0 && window >= 1 && epoch >= 0 && n_pairs >= 0);
  if (nc == 0 || n_pairs == 0) return LR_OK;
  LR_CHECK_ARG(nc < (int64_t{1} << 31) && ctok && craw && csent && cptr && offs && in_ids && pred && centre);
  hipLaunchKernelGGL((w2v_pairs_kernel<true>), dim3(grid_for(nc, kBlock)), dim3(kBlock), 0, as_stream(stream), ctok, craw, csent,
                     cptr, nc, n_sent, window, seed, static_cast<uint64_t>(epoch), nullptr, offs, n_pairs, in_ids, pred, centre);
  return launch_status();
}

extern "C" int lr_w2v_targets_i32(const int32_t* in_ids, const int32_t* pred, int64_t W, int64_t pair_base, int64_t n_items,
                                  const int64_t* cum, const int32_t* hs_ptr, const int32_t* hs_nodes, const int32_t* hs_codes,
                                  int64_t hs_len, uint64_t seed, int64_t epoch, const int64_t* offs, int32_t* lens,
                                  int64_t n_slots, int32_t* rows, int32_t* labels, int32_t* slot_in, lr_stream_t stream) {
  LR_CHECK_ARG(W >= 0 && pair_base >= 0 && n_items >= 1 && epoch >= 0 && hs_len >= 0 && n_slots >= 0);
  if (W == 0) return LR_OK;
  LR_CHECK_ARG(W < (int64_t{1} << 31) && pred && cum);
  LR_CHECK_ARG(hs_ptr == nullptr || hs_len == 0 || (hs_nodes && hs_codes));
  hipStream_t st = as_stream(stream);
  if (offs == nullptr) {                                    // count
    LR_CHECK_ARG(lens != nullptr);
    hipLaunchKernelGGL((w2v_targets_kernel<false>), dim3(grid_for(W, kBlock)), dim3(kBlock), 0, st, in_ids, pred, W, pair_base,
                       n_items, cum, hs_ptr, hs_nodes, hs_codes, hs_len, seed, static_cast<uint64_t>(epoch), offs, lens, n_slots,
                       rows, labels, slot_in);
  } else {                                                  // fill
    LR_CHECK_ARG(in_ids && rows && labels && slot_in);
    hipLaunchKernelGGL((w2v_targets_kernel<true>), dim3(grid_for(W, kBlock)), dim3(kBlock), 0, st, in_ids, pred, W, pair_base,
                       n_items, cum, hs_ptr, hs_nodes, hs_codes, hs_len, seed, static_cast<uint64_t>(epoch), offs, lens, n_slots,
                       rows, labels, slot_in);
  }
  return launch_status();
}

extern "C" int lr_w2v_score_f32(const float* syn0, int64_t n_items, const float* syn1, int64_t V1, int D, const int32_t* in_ids,
                                const int32_t* centre, int64_t W, const int64_t* offs, const int32_t* rows,
                                const int32_t* labels, int64_t n_slots, double pos0, double inv_total, float* g, float* stash,
                                float* loss, lr_stream_t stream) {
  LR_CHECK_ARG(W >= 0 && n_items >= 1 && V1 >= 1 && n_slots >= 0);
  if (!lr_w2v_supported(D)) return LR_ESHAPE;
  if (W == 0) return LR_OK;
  LR_CHECK_ARG(W < (int64_t{1} << 30) && n_slots < (int64_t{1} << 31));
  LR_CHECK_ARG(syn0 && syn1 && in_ids && centre && offs && rows && labels && g && stash);
  hipStream_t st = as_stream(stream);
#define LR_W2V_SCORE_CALL(G, R) \
  w2v_score_launch<G, R>(st, syn0, n_items, syn1, V1, D, in_ids, centre, W, offs, rows, labels, n_slots, pos0, inv_total, g, stash, loss)
  LR_ROW_GROUP_DISPATCH_256(D, LR_W2V_SCORE_CALL);
#undef LR_W2V_SCORE_CALL
}

extern "C" int lr_w2v_out_update_f32(float* table, int64_t V, int D, const int32_t* seg_pos, const int32_t* seg_rows,
                                     const int32_t* seg_start, const int32_t* n_seg, int64_t n, const float* g,
                                     const int32_t* slot_in, const float* other, int64_t other_rows, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && V >= 1);
  if (!lr_w2v_supported(D)) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(n < (int64_t{1} << 31));
  LR_CHECK_ARG(table && seg_pos && seg_rows && seg_start && n_seg && other && other_rows >= 1);
  LR_CHECK_ARG((g == nullptr) == (slot_in == nullptr));
  LR_CHECK_ARG(slot_in != nullptr || other_rows >= n);
  hipStream_t st = as_stream(stream);
#define LR_W2V_UPD(G, R) w2v_update_launch<G, R>(st, table, V, D, seg_pos, seg_rows, seg_start, n_seg, n, g, slot_in, other, other_rows)
  LR_ROW_GROUP_DISPATCH_256(D, LR_W2V_UPD);
#undef LR_W2V_UPD
}
