// GraphSage: the neighbour sampling and the tower of `libreco/algorithms/graphsage.py`, which the reference
// assembles batch by batch with Python's `random` and a chain of embedding_bag / cat / Linear calls per tree level.
//
// Sampling.  Every draw is H(seed, stream, a, b) of §7.9 (the same three rounds of mix64 as word2vec.hip), a pure function of
// the seed, the step and the draw's coordinates; an index below `len` is ((h >> 32) * len) >> 32.  Streams:
//   16 kSgNeighbor  a = step * 8 + level,  b = ((node * 16 + slot) * 16 + attempt) * 2 + half   (half 0: the consumer, 1: the item)
//   17 kSgWalk      a = step,              b = (((start * num_walks + walk) * walk_len) + s) * 2 + half
//   18 kSgStart     a = step,              b = index of the start node
//   19 kSgNegative  a = step,              b = (i * num_neg + k) * 16 + attempt
//   20 kSgDropout   a = step,              b = (((node * 128 + column) * 2 + role) * 4 + level) * 4 + layer   (role 0: the node
//                                              itself, 1: the node as a neighbour)
//   sg_neighbors_kernel  one thread per node of a level: `num_neighbors` slots by the retry ladder of `bipartite_neighbors`
//   sg_pairs_kernel      count / emit of the (item, positive) pairs of `pairs_from_random_walk`, one thread per (start, walk)
//   sg_starts_kernel     start nodes, uniform or from a cumulative table scaled to 2^32
//   sg_negatives_kernel  the i2i negatives (random, popular, out-batch) with the bounded retries of `sampling/negatives.py`
//   sg_dropout_kernel    the keep flags of one (layer, level, role), for the composed path and the tests
//
// The tower.  A tree has levels 0 .. L of n^k nodes; node i of level k has the children i n .. i n + n - 1 of level k + 1.  A
// node's input is T slots (row of the stacked table, scale); h_0 = proj(concat(scale * row)), and layer l gives
// h_{l+1}[v] = act(W_l [drop(h_l[v]) ; mean_children drop(h_l[child])] + b_l) for the nodes of levels 0 .. L - l - 1.
//   sg_fwd_kernel     a workgroup owns TB trees.  Slot by slot the rows go through LDS once (coalesced gather, broadcast reads)
//                     into the projection; the activations of every layer stay in LDS; only repr [B, K] goes to HBM.  Every
//                     output element is ONE fmaf chain (bias, then inputs ascending) whoever computes it, so a target has the
//                     same bits alone and inside any batch.
//   sg_bwd_kernel     recomputes a tile's activations (nothing but repr is saved), then walks the layers down: per layer the
//                     parameter-gradient partial of the tile (tree, node ascending), the gradient of the layer's input, at the
//                     end the projection's partial and the slot-row gradients (already times the slot's scale).  Workgroup w
//                     owns the tiles w, w + grid, ... and ONE slab of partials, which it alone reads and writes.
//   sg_reduce_kernel  adds the slabs in order.  No float atomics: same bits from run to run.
// Weights are stored transposed ([input][output]) so that the lanes of a wave, which differ in the output column, read
// consecutive floats.  A row id outside [0, V) is never dereferenced: a zero input row with a gradient of exactly 0.
#include <math.h>

#include "common.hpp"
#include "mix64.hpp"

namespace lr {

constexpr uint64_t kSgGold = 0x9e3779b97f4a7c15ull;
enum : uint64_t { kSgNeighbor = 16, kSgWalk = 17, kSgStart = 18, kSgNegative = 19, kSgDropout = 20 };
constexpr int kSgMaxK = 64, kSgMaxT = 16, kSgMaxL = 3, kSgMaxN = 10, kSgMaxLeaves = 100;
constexpr int kSgMaxTB = 64;
constexpr int kSgMaxSlabs = 256;
constexpr int64_t kSgMaxWsFloats = int64_t{1} << 25;
constexpr size_t kSgLdsSoft = 48 * 1024, kSgLdsHard = 96 * 1024;
constexpr int kSgTolerance = 5, kSgNegTries = 10;

__host__ __device__ inline uint64_t sg_hash(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b) {
  uint64_t z = mix64(seed + kSgGold * stream);
  z = mix64(z + kSgGold * (a + 1));
  return mix64(z + kSgGold * (b + 1));
}
__host__ __device__ inline int64_t sg_below(uint64_t h, int64_t len) {
  return static_cast<int64_t>(((h >> 32) * static_cast<uint64_t>(len)) >> 32);
}

// ---- sampling --------------------------------------------------------------------------------
struct SgGraph {
  const int64_t* iptr;     // [n_items + 1]: the consumers of an item
  const int32_t* iidx;
  const int64_t* uptr;     // [n_users + 1]: the items of a user
  const int32_t* uidx;
  int64_t n_items, n_users, n_iidx, n_uidx;
};

// item -> uniform consumer -> uniform item of that consumer.  An item nobody consumed, or a broken list, returns `item`.
__device__ __forceinline__ int32_t sg_one_walk(const SgGraph& g, int32_t item, uint64_t seed, uint64_t stream, uint64_t a,
                                               uint64_t b2) {
  if (item < 0 || item >= g.n_items) return item;
  const int64_t lo = g.iptr[item], hi = g.iptr[item + 1];
  if (lo < 0 || hi > g.n_iidx || hi <= lo) return item;
  const int32_t u = g.iidx[lo + sg_below(sg_hash(seed, stream, a, b2), hi - lo)];
  if (u < 0 || u >= g.n_users) return item;
  const int64_t ulo = g.uptr[u], uhi = g.uptr[u + 1];
  if (ulo < 0 || uhi > g.n_uidx || uhi <= ulo) return item;
  const int32_t nxt = g.uidx[ulo + sg_below(sg_hash(seed, stream, a, b2 + 1), uhi - ulo)];
  return (nxt >= 0 && nxt < g.n_items) ? nxt : item;
}

__global__ __launch_bounds__(kBlock) void sg_neighbors_kernel(SgGraph g, const int32_t* __restrict__ nodes, int64_t n_nodes,
                                                              int nn, uint64_t seed, uint64_t a, int32_t* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n_nodes; i += stride) {
    const int32_t node = nodes[i];
    int32_t got[kSgMaxN];
    for (int j = 0; j < nn; ++j) {
      const uint64_t base = (static_cast<uint64_t>(i) * 16 + j) * 16;
      auto draw = [&](int attempt) { return sg_one_walk(g, node, seed, kSgNeighbor, a, (base + attempt) * 2); };
      auto taken = [&](int32_t x) {
        bool t = false;
        for (int q = 0; q < j; ++q) t = t || got[q] == x;
        return t;
      };
      int32_t x = draw(0);
      if (x == node || taken(x)) {
        bool success = false;
        for (int t = 1; t <= kSgTolerance && !success; ++t) {
          x = draw(t);
          success = x != node && !taken(x);
        }
        for (int t = 1; t <= kSgTolerance && !success; ++t) {
          x = draw(kSgTolerance + t);
          success = x != node;
        }
        if (!success) x = draw(2 * kSgTolerance + 1);
      }
      got[j] = x;
      out[i * nn + j] = x;
    }
  }
}

// every consumer of `item` holds one item only
__device__ __forceinline__ bool sg_no_neighbor(const SgGraph& g, int32_t item) {
  if (item < 0 || item >= g.n_items) return true;
  const int64_t lo = g.iptr[item], hi = g.iptr[item + 1];
  if (lo < 0 || hi > g.n_iidx) return true;
  for (int64_t e = lo; e < hi; ++e) {
    const int32_t u = g.iidx[e];
    if (u >= 0 && u < g.n_users && g.uptr[u + 1] - g.uptr[u] > 1) return false;
  }
  return true;
}

template <bool EMIT>
__global__ __launch_bounds__(kBlock) void sg_pairs_kernel(SgGraph g, const int32_t* __restrict__ starts, int64_t n_starts,
                                                          int num_walks, int walk_len, int focus_start, uint64_t seed,
                                                          uint64_t step, int32_t* __restrict__ counts,
                                                          const int64_t* __restrict__ offs, int64_t n_pairs,
                                                          int32_t* __restrict__ items, int32_t* __restrict__ items_pos) {
  const int64_t total = n_starts * num_walks;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; w < total; w += stride) {
    const int32_t node = starts[w / num_walks];
    int64_t o = EMIT ? offs[w] : 0;
    int cnt = 0;
    auto emit = [&](int32_t x, int32_t y) {
      if (EMIT && o >= 0 && o < n_pairs) {
        items[o] = x;
        items_pos[o] = y;
      }
      ++o;
      ++cnt;
    };
    if (w % num_walks == 0 && sg_no_neighbor(g, node)) emit(node, node);
    int32_t cur = node;
    for (int s = 0; s < walk_len; ++s) {
      const int32_t nxt = sg_one_walk(g, cur, seed, kSgWalk, step, (static_cast<uint64_t>(w) * walk_len + s) * 2);
      if (focus_start) {
        if (nxt != node) emit(node, nxt);
      } else if (nxt != cur) {
        emit(cur, nxt);
      }
      cur = nxt;
    }
    if (!EMIT) counts[w] = cnt;
  }
}

// the first entry of the cumulative table that exceeds r
__device__ __forceinline__ int64_t sg_table_pick(const int64_t* __restrict__ cum, int64_t n, int64_t r) {
  int64_t a = 0, b = n;
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (cum[mid] > r) b = mid; else a = mid + 1;
  }
  return a < n ? a : n - 1;
}

__global__ __launch_bounds__(kBlock) void sg_starts_kernel(int64_t n, int64_t n_items, const int64_t* __restrict__ cum,
                                                           uint64_t seed, uint64_t step, int32_t* __restrict__ out) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t h = sg_hash(seed, kSgStart, step, static_cast<uint64_t>(i));
    out[i] = static_cast<int32_t>(cum != nullptr ? sg_table_pick(cum, n_items, static_cast<int64_t>(h >> 32)) : sg_below(h, n_items));
  }
}

// mode 0 random, 1 popular (`cum`), 2 out-batch (`in_batch` [n_items] flags)
__global__ __launch_bounds__(kBlock) void sg_negatives_kernel(const int32_t* __restrict__ items, const int32_t* __restrict__ items_pos,
                                                              int64_t n, int num_neg, int64_t n_items, int mode,
                                                              const int64_t* __restrict__ cum, const uint8_t* __restrict__ in_batch,
                                                              uint64_t seed, uint64_t step, int32_t* __restrict__ out) {
  const int64_t total = n * num_neg;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < total; q += stride) {
    const int64_t i = q / num_neg;
    const int32_t pos = items_pos[i], it = items != nullptr ? items[i] : -1;
    const int tries = mode == 1 ? 1 : kSgNegTries;
    int64_t d = 0;
    for (int t = 0; t <= tries; ++t) {
      const uint64_t h = sg_hash(seed, kSgNegative, step, static_cast<uint64_t>(q) * 16 + t);
      d = mode == 1 ? sg_table_pick(cum, n_items, static_cast<int64_t>(h >> 32)) : sg_below(h, n_items);
      const bool invalid = mode == 2 ? in_batch[d] != 0 : (d == pos || d == it);
      if (!invalid) break;
    }
    out[q] = static_cast<int32_t>(d);
  }
}

__host__ __device__ inline uint64_t sg_drop_coord(int layer, int level, int role, uint64_t node, int col) {
  return (((node * 128 + static_cast<uint64_t>(col)) * 2 + static_cast<uint64_t>(role)) * 4 + static_cast<uint64_t>(level)) * 4 +
         static_cast<uint64_t>(layer);
}

__global__ __launch_bounds__(kBlock) void sg_dropout_kernel(int64_t n_nodes, int K, uint64_t thr, uint64_t seed, uint64_t step,
                                                            int layer, int level, int role, uint8_t* __restrict__ keep) {
  const int64_t total = n_nodes * K;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; e < total; e += stride) {
    const uint64_t h = sg_hash(seed, kSgDropout, step, sg_drop_coord(layer, level, role, static_cast<uint64_t>(e / K), static_cast<int>(e % K)));
    keep[e] = (h >> 32) >= thr ? 1 : 0;
  }
}

// ---- the tower -------------------------------------------------------------------------------
struct SgArgs {
  const float* table;      // [V, K]: the stacked tables
  int64_t V;
  const int32_t* rows;     // [B N, T], level-major: level k at node offset B lvl_off[k], tree b's nodes at b n^k
  const float* scale;      // [B N, T] or null (all 1)
  int64_t B;
  int K, T, L, n, KS;
  int N;                   // nodes of a tree
  int N1;                  // nodes with an output in layer 0: levels 0 .. L - 1
  int NH;                  // rows of a tree's activations over all layers
  int lvl_cnt[kSgMaxL + 1];
  int lvl_off[kSgMaxL + 2];
  int hoff[kSgMaxL + 1];   // row of layer l's activations inside a tree's image
  int64_t np;              // floats of the parameter pack
  uint64_t thr, seed, step;
  float inv_keep;
  int drop;                // 1: dropout is drawn
};

__host__ __device__ inline int64_t sg_layer_off(int l, int K, int T) {
  return static_cast<int64_t>(T) * K * K + K + static_cast<int64_t>(l) * (2 * K * K + K);
}

__device__ __forceinline__ int sg_level_of(const SgArgs& a, int v) {
  int k = 0;
  while (k < a.L && v >= a.lvl_off[k + 1]) ++k;
  return k;
}
// index of node v of tree b inside its level, and the node's position in the level-major arrays
__device__ __forceinline__ int64_t sg_node_in_level(const SgArgs& a, int64_t b, int v, int k) {
  return b * a.lvl_cnt[k] + (v - a.lvl_off[k]);
}
__device__ __forceinline__ float sg_drop(const SgArgs& a, float x, int layer, int level, int role, int64_t node, int col) {
  if (!a.drop) return x;
  const uint64_t h = sg_hash(a.seed, kSgDropout, a.step, sg_drop_coord(layer, level, role, static_cast<uint64_t>(node), col));
  return (h >> 32) >= a.thr ? x * a.inv_keep : 0.f;
}
__device__ __forceinline__ bool sg_kept(const SgArgs& a, int layer, int level, int role, int64_t node, int col) {
  if (!a.drop) return true;
  const uint64_t h = sg_hash(a.seed, kSgDropout, a.step, sg_drop_coord(layer, level, role, static_cast<uint64_t>(node), col));
  return (h >> 32) >= a.thr;
}

extern __shared__ float sg_lds[];

// xs[row][c] = scale * table[rows[node, t]][c] for the nt * N nodes of the tile (0 for a row id outside the table)
__device__ __forceinline__ void sg_stage_slot(const SgArgs& a, int64_t b0, int nt, int t, float* __restrict__ xs) {
  const int K = a.K, N = a.N;
  for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
    const int row = idx / K, c = idx - row * K;
    const int s = row / N, v = row - s * N;
    const int k = sg_level_of(a, v);
    const int64_t g = a.B * a.lvl_off[k] + sg_node_in_level(a, b0 + s, v, k);
    const int64_t r = a.rows[g * a.T + t];
    float x = 0.f;
    if (r >= 0 && r < a.V) {
      x = a.table[r * K + c];
      if (a.scale != nullptr) x *= a.scale[g * a.T + t];
    }
    xs[row * a.KS + c] = x;
  }
}

// Z[((s N1 + v) 2 + half) KS + c] of layer l from its input activations Hl (rows s * NH + v)
__device__ __forceinline__ void sg_build_z(const SgArgs& a, int64_t b0, int nt, int l, const float* __restrict__ Hl,
                                           float* __restrict__ Z) {
  const int K = a.K, KS = a.KS, n = a.n;
  const int nout = a.lvl_off[a.L - l];
  for (int idx = threadIdx.x; idx < nt * nout * K; idx += kBlock) {
    const int row = idx / K, c = idx - row * K;
    const int s = row / nout, v = row - s * nout;
    const int k = sg_level_of(a, v);
    const int64_t node = sg_node_in_level(a, b0 + s, v, k);
    const float* ht = Hl + static_cast<int64_t>(s) * a.NH * KS;
    const float zs = sg_drop(a, ht[v * KS + c], l, k, 0, node, c);
    const int i = v - a.lvl_off[k];
    float sum = 0.f;
    for (int q = 0; q < n; ++q) {
      const int child = a.lvl_off[k + 1] + i * n + q;
      sum += sg_drop(a, ht[child * KS + c], l, k + 1, 1, node * n + q, c);
    }
    float* z = Z + (static_cast<int64_t>(s) * a.N1 + v) * 2 * KS;
    z[c] = zs;
    z[KS + c] = sum / static_cast<float>(n);
  }
}

// The activations of every layer of the tile's trees: H[(s NH + hoff[l] + v) KS + c].  `xs` [TB N][KS] and `Z` are scratch.
__device__ __forceinline__ void sg_forward_tile(const SgArgs& a, const float* __restrict__ params, int64_t b0, int nt,
                                                float* __restrict__ H, float* __restrict__ xs, float* __restrict__ Z) {
  const int K = a.K, KS = a.KS, N = a.N, T = a.T;
  const float* bp = params + static_cast<int64_t>(T) * K * K;
  for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
    const int row = idx / K, j = idx - row * K;
    const int s = row / N, v = row - s * N;
    H[(static_cast<int64_t>(s) * a.NH + v) * KS + j] = bp[j];
  }
  for (int t = 0; t < T; ++t) {
    sg_stage_slot(a, b0, nt, t, xs);
    __syncthreads();
    const float* Wt = params + static_cast<int64_t>(t) * K * K;
    for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
      const int row = idx / K, j = idx - row * K;
      const int s = row / N, v = row - s * N;
      float* h = H + (static_cast<int64_t>(s) * a.NH + v) * KS + j;
      const float* x = xs + row * KS;
      float acc = *h;
      for (int c = 0; c < K; ++c) acc = fmaf(x[c], Wt[c * K + j], acc);
      *h = acc;
    }
    __syncthreads();
  }
  for (int l = 0; l < a.L; ++l) {
    const float* Hl = H + a.hoff[l] * KS;
    float* Hn = H + a.hoff[l + 1] * KS;
    sg_build_z(a, b0, nt, l, Hl, Z);
    __syncthreads();
    const float* Wt = params + sg_layer_off(l, K, T);
    const float* bl = Wt + 2 * K * K;
    const int nout = a.lvl_off[a.L - l];
    const bool relu = l + 1 < a.L;
    for (int idx = threadIdx.x; idx < nt * nout * K; idx += kBlock) {
      const int row = idx / K, j = idx - row * K;
      const int s = row / nout, v = row - s * nout;
      const float* z = Z + (static_cast<int64_t>(s) * a.N1 + v) * 2 * KS;
      float acc = bl[j];
      for (int c = 0; c < K; ++c) acc = fmaf(z[c], Wt[c * K + j], acc);
      for (int c = 0; c < K; ++c) acc = fmaf(z[KS + c], Wt[(K + c) * K + j], acc);
      Hn[(static_cast<int64_t>(s) * a.NH + v) * KS + j] = (relu && !(acc > 0.f)) ? 0.f : acc;
    }
    __syncthreads();
  }
}

// LDS: H [TB NH][KS] | xs [TB N][KS] | Z [TB N1 2][KS]
__global__ __launch_bounds__(kBlock) void sg_fwd_kernel(SgArgs a, const float* __restrict__ params, int TB,
                                                        float* __restrict__ repr) {
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB;
  const int nt = static_cast<int>(a.B - b0 < TB ? a.B - b0 : TB);
  float* H = sg_lds;
  float* xs = H + static_cast<int64_t>(TB) * a.NH * a.KS;
  float* Z = xs + static_cast<int64_t>(TB) * a.N * a.KS;
  sg_forward_tile(a, params, b0, nt, H, xs, Z);
  const float* top = H + a.hoff[a.L] * a.KS;
  for (int idx = threadIdx.x; idx < nt * a.K; idx += kBlock) {
    const int s = idx / a.K, j = idx - s * a.K;
    repr[(b0 + s) * a.K + j] = top[static_cast<int64_t>(s) * a.NH * a.KS + j];
  }
}

// LDS: H [TB NH][KS] | gA [TB N][KS] | gB [TB N1'][KS] | Z [TB N1 2][KS]   (N1' = max(N1, 1))
// The gradient of layer l's activations lives in gA for even l and in gB for odd l, rows (s * N + v) and (s * N1' + v).
__global__ __launch_bounds__(kBlock) void sg_bwd_kernel(SgArgs a, const float* __restrict__ params, int TB, int64_t n_tiles,
                                                        const float* __restrict__ grepr, float* __restrict__ grow,
                                                        float* __restrict__ part, uint8_t* __restrict__ relu_out) {
  const int K = a.K, KS = a.KS, N = a.N, T = a.T, L = a.L, NH = a.NH, n = a.n;
  const int NB = a.N1 > 0 ? a.N1 : 1;
  float* H = sg_lds;
  float* gA = H + static_cast<int64_t>(TB) * NH * KS;
  float* gB = gA + static_cast<int64_t>(TB) * N * KS;
  float* Z = gB + static_cast<int64_t>(TB) * NB * KS;
  float* slab = part + static_cast<int64_t>(blockIdx.x) * a.np;
  const int tid = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool first = tile == static_cast<int64_t>(blockIdx.x);
    const int64_t b0 = tile * TB;
    const int nt = static_cast<int>(a.B - b0 < TB ? a.B - b0 : TB);
    sg_forward_tile(a, params, b0, nt, H, gA, Z);
    float* gtop = (L & 1) ? gB : gA;
    const int top_stride = (L & 1) ? NB : N;
    for (int idx = tid; idx < nt * K; idx += kBlock) {
      const int s = idx / K, j = idx - s * K;
      gtop[static_cast<int64_t>(s) * top_stride * KS + j] = grepr[(b0 + s) * K + j];
    }
    __syncthreads();
    int64_t relu_base = 0;                                    // rows of relu_out before layer l
    for (int l = L - 1; l >= 0; --l) {
      float* gout = ((l + 1) & 1) ? gB : gA;
      float* gin = (l & 1) ? gB : gA;
      const int so = ((l + 1) & 1) ? NB : N, si = (l & 1) ? NB : N;
      const int nout = a.lvl_off[L - l], nin = a.lvl_off[L - l + 1];
      const float* Hl = H + a.hoff[l] * KS;
      const float* Hn = H + a.hoff[l + 1] * KS;
      sg_build_z(a, b0, nt, l, Hl, Z);
      if (l + 1 < L) {                                        // the ReLU of this layer's output
        relu_base = 0;
        for (int q = 0; q < l; ++q) relu_base += a.B * a.lvl_off[L - q];
        for (int idx = tid; idx < nt * nout * K; idx += kBlock) {
          const int row = idx / K, j = idx - row * K;
          const int s = row / nout, v = row - s * nout;
          const bool on = Hn[(static_cast<int64_t>(s) * NH + v) * KS + j] > 0.f;
          float* g = gout + (static_cast<int64_t>(s) * so + v) * KS + j;
          if (!on) *g = 0.f;
          if (relu_out != nullptr) relu_out[(relu_base + (b0 + s) * nout + v) * K + j] = on ? 1 : 0;
        }
      }
      __syncthreads();
      // the layer's parameter gradients over the tile: trees ascending, nodes ascending
      const int64_t off = sg_layer_off(l, K, T);
      for (int e = tid; e < 2 * K * K + K; e += kBlock) {
        float acc = 0.f;
        if (e < 2 * K * K) {
          const int i = e / K, j = e - i * K;
          const int zo = i < K ? i : KS + (i - K);
          for (int s = 0; s < nt; ++s)
            for (int v = 0; v < nout; ++v)
              acc = fmaf(gout[(static_cast<int64_t>(s) * so + v) * KS + j], Z[(static_cast<int64_t>(s) * a.N1 + v) * 2 * KS + zo], acc);
        } else {
          const int j = e - 2 * K * K;
          for (int s = 0; s < nt; ++s)
            for (int v = 0; v < nout; ++v) acc += gout[(static_cast<int64_t>(s) * so + v) * KS + j];
        }
        slab[off + e] = first ? acc : slab[off + e] + acc;
      }
      __syncthreads();
      // GZ = W^T gout per output node, both halves, over Z
      const float* Wt = params + off;
      for (int idx = tid; idx < nt * nout * 2 * K; idx += kBlock) {
        const int row = idx / (2 * K), i = idx - row * (2 * K);
        const int s = row / nout, v = row - s * nout;
        const float* g = gout + (static_cast<int64_t>(s) * so + v) * KS;
        float acc = 0.f;
        for (int j = 0; j < K; ++j) acc = fmaf(g[j], Wt[i * K + j], acc);
        Z[(static_cast<int64_t>(s) * a.N1 + v) * 2 * KS + (i < K ? i : KS + (i - K))] = acc;
      }
      __syncthreads();
      // the gradient of the layer's input: the node's own part, then its part as a neighbour of its parent
      for (int idx = tid; idx < nt * nin * K; idx += kBlock) {
        const int row = idx / K, c = idx - row * K;
        const int s = row / nin, u = row - s * nin;
        const int k = sg_level_of(a, u);
        const int i = u - a.lvl_off[k];
        const int64_t node = sg_node_in_level(a, b0 + s, u, k);
        float val = 0.f;
        if (k < L - l) {
          const float gz = Z[(static_cast<int64_t>(s) * a.N1 + u) * 2 * KS + c];
          val = sg_kept(a, l, k, 0, node, c) ? (a.drop ? gz * a.inv_keep : gz) : 0.f;
        }
        if (k >= 1) {
          const int pv = a.lvl_off[k - 1] + i / n;
          const float gz = Z[(static_cast<int64_t>(s) * a.N1 + pv) * 2 * KS + KS + c] / static_cast<float>(n);
          val += sg_kept(a, l, k, 1, node, c) ? (a.drop ? gz * a.inv_keep : gz) : 0.f;
        }
        gin[(static_cast<int64_t>(s) * si + u) * KS + c] = val;
      }
      __syncthreads();
    }
    // the projection: g0 = gA [nt N rows]; the slot rows go through LDS again (over H, which is no longer needed)
    float* xs = H;
    for (int t = 0; t < T; ++t) {
      sg_stage_slot(a, b0, nt, t, xs);
      __syncthreads();
      const float* Wt = params + static_cast<int64_t>(t) * K * K;
      for (int e = tid; e < K * K + (t == 0 ? K : 0); e += kBlock) {
        float acc = 0.f;
        int64_t at;
        if (e < K * K) {
          const int c = e / K, j = e - c * K;
          for (int row = 0; row < nt * N; ++row) acc = fmaf(gA[row * KS + j], xs[row * KS + c], acc);
          at = static_cast<int64_t>(t) * K * K + e;
        } else {
          const int j = e - K * K;
          for (int row = 0; row < nt * N; ++row) acc += gA[row * KS + j];
          at = static_cast<int64_t>(T) * K * K + j;
        }
        slab[at] = first ? acc : slab[at] + acc;
      }
      for (int idx = tid; idx < nt * N * K; idx += kBlock) {
        const int row = idx / K, c = idx - row * K;
        const int s = row / N, v = row - s * N;
        const int k = sg_level_of(a, v);
        const int64_t g = a.B * a.lvl_off[k] + sg_node_in_level(a, b0 + s, v, k);
        const int64_t r = a.rows[g * T + t];
        float acc = 0.f;
        if (r >= 0 && r < a.V) {
          const float* gr = gA + row * KS;
          for (int j = 0; j < K; ++j) acc = fmaf(gr[j], Wt[c * K + j], acc);
          if (a.scale != nullptr) acc *= a.scale[g * T + t];
        }
        grow[(g * T + t) * K + c] = acc;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kBlock) void sg_reduce_kernel(const float* __restrict__ part, int n_slabs, int64_t np,
                                                           float* __restrict__ gparams) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= np) return;
  double t = 0.0;
  for (int s = 0; s < n_slabs; ++s) t += static_cast<double>(part[static_cast<int64_t>(s) * np + e]);
  gparams[e] = static_cast<float>(t);
}

// ---- host ------------------------------------------------------------------------------------
static inline bool sg_shape_ok(int K, int T, int L, int n) {
  if (K < 1 || K > kSgMaxK || T < 1 || T > kSgMaxT || L < 0 || L > kSgMaxL) return false;
  if (L == 0) return true;
  if (n < 1 || n > kSgMaxN) return false;
  int64_t leaves = 1;
  for (int l = 0; l < L; ++l) leaves *= n;
  return leaves <= kSgMaxLeaves;
}
static inline SgArgs sg_args(const float* table, int64_t V, const int32_t* rows, const float* scale, int64_t B, int K, int T,
                             int L, int n, double p, uint64_t seed, uint64_t step, int train) {
  SgArgs a{};
  a.table = table; a.V = V; a.rows = rows; a.scale = scale; a.B = B;
  a.K = K; a.T = T; a.L = L; a.n = L == 0 ? 1 : n;
  a.KS = K | 1;
  int cnt = 1, off = 0;
  for (int k = 0; k <= L; ++k) {
    a.lvl_cnt[k] = cnt;
    a.lvl_off[k] = off;
    off += cnt;
    cnt *= a.n;
  }
  a.lvl_off[L + 1] = off;
  a.N = off;
  a.N1 = a.lvl_off[L];
  int h = 0;
  for (int l = 0; l <= L; ++l) {
    a.hoff[l] = h;
    h += a.lvl_off[L - l + 1];
  }
  a.NH = h;
  a.np = sg_layer_off(L, K, T);
  a.drop = (train && p > 0.0) ? 1 : 0;
  a.thr = a.drop ? static_cast<uint64_t>(p * 4294967296.0) : 0;
  a.inv_keep = a.drop ? static_cast<float>(1.0 / (1.0 - p)) : 1.f;
  a.seed = seed; a.step = step;
  return a;
}
static inline size_t sg_fwd_lds(const SgArgs& a, int TB) {
  return static_cast<size_t>(TB) * (a.NH + a.N + 2 * a.N1) * a.KS * 4;
}
static inline size_t sg_bwd_lds(const SgArgs& a, int TB) {
  return static_cast<size_t>(TB) * (a.NH + a.N + (a.N1 > 0 ? a.N1 : 1) + 2 * a.N1) * a.KS * 4;
}
template <typename LdsOf>
static inline int sg_tb(const SgArgs& a, LdsOf lds_of) {
  int64_t tb = a.B / (2 * kNumCU);
  if (tb > kSgMaxTB) tb = kSgMaxTB;
  while (tb > 1 && lds_of(a, static_cast<int>(tb)) > kSgLdsSoft) --tb;
  return tb < 1 ? 1 : static_cast<int>(tb);
}
static inline int sg_slabs(const SgArgs& a) {
  const int TB = sg_tb(a, sg_bwd_lds);
  int64_t s = ceil_div(a.B > 0 ? a.B : 1, TB);
  const int64_t by_ws = kSgMaxWsFloats / a.np;
  if (s > by_ws) s = by_ws;
  if (s > kSgMaxSlabs) s = kSgMaxSlabs;
  return s < 1 ? 1 : static_cast<int>(s);
}
template <typename Kern>
static int sg_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  if (bytes > kSgLdsHard) return LR_ESHAPE;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}
static inline bool sg_graph_ok(const SgGraph& g) {
  return g.n_items >= 1 && g.n_users >= 1 && g.n_iidx >= 0 && g.n_uidx >= 0 && g.iptr && g.uptr && (g.iidx || g.n_iidx == 0) &&
         (g.uidx || g.n_uidx == 0);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_sage_supported(int K, int T, int num_layers, int num_neighbors) {
  if (!sg_shape_ok(K, T, num_layers, num_neighbors)) return 0;
  const SgArgs a = sg_args(nullptr, 0, nullptr, nullptr, 1, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0);
  return sg_bwd_lds(a, 1) <= kSgLdsHard ? 1 : 0;
}

extern "C" size_t lr_sage_params_bytes(int K, int T, int num_layers) {
  if (K < 1 || K > kSgMaxK || T < 1 || T > kSgMaxT || num_layers < 0 || num_layers > kSgMaxL) return 0;
  return static_cast<size_t>(sg_layer_off(num_layers, K, T)) * sizeof(float);
}

extern "C" int lr_sage_bwd_slabs(int64_t B, int K, int T, int num_layers, int num_neighbors) {
  if (B < 0 || !lr_sage_supported(K, T, num_layers, num_neighbors)) return 0;
  return sg_slabs(sg_args(nullptr, 0, nullptr, nullptr, B, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0));
}

extern "C" size_t lr_sage_bwd_ws_bytes(int64_t B, int K, int T, int num_layers, int num_neighbors) {
  if (B < 0 || !lr_sage_supported(K, T, num_layers, num_neighbors)) return 0;
  const SgArgs a = sg_args(nullptr, 0, nullptr, nullptr, B, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0);
  return (static_cast<size_t>(a.np) * sg_slabs(a) * sizeof(float) + 255) / 256 * 256;
}

extern "C" int lr_sage_neighbors_i32(const int32_t* nodes, int64_t n_nodes, int num_neighbors, const int64_t* item_ptr,
                                     const int32_t* item_idx, int64_t n_items, int64_t n_item_idx, const int64_t* user_ptr,
                                     const int32_t* user_idx, int64_t n_users, int64_t n_user_idx, uint64_t seed, int64_t step,
                                     int level, int32_t* out, lr_stream_t stream) {
  const SgGraph g{item_ptr, item_idx, user_ptr, user_idx, n_items, n_users, n_item_idx, n_user_idx};
  LR_CHECK_ARG(n_nodes >= 0 && num_neighbors >= 1 && num_neighbors <= kSgMaxN && step >= 0 && level >= 0 && level < 8);
  LR_CHECK_ARG(sg_graph_ok(g));
  if (n_nodes == 0) return LR_OK;
  LR_CHECK_ARG(n_nodes * num_neighbors < (int64_t{1} << 31) && nodes && out);
  hipLaunchKernelGGL(sg_neighbors_kernel, dim3(grid_for(n_nodes, kBlock)), dim3(kBlock), 0, as_stream(stream), g, nodes, n_nodes,
                     num_neighbors, seed, static_cast<uint64_t>(step) * 8 + level, out);
  return launch_status();
}

extern "C" int lr_sage_pairs_i32(const int32_t* starts, int64_t n_starts, int num_walks, int walk_len, int focus_start,
                                 const int64_t* item_ptr, const int32_t* item_idx, int64_t n_items, int64_t n_item_idx,
                                 const int64_t* user_ptr, const int32_t* user_idx, int64_t n_users, int64_t n_user_idx,
                                 uint64_t seed, int64_t step, int32_t* counts, const int64_t* offs, int64_t n_pairs,
                                 int32_t* items, int32_t* items_pos, lr_stream_t stream) {
  const SgGraph g{item_ptr, item_idx, user_ptr, user_idx, n_items, n_users, n_item_idx, n_user_idx};
  LR_CHECK_ARG(n_starts >= 0 && num_walks >= 1 && walk_len >= 1 && step >= 0 && n_pairs >= 0 && sg_graph_ok(g));
  if (n_starts == 0) return LR_OK;
  LR_CHECK_ARG(n_starts * num_walks * walk_len < (int64_t{1} << 30) && starts);
  const int grid = grid_for(n_starts * num_walks, kBlock);
  if (offs == nullptr) {                                      // count
    LR_CHECK_ARG(counts != nullptr);
    hipLaunchKernelGGL((sg_pairs_kernel<false>), dim3(grid), dim3(kBlock), 0, as_stream(stream), g, starts, n_starts, num_walks,
                       walk_len, focus_start, seed, static_cast<uint64_t>(step), counts, offs, n_pairs, items, items_pos);
  } else {                                                    // emit
    if (n_pairs == 0) return LR_OK;
    LR_CHECK_ARG(items && items_pos);
    hipLaunchKernelGGL((sg_pairs_kernel<true>), dim3(grid), dim3(kBlock), 0, as_stream(stream), g, starts, n_starts, num_walks,
                       walk_len, focus_start, seed, static_cast<uint64_t>(step), counts, offs, n_pairs, items, items_pos);
  }
  return launch_status();
}

extern "C" int lr_sage_starts_i32(int64_t n, int64_t n_items, const int64_t* cum, uint64_t seed, int64_t step, int32_t* out,
                                  lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && n_items >= 1 && n_items < (int64_t{1} << 31) && step >= 0);
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(out != nullptr);
  hipLaunchKernelGGL(sg_starts_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, as_stream(stream), n, n_items, cum, seed,
                     static_cast<uint64_t>(step), out);
  return launch_status();
}

extern "C" int lr_sage_negatives_i32(const int32_t* items, const int32_t* items_pos, int64_t n, int num_neg, int64_t n_items,
                                     int mode, const int64_t* cum, const uint8_t* in_batch, uint64_t seed, int64_t step,
                                     int32_t* out, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && num_neg >= 1 && n_items >= 1 && n_items < (int64_t{1} << 31) && step >= 0 && mode >= 0 && mode <= 2);
  LR_CHECK_ARG((mode != 1 || cum != nullptr) && (mode != 2 || in_batch != nullptr));
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(n * num_neg < (int64_t{1} << 31) && items_pos && out);
  hipLaunchKernelGGL(sg_negatives_kernel, dim3(grid_for(n * num_neg, kBlock)), dim3(kBlock), 0, as_stream(stream), items, items_pos,
                     n, num_neg, n_items, mode, cum, in_batch, seed, static_cast<uint64_t>(step), out);
  return launch_status();
}

extern "C" int lr_sage_dropout_u8(int64_t n_nodes, int K, double p, uint64_t seed, int64_t step, int layer, int level, int role,
                                  uint8_t* keep, lr_stream_t stream) {
  LR_CHECK_ARG(n_nodes >= 0 && K >= 1 && K <= 128 && p >= 0.0 && p < 1.0 && step >= 0);
  LR_CHECK_ARG(layer >= 0 && layer < 4 && level >= 0 && level < 4 && (role == 0 || role == 1));
  if (n_nodes == 0) return LR_OK;
  LR_CHECK_ARG(keep != nullptr && n_nodes * K < (int64_t{1} << 40));
  hipLaunchKernelGGL(sg_dropout_kernel, dim3(grid_for(n_nodes * K, kBlock)), dim3(kBlock), 0, as_stream(stream), n_nodes, K,
                     static_cast<uint64_t>(p * 4294967296.0), seed, static_cast<uint64_t>(step), layer, level, role, keep);
  return launch_status();
}

extern "C" int lr_sage_fwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, int64_t B, int K, int T,
                               int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed,
                               int64_t step, int train, float* repr, lr_stream_t stream) {
  if (!lr_sage_supported(K, T, num_layers, num_neighbors)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && dropout >= 0.0 && dropout < 1.0 && step >= 0);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(rows && repr);
  const SgArgs a = sg_args(table, V, rows, scale, B, K, T, num_layers, num_neighbors, dropout, seed, static_cast<uint64_t>(step), train);
  LR_CHECK_ARG(B * a.N < (int64_t{1} << 31) / (T * K));
  const int TB = sg_tb(a, sg_fwd_lds);
  const size_t lds = sg_fwd_lds(a, TB);
  const int rc = sg_set_lds(sg_fwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(sg_fwd_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, as_stream(stream), a, params,
                     TB, repr);
  return launch_status();
}

extern "C" int lr_sage_bwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, int64_t B, int K, int T,
                               int num_layers, int num_neighbors, const float* params, double dropout, uint64_t seed,
                               int64_t step, const float* grepr, float* grow, float* gparams, uint8_t* relu_out, void* ws,
                               size_t ws_bytes, lr_stream_t stream) {
  if (!lr_sage_supported(K, T, num_layers, num_neighbors)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && gparams && ws && dropout >= 0.0 && dropout < 1.0 && step >= 0);
  if (ws_bytes < lr_sage_bwd_ws_bytes(B, K, T, num_layers, num_neighbors)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (rows && grepr && grow));
  const SgArgs a = sg_args(table, V, rows, scale, B, K, T, num_layers, num_neighbors, dropout, seed, static_cast<uint64_t>(step), 1);
  LR_CHECK_ARG(B * a.N < (int64_t{1} << 31) / (T * K));
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(ws);
  int ns = 0;
  if (B > 0) {
    const int TB = sg_tb(a, sg_bwd_lds);
    const size_t lds = sg_bwd_lds(a, TB);
    const int rc = sg_set_lds(sg_bwd_kernel, lds);
    if (rc != LR_OK) return rc;
    ns = sg_slabs(a);
    hipLaunchKernelGGL(sg_bwd_kernel, dim3(static_cast<unsigned>(ns)), dim3(kBlock), lds, st, a, params, TB, ceil_div(B, TB), grepr,
                       grow, part, relu_out);
  }
  hipLaunchKernelGGL(sg_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(a.np, kBlock))), dim3(kBlock), 0, st, part, ns, a.np, gparams);
  return launch_status();
}
