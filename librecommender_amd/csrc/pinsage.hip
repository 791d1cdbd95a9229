// PinSage: the importance-walk neighbour sampling and the tower of `libreco/algorithms/pinsage.py`
// (sampling/random_walks.py:74-154, graph/neighbor_walk.py:52-81, torch_modules/pinsage_module.py:59-96), which the reference
// assembles with Python's `random` per walk step and a chain of Linear / embedding_bag calls per tree level.
//
// Sampling.  Every draw is H(seed, stream, a, b) of §7.9 / §7.11 on the new stream
//   21 kPsWalk   a = step * 8 + level,  b = ((i * 64 + walk * walk_len + s) * 4 + kind)
// with i the node's index inside its level, s the step of the walk and kind 0 the consumer, 1 the item, 2 the continue draw
// (num_walks * walk_len <= 64).  Step 0 of a walk is always taken; before step s > 0 the walk continues iff
// hi32(H(kind 2)) >= floor(termination_prob * 2^32), compared in 64 bits (termination_prob >= 1: never, 0: always).
//   ps_neighbors_kernel  one thread per node of a level.  The visited items in ascending (walk, step) go to the thread's LDS
//                        segment; `remove_target_node` with the node itself, then (where the node is its tree's target and the
//                        tree carries an exclusion) with the excluded item; then the distinct items in first-visit order with
//                        their counts, and the `num_neighbors` highest counts, ties by first visit (Counter.most_common).  A
//                        node without a neighbour (`has_no_neighbor`, an unconsumed item, an id outside the graph) gives itself
//                        with count 1.  Unused slots: id -1, count 0.
//
// The tower.  Trees, slots and the level-major layout are those of sage.hip; `weights` [B (N - 1)] holds the importance weight
// of every node of the levels 1 .. L (position of the node in the level-major arrays minus B).  Layer l, for the nodes v of the
// levels k < L - l:
//   nb[c]  = drop(relu(Q h[c] + bq))            the children c of v; dropout role 1, layer l, level k + 1 of stream 20
//   agg    = sum_j w_j nb_j                      child order, one fma chain from 0; a child of weight 0 is skipped
//   z      = relu(W [h[v] ; agg] + bw)
//   h'[v]  = z / |z|                             |z|^2 one fma chain over the columns ascending; a norm of exactly 0 counts as 1
// and repr = G2 relu(G1 h[0] + b1).  Parameter pack: proj W^T [T K, K], b [K]; per layer Q^T [K, K], bq [K], W^T [2 K, K],
// bw [K]; head G1^T [K, K], b1 [K], G2^T [K, K].  num_layers = 0 is projection plus head (the u2i user tower).
//   ps_fwd_kernel     a workgroup owns TB trees; the activations of every layer stay in LDS; only repr [B, K] goes to HBM.
//                     Every output element is ONE fma chain (bias, then inputs ascending; f64 accumulator, rounded to f32 once)
//                     whoever computes it, and the norm is a fixed-order sum: a target has the same bits alone and in any batch.
//   ps_bwd_kernel     recomputes a tile's activations and norms, then the head and the layers downwards.  Through the
//                     normalisation g_z = (g - y (y.g)) / |z| with the same fixed-order dot product; the ReLU patterns are
//                     those of the recomputed activations.  Workgroup w owns the tiles w, w + grid, ... and ONE slab of
//                     partials; ps_reduce_kernel adds the slabs in order in f64.  No float atomics.
//   relu_out (optional): per layer l a block [B, n_l - 1, K] of the q flags (the nodes 1 .. n_l - 1 of a tree, n_l the nodes of
//                     the levels 0 .. L - l; 1 where Q h + bq > 0) and a block [B, m_l, K] of the w flags (m_l the nodes of the
//                     levels 0 .. L - l - 1); after the last layer the head's flags [B, K].
#include <math.h>

#include "common.hpp"
#include "mix64.hpp"

namespace lr {

constexpr uint64_t kPsGold = 0x9e3779b97f4a7c15ull;
enum : uint64_t { kPsWalk = 21, kPsDropout = 20 };
constexpr int kPsMaxK = 64, kPsMaxT = 16, kPsMaxL = 3, kPsMaxN = 10, kPsMaxLeaves = 100, kPsMaxVisits = 64;
constexpr int kPsMaxTB = 64;
constexpr int kPsMaxSlabs = 256;
constexpr int64_t kPsMaxWsFloats = int64_t{1} << 25;
constexpr size_t kPsLdsSoft = 48 * 1024, kPsLdsHard = 96 * 1024;
constexpr int kPsSampleBlock = 128;

__host__ __device__ inline uint64_t ps_hash(uint64_t seed, uint64_t stream, uint64_t a, uint64_t b) {
  uint64_t z = mix64(seed + kPsGold * stream);
  z = mix64(z + kPsGold * (a + 1));
  return mix64(z + kPsGold * (b + 1));
}
__host__ __device__ inline int64_t ps_below(uint64_t h, int64_t len) {
  return static_cast<int64_t>(((h >> 32) * static_cast<uint64_t>(len)) >> 32);
}

// ---- sampling --------------------------------------------------------------------------------
struct PsGraph {
  const int64_t* iptr;     // [n_items + 1]: the consumers of an item
  const int32_t* iidx;
  const int64_t* uptr;     // [n_users + 1]: the items of a user
  const int32_t* uidx;
  int64_t n_items, n_users, n_iidx, n_uidx;
};

// item -> uniform consumer (draw b2) -> uniform item of that consumer (draw b2 + 1); the one-walk rule of sage.hip
__device__ __forceinline__ int32_t ps_one_walk(const PsGraph& g, int32_t item, uint64_t seed, uint64_t a, uint64_t b2) {
  if (item < 0 || item >= g.n_items) return item;
  const int64_t lo = g.iptr[item], hi = g.iptr[item + 1];
  if (lo < 0 || hi > g.n_iidx || hi <= lo) return item;
  const int32_t u = g.iidx[lo + ps_below(ps_hash(seed, kPsWalk, a, b2), hi - lo)];
  if (u < 0 || u >= g.n_users) return item;
  const int64_t ulo = g.uptr[u], uhi = g.uptr[u + 1];
  if (ulo < 0 || uhi > g.n_uidx || uhi <= ulo) return item;
  const int32_t nxt = g.uidx[ulo + ps_below(ps_hash(seed, kPsWalk, a, b2 + 1), uhi - ulo)];
  return (nxt >= 0 && nxt < g.n_items) ? nxt : item;
}

// every consumer of `item` holds one item only
__device__ __forceinline__ bool ps_no_neighbor(const PsGraph& g, int32_t item) {
  if (item < 0 || item >= g.n_items) return true;
  const int64_t lo = g.iptr[item], hi = g.iptr[item + 1];
  if (lo < 0 || hi > g.n_iidx) return true;
  for (int64_t e = lo; e < hi; ++e) {
    const int32_t u = g.iidx[e];
    if (u >= 0 && u < g.n_users && g.uptr[u + 1] - g.uptr[u] > 1) return false;
  }
  return true;
}

// `remove_target_node` on the thread's segment v[e * kPsSampleBlock]: the new length
__device__ __forceinline__ int ps_remove(int32_t* v, int len, int32_t x) {
  int cnt = 0;
  for (int e = 0; e < len; ++e) cnt += v[e * kPsSampleBlock] == x ? 1 : 0;
  if (cnt == 0) return len;
  if (cnt == len) {
    v[0] = x;
    return 1;
  }
  int m = 0;
  for (int e = 0; e < len; ++e) {
    const int32_t y = v[e * kPsSampleBlock];
    if (y != x) v[(m++) * kPsSampleBlock] = y;
  }
  return m;
}

__global__ __launch_bounds__(kPsSampleBlock) void ps_neighbors_kernel(PsGraph g, const int32_t* __restrict__ nodes, int64_t n_nodes,
                                                                       int nn, int num_walks, int walk_len, uint64_t thr,
                                                                       const int32_t* __restrict__ tree_target,
                                                                       const int32_t* __restrict__ tree_exclude, int64_t n_trees,
                                                                       int64_t per_tree, uint64_t seed, uint64_t a,
                                                                       int32_t* __restrict__ ids, int32_t* __restrict__ counts) {
  __shared__ int32_t visits[kPsMaxVisits * kPsSampleBlock];
  __shared__ uint8_t cnts[kPsMaxVisits * kPsSampleBlock];
  int32_t* v = visits + threadIdx.x;
  uint8_t* c = cnts + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPsSampleBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kPsSampleBlock + threadIdx.x; i < n_nodes; i += stride) {
    const int32_t node = nodes[i];
    int32_t* oid = ids + i * nn;
    int32_t* ocn = counts + i * nn;
    for (int j = 0; j < nn; ++j) {
      oid[j] = -1;
      ocn[j] = 0;
    }
    if (ps_no_neighbor(g, node)) {
      oid[0] = node;
      ocn[0] = 1;
      continue;
    }
    int len = 0;
    for (int w = 0; w < num_walks; ++w) {
      int32_t cur = node;
      for (int s = 0; s < walk_len; ++s) {
        const uint64_t b = (static_cast<uint64_t>(i) * 64 + static_cast<uint64_t>(w * walk_len + s)) * 4;
        if (s > 0 && (ps_hash(seed, kPsWalk, a, b + 2) >> 32) < thr) break;
        cur = ps_one_walk(g, cur, seed, a, b);
        v[(len++) * kPsSampleBlock] = cur;
      }
    }
    len = ps_remove(v, len, node);
    if (tree_exclude != nullptr) {
      const int64_t t = i / per_tree;
      if (t < n_trees && tree_exclude[t] >= 0 && tree_target[t] == node) len = ps_remove(v, len, tree_exclude[t]);
    }
    // the distinct items in first-visit order (in place: m <= e) and their counts
    int m = 0;
    for (int e = 0; e < len; ++e) {
      const int32_t x = v[e * kPsSampleBlock];
      int at = 0;
      while (at < m && v[at * kPsSampleBlock] != x) ++at;
      if (at == m) {
        v[m * kPsSampleBlock] = x;
        c[m * kPsSampleBlock] = 1;
        ++m;
      } else {
        c[at * kPsSampleBlock] += 1;
      }
    }
    for (int j = 0; j < nn && j < m; ++j) {
      int best = -1, bc = 0;
      for (int e = 0; e < m; ++e) {
        const int ce = c[e * kPsSampleBlock];
        if (ce > bc) {
          bc = ce;
          best = e;
        }
      }
      oid[j] = v[best * kPsSampleBlock];
      ocn[j] = bc;
      c[best * kPsSampleBlock] = 0;
    }
  }
}

// ---- the tower -------------------------------------------------------------------------------
struct PsArgs {
  const float* table;      // [V, K]: the stacked tables
  int64_t V;
  const int32_t* rows;     // [B N, T], level-major: level k at node offset B lvl_off[k], tree b's nodes at b n^k
  const float* scale;      // [B N, T] or null (all 1)
  const float* weights;    // [B (N - 1)]: the nodes of the levels 1 .. L
  int64_t B;
  int K, T, L, n, KS;
  int N;                   // nodes of a tree
  int N1;                  // nodes with an output in layer 0: levels 0 .. L - 1
  int NH;                  // rows of a tree's activations over all layers
  int NN;                  // norms of a tree over all layers
  int NBS;                 // rows of a tree's neighbour buffer: max(N - 1, 1)
  int lvl_cnt[kPsMaxL + 1];
  int lvl_off[kPsMaxL + 2];
  int hoff[kPsMaxL + 1];   // row of layer l's activations inside a tree's image
  int noff[kPsMaxL + 1];   // first norm of layer l's output inside a tree's norms
  int64_t np;              // floats of the parameter pack
  uint64_t thr, seed, step;
  float inv_keep;
  int drop;                // 1: dropout is drawn
};

__host__ __device__ inline int64_t ps_layer_off(int l, int K, int T) {
  return static_cast<int64_t>(T) * K * K + K + static_cast<int64_t>(l) * (3 * K * K + 2 * K);
}

__device__ __forceinline__ int ps_level_of(const PsArgs& a, int v) {
  int k = 0;
  while (k < a.L && v >= a.lvl_off[k + 1]) ++k;
  return k;
}
// index of node v of tree b inside its level
__device__ __forceinline__ int64_t ps_node_in_level(const PsArgs& a, int64_t b, int v, int k) {
  return b * a.lvl_cnt[k] + (v - a.lvl_off[k]);
}
__device__ __forceinline__ bool ps_kept(const PsArgs& a, int layer, int level, int64_t node, int col) {
  if (!a.drop) return true;
  const uint64_t coord = (((static_cast<uint64_t>(node) * 128 + static_cast<uint64_t>(col)) * 2 + 1) * 4 + static_cast<uint64_t>(level)) * 4 +
                         static_cast<uint64_t>(layer);
  return (ps_hash(a.seed, kPsDropout, a.step, coord) >> 32) >= a.thr;
}
// the weight of node u >= 1 (level k) of tree b
__device__ __forceinline__ float ps_weight(const PsArgs& a, int64_t b, int u, int k) {
  return a.weights[a.B * (a.lvl_off[k] - 1) + ps_node_in_level(a, b, u, k)];
}

// Every chain of the tower accumulates in f64 (the product of two f32 values is exact there) and is rounded to f32 once, at its
// end: a slot-row gradient that is the residue of cancelling terms keeps its leading digits, which Adam's division by
// sqrt(v) + eps otherwise turns into a visible move of the row.
using ps_acc = double;
__device__ __forceinline__ ps_acc ps_fma(float a, float b, ps_acc c) { return fma(static_cast<ps_acc>(a), static_cast<ps_acc>(b), c); }

extern __shared__ float ps_lds[];

// xs[row][c] = scale * table[rows[node, t]][c] for the nt * N nodes of the tile (0 for a row id outside the table)
__device__ __forceinline__ void ps_stage_slot(const PsArgs& a, int64_t b0, int nt, int t, float* __restrict__ xs) {
  const int K = a.K, N = a.N;
  for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
    const int row = idx / K, c = idx - row * K;
    const int s = row / N, v = row - s * N;
    const int k = ps_level_of(a, v);
    const int64_t g = a.B * a.lvl_off[k] + ps_node_in_level(a, b0 + s, v, k);
    const int64_t r = a.rows[g * a.T + t];
    float x = 0.f;
    if (r >= 0 && r < a.V) {
      x = a.table[r * K + c];
      if (a.scale != nullptr) x *= a.scale[g * a.T + t];
    }
    xs[row * a.KS + c] = x;
  }
}

// NB[(s NBS + u - 1) KS + j] = drop(relu(Q Hl[u] + bq)) for the nodes u of the levels 1 .. L - l; `qflags` (or null) takes
// the sign of the pre-activation at its block's base
__device__ __forceinline__ void ps_build_nb(const PsArgs& a, const float* __restrict__ params, int64_t b0, int nt, int l,
                                            const float* __restrict__ Hl, float* __restrict__ NB, uint8_t* __restrict__ qflags) {
  const int K = a.K, KS = a.KS;
  const int nin = a.lvl_off[a.L - l + 1], nc = nin - 1;
  const float* Qt = params + ps_layer_off(l, K, a.T);
  const float* bq = Qt + K * K;
  for (int idx = threadIdx.x; idx < nt * nc * K; idx += kBlock) {
    const int row = idx / K, j = idx - row * K;
    const int s = row / nc, u = row - s * nc + 1;
    const float* h = Hl + (static_cast<int64_t>(s) * a.NH + u) * KS;
    ps_acc acc = bq[j];
    for (int c = 0; c < K; ++c) acc = ps_fma(h[c], Qt[c * K + j], acc);
    const float pre = static_cast<float>(acc);
    const bool on = pre > 0.f;
    if (qflags != nullptr) qflags[((b0 + s) * nc + (u - 1)) * K + j] = on ? 1 : 0;
    float x = on ? pre : 0.f;
    if (a.drop) {
      const int k = ps_level_of(a, u);
      x = ps_kept(a, l, k, ps_node_in_level(a, b0 + s, u, k), j) ? x * a.inv_keep : 0.f;
    }
    NB[(static_cast<int64_t>(s) * a.NBS + u - 1) * KS + j] = x;
  }
}

// AGG[(s N1 + v) KS + c] = sum over the children of v of weight * NB, child order, weight 0 skipped
__device__ __forceinline__ void ps_build_agg(const PsArgs& a, int64_t b0, int nt, int l, const float* __restrict__ NB,
                                             float* __restrict__ AGG) {
  const int K = a.K, KS = a.KS, n = a.n;
  const int nout = a.lvl_off[a.L - l];
  for (int idx = threadIdx.x; idx < nt * nout * K; idx += kBlock) {
    const int row = idx / K, c = idx - row * K;
    const int s = row / nout, v = row - s * nout;
    const int k = ps_level_of(a, v);
    const int i = v - a.lvl_off[k];
    ps_acc sum = 0.f;
    for (int q = 0; q < n; ++q) {
      const int child = a.lvl_off[k + 1] + i * n + q;
      const float w = ps_weight(a, b0 + s, child, k + 1);
      if (w != 0.f) sum = ps_fma(w, NB[(static_cast<int64_t>(s) * a.NBS + child - 1) * KS + c], sum);
    }
    AGG[(static_cast<int64_t>(s) * a.N1 + v) * KS + c] = sum;
  }
}

// The activations of every layer of the tile's trees, H[(s NH + hoff[l] + v) KS + c], and the norms NRM[s NN + noff[l] + v] of
// layer l's outputs.  `xs` [TB N][KS] is scratch; NB and AGG are left holding the last layer's values.
__device__ __forceinline__ void ps_forward_tile(const PsArgs& a, const float* __restrict__ params, int64_t b0, int nt,
                                                float* __restrict__ H, float* __restrict__ xs, float* __restrict__ NB,
                                                float* __restrict__ AGG, float* __restrict__ NRM) {
  const int K = a.K, KS = a.KS, N = a.N, T = a.T;
  const float* bp = params + static_cast<int64_t>(T) * K * K;
  for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
    const int row = idx / K, j = idx - row * K;
    const int s = row / N, v = row - s * N;
    H[(static_cast<int64_t>(s) * a.NH + v) * KS + j] = bp[j];
  }
  for (int t = 0; t < T; ++t) {
    ps_stage_slot(a, b0, nt, t, xs);
    __syncthreads();
    const float* Wt = params + static_cast<int64_t>(t) * K * K;
    for (int idx = threadIdx.x; idx < nt * N * K; idx += kBlock) {
      const int row = idx / K, j = idx - row * K;
      const int s = row / N, v = row - s * N;
      float* h = H + (static_cast<int64_t>(s) * a.NH + v) * KS + j;
      const float* x = xs + row * KS;
      ps_acc acc = *h;
      for (int c = 0; c < K; ++c) acc = ps_fma(x[c], Wt[c * K + j], acc);
      *h = acc;
    }
    __syncthreads();
  }
  for (int l = 0; l < a.L; ++l) {
    const float* Hl = H + a.hoff[l] * KS;
    float* Hn = H + a.hoff[l + 1] * KS;
    ps_build_nb(a, params, b0, nt, l, Hl, NB, nullptr);
    __syncthreads();
    ps_build_agg(a, b0, nt, l, NB, AGG);
    __syncthreads();
    const float* Wt = params + ps_layer_off(l, K, T) + K * K + K;
    const float* bw = Wt + 2 * K * K;
    const int nout = a.lvl_off[a.L - l];
    for (int idx = threadIdx.x; idx < nt * nout * K; idx += kBlock) {
      const int row = idx / K, j = idx - row * K;
      const int s = row / nout, v = row - s * nout;
      const float* h = Hl + (static_cast<int64_t>(s) * a.NH + v) * KS;
      const float* g = AGG + (static_cast<int64_t>(s) * a.N1 + v) * KS;
      ps_acc acc = bw[j];
      for (int c = 0; c < K; ++c) acc = ps_fma(h[c], Wt[c * K + j], acc);
      for (int c = 0; c < K; ++c) acc = ps_fma(g[c], Wt[(K + c) * K + j], acc);
      const float pre = static_cast<float>(acc);
      Hn[(static_cast<int64_t>(s) * a.NH + v) * KS + j] = pre > 0.f ? pre : 0.f;
    }
    __syncthreads();
    for (int row = threadIdx.x; row < nt * nout; row += kBlock) {
      const int s = row / nout, v = row - s * nout;
      const float* z = Hn + (static_cast<int64_t>(s) * a.NH + v) * KS;
      ps_acc ss = 0.f;
      for (int c = 0; c < K; ++c) ss = ps_fma(z[c], z[c], ss);
      const float nrm = static_cast<float>(sqrt(ss));
      NRM[s * a.NN + a.noff[l] + v] = nrm == 0.f ? 1.f : nrm;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nt * nout * K; idx += kBlock) {
      const int row = idx / K, j = idx - row * K;
      const int s = row / nout, v = row - s * nout;
      float* z = Hn + (static_cast<int64_t>(s) * a.NH + v) * KS + j;
      *z = *z / NRM[s * a.NN + a.noff[l] + v];
    }
    __syncthreads();
  }
}

// HT[(s 2) KS + j] = relu(G1 h[0] + b1) of the tile's trees (h[0]: the top activations)
__device__ __forceinline__ void ps_head_hidden(const PsArgs& a, const float* __restrict__ params, int nt, const float* __restrict__ H,
                                               float* __restrict__ HT) {
  const int K = a.K, KS = a.KS;
  const float* G1t = params + ps_layer_off(a.L, K, a.T);
  const float* b1 = G1t + K * K;
  const float* top = H + a.hoff[a.L] * KS;
  for (int idx = threadIdx.x; idx < nt * K; idx += kBlock) {
    const int s = idx / K, j = idx - s * K;
    const float* h = top + static_cast<int64_t>(s) * a.NH * KS;
    ps_acc acc = b1[j];
    for (int c = 0; c < K; ++c) acc = ps_fma(h[c], G1t[c * K + j], acc);
    const float pre = static_cast<float>(acc);
    HT[(static_cast<int64_t>(s) * 2) * KS + j] = pre > 0.f ? pre : 0.f;
  }
}

// LDS: H [TB NH][KS] | S [TB max(N, NBS + N1)][KS] (xs, then NB | AGG) | HT [TB 2][KS] | NRM [TB NN]
__global__ __launch_bounds__(kBlock) void ps_fwd_kernel(PsArgs a, const float* __restrict__ params, int TB, float* __restrict__ repr) {
  const int K = a.K, KS = a.KS;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB;
  const int nt = static_cast<int>(a.B - b0 < TB ? a.B - b0 : TB);
  const int srows = a.N > a.NBS + a.N1 ? a.N : a.NBS + a.N1;
  float* H = ps_lds;
  float* S = H + static_cast<int64_t>(TB) * a.NH * KS;
  float* NB = S;
  float* AGG = S + static_cast<int64_t>(TB) * a.NBS * KS;
  float* HT = S + static_cast<int64_t>(TB) * srows * KS;
  float* NRM = HT + static_cast<int64_t>(TB) * 2 * KS;
  ps_forward_tile(a, params, b0, nt, H, S, NB, AGG, NRM);
  ps_head_hidden(a, params, nt, H, HT);
  __syncthreads();
  const float* G2t = params + ps_layer_off(a.L, K, a.T) + K * K + K;
  for (int idx = threadIdx.x; idx < nt * K; idx += kBlock) {
    const int s = idx / K, j = idx - s * K;
    const float* t = HT + (static_cast<int64_t>(s) * 2) * KS;
    ps_acc acc = 0.f;
    for (int c = 0; c < K; ++c) acc = ps_fma(t[c], G2t[c * K + j], acc);
    repr[(b0 + s) * K + j] = acc;
  }
}

// LDS: H [TB NH][KS] | gA [TB N][KS] | gB [TB N1'][KS] | NB [TB NBS][KS] | AGG [TB N1'][KS] | HT [TB 2][KS] | NRM [TB NN] |
// DOT [TB N1']   (N1' = max(N1, 1)).  The gradient of layer l's activations lives in gA for even l and in gB for odd l.
__global__ __launch_bounds__(kBlock) void ps_bwd_kernel(PsArgs a, const float* __restrict__ params, int TB, int64_t n_tiles,
                                                        const float* __restrict__ grepr, float* __restrict__ grow,
                                                        float* __restrict__ part, uint8_t* __restrict__ relu_out) {
  const int K = a.K, KS = a.KS, N = a.N, T = a.T, L = a.L, NH = a.NH, n = a.n;
  const int NB1 = a.N1 > 0 ? a.N1 : 1;
  float* H = ps_lds;
  float* gA = H + static_cast<int64_t>(TB) * NH * KS;
  float* gB = gA + static_cast<int64_t>(TB) * N * KS;
  float* NB = gB + static_cast<int64_t>(TB) * NB1 * KS;
  float* AGG = NB + static_cast<int64_t>(TB) * a.NBS * KS;
  float* HT = AGG + static_cast<int64_t>(TB) * NB1 * KS;
  float* NRM = HT + static_cast<int64_t>(TB) * 2 * KS;
  float* DOT = NRM + static_cast<int64_t>(TB) * a.NN;
  float* slab = part + static_cast<int64_t>(blockIdx.x) * a.np;
  const int tid = threadIdx.x;
  // rows of relu_out before the head's flags
  int64_t head_base = 0;
  for (int q = 0; q < L; ++q) head_base += a.B * (a.lvl_off[L - q + 1] - 1 + a.lvl_off[L - q]);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool first = tile == static_cast<int64_t>(blockIdx.x);
    const int64_t b0 = tile * TB;
    const int nt = static_cast<int>(a.B - b0 < TB ? a.B - b0 : TB);
    ps_forward_tile(a, params, b0, nt, H, gA, NB, AGG, NRM);
    ps_head_hidden(a, params, nt, H, HT);
    for (int idx = tid; idx < nt * K; idx += kBlock) {
      const int s = idx / K, j = idx - s * K;
      HT[(static_cast<int64_t>(s) * 2 + 1) * KS + j] = grepr[(b0 + s) * K + j];
    }
    __syncthreads();
    // ---- the head: repr = G2 t, t = relu(G1 h + b1) ------------------------------------------
    const int64_t hoffp = ps_layer_off(L, K, T);
    const float* G1t = params + hoffp;
    const float* G2t = G1t + K * K + K;
    const float* top = H + a.hoff[L] * KS;
    for (int e = tid; e < K * K; e += kBlock) {                 // g G2^T[c][j] = sum_s t[c] grepr[j]
      const int c = e / K, j = e - c * K;
      ps_acc acc = 0.f;
      for (int s = 0; s < nt; ++s) acc = ps_fma(HT[(static_cast<int64_t>(s) * 2) * KS + c], HT[(static_cast<int64_t>(s) * 2 + 1) * KS + j], acc);
      const int64_t at = hoffp + K * K + K + e;
      slab[at] = first ? acc : slab[at] + acc;
    }
    __syncthreads();
    float* gtop = (L & 1) ? gB : gA;
    const int top_stride = (L & 1) ? NB1 : N;
    // g_pre[c] = (t[c] > 0) sum_j grepr[j] G2^T[c][j], into the row of the tree in DOT-free scratch: gtop's row 0 is still free
    for (int idx = tid; idx < nt * K; idx += kBlock) {
      const int s = idx / K, c = idx - s * K;
      const float* g = HT + (static_cast<int64_t>(s) * 2 + 1) * KS;
      const bool on = HT[(static_cast<int64_t>(s) * 2) * KS + c] > 0.f;
      ps_acc acc = 0.f;
      for (int j = 0; j < K; ++j) acc = ps_fma(g[j], G2t[c * K + j], acc);
      if (relu_out != nullptr) relu_out[(head_base + b0 + s) * K + c] = on ? 1 : 0;
      gtop[static_cast<int64_t>(s) * top_stride * KS + c] = on ? acc : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < nt * K; idx += kBlock) {          // g_pre moves beside t: grepr is no longer needed
      const int s = idx / K, c = idx - s * K;
      HT[(static_cast<int64_t>(s) * 2 + 1) * KS + c] = gtop[static_cast<int64_t>(s) * top_stride * KS + c];
    }
    __syncthreads();
    for (int e = tid; e < K * K + K; e += kBlock) {             // g G1^T[c][j] = sum_s h[c] g_pre[j]; g b1
      ps_acc acc = 0.f;
      if (e < K * K) {
        const int c = e / K, j = e - c * K;
        for (int s = 0; s < nt; ++s) acc = ps_fma(HT[(static_cast<int64_t>(s) * 2 + 1) * KS + j], top[static_cast<int64_t>(s) * NH * KS + c], acc);
      } else {
        const int j = e - K * K;
        for (int s = 0; s < nt; ++s) acc += HT[(static_cast<int64_t>(s) * 2 + 1) * KS + j];
      }
      slab[hoffp + e] = first ? acc : slab[hoffp + e] + acc;
    }
    for (int idx = tid; idx < nt * K; idx += kBlock) {          // g h[0]
      const int s = idx / K, c = idx - s * K;
      const float* g = HT + (static_cast<int64_t>(s) * 2 + 1) * KS;
      ps_acc acc = 0.f;
      for (int j = 0; j < K; ++j) acc = ps_fma(g[j], G1t[c * K + j], acc);
      gtop[static_cast<int64_t>(s) * top_stride * KS + c] = acc;
    }
    __syncthreads();
    // ---- the layers, downwards ---------------------------------------------------------------
    for (int l = L - 1; l >= 0; --l) {
      float* gout = ((l + 1) & 1) ? gB : gA;
      float* gin = (l & 1) ? gB : gA;
      const int so = ((l + 1) & 1) ? NB1 : N, si = (l & 1) ? NB1 : N;
      const int nout = a.lvl_off[L - l], nin = a.lvl_off[L - l + 1], nc = nin - 1;
      const float* Hl = H + a.hoff[l] * KS;
      const float* Hn = H + a.hoff[l + 1] * KS;
      int64_t qbase = 0;
      for (int q = 0; q < l; ++q) qbase += a.B * (a.lvl_off[L - q + 1] - 1 + a.lvl_off[L - q]);
      const int64_t wbase = qbase + a.B * nc;
      ps_build_nb(a, params, b0, nt, l, Hl, NB, relu_out != nullptr ? relu_out + qbase * K : nullptr);
      for (int row = tid; row < nt * nout; row += kBlock) {     // y . g
        const int s = row / nout, v = row - s * nout;
        const float* y = Hn + (static_cast<int64_t>(s) * NH + v) * KS;
        const float* g = gout + (static_cast<int64_t>(s) * so + v) * KS;
        ps_acc d = 0.f;
        for (int c = 0; c < K; ++c) d = ps_fma(y[c], g[c], d);
        DOT[s * NB1 + v] = d;
      }
      __syncthreads();
      ps_build_agg(a, b0, nt, l, NB, AGG);
      for (int idx = tid; idx < nt * nout * K; idx += kBlock) { // g_z = (g - y (y.g)) / |z| where z > 0
        const int row = idx / K, j = idx - row * K;
        const int s = row / nout, v = row - s * nout;
        const float y = Hn[(static_cast<int64_t>(s) * NH + v) * KS + j];
        float* g = gout + (static_cast<int64_t>(s) * so + v) * KS + j;
        const bool on = y > 0.f;
        if (relu_out != nullptr) relu_out[(wbase + (b0 + s) * nout + v) * K + j] = on ? 1 : 0;
        *g = on ? (*g - y * DOT[s * NB1 + v]) / NRM[s * a.NN + a.noff[l] + v] : 0.f;
      }
      __syncthreads();
      // W's and bw's gradients over the tile: trees ascending, nodes ascending
      const int64_t off = ps_layer_off(l, K, T);
      const int64_t woff = off + K * K + K;
      for (int e = tid; e < 2 * K * K + K; e += kBlock) {
        ps_acc acc = 0.f;
        if (e < 2 * K * K) {
          const int i = e / K, j = e - i * K;
          for (int s = 0; s < nt; ++s)
            for (int v = 0; v < nout; ++v) {
              const float x = i < K ? Hl[(static_cast<int64_t>(s) * NH + v) * KS + i] : AGG[(static_cast<int64_t>(s) * a.N1 + v) * KS + i - K];
              acc = ps_fma(gout[(static_cast<int64_t>(s) * so + v) * KS + j], x, acc);
            }
        } else {
          const int j = e - 2 * K * K;
          for (int s = 0; s < nt; ++s)
            for (int v = 0; v < nout; ++v) acc += gout[(static_cast<int64_t>(s) * so + v) * KS + j];
        }
        slab[woff + e] = first ? acc : slab[woff + e] + acc;
      }
      __syncthreads();
      // W^T g_z: the node's own half into gin, the aggregate's half over AGG
      const float* Wt = params + woff;
      for (int idx = tid; idx < nt * nout * 2 * K; idx += kBlock) {
        const int row = idx / (2 * K), i = idx - row * (2 * K);
        const int s = row / nout, v = row - s * nout;
        const float* g = gout + (static_cast<int64_t>(s) * so + v) * KS;
        ps_acc acc = 0.f;
        for (int j = 0; j < K; ++j) acc = ps_fma(g[j], Wt[i * K + j], acc);
        if (i < K) gin[(static_cast<int64_t>(s) * si + v) * KS + i] = acc;
        else AGG[(static_cast<int64_t>(s) * a.N1 + v) * KS + i - K] = acc;
      }
      __syncthreads();
      // g_q over NB: weight, dropout and the ReLU of the neighbour branch
      for (int idx = tid; idx < nt * nc * K; idx += kBlock) {
        const int row = idx / K, c = idx - row * K;
        const int s = row / nc, u = row - s * nc + 1;
        const int k = ps_level_of(a, u);
        const int pv = a.lvl_off[k - 1] + (u - a.lvl_off[k]) / n;
        const float w = ps_weight(a, b0 + s, u, k);
        float* x = NB + (static_cast<int64_t>(s) * a.NBS + u - 1) * KS + c;
        float g = 0.f;
        if (w != 0.f && *x > 0.f) {
          g = w * AGG[(static_cast<int64_t>(s) * a.N1 + pv) * KS + c];
          if (a.drop) g *= a.inv_keep;
        }
        *x = g;
      }
      __syncthreads();
      for (int e = tid; e < K * K + K; e += kBlock) {           // Q's and bq's gradients
        ps_acc acc = 0.f;
        if (e < K * K) {
          const int i = e / K, j = e - i * K;
          for (int s = 0; s < nt; ++s)
            for (int u = 1; u < nin; ++u)
              acc = ps_fma(NB[(static_cast<int64_t>(s) * a.NBS + u - 1) * KS + j], Hl[(static_cast<int64_t>(s) * NH + u) * KS + i], acc);
        } else {
          const int j = e - K * K;
          for (int s = 0; s < nt; ++s)
            for (int u = 1; u < nin; ++u) acc += NB[(static_cast<int64_t>(s) * a.NBS + u - 1) * KS + j];
        }
        slab[off + e] = first ? acc : slab[off + e] + acc;
      }
      // the gradient of the layer's input: the node's own part, then its part as a neighbour
      const float* Qt = params + off;
      for (int idx = tid; idx < nt * nin * K; idx += kBlock) {
        const int row = idx / K, c = idx - row * K;
        const int s = row / nin, u = row - s * nin;
        float* gi = gin + (static_cast<int64_t>(s) * si + u) * KS + c;
        float val = u < nout ? *gi : 0.f;
        if (u >= 1) {
          const float* g = NB + (static_cast<int64_t>(s) * a.NBS + u - 1) * KS;
          ps_acc acc = 0.f;
          for (int j = 0; j < K; ++j) acc = ps_fma(g[j], Qt[c * K + j], acc);
          val += acc;
        }
        *gi = val;
      }
      __syncthreads();
    }
    // the projection: g0 = gA [nt N rows]; the slot rows go through LDS again (over H, which is no longer needed)
    float* xs = H;
    for (int t = 0; t < T; ++t) {
      ps_stage_slot(a, b0, nt, t, xs);
      __syncthreads();
      const float* Wt = params + static_cast<int64_t>(t) * K * K;
      for (int e = tid; e < K * K + (t == 0 ? K : 0); e += kBlock) {
        ps_acc acc = 0.f;
        int64_t at;
        if (e < K * K) {
          const int c = e / K, j = e - c * K;
          for (int row = 0; row < nt * N; ++row) acc = ps_fma(gA[row * KS + j], xs[row * KS + c], acc);
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
        const int k = ps_level_of(a, v);
        const int64_t g = a.B * a.lvl_off[k] + ps_node_in_level(a, b0 + s, v, k);
        const int64_t r = a.rows[g * T + t];
        ps_acc acc = 0.f;
        if (r >= 0 && r < a.V) {
          const float* gr = gA + row * KS;
          for (int j = 0; j < K; ++j) acc = ps_fma(gr[j], Wt[c * K + j], acc);
          if (a.scale != nullptr) acc *= a.scale[g * T + t];
        }
        grow[(g * T + t) * K + c] = acc;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kBlock) void ps_reduce_kernel(const float* __restrict__ part, int n_slabs, int64_t np,
                                                           float* __restrict__ gparams) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= np) return;
  double t = 0.0;
  for (int s = 0; s < n_slabs; ++s) t += static_cast<double>(part[static_cast<int64_t>(s) * np + e]);
  gparams[e] = static_cast<float>(t);
}

// ---- host ------------------------------------------------------------------------------------
static inline bool ps_shape_ok(int K, int T, int L, int n) {
  if (K < 1 || K > kPsMaxK || T < 1 || T > kPsMaxT || L < 0 || L > kPsMaxL) return false;
  if (L == 0) return true;
  if (n < 1 || n > kPsMaxN) return false;
  int64_t leaves = 1;
  for (int l = 0; l < L; ++l) leaves *= n;
  return leaves <= kPsMaxLeaves;
}
static inline PsArgs ps_args(const float* table, int64_t V, const int32_t* rows, const float* scale, const float* weights, int64_t B,
                             int K, int T, int L, int n, double p, uint64_t seed, uint64_t step, int train) {
  PsArgs a{};
  a.table = table; a.V = V; a.rows = rows; a.scale = scale; a.weights = weights; a.B = B;
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
  a.NBS = a.N > 1 ? a.N - 1 : 1;
  int h = 0, nn = 0;
  for (int l = 0; l <= L; ++l) {
    a.hoff[l] = h;
    h += a.lvl_off[L - l + 1];
    a.noff[l] = nn;
    if (l < L) nn += a.lvl_off[L - l];
  }
  a.NH = h;
  a.NN = nn > 0 ? nn : 1;
  a.np = ps_layer_off(L, K, T) + 2 * K * K + K;
  a.drop = (train && p > 0.0) ? 1 : 0;
  a.thr = a.drop ? static_cast<uint64_t>(p * 4294967296.0) : 0;
  a.inv_keep = a.drop ? static_cast<float>(1.0 / (1.0 - p)) : 1.f;
  a.seed = seed; a.step = step;
  return a;
}
static inline size_t ps_fwd_lds(const PsArgs& a, int TB) {
  const int srows = a.N > a.NBS + a.N1 ? a.N : a.NBS + a.N1;
  return static_cast<size_t>(TB) * ((a.NH + srows + 2) * a.KS + a.NN) * 4;
}
static inline size_t ps_bwd_lds(const PsArgs& a, int TB) {
  const int nb1 = a.N1 > 0 ? a.N1 : 1;
  return static_cast<size_t>(TB) * ((a.NH + a.N + 2 * nb1 + a.NBS + 2) * a.KS + a.NN + nb1) * 4;
}
template <typename LdsOf>
static inline int ps_tb(const PsArgs& a, LdsOf lds_of) {
  int64_t tb = a.B / (2 * kNumCU);
  if (tb > kPsMaxTB) tb = kPsMaxTB;
  while (tb > 1 && lds_of(a, static_cast<int>(tb)) > kPsLdsSoft) --tb;
  return tb < 1 ? 1 : static_cast<int>(tb);
}
static inline int ps_slabs(const PsArgs& a) {
  const int TB = ps_tb(a, ps_bwd_lds);
  int64_t s = ceil_div(a.B > 0 ? a.B : 1, TB);
  const int64_t by_ws = kPsMaxWsFloats / a.np;
  if (s > by_ws) s = by_ws;
  if (s > kPsMaxSlabs) s = kPsMaxSlabs;
  return s < 1 ? 1 : static_cast<int>(s);
}
template <typename Kern>
static int ps_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  if (bytes > kPsLdsHard) return LR_ESHAPE;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}
static inline bool ps_graph_ok(const PsGraph& g) {
  return g.n_items >= 1 && g.n_users >= 1 && g.n_iidx >= 0 && g.n_uidx >= 0 && g.iptr && g.uptr && (g.iidx || g.n_iidx == 0) &&
         (g.uidx || g.n_uidx == 0);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_pinsage_supported(int K, int T, int num_layers, int num_neighbors) {
  if (!ps_shape_ok(K, T, num_layers, num_neighbors)) return 0;
  const PsArgs a = ps_args(nullptr, 0, nullptr, nullptr, nullptr, 1, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0);
  return ps_bwd_lds(a, 1) <= kPsLdsHard ? 1 : 0;
}

extern "C" size_t lr_pinsage_params_bytes(int K, int T, int num_layers) {
  if (K < 1 || K > kPsMaxK || T < 1 || T > kPsMaxT || num_layers < 0 || num_layers > kPsMaxL) return 0;
  return static_cast<size_t>(ps_layer_off(num_layers, K, T) + 2 * K * K + K) * sizeof(float);
}

extern "C" int lr_pinsage_bwd_slabs(int64_t B, int K, int T, int num_layers, int num_neighbors) {
  if (B < 0 || !lr_pinsage_supported(K, T, num_layers, num_neighbors)) return 0;
  return ps_slabs(ps_args(nullptr, 0, nullptr, nullptr, nullptr, B, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0));
}

extern "C" size_t lr_pinsage_bwd_ws_bytes(int64_t B, int K, int T, int num_layers, int num_neighbors) {
  if (B < 0 || !lr_pinsage_supported(K, T, num_layers, num_neighbors)) return 0;
  const PsArgs a = ps_args(nullptr, 0, nullptr, nullptr, nullptr, B, K, T, num_layers, num_neighbors, 0.0, 0, 0, 0);
  return (static_cast<size_t>(a.np) * ps_slabs(a) * sizeof(float) + 255) / 256 * 256;
}

extern "C" int lr_pinsage_neighbors_i32(const int32_t* nodes, int64_t n_nodes, int num_neighbors, int num_walks, int walk_len,
                                        double termination_prob, const int32_t* tree_target, const int32_t* tree_exclude,
                                        int64_t n_trees, const int64_t* item_ptr, const int32_t* item_idx, int64_t n_items,
                                        int64_t n_item_idx, const int64_t* user_ptr, const int32_t* user_idx, int64_t n_users,
                                        int64_t n_user_idx, uint64_t seed, int64_t step, int level, int32_t* ids, int32_t* counts,
                                        lr_stream_t stream) {
  const PsGraph g{item_ptr, item_idx, user_ptr, user_idx, n_items, n_users, n_item_idx, n_user_idx};
  if (num_neighbors < 1 || num_neighbors > kPsMaxN || num_walks < 1 || walk_len < 1 || num_walks > kPsMaxVisits ||
      walk_len > kPsMaxVisits || num_walks * walk_len > kPsMaxVisits)
    return LR_ESHAPE;
  LR_CHECK_ARG(n_nodes >= 0 && step >= 0 && level >= 0 && level < 8 && termination_prob == termination_prob);
  LR_CHECK_ARG(ps_graph_ok(g));
  int64_t per_tree = 1;
  for (int k = 0; k < level; ++k) per_tree *= num_neighbors;
  if (tree_exclude != nullptr) LR_CHECK_ARG(tree_target != nullptr && n_trees >= 0 && n_nodes == n_trees * per_tree);
  if (n_nodes == 0) return LR_OK;
  LR_CHECK_ARG(n_nodes * num_neighbors < (int64_t{1} << 31) && nodes && ids && counts);
  const uint64_t thr = termination_prob >= 1.0 ? (uint64_t{1} << 32)
                                               : (termination_prob <= 0.0 ? 0 : static_cast<uint64_t>(termination_prob * 4294967296.0));
  hipLaunchKernelGGL(ps_neighbors_kernel, dim3(grid_for(n_nodes, kPsSampleBlock)), dim3(kPsSampleBlock), 0, as_stream(stream), g, nodes,
                     n_nodes, num_neighbors, num_walks, walk_len, thr, tree_target, tree_exclude, n_trees, per_tree, seed,
                     static_cast<uint64_t>(step) * 8 + level, ids, counts);
  return launch_status();
}

extern "C" int lr_pinsage_fwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, const float* weights,
                                  int64_t B, int K, int T, int num_layers, int num_neighbors, const float* params, double dropout,
                                  uint64_t seed, int64_t step, int train, float* repr, lr_stream_t stream) {
  if (!lr_pinsage_supported(K, T, num_layers, num_neighbors)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && dropout >= 0.0 && dropout < 1.0 && step >= 0);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(rows && repr && (weights || num_layers == 0));
  const PsArgs a = ps_args(table, V, rows, scale, weights, B, K, T, num_layers, num_neighbors, dropout, seed,
                           static_cast<uint64_t>(step), train);
  LR_CHECK_ARG(B * a.N < (int64_t{1} << 31) / (T * K));
  const int TB = ps_tb(a, ps_fwd_lds);
  const size_t lds = ps_fwd_lds(a, TB);
  const int rc = ps_set_lds(ps_fwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(ps_fwd_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, as_stream(stream), a, params,
                     TB, repr);
  return launch_status();
}

extern "C" int lr_pinsage_bwd_f32(const float* table, int64_t V, const int32_t* rows, const float* scale, const float* weights,
                                  int64_t B, int K, int T, int num_layers, int num_neighbors, const float* params, double dropout,
                                  uint64_t seed, int64_t step, const float* grepr, float* grow, float* gparams, uint8_t* relu_out,
                                  void* ws, size_t ws_bytes, lr_stream_t stream) {
  if (!lr_pinsage_supported(K, T, num_layers, num_neighbors)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && gparams && ws && dropout >= 0.0 && dropout < 1.0 && step >= 0);
  if (ws_bytes < lr_pinsage_bwd_ws_bytes(B, K, T, num_layers, num_neighbors)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (rows && grepr && grow && (weights || num_layers == 0)));
  const PsArgs a = ps_args(table, V, rows, scale, weights, B, K, T, num_layers, num_neighbors, dropout, seed,
                           static_cast<uint64_t>(step), 1);
  LR_CHECK_ARG(B * a.N < (int64_t{1} << 31) / (T * K));
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(ws);
  int ns = 0;
  if (B > 0) {
    const int TB = ps_tb(a, ps_bwd_lds);
    const size_t lds = ps_bwd_lds(a, TB);
    const int rc = ps_set_lds(ps_bwd_kernel, lds);
    if (rc != LR_OK) return rc;
    ns = ps_slabs(a);
    hipLaunchKernelGGL(ps_bwd_kernel, dim3(static_cast<unsigned>(ns)), dim3(kBlock), lds, st, a, params, TB, ceil_div(B, TB), grepr,
                       grow, part, relu_out);
  }
  hipLaunchKernelGGL(ps_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(a.np, kBlock))), dim3(kBlock), 0, st, part, ns, a.np, gparams);
  return launch_status();
}
