// The user side of Caser (`libreco/algorithms/caser.py:177-221`): over the rows of a sequence table that a window's L ids
// name, L "horizontal" convolutions of kernel sizes 1 .. L (valid padding, ReLU, a global max over time) and one "vertical"
// convolution that mixes the L positions per embedding channel (ReLU), f32 on the VALU.
//   cs_fwd_kernel      one launch.  A workgroup owns TB samples; their rows go through the ids into LDS once ([sample][t][KS],
//                      KS = K rounded up to 4 with KS / 4 odd: the 16 lanes of a ds_read_b128 group then sit on 16 different
//                      16-byte slots).  A wave takes (kernel size i, tile of FT filters) items in turn; its lanes are the
//                      (sample, position) pairs of the tile, so the weights are wave-uniform (scalar loads from L2, an SGPR
//                      operand of the fma) and an input is one 16-byte LDS read per 4 FT fmas.  A position's value is ONE fmaf
//                      chain (bias, then tau ascending, c ascending) whatever lane computes it.  ReLU'd values go to a per-wave
//                      LDS scratch, then one lane per (sample, filter) walks t ascending and keeps the first maximum.  The
//                      vertical layer is one chain over t per (sample, c, g).  Only feat and arg go to HBM.
//   cs_bwd_x_kernel    gx in gather form per (sample, t, c): kernel sizes ascending, filters ascending (a unit takes part iff
//                      feat > 0 and arg <= t < arg + i), then the vertical filters ascending.
//   cs_wgrad_kernel    one thread per element of a slab's partial buffer (the parameter layout up to the vertical layer, then
//                      the vertical kernel and bias per channel c), summed over the slab's samples in ascending order;
//   cs_reduce_kernel   adds the slabs (and the channels of the vertical layer) in order.  No float atomics: same bits from
//                      run to run.
// An id outside [0, V) is never dereferenced: it is a zero input row and gets a gradient of exactly 0.
#include "common.hpp"

namespace lr {

constexpr int kCsMaxL = 64, kCsMaxK = 128, kCsMaxF = 64;   // L; K; nh and nv
constexpr int kCsMaxTB = 64;                               // samples per workgroup
constexpr int kCsWaves = kBlock / kWave;
constexpr int kCsMaxSlabs = 128;
constexpr int64_t kCsMaxWsFloats = int64_t{1} << 25;       // 128 MB of partials, unless one slab alone is larger
constexpr size_t kCsLdsSoft = 64 * 1024;
constexpr size_t kCsFwdLdsSoft = 32 * 1024;                // the forward: five workgroups per compute unit rather than larger tiles

struct CsArgs {
  const float* table;      // [V, K]
  int64_t V;
  const int32_t* ids;      // [B, L]
  int64_t B;
  int L, K, nh, nv;
  int KS;                  // LDS row stride
  int W;                   // L nh + K nv: the width of feat
  int64_t offV;            // offset of the vertical kernel in the parameter buffer
  int64_t np;              // length of the parameter buffer
  int64_t pp;              // length of one slab of partials: offV + L nv K + nv K
};

__host__ __device__ inline int64_t cs_pad4(int64_t n) { return (n + 3) / 4 * 4; }
// floats of horizontal layer i (kernel [i, K, nh], bias [nh], each on a 16-byte boundary)
__host__ __device__ inline int64_t cs_layer_floats(int i, int K, int nh) {
  return cs_pad4(static_cast<int64_t>(i) * K * nh) + cs_pad4(nh);
}
// offset of the kernel of horizontal layer i (1-based); i == L + 1: the vertical kernel
__host__ __device__ inline int64_t cs_kernel_off(int i, int K, int nh) {
  int64_t off = 0;
  for (int j = 1; j < i; ++j) off += cs_layer_floats(j, K, nh);
  return off;
}

__device__ __forceinline__ bool cs_id_ok(const CsArgs& a, int64_t at, int64_t* id) {
  const int64_t v = a.ids[at];
  *id = v;
  return v >= 0 && v < a.V;
}

extern __shared__ float cs_lds[];

// ---- forward ---------------------------------------------------------------------------------
// LDS: x [TB][L][KS] | scratch [kCsWaves][TB * L * FT]
template <int FT>
__global__ __launch_bounds__(kBlock) void cs_fwd_kernel(CsArgs a, const float* __restrict__ params, int TB,
                                                        float* __restrict__ feat, int32_t* __restrict__ arg) {
  const int L = a.L, K = a.K, nh = a.nh, nv = a.nv, KS = a.KS, W = a.W;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB;
  float* xs = cs_lds;
  float* scratch = cs_lds + TB * L * KS + wave * (TB * L * FT);
  for (int idx = tid; idx < TB * L * (KS / 4); idx += kBlock) {
    const int row = idx / (KS / 4), k = (idx - row * (KS / 4)) * 4;
    const int64_t b = b0 + row / L;
    int64_t id = 0;
    const bool ok = b < a.B && cs_id_ok(a, b0 * L + row, &id);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (ok && k + q < K) ? a.table[id * K + k + q] : 0.f;
    st4(xs + row * KS + k, make_float4(v[0], v[1], v[2], v[3]));
  }
  __syncthreads();
  const int nfg = (nh + FT - 1) / FT, n_items = L * nfg;
  const int per_round = kCsWaves * gridDim.y;                         // the workgroups of a tile (blockIdx.y) share its items
  const int n_rounds = (n_items + per_round - 1) / per_round;         // the same for every wave: the barriers below are uniform
  for (int round = 0; round < n_rounds; ++round) {
    const int item = (round * gridDim.y + blockIdx.y) * kCsWaves + wave;
    const bool live = item < n_items;
    const int i = live ? item % L + 1 : 1, fg = live ? item / L : 0;
    const int P = L - i + 1, R = TB * P, f0 = fg * FT;
    if (live) {
      const float* Wi = params + cs_kernel_off(i, K, nh);
      const float* bi = Wi + cs_pad4(static_cast<int64_t>(i) * K * nh);
      int fc[FT];
      float bias[FT];
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) {
        fc[ft] = f0 + ft < nh ? f0 + ft : nh - 1;                      // a filter past nh repeats the last one and is dropped
        bias[ft] = bi[fc[ft]];
      }
      for (int base = 0; base < R; base += kWave) {
        const int p = base + lane;
        const int pc = p < R ? p : 0;
        const int s = pc / P, t = pc - s * P;
        const float* xr = xs + (s * L + t) * KS;
        float acc[FT];
#pragma unroll
        for (int ft = 0; ft < FT; ++ft) acc[ft] = bias[ft];
        for (int tau = 0; tau < i; ++tau) {
          const float* wr = Wi + static_cast<int64_t>(tau) * K * nh;
          int c = 0;
          for (; c + 4 <= K; c += 4) {
            const float4 x4 = ld4(xr + tau * KS + c);
            const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
              for (int ft = 0; ft < FT; ++ft) acc[ft] = fmaf(xv[q], wr[(c + q) * nh + fc[ft]], acc[ft]);
            }
          }
          if (c < K) {                                                   // the last 1 .. 3 channels: the row's tail holds zeros
            const float4 x4 = ld4(xr + tau * KS + c);
            const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              if (c + q < K) {
#pragma unroll
                for (int ft = 0; ft < FT; ++ft) acc[ft] = fmaf(xv[q], wr[(c + q) * nh + fc[ft]], acc[ft]);
              }
            }
          }
        }
        if (p < R) {
#pragma unroll
          for (int ft = 0; ft < FT; ++ft) scratch[p * FT + ft] = acc[ft] > 0.f ? acc[ft] : 0.f;
        }
      }
    }
    __syncthreads();
    if (live) {
      // the pool: the first t that attains the maximum
      for (int idx = lane; idx < TB * FT; idx += kWave) {
        const int s = idx / FT, ft = idx - s * FT;
        const int64_t b = b0 + s;
        const int f = f0 + ft;
        if (b >= a.B || f >= nh) continue;
        const float* col = scratch + s * P * FT + ft;
        float best = col[0];
        int at = 0;
        for (int t = 1; t < P; ++t) {
          const float v = col[t * FT];
          if (v > best) {
            best = v;
            at = t;
          }
        }
        feat[b * W + (i - 1) * nh + f] = best;
        if (arg != nullptr) arg[b * (L * nh) + (i - 1) * nh + f] = at;
      }
    }
    __syncthreads();
  }
  // the vertical layer: v[s, c, g] = relu(bv[g] + sum_t x[s, t, c] Wv[t, g])
  if (blockIdx.y != 0) return;
  const float* Wv = params + a.offV;
  const float* bv = Wv + cs_pad4(static_cast<int64_t>(L) * nv);
  for (int idx = tid; idx < TB * K * nv; idx += kBlock) {
    const int s = idx / (K * nv), r = idx - s * (K * nv);
    const int c = r / nv, g = r - c * nv;
    const int64_t b = b0 + s;
    if (b >= a.B) continue;
    float acc = bv[g];
    for (int t = 0; t < L; ++t) acc = fmaf(xs[(s * L + t) * KS + c], Wv[t * nv + g], acc);
    feat[b * W + L * nh + r] = acc > 0.f ? acc : 0.f;
  }
}

// ---- backward: the input gradient -------------------------------------------------------------
// LDS: gh [TB][L nh] (the upstream gradient of the live horizontal units, 0 for the dead) | ah int [TB][L nh] | gv [TB][K nv]
__global__ __launch_bounds__(kBlock) void cs_bwd_x_kernel(CsArgs a, const float* __restrict__ params, int TB,
                                                          const float* __restrict__ feat, const int32_t* __restrict__ arg,
                                                          const float* __restrict__ gfeat, float* __restrict__ gx) {
  const int L = a.L, K = a.K, nh = a.nh, nv = a.nv, W = a.W, H = L * nh, KV = K * nv;
  const int tid = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB;
  float* gh = cs_lds;
  int* ah = reinterpret_cast<int*>(cs_lds + TB * H);
  float* gv = cs_lds + 2 * TB * H;
  for (int idx = tid; idx < TB * H; idx += kBlock) {
    const int s = idx / H, j = idx - s * H;
    const int64_t b = b0 + s;
    float g = 0.f;
    int at = 0;
    if (b < a.B) {
      g = feat[b * W + j] > 0.f ? gfeat[b * W + j] : 0.f;
      at = arg[b * H + j];
    }
    gh[idx] = g;
    ah[idx] = at;
  }
  for (int idx = tid; idx < TB * KV; idx += kBlock) {
    const int s = idx / KV, r = idx - s * KV;
    const int64_t b = b0 + s;
    gv[idx] = (b < a.B && feat[b * W + H + r] > 0.f) ? gfeat[b * W + H + r] : 0.f;
  }
  __syncthreads();
  const float* Wv = params + a.offV;
  for (int idx = tid; idx < TB * L * K; idx += kBlock) {
    const int s = idx / (L * K), r = idx - s * (L * K);
    const int t = r / K, c = r - t * K;
    const int64_t b = b0 + s;
    if (b >= a.B) continue;
    int64_t id = 0;
    float acc = 0.f;
    if (cs_id_ok(a, b * L + t, &id)) {
      const float* Wi = params;
      for (int i = 1; i <= L; ++i) {
        for (int f = 0; f < nh; ++f) {
          const float g = gh[s * H + (i - 1) * nh + f];
          const int tau = t - ah[s * H + (i - 1) * nh + f];
          if (g != 0.f && tau >= 0 && tau < i) acc = fmaf(g, Wi[(static_cast<int64_t>(tau) * K + c) * nh + f], acc);
        }
        Wi += cs_layer_floats(i, K, nh);
      }
      for (int g = 0; g < nv; ++g) acc = fmaf(gv[s * KV + c * nv + g], Wv[t * nv + g], acc);
    }
    gx[b * (L * K) + r] = acc;
  }
}

// ---- backward: the parameter gradients --------------------------------------------------------
// sum over b in [b0, b1), ascending, of g[b] x[b, t_b, c]: g the upstream gradient of unit j where feat > 0, t_b = arg[b, j] +
// tau (the forward's arg <= L - i: t_b < L) or, without arg, tau itself.  The dependent loads (arg -> id -> row) of eight
// samples are issued together; the sum is one fmaf chain in sample order either way.
__device__ __forceinline__ float cs_wgrad_sum(const CsArgs& a, const float* __restrict__ feat, const float* __restrict__ gfeat,
                                              const int32_t* __restrict__ arg, int64_t b0, int64_t b1, int j, int tau, int c) {
  constexpr int U = 8;
  const int L = a.L, K = a.K, W = a.W, H = a.L * a.nh;
  float acc = 0.f;
  int64_t b = b0;
  for (; b + U <= b1; b += U) {
    float g[U], x[U];
    int t[U];
    int64_t id[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      g[u] = feat[(b + u) * W + j] > 0.f ? gfeat[(b + u) * W + j] : 0.f;
      t[u] = (arg != nullptr ? arg[(b + u) * H + j] : 0) + tau;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      t[u] = (t[u] >= 0 && t[u] < L) ? t[u] : -1;
      id[u] = t[u] >= 0 ? static_cast<int64_t>(a.ids[(b + u) * L + t[u]]) : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = (id[u] >= 0 && id[u] < a.V) ? a.table[id[u] * K + c] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) acc = fmaf(g[u], x[u], acc);
  }
  for (; b < b1; ++b) {
    const float g = feat[b * W + j] > 0.f ? gfeat[b * W + j] : 0.f;
    const int t = (arg != nullptr ? arg[b * H + j] : 0) + tau;
    int64_t id = 0;
    const float x = (t >= 0 && t < L && cs_id_ok(a, b * L + t, &id)) ? a.table[id * K + c] : 0.f;
    acc = fmaf(g, x, acc);
  }
  return acc;
}

// part [n_slabs][pp]: element e < offV is element e of the parameter buffer; offV + (t nv + g) K + c is the vertical kernel's
// (t, g) from channel c alone; offV + L nv K + g K + c the vertical bias's g from channel c.
__global__ __launch_bounds__(kBlock) void cs_wgrad_kernel(CsArgs a, const float* __restrict__ feat, const int32_t* __restrict__ arg,
                                                          const float* __restrict__ gfeat, int64_t per_slab,
                                                          float* __restrict__ part) {
  const int L = a.L, K = a.K, nh = a.nh, nv = a.nv, W = a.W, H = L * nh;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= a.pp) return;
  const int64_t b0 = static_cast<int64_t>(blockIdx.y) * per_slab;
  const int64_t b1 = b0 + per_slab < a.B ? b0 + per_slab : a.B;
  float acc = 0.f;
  if (e < a.offV) {
    int i = 1;
    int64_t local = e;
    for (; i < L; ++i) {
      const int64_t n = cs_layer_floats(i, K, nh);
      if (local < n) break;
      local -= n;
    }
    const int64_t nk = static_cast<int64_t>(i) * K * nh, nk4 = cs_pad4(nk);
    if (local < nk) {
      const int tau = static_cast<int>(local / (K * nh));
      const int r = static_cast<int>(local - static_cast<int64_t>(tau) * (K * nh));
      const int c = r / nh, f = r - c * nh, j = (i - 1) * nh + f;
      acc = cs_wgrad_sum(a, feat, gfeat, arg, b0, b1, j, tau, c);
    } else if (local >= nk4 && local < nk4 + nh) {
      const int j = (i - 1) * nh + static_cast<int>(local - nk4);
      for (int64_t b = b0; b < b1; ++b) acc += feat[b * W + j] > 0.f ? gfeat[b * W + j] : 0.f;
    }
  } else if (e < a.offV + static_cast<int64_t>(L) * nv * K) {
    const int64_t r = e - a.offV;
    const int c = static_cast<int>(r % K), tg = static_cast<int>(r / K);
    const int t = tg / nv, g = tg - t * nv, j = H + c * nv + g;
    acc = cs_wgrad_sum(a, feat, gfeat, nullptr, b0, b1, j, t, c);
  } else {
    const int64_t r = e - a.offV - static_cast<int64_t>(L) * nv * K;
    const int c = static_cast<int>(r % K), g = static_cast<int>(r / K), j = H + c * nv + g;
    for (int64_t b = b0; b < b1; ++b) acc += feat[b * W + j] > 0.f ? gfeat[b * W + j] : 0.f;
  }
  part[static_cast<int64_t>(blockIdx.y) * a.pp + e] = acc;
}

__global__ __launch_bounds__(kBlock) void cs_reduce_kernel(CsArgs a, const float* __restrict__ part, int n_slabs,
                                                           float* __restrict__ gparams) {
  const int L = a.L, K = a.K, nh = a.nh, nv = a.nv;
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= a.np) return;
  double t = 0.0;
  if (e < a.offV) {
    int i = 1;
    int64_t local = e;
    for (; i < L; ++i) {
      const int64_t n = cs_layer_floats(i, K, nh);
      if (local < n) break;
      local -= n;
    }
    const int64_t nk = static_cast<int64_t>(i) * K * nh, nk4 = cs_pad4(nk);
    const bool gap = local < nk4 ? local >= nk : local - nk4 >= nh;       // the alignment gaps hold no gradient: 0
    if (!gap)
      for (int s = 0; s < n_slabs; ++s) t += static_cast<double>(part[static_cast<int64_t>(s) * a.pp + e]);       // slab order
  } else {
    const int64_t local = e - a.offV, nk = static_cast<int64_t>(L) * nv, nk4 = cs_pad4(nk);
    int64_t src = -1;                                                     // the K per-channel partials of this element
    if (local < nk) src = a.offV + local * K;
    else if (local >= nk4 && local - nk4 < nv) src = a.offV + nk * K + (local - nk4) * K;
    if (src >= 0)
      for (int s = 0; s < n_slabs; ++s)
        for (int c = 0; c < K; ++c) t += static_cast<double>(part[static_cast<int64_t>(s) * a.pp + src + c]);
  }
  gparams[e] = static_cast<float>(t);
}

// ---- host ------------------------------------------------------------------------------------
static inline size_t cs_align(size_t x) { return (x + 255) / 256 * 256; }
static inline bool cs_shape_ok(int L, int K, int nh, int nv) {
  return L >= 1 && L <= kCsMaxL && K >= 1 && K <= kCsMaxK && nh >= 1 && nh <= kCsMaxF && nv >= 1 && nv <= kCsMaxF;
}
static inline CsArgs cs_args(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int K, int nh, int nv) {
  int KS = (K + 3) & ~3;
  if ((KS / 4) % 2 == 0) KS += 4;
  const int64_t offV = cs_kernel_off(L + 1, K, nh);
  const int64_t np = offV + cs_pad4(static_cast<int64_t>(L) * nv) + cs_pad4(nv);
  return CsArgs{table, V, ids, B, L, K, nh, nv, KS, L * nh + K * nv, offV, np, offV + static_cast<int64_t>(L) * nv * K + static_cast<int64_t>(nv) * K};
}
static inline int cs_ft(int nh) { return nh == 1 ? 1 : nh == 2 ? 2 : 4; }
static inline size_t cs_fwd_lds(const CsArgs& a, int TB) {
  return (static_cast<size_t>(TB) * a.L * a.KS + static_cast<size_t>(kCsWaves) * TB * a.L * cs_ft(a.nh)) * 4;
}
static inline size_t cs_bwd_lds(const CsArgs& a, int TB) {
  return static_cast<size_t>(TB) * (2 * a.L * a.nh + a.K * a.nv) * 4;
}
// samples per workgroup: as many as `soft` bytes of LDS hold (one always fits in 64 KB), while that leaves two workgroups for
// every compute unit
template <typename LdsOf>
static inline int cs_tb(const CsArgs& a, LdsOf lds_of, size_t soft) {
  int64_t tb = a.B / (2 * kNumCU);
  if (tb > kCsMaxTB) tb = kCsMaxTB;
  while (tb > 1 && lds_of(a, static_cast<int>(tb)) > soft) --tb;
  return tb < 1 ? 1 : static_cast<int>(tb);
}
// slabs of the batch for the parameter gradients: enough for about four workgroups per compute unit, at least 16 samples
// each, at most kCsMaxSlabs, and no more than kCsMaxWsFloats of partials hold
static inline int cs_slabs(const CsArgs& a) {
  int64_t n = ceil_div(4 * kNumCU, ceil_div(a.pp, kBlock));
  const int64_t by_batch = ceil_div(a.B, 16), by_ws = kCsMaxWsFloats / a.pp;
  if (n > by_batch) n = by_batch;
  if (n > by_ws) n = by_ws;
  if (n > kCsMaxSlabs) n = kCsMaxSlabs;
  return n < 1 ? 1 : static_cast<int>(n);
}
template <typename Kern>
static int cs_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}
template <int FT>
static int cs_launch_fwd(const CsArgs& a, const float* params, float* feat, int32_t* arg, hipStream_t st) {
  const int TB = cs_tb(a, cs_fwd_lds, kCsFwdLdsSoft);
  const size_t lds = cs_fwd_lds(a, TB);
  const int rc = cs_set_lds(cs_fwd_kernel<FT>, lds);
  if (rc != LR_OK) return rc;
  // a tile's (kernel size, filter tile) items go to ny workgroups while that keeps the grid under about eight per compute unit:
  // the weight loads are latency the other waves of a compute unit have to cover
  const int64_t tiles = ceil_div(a.B, TB), n_items = static_cast<int64_t>(a.L) * ceil_div(a.nh, FT);
  int64_t ny = (8 * kNumCU) / tiles;
  if (ny > ceil_div(n_items, kCsWaves)) ny = ceil_div(n_items, kCsWaves);
  if (ny < 1) ny = 1;
  hipLaunchKernelGGL(cs_fwd_kernel<FT>, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(ny)), dim3(kBlock), lds, st, a, params,
                     TB, feat, arg);
  return launch_status();
}

}  // namespace lr

using namespace lr;

extern "C" int lr_caser_supported(int L, int K, int nh, int nv) { return cs_shape_ok(L, K, nh, nv) ? 1 : 0; }

extern "C" size_t lr_caser_params_bytes(int L, int K, int nh, int nv) {
  if (!cs_shape_ok(L, K, nh, nv)) return 0;
  return static_cast<size_t>(cs_args(nullptr, 0, nullptr, 0, L, K, nh, nv).np) * sizeof(float);
}

extern "C" size_t lr_caser_bwd_ws_bytes(int64_t B, int L, int K, int nh, int nv) {
  if (B < 0 || !cs_shape_ok(L, K, nh, nv)) return 0;
  const CsArgs a = cs_args(nullptr, 0, nullptr, B, L, K, nh, nv);
  return cs_align(static_cast<size_t>(a.pp) * cs_slabs(a) * sizeof(float));
}

extern "C" int lr_caser_fwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int K, int nh, int nv,
                                const float* params, float* feat, int32_t* arg, lr_stream_t stream) {
  if (!cs_shape_ok(L, K, nh, nv)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(ids && feat);
  const CsArgs a = cs_args(table, V, ids, B, L, K, nh, nv);
  switch (cs_ft(nh)) {
    case 1: return cs_launch_fwd<1>(a, params, feat, arg, as_stream(stream));
    case 2: return cs_launch_fwd<2>(a, params, feat, arg, as_stream(stream));
    default: return cs_launch_fwd<4>(a, params, feat, arg, as_stream(stream));
  }
}

extern "C" int lr_caser_bwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int K, int nh, int nv,
                                const float* params, const float* feat, const int32_t* arg, const float* gfeat, float* gx,
                                float* gparams, void* ws, size_t ws_bytes, lr_stream_t stream) {
  if (!cs_shape_ok(L, K, nh, nv)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && gparams && ws);
  if (ws_bytes < lr_caser_bwd_ws_bytes(B, L, K, nh, nv)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (ids && feat && arg && gfeat && gx));
  const CsArgs a = cs_args(table, V, ids, B, L, K, nh, nv);
  hipStream_t st = as_stream(stream);
  if (B > 0) {
    const int TB = cs_tb(a, cs_bwd_lds, kCsLdsSoft);
    const size_t lds = cs_bwd_lds(a, TB);
    const int rc = cs_set_lds(cs_bwd_x_kernel, lds);
    if (rc != LR_OK) return rc;
    hipLaunchKernelGGL(cs_bwd_x_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, st, a, params, TB, feat, arg,
                       gfeat, gx);
  }
  const int ns = cs_slabs(a);
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(cs_wgrad_kernel, dim3(static_cast<unsigned>(ceil_div(a.pp, kBlock)), ns), dim3(kBlock), 0, st, a, feat, arg, gfeat,
                     ceil_div(B > 0 ? B : 1, ns), part);
  hipLaunchKernelGGL(cs_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(a.np, kBlock))), dim3(kBlock), 0, st, a, part, ns, gparams);
  return launch_status();
}
