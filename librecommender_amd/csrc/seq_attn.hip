// The scaled-dot-product core of the sequence models on already projected rows (`libreco/layers/attention.py:5-25`, the
// `tf_attention` pooling, and `:67-126`, the Keras `MultiHeadAttention` branch, with the mask of `transformer.py:281-328`): one
// launch forward, one backward, for the Transformer layers and read-out, SIM's exact search unit and short window, and
// DIN's `use_tf_attention` pooling.  f32 on the VALU: head widths of 8 to 80 and windows of at most 64 give MFMA nothing to do
// (the finding at the top of autoint.hip); the kernels are bound by streaming q, k and v.
//   A unit is one (sample, head).  A workgroup owns TB consecutive units: their scores S / probabilities P [Tq][Tk] stay in
//   LDS, the head's columns of q, k, v (and gout) pass through LDS in chunks of CW columns, so that any supported shape fits
//   64 KB (one chunk up to T = 50 at hd = 80).  Small windows take many units per workgroup (TB up to 64).
//   sa_fwd_kernel   S = (q scale) k^T chunk by chunk, mask, softmax, O = P v chunk by chunk, stored straight to `out`; with
//                   v == k and a single chunk the key chunk in LDS serves as the value chunk: rows are read once.
//                   `saved` takes each row's maximum and exp-sum.
//   sa_bwd_kernel   recomputes S with the forward's own instruction sequence and P from the saved maximum and sum; dP = gout v^T
//                   and gv = P^T gout share one pass over the chunks of gout and v; dS = P (dP - rowsum(dP P)) in place;
//                   gq = (dS k) scale and gk = dS^T (q scale) share one pass over the chunks of q and k.
// Chunk rows are zero-padded to a multiple of 4 columns and read 16 bytes at a time; their stride is an odd number of 16-byte
// slots, the stride of S is an odd number of floats (rows are walked by adjacent lanes).  A thread forms four scores (or two
// rows of four output columns) at once, so that an LDS read feeds four fmas.  A softmax row is shared by G lanes (G from Tk
// alone).
// No atomics.  Every product element is one sequential fmaf chain over its contraction index (a chunk boundary carries the
// partial sum through LDS, which does not change it; the padding adds fmaf(0, 0, .)), whatever thread computes it, and the
// softmax sums depend on Tk alone: a sample's output and gradients have the same bits at B = 1 and inside any batch, and from
// run to run.
#include <math.h>

#include "common.hpp"

namespace lr {

constexpr int kSaMaxT = 64;          // Tq, Tk
constexpr int kSaMaxHd = 128;
constexpr int kSaMaxHeads = 8;
constexpr int kSaMaxM = 256;         // H * hd
constexpr int kSaMaxTB = 64;
constexpr size_t kSaLds = 64 * 1024;

struct SaArgs {
  int64_t U;                         // B * H units
  int Tq, Tk, H, hd, M;
  int CW, nch;                       // columns per chunk, chunks per head
  int CS, ST;                        // LDS row strides in floats: 4 (ceil(CW / 4) | 1), Tk | 1
  int TB;                            // units per workgroup
  int G;                             // lanes per softmax row: 1, 2, 4 or 8
  int vec;                           // hd % 4 == 0 and every pointer on a 16-byte boundary: rows move 16 bytes at a time
  int mask_mode;                     // 0: every key valid, 1: key_ok uint8 [B, Tk], 2: lens int32 [B]
  int causal;
  float scale;
};

extern __shared__ __attribute__((aligned(16))) float sa_lds[];

__host__ __device__ inline int sa_up4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int sa_tab_floats(int TB) { return sa_up4(6 * TB); }      // three int64 per unit

// the per-unit table: sample b, and the offsets of the unit's head columns in a [B, Tq, M] and a [B, Tk, M] tensor
struct SaUnits {
  const int64_t* b;
  const int64_t* oq;
  const int64_t* ok;
};
__device__ __forceinline__ SaUnits sa_units(const SaArgs& a, int64_t u0, int nu) {
  int64_t* tab = reinterpret_cast<int64_t*>(sa_lds);
  for (int u = threadIdx.x; u < nu; u += kBlock) {
    const int64_t g = u0 + u, b = g / a.H;
    const int64_t col = (g - b * a.H) * a.hd;
    tab[u] = b;
    tab[a.TB + u] = b * a.Tq * a.M + col;
    tab[2 * a.TB + u] = b * a.Tk * a.M + col;
  }
  __syncthreads();
  return SaUnits{tab, tab + a.TB, tab + 2 * a.TB};
}

// dst [(u T + t) CS + c] = src[off[u] + t M + c0 + c] (* mul) for c < cw, 0 up to the next multiple of 4
__device__ __forceinline__ void sa_load(const float* __restrict__ src, float* dst, const SaArgs& a, const int64_t* off, int nu,
                                        int T, int c0, int cw, float mul) {
  const int cw4 = sa_up4(cw);
  if (a.vec) {
    const int q4 = cw4 >> 2, n = nu * T * q4;
    for (int idx = threadIdx.x; idx < n; idx += kBlock) {
      const int r = idx / q4, c = (idx - r * q4) << 2;
      const int u = r / T, t = r - u * T;
      st4(dst + r * a.CS + c, f4_scale(ld4(src + off[u] + static_cast<int64_t>(t) * a.M + c0 + c), mul));
    }
  } else {
    const int n = nu * T * cw4;
    for (int idx = threadIdx.x; idx < n; idx += kBlock) {
      const int r = idx / cw4, c = idx - r * cw4;
      const int u = r / T, t = r - u * T;
      dst[r * a.CS + c] = c < cw ? src[off[u] + static_cast<int64_t>(t) * a.M + c0 + c] * mul : 0.f;
    }
  }
}

// S [(u Tq + i) ST + j] (+)= sum_c A [(u Tq + i) CS + c] Bm [(u Tk + j) CS + c].  A thread owns the keys jt, jt + NJ, jt + 2 NJ,
// jt + 3 NJ of one query row, in every chunk.
__device__ __forceinline__ void sa_dots(const float* A, const float* Bm, float* S, const SaArgs& a, int nu, int cw, bool first) {
  const int NJ = (a.Tk + 3) >> 2, per = a.Tq * NJ, n = nu * per, q4 = sa_up4(cw) >> 2;
  for (int idx = threadIdx.x; idx < n; idx += kBlock) {
    const int u = idx / per, rem = idx - u * per;
    const int i = rem / NJ, jt = rem - i * NJ;
    const float* x = A + (u * a.Tq + i) * a.CS;
    float* s = S + (u * a.Tq + i) * a.ST;
    const float* y[4];
    float acc[4];
    int j[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      j[m] = jt + m * NJ;
      const int jr = j[m] < a.Tk ? j[m] : a.Tk - 1;            // a tile past the last key reads the last key and stores nothing
      y[m] = Bm + (u * a.Tk + jr) * a.CS;
      acc[m] = first || j[m] >= a.Tk ? 0.f : s[jr];
    }
    for (int c = 0; c < q4; ++c) {
      const float4 xv = ld4(x + 4 * c);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float4 yv = ld4(y[m] + 4 * c);
        acc[m] = fmaf(xv.w, yv.w, fmaf(xv.z, yv.z, fmaf(xv.y, yv.y, fmaf(xv.x, yv.x, acc[m]))));
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (j[m] < a.Tk) s[j[m]] = acc[m];
  }
}

__device__ __forceinline__ float sa_group_max(float x, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float sa_group_sum(float x, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// P = softmax(S + mask) row by row, G adjacent lanes per row (lane l takes the keys l, l + G, ...).  Forward (`stats_out`): the
// row maximum and the sum of exponentials are computed and stored; backward (`stats_in`): they are the forward's.
__device__ __forceinline__ void sa_softmax(float* S, const SaArgs& a, const SaUnits& un, int64_t u0, int nu,
                                           const uint8_t* __restrict__ key_ok, const int32_t* __restrict__ lens,
                                           const float* __restrict__ stats_in, float* __restrict__ stats_out) {
  const int G = a.G, n = nu * a.Tq * G;
  for (int w = threadIdx.x; w < n; w += kBlock) {
    const int r = w / G, l = w - r * G;
    const int u = r / a.Tq, i = r - u * a.Tq;
    const int64_t b = un.b[u], row = (u0 + u) * a.Tq + i;
    float* p = S + r * a.ST;
    const int len = a.mask_mode == 2 ? lens[b] : 0;
    const uint8_t* ok = a.mask_mode == 1 ? key_ok + b * a.Tk : nullptr;
    float m = -INFINITY;
    for (int j = l; j < a.Tk; j += G) {
      const bool allowed = a.mask_mode == 0 || (a.mask_mode == 1 ? ok[j] != 0 : j < len) || (a.causal && j <= i);
      float s = p[j];
      if (!allowed) {
        s = s + -1e9f;                                         // an f32 addition (keras `_masked_softmax` / `_apply_scores`)
        p[j] = s;
      }
      m = fmaxf(m, s);
    }
    float sum;
    if (stats_in != nullptr) {
      m = stats_in[row * 2];
      sum = stats_in[row * 2 + 1];
      for (int j = l; j < a.Tk; j += G) p[j] = expf(p[j] - m);
    } else {
      m = sa_group_max(m, G);
      sum = 0.f;
      for (int j = l; j < a.Tk; j += G) {
        const float e = expf(p[j] - m);
        p[j] = e;
        sum += e;
      }
      sum = sa_group_sum(sum, G);
      if (stats_out != nullptr && l == 0) {
        stats_out[row * 2] = m;
        stats_out[row * 2 + 1] = sum;
      }
    }
    for (int j = l; j < a.Tk; j += G) p[j] = p[j] / sum;
  }
}

// S of every unit of the tile: chunks of q (scaled) and k through Ac, Bc.  Ends with a barrier.
__device__ __forceinline__ void sa_scores(const float* __restrict__ q, const float* __restrict__ k, float* S, float* Ac, float* Bc,
                                          const SaArgs& a, const SaUnits& un, int nu) {
  for (int ch = 0; ch < a.nch; ++ch) {
    const int c0 = ch * a.CW, cw = a.hd - c0 < a.CW ? a.hd - c0 : a.CW;
    sa_load(q, Ac, a, un.oq, nu, a.Tq, c0, cw, a.scale);
    sa_load(k, Bc, a, un.ok, nu, a.Tk, c0, cw, 1.f);
    __syncthreads();
    sa_dots(Ac, Bc, S, a, nu, cw, ch == 0);
    __syncthreads();
  }
}

// The products of P / dS (W, stride ST) with a chunk X (stride CS), times mul, stored to dst at the unit offsets `off`:
//   by_row:  row t is a query i:  dst[t][c] = sum over keys j of W[i][j] X[j][c]        (O = P v, gq = dS k)
//   !by_row: row t is a key j:    dst[t][c] = sum over queries i of W[i][j] X[i][c]     (gv = P^T gout, gk = dS^T q)
// A thread owns four columns of the rows t and t + ceil(T / 2).
__device__ __forceinline__ void sa_apply(const float* W, const float* X, float* __restrict__ dst, const SaArgs& a,
                                         const int64_t* off, int nu, int c0, int cw, bool by_row, float mul) {
  const int T = by_row ? a.Tq : a.Tk, Tn = by_row ? a.Tk : a.Tq;
  const int Th = (T + 1) >> 1, q4 = sa_up4(cw) >> 2, per = Th * q4, n = nu * per;
  const int ws = by_row ? 1 : a.ST;
  for (int idx = threadIdx.x; idx < n; idx += kBlock) {
    const int u = idx / per, rem = idx - u * per;
    const int t0 = rem / q4, c = (rem - t0 * q4) << 2;
    const int t1 = t0 + Th;
    const bool two = t1 < T;
    const float* wu = W + u * a.Tq * a.ST;
    const float* w0 = by_row ? wu + t0 * a.ST : wu + t0;
    const float* w1 = two ? (by_row ? wu + t1 * a.ST : wu + t1) : w0;
    const float* x = X + u * Tn * a.CS + c;
    float4 acc0 = f4_zero(), acc1 = f4_zero();
    for (int m = 0; m < Tn; ++m) {
      const float4 xv = ld4(x + m * a.CS);
      const float a0 = w0[m * ws], a1 = w1[m * ws];
      acc0 = f4_fma(make_float4(a0, a0, a0, a0), xv, acc0);
      acc1 = f4_fma(make_float4(a1, a1, a1, a1), xv, acc1);
    }
    acc0 = f4_scale(acc0, mul);
    acc1 = f4_scale(acc1, mul);
    float* d0 = dst + off[u] + static_cast<int64_t>(t0) * a.M + c0 + c;
    float* d1 = dst + off[u] + static_cast<int64_t>(t1) * a.M + c0 + c;
    if (a.vec) {
      st4(d0, acc0);
      if (two) st4(d1, acc1);
    } else {
      const float r0[4] = {acc0.x, acc0.y, acc0.z, acc0.w}, r1[4] = {acc1.x, acc1.y, acc1.z, acc1.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < cw) {
          d0[e] = r0[e];
          if (two) d1[e] = r1[e];
        }
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sa_fwd_kernel(SaArgs a, const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, const uint8_t* __restrict__ key_ok,
                                                        const int32_t* __restrict__ lens, float* __restrict__ out,
                                                        float* __restrict__ stats) {
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * a.TB;
  const int nu = a.U - u0 < a.TB ? static_cast<int>(a.U - u0) : a.TB;
  float* Ac = sa_lds + sa_tab_floats(a.TB);    // [TB Tq][CS]
  float* Bc = Ac + a.TB * a.Tq * a.CS;         // [TB Tk][CS]
  float* S = Bc + a.TB * a.Tk * a.CS;          // [TB Tq][ST]
  const SaUnits un = sa_units(a, u0, nu);
  sa_scores(q, k, S, Ac, Bc, a, un, nu);
  sa_softmax(S, a, un, u0, nu, key_ok, lens, nullptr, stats);
  __syncthreads();
  const bool reuse = v == k && a.nch == 1;     // the key chunk in LDS is the value chunk
  for (int ch = 0; ch < a.nch; ++ch) {
    const int c0 = ch * a.CW, cw = a.hd - c0 < a.CW ? a.hd - c0 : a.CW;
    if (!reuse) {
      sa_load(v, Bc, a, un.ok, nu, a.Tk, c0, cw, 1.f);
      __syncthreads();
    }
    sa_apply(S, Bc, out, a, un.oq, nu, c0, cw, true, 1.f);
    __syncthreads();
  }
}

// ---- backward --------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sa_bwd_kernel(SaArgs a, const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, const uint8_t* __restrict__ key_ok,
                                                        const int32_t* __restrict__ lens, const float* __restrict__ stats,
                                                        const float* __restrict__ gout, float* __restrict__ gq,
                                                        float* __restrict__ gk, float* __restrict__ gv) {
  const int64_t u0 = static_cast<int64_t>(blockIdx.x) * a.TB;
  const int nu = a.U - u0 < a.TB ? static_cast<int>(a.U - u0) : a.TB;
  float* Ac = sa_lds + sa_tab_floats(a.TB);    // [TB Tq][CS]
  float* Bc = Ac + a.TB * a.Tq * a.CS;         // [TB Tk][CS]
  float* P = Bc + a.TB * a.Tk * a.CS;          // [TB Tq][ST]
  float* dP = P + a.TB * a.Tq * a.ST;          // dP, then dS in place
  const SaUnits un = sa_units(a, u0, nu);
  sa_scores(q, k, P, Ac, Bc, a, un, nu);
  sa_softmax(P, a, un, u0, nu, key_ok, lens, stats, nullptr);
  __syncthreads();
  for (int ch = 0; ch < a.nch; ++ch) {         // dP = gout v^T, gv = P^T gout
    const int c0 = ch * a.CW, cw = a.hd - c0 < a.CW ? a.hd - c0 : a.CW;
    sa_load(gout, Ac, a, un.oq, nu, a.Tq, c0, cw, 1.f);
    sa_load(v, Bc, a, un.ok, nu, a.Tk, c0, cw, 1.f);
    __syncthreads();
    sa_dots(Ac, Bc, dP, a, nu, cw, ch == 0);
    sa_apply(P, Ac, gv, a, un.ok, nu, c0, cw, false, 1.f);
    __syncthreads();
  }
  {                                            // dS = P (dP - rowsum(dP P)), G lanes per row
    const int G = a.G, n = nu * a.Tq * G;
    for (int w = threadIdx.x; w < n; w += kBlock) {
      const int r = w / G, l = w - r * G;
      const float* p = P + r * a.ST;
      float* g = dP + r * a.ST;
      float dot = 0.f;
      for (int j = l; j < a.Tk; j += G) dot = fmaf(g[j], p[j], dot);
      dot = sa_group_sum(dot, G);
      for (int j = l; j < a.Tk; j += G) g[j] = p[j] * (g[j] - dot);
    }
  }
  __syncthreads();
  for (int ch = 0; ch < a.nch; ++ch) {         // gq = (dS k) scale, gk = dS^T (q scale)
    const int c0 = ch * a.CW, cw = a.hd - c0 < a.CW ? a.hd - c0 : a.CW;
    sa_load(q, Ac, a, un.oq, nu, a.Tq, c0, cw, a.scale);
    sa_load(k, Bc, a, un.ok, nu, a.Tk, c0, cw, 1.f);
    __syncthreads();
    sa_apply(dP, Bc, gq, a, un.oq, nu, c0, cw, true, a.scale);
    sa_apply(dP, Ac, gk, a, un.ok, nu, c0, cw, false, 1.f);
    __syncthreads();
  }
}

// ---- host ------------------------------------------------------------------------------------
static inline bool sa_shape_ok(int Tq, int Tk, int H, int hd) {
  return Tq >= 1 && Tq <= kSaMaxT && Tk >= 1 && Tk <= kSaMaxT && H >= 1 && H <= kSaMaxHeads && hd >= 1 && hd <= kSaMaxHd &&
         H * hd <= kSaMaxM;
}
static inline size_t sa_lds_bytes(const SaArgs& a, int TB, bool bwd) {
  return (sa_tab_floats(TB) + static_cast<size_t>(TB) * ((bwd ? 2 : 1) * a.Tq * a.ST + (a.Tq + a.Tk) * a.CS)) * sizeof(float);
}
static inline bool sa_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
// The chunking and the softmax groups depend on the shape alone (the fewest chunks with which one unit fits the LDS budget); the
// units per workgroup on the batch too: as many as the budget holds, while that leaves two workgroups for every compute unit.
static inline SaArgs sa_args(int64_t B, int Tq, int Tk, int H, int hd, float scale, int mask_mode, int causal, bool bwd, bool vec) {
  SaArgs a{};
  a.U = B * H;
  a.Tq = Tq;
  a.Tk = Tk;
  a.H = H;
  a.hd = hd;
  a.M = H * hd;
  a.ST = Tk | 1;
  a.mask_mode = mask_mode;
  a.causal = causal ? 1 : 0;
  a.scale = scale;
  a.vec = vec && hd % 4 == 0 ? 1 : 0;
  a.G = 1;
  while (a.G < 8 && Tk > 8 * a.G) a.G *= 2;
  for (int n = 1; n <= hd; ++n) {
    a.CW = static_cast<int>(ceil_div(hd, n));
    if (n > 1) a.CW = sa_up4(a.CW);                            // chunks start on a multiple of 4 columns
    a.CS = 4 * ((sa_up4(a.CW) >> 2) | 1);
    if (sa_lds_bytes(a, 1, bwd) <= kSaLds) break;
  }
  a.nch = static_cast<int>(ceil_div(hd, a.CW));
  int64_t tb = a.U / (2 * kNumCU);
  if (tb > kSaMaxTB) tb = kSaMaxTB;
  if (tb < 1) tb = 1;
  while (tb > 1 && sa_lds_bytes(a, static_cast<int>(tb), bwd) > kSaLds) --tb;
  a.TB = static_cast<int>(tb);
  return a;
}
template <typename Kern>
static int sa_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_seq_attn_supported(int Tq, int Tk, int H, int hd) { return sa_shape_ok(Tq, Tk, H, hd) ? 1 : 0; }

extern "C" size_t lr_seq_attn_saved_bytes(int64_t B, int Tq, int Tk, int H, int hd) {
  if (B < 0 || !sa_shape_ok(Tq, Tk, H, hd)) return 0;
  return static_cast<size_t>(B) * H * Tq * 2 * sizeof(float);          // every row's maximum and sum of exponentials
}

// The launch plan of a call, from the launches' own sa_args and sa_lds_bytes.  Host only.
extern "C" int lr_seq_attn_plan_params(int64_t B, int Tq, int Tk, int H, int hd, int bwd, int aligned, int32_t* out8) {
  if (!sa_shape_ok(Tq, Tk, H, hd)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 1 && out8 != nullptr);
  const SaArgs a = sa_args(B, Tq, Tk, H, hd, 1.f, 0, 0, bwd != 0, aligned != 0);
  out8[0] = a.TB;
  out8[1] = a.nch;
  out8[2] = a.CW;
  out8[3] = a.CS;
  out8[4] = a.ST;
  out8[5] = a.G;
  out8[6] = a.vec;
  out8[7] = static_cast<int32_t>(sa_lds_bytes(a, a.TB, bwd != 0));
  return LR_OK;
}

extern "C" int lr_seq_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t B, int Tq, int Tk, int H, int hd,
                                   float scale, const uint8_t* key_ok, const int32_t* lens, int causal_or, float* out,
                                   void* saved, size_t saved_bytes, lr_stream_t stream) {
  if (!sa_shape_ok(Tq, Tk, H, hd)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && !(key_ok && lens) && !(causal_or && Tq != Tk));
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(q && k && v && out);
  if (saved != nullptr && saved_bytes < lr_seq_attn_saved_bytes(B, Tq, Tk, H, hd)) return LR_EWORKSPACE;
  const bool vec = sa_aligned(q) && sa_aligned(k) && sa_aligned(v) && sa_aligned(out);
  const SaArgs a = sa_args(B, Tq, Tk, H, hd, scale, key_ok ? 1 : lens ? 2 : 0, causal_or, false, vec);
  const size_t lds = sa_lds_bytes(a, a.TB, false);
  const int rc = sa_set_lds(sa_fwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(sa_fwd_kernel, dim3(static_cast<unsigned>(ceil_div(a.U, a.TB))), dim3(kBlock), lds, as_stream(stream), a, q, k,
                     v, key_ok, lens, out, static_cast<float*>(saved));
  return launch_status();
}

extern "C" int lr_seq_attn_bwd_f32(const float* q, const float* k, const float* v, int64_t B, int Tq, int Tk, int H, int hd,
                                   float scale, const uint8_t* key_ok, const int32_t* lens, int causal_or, const void* saved,
                                   const float* gout, float* gq, float* gk, float* gv, lr_stream_t stream) {
  if (!sa_shape_ok(Tq, Tk, H, hd)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && !(key_ok && lens) && !(causal_or && Tq != Tk));
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(q && k && v && saved && gout && gq && gk && gv && gk != gv);
  const bool vec = sa_aligned(q) && sa_aligned(k) && sa_aligned(v) && sa_aligned(gout) && sa_aligned(gq) && sa_aligned(gk) &&
                   sa_aligned(gv);
  const SaArgs a = sa_args(B, Tq, Tk, H, hd, scale, key_ok ? 1 : lens ? 2 : 0, causal_or, true, vec);
  const size_t lds = sa_lds_bytes(a, a.TB, true);
  const int rc = sa_set_lds(sa_bwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(sa_bwd_kernel, dim3(static_cast<unsigned>(ceil_div(a.U, a.TB))), dim3(kBlock), lds, as_stream(stream), a, q, k,
                     v, key_ok, lens, static_cast<const float*>(saved), gout, gq, gk, gv);
  return launch_status();
}
