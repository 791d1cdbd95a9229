// AutoInt's interaction stack (`libreco/algorithms/autoint.py:146-168` with `layers/attention.py:67-101`, the Keras
// `MultiHeadAttention(use_bias=False)` branch): n layers of multi-head self-attention over the T feature fields of a sample, with
// an optional residual, and the Dense(1) read-out of the flattened result.  f32 on the VALU: head dimensions of 8 and a dozen
// fields give MFMA nothing to do.
//   ai_fwd_kernel     one launch for the whole stack and the read-out.  A workgroup owns TB samples (R = TB T rows) for all
//                     layers: A [R][D], Q (scaled, later the heads' outputs O) / Kx / V [R][M] and one head's P [T][T] per sample
//                     live in LDS, the weights stream from L2.  With `acts` == nullptr (inference) only the logits are written.
//   ai_bwd_kernel     a fixed number of workgroups, each walking over tiles of TB samples.  Per layer, last to first, a tile
//                     reloads A_{l-1} (acts or x) and RECOMPUTES Q, Kx, V and, per head, P and O with the forward's own
//                     instruction sequence (nothing but the layer outputs is saved), then runs the chain of the header.  The
//                     gradients of Q, Kx, V take the LDS of dO, O and V once those are dead.  Weight gradients of a tile are
//                     added to the workgroup's own slab of `ws` (laid out like the parameters, zeroed by the workgroup itself);
//   ai_reduce_kernel  adds the slabs in slab order.  No float atomics: the same bits from run to run.
// Every output element is one sequential fmaf chain over its contraction index, whatever thread computes it: a sample's logit
// has the same bits at B = 1 and inside any batch.  All LDS row strides are odd (rows are walked by adjacent lanes).
#include <math.h>

#include "common.hpp"

namespace lr {

constexpr int kAiMax = 64;         // T, D and H * hd in [1, 64]
constexpr int kAiMaxHeads = 8;
constexpr int kAiMaxLayers = 8;
constexpr int kAiBwdGroups = 2 * kNumCU;
constexpr size_t kAiLdsSoft = 64 * 1024;

struct AiArgs {
  int64_t B;
  int T, D, H, nl, residual;
  int hd[kAiMaxLayers];
  float scale[kAiMaxLayers];      // 1 / sqrt(hd), rounded from double
  int SD, ST, SM;                 // LDS row strides: D | 1, T | 1, max(H hd) | 1
};

__host__ __device__ inline int64_t ai_pad4(int64_t n) { return (n + 3) / 4 * 4; }
// offset of layer l's query kernel in the parameter buffer (l == nl: dense/kernel); key, value [D, M] and attention_output
// [M, D] follow the query kernel, each on a 16-byte boundary
__host__ __device__ inline int64_t ai_layer_off(const AiArgs& a, int l) {
  int64_t off = 0;
  for (int i = 0; i < l; ++i) off += 4 * ai_pad4(static_cast<int64_t>(a.D) * a.H * a.hd[i]);
  return off;
}
__host__ __device__ inline int64_t ai_n_params(const AiArgs& a) {
  return ai_layer_off(a, a.nl) + ai_pad4(static_cast<int64_t>(a.T) * a.D) + 4;
}

extern __shared__ float ai_lds[];

// Q (scaled by 1 / sqrt(hd)), Kx, V [R][M] = A [R][D] times the three kernels at W
__device__ __forceinline__ void ai_project(const float* A, float* Q, float* Kx, float* V, const float* __restrict__ W, int R, int D,
                                           int M, int SD, int SM, float scale) {
  const int64_t wstride = ai_pad4(static_cast<int64_t>(D) * M);
  const int RM = R * M;
  for (int idx = threadIdx.x; idx < 3 * RM; idx += kBlock) {
    const int which = idx / RM, rem = idx - which * RM;
    const int r = rem / M, n = rem - r * M;
    const float* w = W + which * wstride + n;
    const float* ar = A + r * SD;
    float acc = 0.f;
    for (int k = 0; k < D; ++k) acc = fmaf(ar[k], w[static_cast<int64_t>(k) * M], acc);
    if (which == 0) Q[r * SM + n] = acc * scale;
    else if (which == 1) Kx[r * SM + n] = acc;
    else V[r * SM + n] = acc;
  }
}

// P [R][T] of head columns [c0, c0 + hd): the scores Q Kx^T of every sample of the tile; then (after a barrier) the softmax of
// every row with the row maximum subtracted.  Ends with a barrier.
__device__ __forceinline__ void ai_probs(const float* Q, const float* Kx, float* P, int nb, int T, int c0, int hd, int SM, int ST) {
  const int TT = T * T;
  for (int idx = threadIdx.x; idx < nb * TT; idx += kBlock) {
    const int s = idx / TT, rem = idx - s * TT;
    const int i = rem / T, j = rem - i * T;
    const float* q = Q + (s * T + i) * SM + c0;
    const float* k = Kx + (s * T + j) * SM + c0;
    float acc = 0.f;
    for (int c = 0; c < hd; ++c) acc = fmaf(q[c], k[c], acc);
    P[(s * T + i) * ST + j] = acc;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < nb * T; r += kBlock) {
    float* p = P + r * ST;
    float m = p[0];
    for (int j = 1; j < T; ++j) m = fmaxf(m, p[j]);
    float sum = 0.f;
    for (int j = 0; j < T; ++j) {
      const float e = expf(p[j] - m);
      p[j] = e;
      sum += e;
    }
    for (int j = 0; j < T; ++j) p[j] = p[j] / sum;
  }
  __syncthreads();
}

// O [R][c0 .. c0 + hd) = P V of every sample of the tile
__device__ __forceinline__ void ai_attend(const float* P, const float* V, float* O, int R, int T, int c0, int hd, int SM, int ST) {
  for (int idx = threadIdx.x; idx < R * hd; idx += kBlock) {
    const int r = idx / hd, c = idx - r * hd;
    const float* p = P + r * ST;
    const float* v = V + (r / T) * T * SM + c0 + c;
    float acc = 0.f;
    for (int j = 0; j < T; ++j) acc = fmaf(p[j], v[j * SM], acc);
    O[r * SM + c0 + c] = acc;
  }
}

// ---- forward ---------------------------------------------------------------------------------
// acts [nl][B][T][D] (nullable), logits [B]
__global__ __launch_bounds__(kBlock) void ai_fwd_kernel(AiArgs a, const float* __restrict__ x, const float* __restrict__ params,
                                                        int TB, float* __restrict__ acts, float* __restrict__ logits) {
  const int T = a.T, D = a.D, SD = a.SD, SM = a.SM, ST = a.ST;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * TB;
  const int nb = a.B - b0 < TB ? static_cast<int>(a.B - b0) : TB;
  const int R = nb * T, RD = R * D;
  float* A = ai_lds;                    // [TB T][SD]
  float* Q = A + TB * T * SD;           // [TB T][SM] each
  float* Kx = Q + TB * T * SM;
  float* V = Kx + TB * T * SM;
  float* P = V + TB * T * SM;           // [TB T][ST]
  float* rowdot = P + TB * T * ST;      // [TB T]
  const int tid = threadIdx.x;
  const int64_t e0 = b0 * T * D, slab = a.B * T * D;
  for (int idx = tid; idx < RD; idx += kBlock) A[(idx / D) * SD + idx % D] = x[e0 + idx];
  __syncthreads();
  for (int l = 0; l < a.nl; ++l) {
    const int hd = a.hd[l], M = a.H * hd;
    const float* W = params + ai_layer_off(a, l);
    ai_project(A, Q, Kx, V, W, R, D, M, SD, SM, a.scale[l]);
    __syncthreads();
    for (int h = 0; h < a.H; ++h) {
      ai_probs(Q, Kx, P, nb, T, h * hd, hd, SM, ST);
      ai_attend(P, V, Q, R, T, h * hd, hd, SM, ST);          // Q's columns of this head are dead: they take O
      __syncthreads();
    }
    const float* Wo = W + 3 * ai_pad4(static_cast<int64_t>(D) * M);
    for (int idx = tid; idx < RD; idx += kBlock) {
      const int r = idx / D, d = idx - r * D;
      const float* o = Q + r * SM;
      float acc = 0.f;
      for (int m = 0; m < M; ++m) acc = fmaf(o[m], Wo[static_cast<int64_t>(m) * D + d], acc);
      const float v = a.residual ? A[r * SD + d] + acc : acc;
      A[r * SD + d] = v;
      if (acts != nullptr) acts[l * slab + e0 + idx] = v;
    }
    __syncthreads();
  }
  const float* wd = params + ai_layer_off(a, a.nl);
  for (int r = tid; r < R; r += kBlock) {
    const float* w = wd + (r % T) * D;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc = fmaf(A[r * SD + d], w[d], acc);
    rowdot[r] = acc;
  }
  __syncthreads();
  for (int s = tid; s < nb; s += kBlock) {
    float acc = wd[ai_pad4(static_cast<int64_t>(T) * D)];
    for (int t = 0; t < T; ++t) acc += rowdot[s * T + t];
    logits[b0 + s] = acc;
  }
}

// ---- backward --------------------------------------------------------------------------------
// part [gridDim.x][n_params]
__global__ __launch_bounds__(kBlock) void ai_bwd_kernel(AiArgs a, const float* __restrict__ x, const float* __restrict__ params,
                                                        int TB, int64_t n_tiles, const float* __restrict__ acts,
                                                        const float* __restrict__ glogits, float* __restrict__ gx,
                                                        int64_t n_params, float* __restrict__ part) {
  const int T = a.T, D = a.D, SD = a.SD, SM = a.SM, ST = a.ST;
  float* A = ai_lds;                    // [TB T][SD]
  float* dA = A + TB * T * SD;
  float* Q = dA + TB * T * SD;          // [TB T][SM] each
  float* Kx = Q + TB * T * SM;
  float* V = Kx + TB * T * SM;          // a head's columns become dV once its dP is formed
  float* O = V + TB * T * SM;           // a head's columns become dKx once its rows of gWo are formed
  float* dO = O + TB * T * SM;          // a head's columns become dQ once its dV is formed
  float* P = dO + TB * T * SM;          // [TB T][ST] each
  float* dP = P + TB * T * ST;          // dP, then dS in place
  const int tid = threadIdx.x;
  float* mine = part + static_cast<int64_t>(blockIdx.x) * n_params;
  for (int64_t i = tid; i < n_params; i += kBlock) mine[i] = 0.f;
  __syncthreads();
  const int64_t slab = a.B * T * D;
  const int64_t off_dense = ai_layer_off(a, a.nl), off_bias = off_dense + ai_pad4(static_cast<int64_t>(T) * D);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t b0 = tile * TB;
    const int nb = a.B - b0 < TB ? static_cast<int>(a.B - b0) : TB;
    const int R = nb * T, RD = R * D, TD = T * D;
    const int64_t e0 = b0 * T * D;
    // the read-out: g flatten(A_n), g, and dA_n = g w
    const float* last = acts + (a.nl - 1) * slab + e0;
    for (int idx = tid; idx < TD; idx += kBlock) {
      float acc = 0.f;
      for (int s = 0; s < nb; ++s) acc = fmaf(glogits[b0 + s], last[s * TD + idx], acc);
      mine[off_dense + idx] += acc;
    }
    if (tid == 0) {
      float acc = 0.f;
      for (int s = 0; s < nb; ++s) acc += glogits[b0 + s];
      mine[off_bias] += acc;
    }
    for (int idx = tid; idx < RD; idx += kBlock) {
      const int r = idx / D, d = idx - r * D;
      dA[r * SD + d] = glogits[b0 + r / T] * params[off_dense + (r % T) * D + d];
    }
    for (int l = a.nl - 1; l >= 0; --l) {
      const int hd = a.hd[l], M = a.H * hd;
      const float scale = a.scale[l];
      const int64_t wstride = ai_pad4(static_cast<int64_t>(D) * M), off = ai_layer_off(a, l);
      const float* W = params + off;
      const float* Wo = W + 3 * wstride;
      const float* in = (l == 0 ? x : acts + (l - 1) * slab) + e0;
      for (int idx = tid; idx < RD; idx += kBlock) A[(idx / D) * SD + idx % D] = in[idx];
      __syncthreads();                                        // A, and dA of the layer above (or of the read-out)
      ai_project(A, Q, Kx, V, W, R, D, M, SD, SM, scale);
      for (int idx = tid; idx < R * M; idx += kBlock) {       // dO = dY Wo^T
        const int r = idx / M, m = idx - r * M;
        const float* w = Wo + static_cast<int64_t>(m) * D;
        float acc = 0.f;
        for (int d = 0; d < D; ++d) acc = fmaf(dA[r * SD + d], w[d], acc);
        dO[r * SM + m] = acc;
      }
      __syncthreads();
      for (int h = 0; h < a.H; ++h) {
        const int c0 = h * hd;
        ai_probs(Q, Kx, P, nb, T, c0, hd, SM, ST);
        ai_attend(P, V, O, R, T, c0, hd, SM, ST);
        const int TT = T * T;
        for (int idx = tid; idx < nb * TT; idx += kBlock) {   // dP = dO_h V_h^T
          const int s = idx / TT, rem = idx - s * TT;
          const int i = rem / T, j = rem - i * T;
          const float* g = dO + (s * T + i) * SM + c0;
          const float* v = V + (s * T + j) * SM + c0;
          float acc = 0.f;
          for (int c = 0; c < hd; ++c) acc = fmaf(g[c], v[c], acc);
          dP[(s * T + i) * ST + j] = acc;
        }
        __syncthreads();
        for (int idx = tid; idx < hd * D; idx += kBlock) {    // rows c0 .. c0 + hd of gWo = O_h^T dY
          const int c = idx / D, d = idx - c * D;
          float acc = 0.f;
          for (int r = 0; r < R; ++r) acc = fmaf(O[r * SM + c0 + c], dA[r * SD + d], acc);
          mine[off + 3 * wstride + static_cast<int64_t>(c0 + c) * D + d] += acc;
        }
        for (int idx = tid; idx < R * hd; idx += kBlock) {    // dV_h = P^T dO_h, over V_h
          const int r = idx / hd, c = idx - r * hd;
          const int s = r / T, j = r - s * T;
          const float* p = P + s * T * ST + j;
          const float* g = dO + s * T * SM + c0 + c;
          float acc = 0.f;
          for (int i = 0; i < T; ++i) acc = fmaf(p[i * ST], g[i * SM], acc);
          V[r * SM + c0 + c] = acc;
        }
        for (int r = tid; r < R; r += kBlock) {               // dS = P (dP - rowsum(dP P)), over dP
          const float* p = P + r * ST;
          float* g = dP + r * ST;
          float dot = 0.f;
          for (int j = 0; j < T; ++j) dot = fmaf(g[j], p[j], dot);
          for (int j = 0; j < T; ++j) g[j] = p[j] * (g[j] - dot);
        }
        __syncthreads();
        for (int idx = tid; idx < R * hd; idx += kBlock) {    // dQ_h = dS Kx_h / sqrt(hd) over dO_h; dKx_h = dS^T Q_h over O_h
          const int r = idx / hd, c = idx - r * hd;
          const int s = r / T, t = r - s * T;
          const float* ds = dP + r * ST;
          const float* k = Kx + s * T * SM + c0 + c;
          float acc = 0.f;
          for (int j = 0; j < T; ++j) acc = fmaf(ds[j], k[j * SM], acc);
          dO[r * SM + c0 + c] = acc * scale;
          const float* dst = dP + s * T * ST + t;
          const float* q = Q + s * T * SM + c0 + c;
          acc = 0.f;
          for (int i = 0; i < T; ++i) acc = fmaf(dst[i * ST], q[i * SM], acc);
          O[r * SM + c0 + c] = acc;
        }
        __syncthreads();
      }
      // dO, O, V now hold dQ, dKx, dV of every head
      const int DM = D * M;
      for (int idx = tid; idx < 3 * DM; idx += kBlock) {      // gWq, gWk, gWv = A^T (dQ, dKx, dV)
        const int which = idx / DM, rem = idx - which * DM;
        const int k = rem / M, n = rem - k * M;
        const float* g = (which == 0 ? dO : which == 1 ? O : V) + n;
        float acc = 0.f;
        for (int r = 0; r < R; ++r) acc = fmaf(A[r * SD + k], g[r * SM], acc);
        mine[off + which * wstride + rem] += acc;
      }
      for (int idx = tid; idx < RD; idx += kBlock) {          // dA_{l-1} = dQ Wq^T + dKx Wk^T + dV Wv^T (+ dY)
        const int r = idx / D, d = idx - r * D;
        const float* wq = W + static_cast<int64_t>(d) * M;
        float acc = a.residual ? dA[r * SD + d] : 0.f;
        for (int m = 0; m < M; ++m) acc = fmaf(dO[r * SM + m], wq[m], acc);
        for (int m = 0; m < M; ++m) acc = fmaf(O[r * SM + m], wq[wstride + m], acc);
        for (int m = 0; m < M; ++m) acc = fmaf(V[r * SM + m], wq[2 * wstride + m], acc);
        dA[r * SD + d] = acc;
      }
      __syncthreads();
    }
    for (int idx = tid; idx < RD; idx += kBlock) gx[e0 + idx] = dA[(idx / D) * SD + idx % D];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void ai_reduce_kernel(const float* __restrict__ part, int n_slabs, int64_t n_params,
                                                           float* __restrict__ gparams) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_params) return;
  double t = 0.0;
  for (int g = 0; g < n_slabs; ++g) t += static_cast<double>(part[static_cast<int64_t>(g) * n_params + i]);   // slab order
  gparams[i] = static_cast<float>(t);
}

// ---- host ------------------------------------------------------------------------------------
static inline bool ai_shape_ok(int T, int D, int H, int n_layers, const int* head_dims) {
  if (!(T >= 1 && T <= kAiMax && D >= 1 && D <= kAiMax && H >= 1 && H <= kAiMaxHeads && n_layers >= 1 &&
        n_layers <= kAiMaxLayers && head_dims != nullptr))
    return false;
  for (int l = 0; l < n_layers; ++l)
    if (head_dims[l] < 1 || H * head_dims[l] > kAiMax) return false;
  return true;
}
static inline AiArgs ai_args(int64_t B, int T, int D, int H, int n_layers, const int* head_dims, int residual) {
  AiArgs a{};
  a.B = B;
  a.T = T;
  a.D = D;
  a.H = H;
  a.nl = n_layers;
  a.residual = residual ? 1 : 0;
  int m = 1;
  for (int l = 0; l < n_layers; ++l) {
    a.hd[l] = head_dims[l];
    a.scale[l] = static_cast<float>(1.0 / sqrt(static_cast<double>(head_dims[l])));
    if (H * head_dims[l] > m) m = H * head_dims[l];
  }
  a.SD = D | 1;
  a.ST = T | 1;
  a.SM = m | 1;
  return a;
}
static inline size_t ai_lds_bytes(const AiArgs& a, int TB, bool bwd) {
  const size_t rows = static_cast<size_t>(TB) * a.T;
  return rows * (bwd ? 2 * a.SD + 5 * a.SM + 2 * a.ST : a.SD + 3 * a.SM + a.ST + 1) * 4;
}
// samples per workgroup: as many as 64 KB of LDS hold, while that leaves two workgroups for every compute unit
static inline int ai_tb(const AiArgs& a, bool bwd) {
  int64_t tb = a.B / (2 * kNumCU);
  if (tb > 64) tb = 64;
  while (tb > 1 && ai_lds_bytes(a, static_cast<int>(tb), bwd) > kAiLdsSoft) --tb;
  return tb < 1 ? 1 : static_cast<int>(tb);
}
static inline int ai_bwd_groups(const AiArgs& a) {
  const int64_t tiles = ceil_div(a.B, ai_tb(a, true));
  return static_cast<int>(tiles < kAiBwdGroups ? tiles : kAiBwdGroups);
}
template <typename Kern>
static int ai_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_autoint_supported(int T, int D, int H, int n_layers, const int* head_dims) {
  return ai_shape_ok(T, D, H, n_layers, head_dims) ? 1 : 0;
}

extern "C" size_t lr_autoint_params_bytes(int T, int D, int H, int n_layers, const int* head_dims) {
  if (!ai_shape_ok(T, D, H, n_layers, head_dims)) return 0;
  return static_cast<size_t>(ai_n_params(ai_args(0, T, D, H, n_layers, head_dims, 0))) * sizeof(float);
}

extern "C" size_t lr_autoint_fwd_acts_bytes(int64_t B, int T, int D, int n_layers) {
  if (B < 0 || T < 1 || T > kAiMax || D < 1 || D > kAiMax || n_layers < 1 || n_layers > kAiMaxLayers) return 0;
  return static_cast<size_t>(n_layers) * B * T * D * sizeof(float);
}

extern "C" size_t lr_autoint_fwd_saved_bytes(int64_t B, int T, int D, int H, int n_layers, const int* head_dims) {
  (void)B, (void)T, (void)D, (void)H, (void)n_layers, (void)head_dims;
  return 0;                            // the backward recomputes Q, Kx, V, P and O from the layer outputs
}

extern "C" size_t lr_autoint_bwd_ws_bytes(int64_t B, int T, int D, int H, int n_layers, const int* head_dims) {
  if (B < 0 || !ai_shape_ok(T, D, H, n_layers, head_dims)) return 0;
  const AiArgs a = ai_args(B, T, D, H, n_layers, head_dims, 0);
  return static_cast<size_t>(ai_bwd_groups(a)) * ai_n_params(a) * sizeof(float);
}

extern "C" int lr_autoint_fwd_f32(const float* x, int64_t B, int T, int D, int H, int n_layers, const int* head_dims,
                                  int residual, const float* params, float* acts, size_t acts_bytes, void* saved,
                                  size_t saved_bytes, float* logits, lr_stream_t stream) {
  (void)saved;
  (void)saved_bytes;
  if (!ai_shape_ok(T, D, H, n_layers, head_dims)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && params);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(x && logits);
  if (acts != nullptr && acts_bytes < lr_autoint_fwd_acts_bytes(B, T, D, n_layers)) return LR_EWORKSPACE;
  const AiArgs a = ai_args(B, T, D, H, n_layers, head_dims, residual);
  const int TB = ai_tb(a, false);
  const size_t lds = ai_lds_bytes(a, TB, false);
  const int rc = ai_set_lds(ai_fwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(ai_fwd_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, as_stream(stream), a, x,
                     params, TB, acts, logits);
  return launch_status();
}

extern "C" int lr_autoint_bwd_f32(const float* x, int64_t B, int T, int D, int H, int n_layers, const int* head_dims,
                                  int residual, const float* params, const float* acts, const void* saved,
                                  const float* glogits, float* gx, float* gparams, void* ws, size_t ws_bytes,
                                  lr_stream_t stream) {
  (void)saved;
  if (!ai_shape_ok(T, D, H, n_layers, head_dims)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && params && gparams);
  if (ws_bytes < lr_autoint_bwd_ws_bytes(B, T, D, H, n_layers, head_dims)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (x && acts && glogits && gx && ws));
  const AiArgs a = ai_args(B, T, D, H, n_layers, head_dims, residual);
  hipStream_t st = as_stream(stream);
  const int64_t np = ai_n_params(a);
  float* part = static_cast<float*>(ws);
  const int groups = B > 0 ? ai_bwd_groups(a) : 0;
  if (B > 0) {
    const int TB = ai_tb(a, true);
    const size_t lds = ai_lds_bytes(a, TB, true);
    const int rc = ai_set_lds(ai_bwd_kernel, lds);
    if (rc != LR_OK) return rc;
    hipLaunchKernelGGL(ai_bwd_kernel, dim3(groups), dim3(kBlock), lds, st, a, x, params, TB, ceil_div(B, TB), acts, glogits, gx, np,
                       part);
  }
  hipLaunchKernelGGL(ai_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(np, kBlock))), dim3(kBlock), 0, st, part, groups, np,
                     gparams);
  return launch_status();
}
