// NCF (He et al. 2017; libreco/algorithms/ncf.py of the reference): the two-field front and back of a training step and the
// whole inference tower in one launch.
//
//   u = table[user row], i = table[item row]            x = [u | i]  (the MLP's input)      gmf = u * i  (one f32 multiply)
//   h_1 = relu(x W_1 + b_1) * s_1 + t_1, ..., h_L = h_{L-1} W_L + b_L  (bare)               logit = gmf . wg + h_L . wd + c
//
// The DeepFM kernels form the pairwise term as 0.5((u+i)^2 - u^2 - i^2): for two fields that is u*i only up to an error of
// order eps * u^2 (tests/test_ncf_cpu.py pins a pair where the two differ), so the product has its own kernel here.
//
//   ncf_pair_fwd_kernel   gathers both rows of every sample, writes x [B, 2K] and gmf [B, K]; 16-byte loads and stores
//   ncf_pair_bwd_kernel   adds the GMF path to the MLP's row gradient G [B, 2K] in place
//   ncf_score_kernel      the inference tower: 256 threads take 64 samples per pass and are persistent over the tiles, so the
//                         weights are staged into LDS once per workgroup.  Products run on v_mfma_f32_32x32x2_f32 from k-major
//                         LDS operands (the scheme of mfma_tile in csrc/deepfm_tail.hip: per output element one k-ordered f32 fma
//                         chain); the activations ping-pong between two transposed [width][68] LDS tiles.  No atomics, no
//                         grid barrier, no spin wait: every output is computed by one workgroup from its own tile.
//
// LDS banking (ds_read_b32 banks = dword address mod 32 per 32-lane half): an MFMA operand read is 32 consecutive floats per
// lane half, conflict-free at any row stride.  The activation tiles' row stride of 68 floats keeps a column's four-row
// pieces 16-byte aligned for the epilogue's ds_write_b128 and spreads the 32 columns of a lane half over all banks
// (68 j mod 32 = 4 j mod 32: eight distinct four-bank slots, the minimum two passes for 16 lanes x 16 bytes).
#include "common.hpp"

namespace lr {

constexpr int kNcfTile = 64;              // samples per pass of a workgroup
constexpr int kNcfTP = kNcfTile + 4;      // row stride of the transposed activation tiles
constexpr int kNcfMaxLayers = 4;
constexpr int kNcfMaxWidth = 256;
constexpr int kNcfMaxK = 128;
constexpr size_t kNcfLdsBytes = 160 * 1024;

__device__ __forceinline__ float4 ncf_row4(const float* __restrict__ table, int64_t V, int K, int32_t row, int c4) {
  return (row >= 0 && row < V) ? ld4(table + static_cast<int64_t>(row) * K + c4) : f4_zero();
}

// ---------------------------------------------------------------------------------------------------
// front: x[b] = [table[idx[b,0]] | table[idx[b,1]]], gmf[b] = u * i.  One thread per 4-wide piece of a sample.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ncf_pair_fwd_kernel(const float* __restrict__ table, int64_t V, int K,
                                                             const int32_t* __restrict__ idx, int64_t B,
                                                             float* __restrict__ x, float* __restrict__ gmf) {
  const int kq = K / 4;
  const int64_t total = B * kq;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < total;
       q += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t b = q / kq;
    const int c4 = static_cast<int>(q - b * kq) * 4;
    const float4 u = ncf_row4(table, V, K, idx[2 * b], c4);
    const float4 i = ncf_row4(table, V, K, idx[2 * b + 1], c4);
    float* xr = x + b * 2 * K;
    st4(xr + c4, u);
    st4(xr + K + c4, i);
    st4(gmf + b * K + c4, f4_mul(u, i));
  }
}

// ---------------------------------------------------------------------------------------------------
// back: G[b, k] += (gl[b] wg[k]) x[b, K + k],  G[b, K + k] += (gl[b] wg[k]) x[b, k]   (one fma each)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ncf_pair_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gl,
                                                             const float* __restrict__ wg, float* __restrict__ G, int64_t B,
                                                             int K) {
  const int kq = K / 4;
  const int64_t total = B * kq;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; q < total;
       q += static_cast<int64_t>(gridDim.x) * kBlock) {
    const int64_t b = q / kq;
    const int c4 = static_cast<int>(q - b * kq) * 4;
    const float4 c = f4_scale(ld4(wg + c4), gl[b]);
    const float* xr = x + b * 2 * K;
    float* gr = G + b * 2 * K;
    const float4 u = ld4(xr + c4), i = ld4(xr + K + c4);
    st4(gr + c4, f4_fma(c, i, ld4(gr + c4)));
    st4(gr + K + c4, f4_fma(c, u, ld4(gr + K + c4)));
  }
}

// ---------------------------------------------------------------------------------------------------
// the inference tower
// ---------------------------------------------------------------------------------------------------
struct NcfScoreArgs {
  const float* table; int64_t V; int K;
  const int32_t* users; const int32_t* items; int64_t n;
  int n_layers;
  int width[kNcfMaxLayers];            // d_out of layer l
  int ldw[kNcfMaxLayers];              // its column stride in LDS: d_out rounded up to 32 (the pad columns hold zeros)
  int w_off[kNcfMaxLayers];            // float offset of its [d_in][ldw] weights in LDS
  int act_off[2];                      // float offsets of the two activation tiles
  const float* W[kNcfMaxLayers]; const float* b[kNcfMaxLayers];
  const float* s[kNcfMaxLayers]; const float* t[kNcfMaxLayers];       // nullable: identity
  const float* wg; const float* wd; float c; float* out;
};

struct NcfPlan { NcfScoreArgs a; size_t lds_bytes; bool ok; };

// The envelope and the LDS layout: the single source of truth of lr_ncf_score_supported and the launcher.
static NcfPlan ncf_plan(int K, int n_layers, const int* widths) {
  NcfPlan p{};
  if (widths == nullptr || K < 4 || K > kNcfMaxK || K % 4 != 0 || n_layers < 1 || n_layers > kNcfMaxLayers) return p;
  int rows[2] = {2 * K, 0};            // tile 0 holds x and the outputs of the odd layers, tile 1 those of the even ones
  int off = 0, d_in = 2 * K;
  for (int l = 0; l < n_layers; ++l) {
    const int w = widths[l];
    if (w < 16 || w > kNcfMaxWidth || w % 16 != 0) return p;
    p.a.width[l] = w;
    p.a.ldw[l] = (w + 31) / 32 * 32;
    p.a.w_off[l] = off;
    off += d_in * p.a.ldw[l];
    int& r = rows[(l + 1) & 1];
    r = r > w ? r : w;
    d_in = w;
  }
  p.a.act_off[0] = off;
  p.a.act_off[1] = off + rows[0] * kNcfTP;
  p.lds_bytes = static_cast<size_t>(off + (rows[0] + rows[1]) * kNcfTP) * sizeof(float);
  p.a.K = K;
  p.a.n_layers = n_layers;
  p.ok = p.lds_bytes <= kNcfLdsBytes;
  return p;
}

using ncf_f32x16 = __attribute__((ext_vector_type(16))) float;

// One 32 x 32 output tile: acc[r] (row (r & 3) + 8 (r >> 2) + 4 h, column j; j = lane & 31, h = lane >> 5) +=
// sum_k A[k][row0 + row] * Bm[k][col0 + j], both operands k-major in LDS; Kd is a multiple of 8.
__device__ __forceinline__ void ncf_mfma_tile(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb, int Kd,
                                              int row0, int col0, ncf_f32x16& acc) {
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const float* ap = A + h * lda + row0 + j;
  const float* bp = Bm + h * ldb + col0 + j;
  for (int k = 0; k < Kd; k += 8) {
    const float a0 = ap[k * lda], a1 = ap[(k + 2) * lda], a2 = ap[(k + 4) * lda], a3 = ap[(k + 6) * lda];
    const float b0 = bp[k * ldb], b1 = bp[(k + 2) * ldb], b2 = bp[(k + 4) * ldb], b3 = bp[(k + 6) * ldb];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc, 0, 0, 0);
  }
}

__global__ __launch_bounds__(kBlock) void ncf_score_kernel(const NcfScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ncf_smem[];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const int K = a.K, L = a.n_layers;
  float* const act[2] = {ncf_smem + a.act_off[0], ncf_smem + a.act_off[1]};
  // ---- the weights, once per workgroup: [d_in][ldw], columns past the layer's width zero -------------------------------
  {
    int d_in = 2 * K;
    for (int l = 0; l < L; ++l) {
      const int w = a.width[l], ldw = a.ldw[l], cq = ldw / 4;
      float* Wl = ncf_smem + a.w_off[l];
      const float* __restrict__ Wg = a.W[l];
      for (int q = tid; q < d_in * cq; q += kBlock) {
        const int r = q / cq, c4 = (q - r * cq) * 4;
        st4(Wl + r * ldw + c4, c4 < w ? ld4(Wg + r * w + c4) : f4_zero());
      }
      d_in = w;
    }
  }
  const int64_t n_tiles = ceil_div(a.n, kNcfTile);
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t s0 = tile * kNcfTile;
    __syncthreads();                   // the weights are staged / the previous tile's last reads of both tiles are done
    // ---- x = [u | i], transposed: act[0][k][sample]; samples past n and ids outside the table read as zero rows ---------
    {
      float* X = act[0];
      const int r = tid & 63;
      const int64_t smp = s0 + r;
      const bool live = smp < a.n;
      const int32_t ru = live ? a.users[smp] : -1, ri = live ? a.items[smp] : -1;
      for (int k4 = (tid >> 6) * 4; k4 < 2 * K; k4 += 4 * (kBlock / 64)) {
        const float4 v = k4 < K ? ncf_row4(a.table, a.V, K, ru, k4) : ncf_row4(a.table, a.V, K, ri, k4 - K);
        X[(k4 + 0) * kNcfTP + r] = v.x;
        X[(k4 + 1) * kNcfTP + r] = v.y;
        X[(k4 + 2) * kNcfTP + r] = v.z;
        X[(k4 + 3) * kNcfTP + r] = v.w;
      }
    }
    __syncthreads();
    // ---- the GMF term of sample `tid` (first wave), one k-ordered chain; act[0] is not written before the next barrier ---
    float gm = 0.f;
    if (tid < kNcfTile) {
      const float* X = act[0];
      for (int k = 0; k < K; ++k) gm = fmaf(X[k * kNcfTP + tid] * X[(K + k) * kNcfTP + tid], a.wg[k], gm);
    }
    // ---- the layers: 2 sample tiles x ldw / 32 column tiles of 32 x 32, dealt to the 4 waves -------------------------------
    int d_in = 2 * K;
    for (int l = 0; l < L; ++l) {
      const float* in = act[l & 1];
      float* out = act[(l + 1) & 1];
      const int w = a.width[l], ldw = a.ldw[l], CT = ldw / 32;
      const float* Wl = ncf_smem + a.w_off[l];
      const bool hidden = l != L - 1;
      for (int t = wid; t < 2 * CT; t += kBlock / 64) {
        const int rt = t / CT, ct = t - rt * CT;
        ncf_f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        ncf_mfma_tile(in, kNcfTP, Wl, ldw, d_in, rt * 32, ct * 32, acc);
        const int col = ct * 32 + j;
        if (col < w) {
          const float bv = a.b[l][col];
          const bool aff = hidden && a.s[l] != nullptr;
          const float sv = aff ? a.s[l][col] : 1.f, tv = aff ? a.t[l][col] : 0.f;
          float* op = out + col * kNcfTP + rt * 32 + 4 * h;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float y = acc[4 * g + e] + bv;
              if (hidden) {
                y = fmaxf(y, 0.f);
                if (aff) y = fmaf(y, sv, tv);
              }
              v[e] = y;
            }
            st4(op + 8 * g, make_float4(v[0], v[1], v[2], v[3]));
          }
        }
      }
      __syncthreads();
      d_in = w;
    }
    // ---- logit = gmf . wg + h_L . wd + c ------------------------------------------------------------------------------
    if (tid < kNcfTile && s0 + tid < a.n) {
      const float* H = act[L & 1];
      float d = 0.f;
      for (int c = 0; c < d_in; ++c) d = fmaf(H[c * kNcfTP + tid], a.wd[c], d);
      a.out[s0 + tid] = (gm + d) + a.c;
    }
  }
}

static inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace lr

using namespace lr;

extern "C" int lr_ncf_pair_fwd_f32(const float* table, int64_t V, int K, const int32_t* idx, int64_t B, float* x, float* gmf,
                                   lr_stream_t stream) {
  LR_CHECK_ARG(V >= 0 && B >= 0 && K >= 4 && K <= kNcfMaxK && K % 4 == 0);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(table && idx && x && gmf && aligned16(table) && aligned16(x) && aligned16(gmf));
  hipLaunchKernelGGL(ncf_pair_fwd_kernel, dim3(grid_for(B * (K / 4), kBlock)), dim3(kBlock), 0, as_stream(stream), table, V, K,
                     idx, B, x, gmf);
  return launch_status();
}

extern "C" int lr_ncf_pair_bwd_f32(const float* x, const float* gl, const float* wg, float* G, int64_t B, int K,
                                   lr_stream_t stream) {
  LR_CHECK_ARG(B >= 0 && K >= 4 && K <= kNcfMaxK && K % 4 == 0);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(x && gl && wg && G && aligned16(x) && aligned16(wg) && aligned16(G));
  hipLaunchKernelGGL(ncf_pair_bwd_kernel, dim3(grid_for(B * (K / 4), kBlock)), dim3(kBlock), 0, as_stream(stream), x, gl, wg, G,
                     B, K);
  return launch_status();
}

extern "C" int lr_ncf_score_supported(int K, int n_layers, const int* widths) {
  return ncf_plan(K, n_layers, widths).ok ? 1 : 0;
}

extern "C" int lr_ncf_score_f32(const float* table, int64_t V, int K, const int32_t* users, const int32_t* items, int64_t n,
                                int n_layers, const int* widths, const float* const* W, const float* const* b,
                                const float* const* s, const float* const* t, const float* wg, const float* wd, float c,
                                float* out, lr_stream_t stream) {
  LR_CHECK_ARG(V >= 0 && n >= 0 && widths != nullptr);
  NcfPlan p = ncf_plan(K, n_layers, widths);
  if (!p.ok) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(table && users && items && W && b && wg && wd && out && aligned16(table));
  LR_CHECK_ARG((s == nullptr) == (t == nullptr));
  NcfScoreArgs& a = p.a;
  for (int l = 0; l < n_layers; ++l) {
    LR_CHECK_ARG(W[l] && b[l] && aligned16(W[l]));
    a.W[l] = W[l];
    a.b[l] = b[l];
    a.s[l] = s != nullptr ? s[l] : nullptr;
    a.t[l] = t != nullptr ? t[l] : nullptr;
    LR_CHECK_ARG((a.s[l] == nullptr) == (a.t[l] == nullptr));
  }
  a.table = table; a.V = V; a.users = users; a.items = items; a.n = n;
  a.wg = wg; a.wd = wd; a.c = c; a.out = out;
  static bool lds_set = false;
  if (!lds_set && p.lds_bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ncf_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(kNcfLdsBytes));
    if (e != hipSuccess) return static_cast<int>(e);
    lds_set = true;
  }
  // persistent over the tiles: as many workgroups as the LDS lets a CU hold (at most 4), never more than there are tiles
  const int64_t per_cu = static_cast<int64_t>(kNcfLdsBytes / p.lds_bytes);
  const int grid = grid_for(n, kNcfTile, kNumCU * static_cast<int>(per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu)));
  hipLaunchKernelGGL(ncf_score_kernel, dim3(grid), dim3(kBlock), p.lds_bytes, as_stream(stream), a);
  return launch_status();
}
