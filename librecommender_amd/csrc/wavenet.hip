// The user side of WaveNet (`libreco/algorithms/wave_net.py:181-222`, the TF2 branch): a stack of kernel-size-2 dilated
// causal convolutions with ReLU over the rows of a sequence table that a window's ids name, a 1x1 convolution with ReLU and
// a max pool over time, f32 on the VALU.
//   wn_fwd_kernel      one launch for the whole stack.  A workgroup owns TB samples (R = TB L rows) for all layers; the
//                      activations of a layer live in LDS ([row][channel], two buffers that swap; at L = 128 and 128 channels
//                      that is 128 KB for one sample, which is why L, D and F stop at 128), every layer's output is also
//                      written to `acts`.  A lane group of jw lanes (the power of two >= the output width, at least 16) owns
//                      rows, lane j of it output channel j: the weights stream from L2 (adjacent lanes read adjacent output
//                      channels, a weight is used for kWnRows rows), the inputs are 16-byte broadcast reads from LDS.  A row
//                      whose earlier tap lies before the window reads a row of zeros: every position runs the same
//                      instruction sequence.
//   wn_bwd_kernel      the same tiling and the same contraction, backwards through the layers in gather form on the
//                      transposed weights (wn_transpose_kernel): da_j[t] = K_j[1] dz[t] + K_j[0] dz[t + d_j]; the
//                      pre-activation gradients of every layer go to LDS and to the workspace.
//   wn_wgrad_kernel    gK_j[tap] = a_j(shifted)^T dz_j and gb_j over the B L rows, as tiles of 32 inputs x 64 filters per
//                      chunk of rows, into per-chunk partials laid out like the parameters;
//   wn_reduce_kernel   adds the chunks in chunk order.  No float atomics: the same bits from run to run.
// An id outside [0, V) is never dereferenced: it is a zero input row and gets a gradient of exactly 0.
#include "common.hpp"

namespace lr {

constexpr int kWnMax = 128;        // L, D, F in [1, 128]
constexpr int kWnMaxLayers = 16;   // dilated layers
constexpr int kWnRows = 4;         // rows per lane and pass
constexpr int kWnTK = 32, kWnTC = 64, kWnChunkRows = 32;
constexpr int kWnMaxChunks = 256;
constexpr size_t kWnLdsSoft = 64 * 1024;

struct WnArgs {
  const float* table;      // [V, D]
  int64_t V;
  const int32_t* ids;      // [B, L]
  int64_t B;
  int L, D, F, nl, npb;    // nl dilated layers, dilation 2^(j mod npb); layer nl is the 1x1
  int S;                   // LDS row stride: max(D, F) rounded up to 4
};

__host__ __device__ inline int64_t wn_pad4(int64_t n) { return (n + 3) / 4 * 4; }
__host__ __device__ inline int wn_in(const WnArgs& a, int j) { return j == 0 ? a.D : a.F; }
__host__ __device__ inline int wn_taps(const WnArgs& a, int j) { return j < a.nl ? 2 : 1; }
// offset of layer j's kernel in the parameter buffer (j == nl + 1: the buffer's length); its bias follows the kernel
__host__ __device__ inline int64_t wn_kernel_off(const WnArgs& a, int j) {
  int64_t off = 0;
  for (int i = 0; i < j; ++i) off += wn_pad4(static_cast<int64_t>(wn_taps(a, i)) * wn_in(a, i) * a.F) + wn_pad4(a.F);
  return off;
}
__host__ __device__ inline int64_t wn_bias_off(const WnArgs& a, int j) {
  return wn_kernel_off(a, j) + wn_pad4(static_cast<int64_t>(wn_taps(a, j)) * wn_in(a, j) * a.F);
}
// element i of the parameter buffer -> its layer; *local: its offset from the layer's kernel
__device__ inline int wn_locate(const WnArgs& a, int64_t i, int64_t* local) {
  int64_t off = 0;
  for (int j = 0; j <= a.nl; ++j) {
    const int64_t n = wn_pad4(static_cast<int64_t>(wn_taps(a, j)) * wn_in(a, j) * a.F) + wn_pad4(a.F);
    if (i < off + n || j == a.nl) {
      *local = i - off;
      return j;
    }
    off += n;
  }
  return a.nl;
}

__device__ __forceinline__ bool wn_id_ok(const WnArgs& a, int64_t grow, int64_t* id) {
  const int64_t v = a.ids[grow];
  *id = v;
  return v >= 0 && v < a.V;
}

extern __shared__ float wn_lds[];      // [R][S] | [R][S] | zero row [S] | id validity [R] (backward)

// out[row][o] = epilogue(sum_c in[row + off][c] W0[c][o] + in[row][c] W1[c][o]) for the R rows of the tile and o < O; a row
// whose other tap leaves its own window reads `zrow`.  MODE 0: + bias, ReLU -> LDS and acts; 1: masked by the ReLU pattern of
// the layer below -> LDS and dZ; 2: masked by the id's validity -> gx.
// `in`, `out` and `zrow` are offsets into `wn_lds` (floats): the loads stay LDS instructions whichever row is chosen.

template <int MODE, bool TWO>
__device__ __forceinline__ void wn_conv(int in, int out, int zrow, int S, int R, int L, int C, int O, int off,
                                        const float* __restrict__ W0, const float* __restrict__ W1,
                                        const float* __restrict__ bias, float* __restrict__ gout,
                                        const float* __restrict__ gmask, const int* idok, int64_t row0, int64_t Rtot) {
  int jw = 16;
  while (jw < O) jw *= 2;
  const int ng = kBlock / jw, j = threadIdx.x % jw, g = threadIdx.x / jw;
  const int jc = j < O ? j : O - 1;
  const int C4 = (C + 3) & ~3, O4 = (O + 3) & ~3;
  const float b0 = MODE == 0 ? bias[jc] : 0.f;
  for (int base = 0; base < R; base += ng * kWnRows) {
    int p0[kWnRows], p1[kWnRows];
    float acc[kWnRows];
#pragma unroll
    for (int i = 0; i < kWnRows; ++i) {
      const int row = base + i * ng + g;
      p0[i] = zrow;
      p1[i] = zrow;
      if (row < R) {
        p1[i] = in + row * S;
        if (TWO) {
          const int ts = row % L + off;
          if (ts >= 0 && ts < L) p0[i] = in + (row + off) * S;
        }
      }
      acc[i] = b0;
    }
    for (int c = 0; c < C4; c += 4) {
      float w0[4], w1[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = c + q < C;
        const int64_t at = static_cast<int64_t>(ok ? c + q : C - 1) * O + jc;
        w1[q] = ok ? W1[at] : 0.f;
        w0[q] = (TWO && ok) ? W0[at] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kWnRows; ++i) {
        const float4 a1 = ld4(wn_lds + p1[i] + c);
        if (TWO) {
          const float4 a0 = ld4(wn_lds + p0[i] + c);
          acc[i] = fmaf(a0.x, w0[0], acc[i]);
          acc[i] = fmaf(a1.x, w1[0], acc[i]);
          acc[i] = fmaf(a0.y, w0[1], acc[i]);
          acc[i] = fmaf(a1.y, w1[1], acc[i]);
          acc[i] = fmaf(a0.z, w0[2], acc[i]);
          acc[i] = fmaf(a1.z, w1[2], acc[i]);
          acc[i] = fmaf(a0.w, w0[3], acc[i]);
          acc[i] = fmaf(a1.w, w1[3], acc[i]);
        } else {
          acc[i] = fmaf(a1.x, w1[0], acc[i]);
          acc[i] = fmaf(a1.y, w1[1], acc[i]);
          acc[i] = fmaf(a1.z, w1[2], acc[i]);
          acc[i] = fmaf(a1.w, w1[3], acc[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kWnRows; ++i) {
      const int row = base + i * ng + g;
      if (row >= R || j >= O4) continue;
      const int64_t grow = row0 + row;
      const bool live = j < O && grow < Rtot;
      float v = acc[i];
      if (MODE == 0) {
        v = v > 0.f ? v : 0.f;
        wn_lds[out + row * S + j] = j < O ? v : 0.f;       // the columns up to the next multiple of four are read, as zeros
        if (live) gout[grow * O + j] = v;
      } else if (MODE == 1) {
        v = (live && gmask[grow * O + j] > 0.f) ? v : 0.f;
        wn_lds[out + row * S + j] = v;
        if (live) gout[grow * O + j] = v;
      } else {
        if (live) gout[grow * O + j] = idok[row] ? v : 0.f;
      }
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------
// acts [nl + 1][B][L][F]
__global__ __launch_bounds__(kBlock) void wn_fwd_kernel(WnArgs a, const float* __restrict__ params, int TB,
                                                        float* __restrict__ acts, float* __restrict__ pooled,
                                                        int32_t* __restrict__ arg) {
  const int L = a.L, D = a.D, F = a.F, S = a.S, R = TB * L;
  int cur = 0, nxt = R * S;              // [R][S] each
  const int zrow = 2 * R * S;            // [S]
  const int tid = threadIdx.x;
  const int64_t blk0 = static_cast<int64_t>(blockIdx.x) * TB, row0 = blk0 * L, Rtot = a.B * L;
  for (int i = tid; i < S; i += kBlock) wn_lds[zrow + i] = 0.f;
  const int D4 = (D + 3) & ~3;
  for (int idx = tid; idx < R * D4; idx += kBlock) {
    const int row = idx / D4, k = idx - row * D4;
    const int64_t grow = row0 + row;
    int64_t id = 0;
    float v = 0.f;
    if (grow < Rtot && k < D && wn_id_ok(a, grow, &id)) v = a.table[id * D + k];
    wn_lds[cur + row * S + k] = v;
  }
  __syncthreads();
  for (int j = 0; j <= a.nl; ++j) {
    const int C = wn_in(a, j);
    const float* K = params + wn_kernel_off(a, j);
    const float* bias = params + wn_bias_off(a, j);
    float* ga = acts + static_cast<int64_t>(j) * Rtot * F;
    if (j < a.nl) {
      const int d = 1 << (j % a.npb);
      wn_conv<0, true>(cur, nxt, zrow, S, R, L, C, F, -d, K, K + static_cast<int64_t>(C) * F, bias, ga, nullptr, nullptr, row0, Rtot);
    } else {
      wn_conv<0, false>(cur, nxt, zrow, S, R, L, C, F, 0, K, K, bias, ga, nullptr, nullptr, row0, Rtot);
    }
    __syncthreads();
    const int t = cur;
    cur = nxt;
    nxt = t;
  }
  // the pool: the first t that attains the maximum
  for (int idx = tid; idx < TB * F; idx += kBlock) {
    const int s = idx / F, f = idx - s * F;
    const int64_t b = blk0 + s;
    if (b >= a.B) continue;
    const float* col = wn_lds + cur + s * L * S + f;
    float best = col[0];
    int at = 0;
    for (int t = 1; t < L; ++t) {
      const float v = col[t * S];
      if (v > best) {
        best = v;
        at = t;
      }
    }
    pooled[b * F + f] = best;
    arg[b * F + f] = at;
  }
}

// ---- backward: the stack ---------------------------------------------------------------------
// KT: the parameter layout with every kernel tap transposed, [tap][F][C]
__global__ __launch_bounds__(kBlock) void wn_transpose_kernel(WnArgs a, const float* __restrict__ params, int64_t n,
                                                              float* __restrict__ KT) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    int64_t local = 0;
    const int j = wn_locate(a, i, &local);
    const int C = wn_in(a, j), F = a.F;
    const int64_t CF = static_cast<int64_t>(C) * F;
    if (local >= wn_taps(a, j) * CF) continue;               // a bias or a gap: not read from KT
    const int tap = static_cast<int>(local / CF);
    const int64_t rem = local - tap * CF;
    const int f = static_cast<int>(rem / C), c = static_cast<int>(rem - static_cast<int64_t>(f) * C);
    KT[i] = params[i - local + tap * CF + static_cast<int64_t>(c) * F + f];
  }
}

// dZ [nl + 1][B][L][F]: the pre-activation gradient of every layer
__global__ __launch_bounds__(kBlock) void wn_bwd_kernel(WnArgs a, const float* __restrict__ KT, int TB,
                                                        const float* __restrict__ acts, const float* __restrict__ gpooled,
                                                        const int32_t* __restrict__ arg, float* __restrict__ gx,
                                                        float* __restrict__ dZ) {
  const int L = a.L, D = a.D, F = a.F, S = a.S, R = TB * L, nl = a.nl;
  int cur = 0, nxt = R * S;
  const int zrow = 2 * R * S;
  int* idok = reinterpret_cast<int*>(wn_lds + zrow + S);          // [R]
  const int tid = threadIdx.x;
  const int64_t blk0 = static_cast<int64_t>(blockIdx.x) * TB, row0 = blk0 * L, Rtot = a.B * L;
  for (int i = tid; i < S; i += kBlock) wn_lds[zrow + i] = 0.f;
  for (int row = tid; row < R; row += kBlock) {
    int64_t id = 0;
    idok[row] = (row0 + row < Rtot && wn_id_ok(a, row0 + row, &id)) ? 1 : 0;
  }
  const int F4 = (F + 3) & ~3;
  const int64_t slab = Rtot * F;
  for (int idx = tid; idx < R * F4; idx += kBlock) {
    const int row = idx / F4, f = idx - row * F4;
    const int64_t grow = row0 + row;
    float v = 0.f;
    if (grow < Rtot && f < F) {
      const int64_t b = grow / L;
      const int t = static_cast<int>(grow - b * L);
      if (arg[b * F + f] == t && acts[nl * slab + grow * F + f] > 0.f) v = gpooled[b * F + f];
      dZ[nl * slab + grow * F + f] = v;
    }
    wn_lds[cur + row * S + f] = v;
  }
  __syncthreads();
  for (int j = nl; j >= 0; --j) {
    const int C = wn_in(a, j);
    const float* K = KT + wn_kernel_off(a, j);
    const int d = 1 << (j % a.npb);
    if (j == nl) {
      wn_conv<1, false>(cur, nxt, zrow, S, R, L, F, C, 0, K, K, nullptr, dZ + (j - 1) * slab, acts + (j - 1) * slab, idok, row0, Rtot);
    } else if (j > 0) {
      wn_conv<1, true>(cur, nxt, zrow, S, R, L, F, C, d, K, K + static_cast<int64_t>(C) * F, nullptr, dZ + (j - 1) * slab,
                       acts + (j - 1) * slab, idok, row0, Rtot);
    } else {
      wn_conv<2, true>(cur, nxt, zrow, S, R, L, F, C, d, K, K + static_cast<int64_t>(C) * F, nullptr, gx, nullptr, idok, row0, Rtot);
    }
    __syncthreads();
    const int t = cur;
    cur = nxt;
    nxt = t;
  }
}

// ---- backward: the parameter gradients --------------------------------------------------------
// blockIdx.z = 2 * layer + tap.  Tap 1 (and the one tap of the 1x1 layer) carries the bias as input row C.
__global__ __launch_bounds__(kBlock) void wn_wgrad_kernel(WnArgs a, const float* __restrict__ acts, const float* __restrict__ dZ,
                                                          int64_t rows_per_chunk, int64_t n_params, float* __restrict__ part) {
  __shared__ float As[kWnChunkRows][kWnTK + 4];
  __shared__ float Ds[kWnChunkRows][kWnTC];
  const int L = a.L, D = a.D, F = a.F;
  const int j = blockIdx.z >> 1, tap = blockIdx.z & 1;
  const bool two = j < a.nl;
  if (!two && tap == 0) return;
  const int C = wn_in(a, j);
  const int KB = tap == 1 ? C + 1 : C;
  const int tiles_c = (F + kWnTC - 1) / kWnTC;
  const int tk = blockIdx.x / tiles_c, tc = blockIdx.x - tk * tiles_c;
  const int k0 = tk * kWnTK, c0 = tc * kWnTC;
  if (k0 >= KB) return;
  const int d = (two && tap == 0) ? 1 << (j % a.npb) : 0;
  const int tid = threadIdx.x, cl = tid % kWnTC, kg = tid / kWnTC;
  const int64_t R = a.B * L, slab = R * F;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < R ? r0 + rows_per_chunk : R;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int64_t rb = r0; rb < r1; rb += kWnChunkRows) {
    for (int idx = tid; idx < kWnChunkRows * kWnTK; idx += kBlock) {
      const int r = idx / kWnTK, kk = idx - r * kWnTK;
      const int64_t row = rb + r;
      const int k = k0 + kk;
      float v = 0.f;
      if (row < r1 && k < KB) {
        const int64_t b = row / L;
        const int t = static_cast<int>(row - b * L);
        if (k == C) {
          v = 1.f;
        } else if (t >= d) {
          const int64_t src = row - d;
          int64_t id = 0;
          if (j > 0) {
            v = acts[(j - 1) * slab + src * F + k];
          } else if (wn_id_ok(a, src, &id)) {
            v = a.table[id * D + k];
          }
        }
      }
      As[r][kk] = v;
    }
    for (int idx = tid; idx < kWnChunkRows * kWnTC; idx += kBlock) {
      const int r = idx / kWnTC, cc = idx - r * kWnTC;
      const int64_t row = rb + r;
      const int c = c0 + cc;
      Ds[r][cc] = (row < r1 && c < F) ? dZ[j * slab + row * F + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kWnChunkRows; ++r) {
      const float dv = Ds[r][cl];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(As[r][kg * 8 + i], dv, acc[i]);
    }
    __syncthreads();
  }
  float* out = part + static_cast<int64_t>(blockIdx.y) * n_params;
  const int64_t ko = wn_kernel_off(a, j) + (two ? static_cast<int64_t>(tap) * C * F : 0), bo = wn_bias_off(a, j);
  const int c = c0 + cl;
  if (c < F) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = k0 + kg * 8 + i;
      if (k < C) out[ko + static_cast<int64_t>(k) * F + c] = acc[i];
      else if (k < KB) out[bo + c] = acc[i];
    }
  }
}

__global__ __launch_bounds__(kBlock) void wn_reduce_kernel(WnArgs a, const float* __restrict__ part, int n_chunks,
                                                           int64_t n_params, float* __restrict__ gparams) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n_params) return;
  int64_t local = 0;
  const int j = wn_locate(a, i, &local);
  const int64_t nk = static_cast<int64_t>(wn_taps(a, j)) * wn_in(a, j) * a.F, nk4 = wn_pad4(nk);
  const bool gap = local < nk4 ? local >= nk : local - nk4 >= a.F;       // the alignment gaps hold no gradient: 0
  double t = 0.0;
  if (!gap)
    for (int ch = 0; ch < n_chunks; ++ch) t += static_cast<double>(part[static_cast<int64_t>(ch) * n_params + i]);   // chunk order
  gparams[i] = static_cast<float>(t);
}

// ---- host ------------------------------------------------------------------------------------
static inline size_t wn_align(size_t x) { return (x + 255) / 256 * 256; }
static inline bool wn_shape_ok(int L, int D, int F, int n_blocks, int n_per_block) {
  return L >= 1 && L <= kWnMax && D >= 1 && D <= kWnMax && F >= 1 && F <= kWnMax && n_blocks >= 1 && n_per_block >= 1 &&
         n_per_block <= kWnMaxLayers && n_blocks <= kWnMaxLayers && n_blocks * n_per_block <= kWnMaxLayers;
}
static inline WnArgs wn_args(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int D, int F, int n_blocks,
                             int n_per_block) {
  const int m = D > F ? D : F;
  return WnArgs{table, V, ids, B, L, D, F, n_blocks * n_per_block, n_per_block, (m + 3) & ~3};
}
static inline size_t wn_lds_bytes(const WnArgs& a, int TB) {
  return (static_cast<size_t>(2) * TB * a.L * a.S + a.S + static_cast<size_t>(TB) * a.L) * 4;
}
// samples per workgroup: as many as 64 KB of LDS hold, while that leaves two workgroups for every compute unit
static inline int wn_tb(const WnArgs& a) {
  int64_t tb = a.B / (2 * kNumCU);
  while (tb > 1 && wn_lds_bytes(a, static_cast<int>(tb)) > kWnLdsSoft) --tb;
  return tb < 1 ? 1 : static_cast<int>(tb);
}
static inline int wn_chunks(const WnArgs& a) {
  const int m = a.D > a.F ? a.D : a.F;
  const int64_t tiles = ceil_div(m + 1, kWnTK) * ceil_div(a.F, kWnTC) * 2 * (a.nl + 1);
  int64_t n = ceil_div(a.B * a.L, 128);
  const int64_t want = ceil_div(4 * kNumCU, tiles);
  if (n > want) n = want;
  if (n > kWnMaxChunks) n = kWnMaxChunks;
  return n < 1 ? 1 : static_cast<int>(n);
}
template <typename Kern>
static int wn_set_lds(Kern kern, size_t bytes) {
  if (bytes <= 48 * 1024) return LR_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     static_cast<int>(bytes));
  return e == hipSuccess ? LR_OK : static_cast<int>(e);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_wavenet_supported(int L, int D, int F, int n_blocks, int n_per_block) {
  return wn_shape_ok(L, D, F, n_blocks, n_per_block) ? 1 : 0;
}

extern "C" size_t lr_wavenet_params_bytes(int D, int F, int n_blocks, int n_per_block) {
  if (!wn_shape_ok(1, D, F, n_blocks, n_per_block)) return 0;
  const WnArgs a = wn_args(nullptr, 0, nullptr, 0, 1, D, F, n_blocks, n_per_block);
  return static_cast<size_t>(wn_kernel_off(a, a.nl + 1)) * sizeof(float);
}

extern "C" size_t lr_wavenet_fwd_acts_bytes(int64_t B, int L, int F, int n_blocks, int n_per_block) {
  if (B < 0 || !wn_shape_ok(L, 1, F, n_blocks, n_per_block)) return 0;
  return static_cast<size_t>(n_blocks * n_per_block + 1) * B * L * F * sizeof(float);
}

extern "C" size_t lr_wavenet_bwd_ws_bytes(int64_t B, int L, int D, int F, int n_blocks, int n_per_block) {
  if (B < 0 || !wn_shape_ok(L, D, F, n_blocks, n_per_block)) return 0;
  const WnArgs a = wn_args(nullptr, 0, nullptr, B, L, D, F, n_blocks, n_per_block);
  const size_t np = static_cast<size_t>(wn_kernel_off(a, a.nl + 1)) * 4;
  return wn_align(lr_wavenet_fwd_acts_bytes(B, L, F, n_blocks, n_per_block)) + wn_align(np) + wn_align(np * wn_chunks(a));
}

extern "C" int lr_wavenet_fwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int D, int F,
                                  int n_blocks, int n_per_block, const float* params, float* acts, size_t acts_bytes,
                                  float* pooled, int32_t* arg, lr_stream_t stream) {
  if (!wn_shape_ok(L, D, F, n_blocks, n_per_block)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params);
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(ids && acts && pooled && arg);
  if (acts_bytes < lr_wavenet_fwd_acts_bytes(B, L, F, n_blocks, n_per_block)) return LR_EWORKSPACE;
  const WnArgs a = wn_args(table, V, ids, B, L, D, F, n_blocks, n_per_block);
  const int TB = wn_tb(a);
  const size_t lds = wn_lds_bytes(a, TB);
  const int rc = wn_set_lds(wn_fwd_kernel, lds);
  if (rc != LR_OK) return rc;
  hipLaunchKernelGGL(wn_fwd_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, as_stream(stream), a, params,
                     TB, acts, pooled, arg);
  return launch_status();
}

extern "C" int lr_wavenet_bwd_f32(const float* table, int64_t V, const int32_t* ids, int64_t B, int L, int D, int F,
                                  int n_blocks, int n_per_block, const float* params, const float* acts,
                                  const float* gpooled, const int32_t* arg, float* gx, float* gparams, void* ws,
                                  size_t ws_bytes, lr_stream_t stream) {
  if (!wn_shape_ok(L, D, F, n_blocks, n_per_block)) return LR_ESHAPE;
  LR_CHECK_ARG(B >= 0 && V >= 1 && table && params && gparams && ws);
  if (ws_bytes < lr_wavenet_bwd_ws_bytes(B, L, D, F, n_blocks, n_per_block)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (ids && acts && gpooled && arg && gx));
  const WnArgs a = wn_args(table, V, ids, B, L, D, F, n_blocks, n_per_block);
  hipStream_t st = as_stream(stream);
  const int64_t np = wn_kernel_off(a, a.nl + 1);
  char* p = static_cast<char*>(ws);
  float* dZ = reinterpret_cast<float*>(p);
  p += wn_align(lr_wavenet_fwd_acts_bytes(B, L, F, n_blocks, n_per_block));
  float* KT = reinterpret_cast<float*>(p);
  p += wn_align(static_cast<size_t>(np) * 4);
  float* part = reinterpret_cast<float*>(p);
  if (B > 0) {
    hipLaunchKernelGGL(wn_transpose_kernel, dim3(grid_for(np, kBlock)), dim3(kBlock), 0, st, a, params, np, KT);
    const int TB = wn_tb(a);
    const size_t lds = wn_lds_bytes(a, TB);
    const int rc = wn_set_lds(wn_bwd_kernel, lds);
    if (rc != LR_OK) return rc;
    hipLaunchKernelGGL(wn_bwd_kernel, dim3(static_cast<unsigned>(ceil_div(B, TB))), dim3(kBlock), lds, st, a, KT, TB, acts,
                       gpooled, arg, gx, dZ);
  }
  const int nch = wn_chunks(a);
  const int64_t R = B * L;
  const int64_t rows_per_chunk = ceil_div(ceil_div(R > 0 ? R : 1, nch), kWnChunkRows) * kWnChunkRows;
  const int m = D > F ? D : F;
  const int tiles = static_cast<int>(ceil_div(m + 1, kWnTK) * ceil_div(F, kWnTC));
  hipLaunchKernelGGL(wn_wgrad_kernel, dim3(tiles, nch, 2 * (a.nl + 1)), dim3(kBlock), 0, st, a, acts, dZ, rows_per_chunk, np, part);
  hipLaunchKernelGGL(wn_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(np, kBlock))), dim3(kBlock), 0, st, a, part, nch, np,
                     gparams);
  return launch_status();
}
