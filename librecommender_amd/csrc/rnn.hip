// One recurrent layer (GRU / LSTM) over a padded, left-aligned batch, f32: the Keras arithmetic of the reference's TF2
// branch (`libreco/layers/recurrent.py:27-45`: GRU with reset_after=True, gate order z, r, h; LSTM with gate order i, f, c, o;
// a sequence mask that carries the state through the steps t >= len).
//   rnn_fwd_kernel     a workgroup owns TB samples for all L steps.  A lane group of jw lanes (the power of two >= H, at least
//                      16) owns SB samples; lane j of it owns hidden unit j of them: the G gate columns of that unit are G
//                      dot products over the D + H inputs, which the group reads from LDS (x_t * in_mask and
//                      h * rec_mask, stored [input][sample] so that the SB samples of a lane are one broadcast read per
//                      sample) while the weights stream from L2 (adjacent lanes read adjacent columns, a weight is used SB
//                      times).  The weights are (D + H) G H floats: 98 KB at 64 / 64 for a GRU, 393 KB at 128 / 128: they are
//                      re-read per step, they do not live in LDS.  The gates, and for the LSTM the cell state, are saved.
//   rnn_bwd_kernel     the same mapping, backwards in time.  The gate pre-activation gradients of a step go to LDS and to
//                      the workspace; the carried dh and gx = dA W^T are contractions over the G H gate columns, read from the
//                      transposed weights (rnn_transpose_kernel) so that adjacent lanes read adjacent floats.
//   rnn_wgrad_kernel   gW = (x * in_mask)^T dA, gU = (h_prev * rec_mask)^T dA and gb over the B L rows, as tiles of 32 inputs
//                      x 64 gate columns per chunk of rows, into per-chunk partials;
//   rnn_reduce_kernel  adds the chunks in chunk order.  No float atomics: the same bits from run to run.
// A step is masked when t >= clamp(len, 0, L), or on the table path when its id is outside [0, V): the id is then never
// dereferenced, h (and c) are carried, hs[b, t] = the carried h, the saved gates and gx are 0.
#include <math.h>

#include "common.hpp"

namespace lr {

constexpr int kRnnMax = 128;       // D, H in [1, 128]
constexpr int kRnnMinGroup = 16;   // lanes of a sample group, at the least
constexpr int kWgTK = 32, kWgTC = 64, kWgRows = 32;
constexpr int kRnnMaxChunks = 256;

struct RnnIn {
  const float* x;          // [B, L, D] or null
  const float* table;      // [V, D] with ids [B, L] when x is null
  int64_t V;
  const int32_t* ids;
  const int32_t* lens;     // [B]
  const float* in_mask;    // [B, D] or null
  const float* rec_mask;   // [B, H] or null
  int64_t B;
  int L, D, H;
};

// 1 / (1 + e) in f64, rounded once: the f32 add and divide would each round, which doubles the gate's error (the f32 exp stays)
__device__ __forceinline__ float rnn_sigmoid(float v) {
  return static_cast<float>(1.0 / (1.0 + static_cast<double>(expf(-v))));
}

__device__ __forceinline__ int rnn_len(const RnnIn& a, int64_t b) {
  if (b >= a.B) return 0;
  const int l = a.lens[b];
  return l < 0 ? 0 : (l > a.L ? a.L : l);
}

// whether step t of sample b (whose clamped length is len) is a valid one; *id: its table row on the table path
__device__ __forceinline__ bool rnn_valid(const RnnIn& a, int64_t b, int t, int len, int64_t* id) {
  if (t >= len) return false;
  if (a.x != nullptr) return true;
  const int64_t v = a.ids[b * a.L + t];
  *id = v;
  return v >= 0 && v < a.V;
}

// ---- forward -------------------------------------------------------------------------------
template <int CELL, int SB>
__global__ __launch_bounds__(kBlock) void rnn_fwd_kernel(RnnIn a, const float* __restrict__ W, const float* __restrict__ U,
                                                         const float* __restrict__ bias, int act, int jw,
                                                         float* __restrict__ hs, float* __restrict__ saved) {
  extern __shared__ float lds[];
  constexpr int G = CELL == LR_RNN_GRU ? 3 : 4;
  constexpr int NS = CELL == LR_RNN_GRU ? 4 : 5;
  const int D = a.D, H = a.H, L = a.L, GH = G * H;
  const int nsg = kBlock / jw, TB = nsg * SB, TBP = TB | 1;
  float* xs = lds;                       // [D][TBP]  x_t * in_mask
  float* hm = xs + D * TBP;              // [H][TBP]  h * rec_mask
  int* slen = reinterpret_cast<int*>(hm + H * TBP);   // [TB]
  const int tid = threadIdx.x, j = tid % jw, sg = tid / jw;
  const bool jin = j < H;
  const int jc = jin ? j : H - 1;
  const int64_t blk0 = static_cast<int64_t>(blockIdx.x) * TB;
  for (int i = tid; i < TB; i += kBlock) slen[i] = rnn_len(a, blk0 + i);
  for (int i = tid; i < H * TBP; i += kBlock) hm[i] = 0.f;
  __syncthreads();
  float h[SB], c[SB], rm[SB];
  int len[SB];
#pragma unroll
  for (int s = 0; s < SB; ++s) {
    const int64_t b = blk0 + sg * SB + s;
    len[s] = slen[sg * SB + s];
    rm[s] = (a.rec_mask != nullptr && b < a.B) ? a.rec_mask[b * H + jc] : 1.f;
    h[s] = 0.f;
    c[s] = 0.f;
  }
  float b0, b1, b2, b3;
  if (CELL == LR_RNN_GRU) {
    b0 = bias[jc] + bias[3 * H + jc];
    b1 = bias[H + jc] + bias[4 * H + jc];
    b2 = bias[2 * H + jc];
    b3 = bias[5 * H + jc];
  } else {
    b0 = bias[jc];
    b1 = bias[H + jc];
    b2 = bias[2 * H + jc];
    b3 = bias[3 * H + jc];
  }
  for (int t = 0; t < L; ++t) {
    for (int idx = tid; idx < TB * D; idx += kBlock) {
      const int bb = idx / D, k = idx - bb * D;
      const int64_t b = blk0 + bb;
      int64_t id = 0;
      float v = 0.f;
      if (rnn_valid(a, b, t, slen[bb], &id)) {
        v = a.x != nullptr ? a.x[(b * L + t) * D + k] : a.table[id * D + k];
        if (a.in_mask != nullptr) v *= a.in_mask[b * D + k];
      }
      xs[k * TBP + bb] = v;
    }
    __syncthreads();
    float a0[SB], a1[SB], a2[SB], a3[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      a0[s] = b0;
      a1[s] = b1;
      a2[s] = b2;
      a3[s] = b3;
    }
    const float* xp = xs + sg * SB;
#pragma unroll 4
    for (int k = 0; k < D; ++k) {
      const float* w = W + static_cast<int64_t>(k) * GH + jc;
      const float w0 = w[0], w1 = w[H], w2 = w[2 * H];
      const float w3 = CELL == LR_RNN_GRU ? 0.f : w[3 * H];
#pragma unroll
      for (int s = 0; s < SB; ++s) {
        const float xv = xp[k * TBP + s];
        a0[s] = fmaf(xv, w0, a0[s]);
        a1[s] = fmaf(xv, w1, a1[s]);
        a2[s] = fmaf(xv, w2, a2[s]);
        if (CELL != LR_RNN_GRU) a3[s] = fmaf(xv, w3, a3[s]);
      }
    }
    const float* hp = hm + sg * SB;
#pragma unroll 4
    for (int k = 0; k < H; ++k) {
      const float* u = U + static_cast<int64_t>(k) * GH + jc;
      const float u0 = u[0], u1 = u[H], u2 = u[2 * H];
      const float u3 = CELL == LR_RNN_GRU ? 0.f : u[3 * H];
#pragma unroll
      for (int s = 0; s < SB; ++s) {
        const float hv = hp[k * TBP + s];
        a0[s] = fmaf(hv, u0, a0[s]);
        a1[s] = fmaf(hv, u1, a1[s]);
        if (CELL == LR_RNN_GRU) {
          a3[s] = fmaf(hv, u2, a3[s]);      // mh_h stays apart from mx_h (reset_after)
        } else {
          a2[s] = fmaf(hv, u2, a2[s]);
          a3[s] = fmaf(hv, u3, a3[s]);
        }
      }
    }
    __syncthreads();                         // every read of xs / hm of this step is done
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const int64_t b = blk0 + sg * SB + s;
      int64_t id = 0;
      const bool ok = rnn_valid(a, b, t, len[s], &id);
      float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
      if (ok) {
        if (CELL == LR_RNN_GRU) {
          const float z = rnn_sigmoid(a0[s]), r = rnn_sigmoid(a1[s]);
          const float pre = fmaf(r, a3[s], a2[s]);
          const float cand = act ? tanhf(pre) : pre;
          h[s] = fmaf(z, h[s] - cand, cand);             // z h + (1 - z) c
          q0 = z;
          q1 = r;
          q2 = cand;
          q3 = a3[s];
        } else {
          const float gi = rnn_sigmoid(a0[s]), gf = rnn_sigmoid(a1[s]), go = rnn_sigmoid(a3[s]);
          const float cand = act ? tanhf(a2[s]) : a2[s];
          c[s] = fmaf(gf, c[s], gi * cand);
          h[s] = go * (act ? tanhf(c[s]) : c[s]);
          q0 = gi;
          q1 = gf;
          q2 = cand;
          q3 = go;
        }
      }
      if (jin && b < a.B) {
        const int64_t row = b * L + t;
        hs[row * H + j] = h[s];
        float* sv = saved + row * NS * H + j;
        sv[0] = q0;
        sv[H] = q1;
        sv[2 * H] = q2;
        sv[3 * H] = q3;
        if (CELL != LR_RNN_GRU) sv[4 * H] = c[s];        // the carried cell at a masked step
      }
      if (jin) hm[j * TBP + sg * SB + s] = h[s] * rm[s];
    }
    // the next step's staging writes xs only; its barrier orders these hm writes before the next reads
  }
}

// ---- backward: the recurrence -----------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rnn_transpose_kernel(const float* __restrict__ W, const float* __restrict__ U, int D,
                                                               int H, int GH, float* __restrict__ WT, float* __restrict__ UT) {
  const int64_t nW = static_cast<int64_t>(D) * GH, nU = static_cast<int64_t>(H) * GH;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < nW + nU; i += stride) {
    if (i < nW) {
      const int c = static_cast<int>(i / D), k = static_cast<int>(i - static_cast<int64_t>(c) * D);
      WT[i] = W[static_cast<int64_t>(k) * GH + c];        // WT [GH][D]
    } else {
      const int64_t q = i - nW;
      const int c = static_cast<int>(q / H), k = static_cast<int>(q - static_cast<int64_t>(c) * H);
      UT[q] = U[static_cast<int64_t>(k) * GH + c];        // UT [GH][H]
    }
  }
}

// dA [B, L, 4, H]: GRU (z, r, h through W, h through U), LSTM (i, f, c, o)
template <int CELL, int SB>
__global__ __launch_bounds__(kBlock) void rnn_bwd_kernel(RnnIn a, const float* __restrict__ WT, const float* __restrict__ UT,
                                                         int act, int jw, const float* __restrict__ hs,
                                                         const float* __restrict__ saved, const float* __restrict__ ghs,
                                                         float* __restrict__ gx, float* __restrict__ dA) {
  extern __shared__ float lds[];
  constexpr int G = CELL == LR_RNN_GRU ? 3 : 4;
  constexpr int NS = CELL == LR_RNN_GRU ? 4 : 5;
  const int D = a.D, H = a.H, L = a.L, GH = G * H;
  const int nsg = kBlock / jw, TB = nsg * SB, TBP = TB | 1;
  float* ds = lds;                       // [4 H][TBP]
  const int tid = threadIdx.x, j = tid % jw, sg = tid / jw;
  const bool jin = j < H;
  const int jc = jin ? j : H - 1;
  const int64_t blk0 = static_cast<int64_t>(blockIdx.x) * TB;
  float dh[SB], dc[SB], rm[SB];
  int len[SB];
#pragma unroll
  for (int s = 0; s < SB; ++s) {
    const int64_t b = blk0 + sg * SB + s;
    len[s] = rnn_len(a, b);
    rm[s] = (a.rec_mask != nullptr && b < a.B) ? a.rec_mask[b * H + jc] : 1.f;
    dh[s] = 0.f;
    dc[s] = 0.f;
  }
  for (int t = L - 1; t >= 0; --t) {
    float direct[SB];
    bool ok[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) {
      const int64_t b = blk0 + sg * SB + s;
      int64_t id = 0;
      ok[s] = rnn_valid(a, b, t, len[s], &id);
      float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
      direct[s] = 0.f;
      if (jin && b < a.B) {
        const int64_t row = b * L + t;
        const float g = ghs[row * H + j] + dh[s];
        if (!ok[s]) {
          direct[s] = g;                                  // the state was carried
        } else {
          const float* sv = saved + row * NS * H + j;
          const float q0 = sv[0], q1 = sv[H], q2 = sv[2 * H], q3 = sv[3 * H];
          if (CELL == LR_RNN_GRU) {
            const float hprev = t > 0 ? hs[(row - 1) * H + j] : 0.f;
            const float dz = g * (hprev - q2);
            const float dpre = g * (1.f - q0) * (act ? 1.f - q2 * q2 : 1.f);
            d0 = dz * q0 * (1.f - q0);
            d1 = dpre * q3 * q1 * (1.f - q1);
            d2 = dpre;
            d3 = dpre * q1;
            direct[s] = g * q0;
          } else {
            const float cn = sv[4 * H];
            const float cprev = t > 0 ? saved[(row - 1) * NS * H + 4 * H + j] : 0.f;
            const float tc = act ? tanhf(cn) : cn;
            const float dcell = fmaf(g * q3, act ? 1.f - tc * tc : 1.f, dc[s]);
            d0 = dcell * q2 * q0 * (1.f - q0);
            d1 = dcell * cprev * q1 * (1.f - q1);
            d2 = dcell * q0 * (act ? 1.f - q2 * q2 : 1.f);
            d3 = g * tc * q3 * (1.f - q3);
            dc[s] = dcell * q1;
          }
        }
        float* o = dA + row * 4 * H + j;
        o[0] = d0;
        o[H] = d1;
        o[2 * H] = d2;
        o[3 * H] = d3;
      }
      if (jin) {
        float* o = ds + j * TBP + sg * SB + s;
        o[0] = d0;
        o[H * TBP] = d1;
        o[2 * H * TBP] = d2;
        o[3 * H * TBP] = d3;
      }
    }
    __syncthreads();
    const float* dp = ds + sg * SB;
    // the carried dh = direct + rec_mask * sum_c dA_U[c] U[j, c]
    float acc[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) acc[s] = 0.f;
#pragma unroll 4
    for (int cidx = 0; cidx < GH; ++cidx) {
      const int src = (CELL == LR_RNN_GRU && cidx >= 2 * H) ? cidx + H : cidx;
      const float u = UT[static_cast<int64_t>(cidx) * H + jc];
#pragma unroll
      for (int s = 0; s < SB; ++s) acc[s] = fmaf(dp[src * TBP + s], u, acc[s]);
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) dh[s] = fmaf(rm[s], acc[s], direct[s]);
    // gx[b, t, k] = in_mask * sum_c dA_W[c] W[k, c]
    for (int k = j; k < D; k += jw) {
#pragma unroll
      for (int s = 0; s < SB; ++s) acc[s] = 0.f;
#pragma unroll 4
      for (int cidx = 0; cidx < GH; ++cidx) {
        const float w = WT[static_cast<int64_t>(cidx) * D + k];
#pragma unroll
        for (int s = 0; s < SB; ++s) acc[s] = fmaf(dp[cidx * TBP + s], w, acc[s]);
      }
#pragma unroll
      for (int s = 0; s < SB; ++s) {
        const int64_t b = blk0 + sg * SB + s;
        if (b < a.B) {
          float v = acc[s];
          if (a.in_mask != nullptr) v *= a.in_mask[b * D + k];
          gx[(b * L + t) * D + k] = ok[s] ? v : 0.f;
        }
      }
    }
    __syncthreads();
  }
}

// ---- backward: the weight gradients ------------------------------------------------------
// side 0: rows k < D of gW from x * in_mask, row D = gb (GRU: gb[0]); side 1: rows k < H of gU from h_prev * rec_mask, row H =
// gb[1] of the GRU.  part [chunk][side 0: (D + 1) GH | side 1: (H + 1) GH].
template <int CELL>
__global__ __launch_bounds__(kBlock) void rnn_wgrad_kernel(RnnIn a, const float* __restrict__ hs, const float* __restrict__ dA,
                                                           int64_t rows_per_chunk, float* __restrict__ part) {
  __shared__ float As[kWgRows][kWgTK + 4];
  __shared__ float Ds[kWgRows][kWgTC];
  constexpr int G = CELL == LR_RNN_GRU ? 3 : 4;
  const int D = a.D, H = a.H, L = a.L, GH = G * H;
  const int side = blockIdx.z;
  const int K = side == 0 ? D : H;                       // + the bias row K (side 1: the GRU only)
  const int KB = (side == 0 || CELL == LR_RNN_GRU) ? K + 1 : K;
  const int tiles_c = (GH + kWgTC - 1) / kWgTC;
  const int tk = blockIdx.x / tiles_c, tc = blockIdx.x - tk * tiles_c;
  const int k0 = tk * kWgTK, c0 = tc * kWgTC;
  if (k0 >= KB) return;
  const int tid = threadIdx.x, cl = tid % kWgTC, kg = tid / kWgTC;
  const int64_t R = a.B * L;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_chunk;
  const int64_t r1 = r0 + rows_per_chunk < R ? r0 + rows_per_chunk : R;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  for (int64_t rb = r0; rb < r1; rb += kWgRows) {
    for (int idx = tid; idx < kWgRows * kWgTK; idx += kBlock) {
      const int r = idx / kWgTK, kk = idx - r * kWgTK;
      const int64_t row = rb + r;
      const int k = k0 + kk;
      float v = 0.f;
      if (row < r1 && k < KB) {
        const int64_t b = row / L;
        const int t = static_cast<int>(row - b * L);
        int64_t id = 0;
        if (rnn_valid(a, b, t, rnn_len(a, b), &id)) {
          if (k == K) {
            v = 1.f;
          } else if (side == 0) {
            v = a.x != nullptr ? a.x[row * D + k] : a.table[id * D + k];
            if (a.in_mask != nullptr) v *= a.in_mask[b * D + k];
          } else {
            v = t > 0 ? hs[(row - 1) * H + k] : 0.f;
            if (a.rec_mask != nullptr) v *= a.rec_mask[b * H + k];
          }
        }
      }
      As[r][kk] = v;
    }
    for (int idx = tid; idx < kWgRows * kWgTC; idx += kBlock) {
      const int r = idx / kWgTC, cc = idx - r * kWgTC;
      const int64_t row = rb + r;
      const int c = c0 + cc;
      float v = 0.f;
      if (row < r1 && c < GH) {
        const int src = (CELL == LR_RNN_GRU && side == 1 && c >= 2 * H) ? c + H : c;
        v = dA[row * 4 * H + src];
      }
      Ds[r][cc] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < kWgRows; ++r) {
      const float d = Ds[r][cl];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(As[r][kg * 8 + i], d, acc[i]);
    }
    __syncthreads();
  }
  const int64_t per_chunk = static_cast<int64_t>(D + 1 + H + 1) * GH;
  float* out = part + static_cast<int64_t>(blockIdx.y) * per_chunk + (side == 0 ? 0 : static_cast<int64_t>(D + 1) * GH);
  const int c = c0 + cl;
  if (c < GH) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = k0 + kg * 8 + i;
      if (k < KB) out[static_cast<int64_t>(k) * GH + c] = acc[i];
    }
  }
}

template <int CELL>
__global__ __launch_bounds__(kBlock) void rnn_reduce_kernel(const float* __restrict__ part, int n_chunks, int D, int H,
                                                            float* __restrict__ gW, float* __restrict__ gU,
                                                            float* __restrict__ gb) {
  constexpr int G = CELL == LR_RNN_GRU ? 3 : 4;
  const int GH = G * H;
  const int64_t per_chunk = static_cast<int64_t>(D + 1 + H + 1) * GH;
  const int64_t n = CELL == LR_RNN_GRU ? per_chunk : per_chunk - GH;       // the LSTM has no second bias row
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  double t = 0.0;
  for (int ch = 0; ch < n_chunks; ++ch) t += static_cast<double>(part[static_cast<int64_t>(ch) * per_chunk + i]);   // chunk order
  const float v = static_cast<float>(t);
  const int64_t nW = static_cast<int64_t>(D) * GH, oU = nW + GH, nU = static_cast<int64_t>(H) * GH;
  if (i < nW) {
    gW[i] = v;
  } else if (i < oU) {
    gb[i - nW] = v;
  } else if (i < oU + nU) {
    gU[i - oU] = v;
  } else {
    gb[GH + (i - oU - nU)] = v;
  }
}

// ---- host ------------------------------------------------------------------------------------
static inline int rnn_group(int H) {
  int jw = kRnnMinGroup;
  while (jw < H) jw *= 2;
  return jw;
}
// samples per lane: four when that still leaves a workgroup for every compute unit, else one
static inline int rnn_sb(int64_t B, int jw) { return ceil_div(B, (kBlock / jw) * 4) >= kNumCU ? 4 : 1; }
static inline size_t rnn_align(size_t x) { return (x + 255) / 256 * 256; }
static inline int rnn_chunks(int64_t R, int D, int H, int GH) {
  const int64_t tiles = (ceil_div(D + 1, kWgTK) + ceil_div(H + 1, kWgTK)) * ceil_div(GH, kWgTC);
  int64_t n = ceil_div(R, 128);
  const int64_t want = ceil_div(4 * kNumCU, tiles);
  if (n > want) n = want;
  if (n > kRnnMaxChunks) n = kRnnMaxChunks;
  return n < 1 ? 1 : static_cast<int>(n);
}

template <int CELL, int SB>
static int rnn_fwd_launch(hipStream_t st, const RnnIn& a, const float* W, const float* U, const float* b, int act, int jw,
                          float* hs, float* saved) {
  const int TB = (kBlock / jw) * SB, TBP = TB | 1;
  const size_t lds = static_cast<size_t>(a.D + a.H) * TBP * 4 + static_cast<size_t>(TB) * 4;
  hipLaunchKernelGGL((rnn_fwd_kernel<CELL, SB>), dim3(static_cast<unsigned>(ceil_div(a.B, TB))), dim3(kBlock), lds, st, a, W,
                     U, b, act, jw, hs, saved);
  return launch_status();
}

template <int CELL, int SB>
static int rnn_bwd_launch(hipStream_t st, const RnnIn& a, const float* WT, const float* UT, int act, int jw, const float* hs,
                          const float* saved, const float* ghs, float* gx, float* dA) {
  const int TB = (kBlock / jw) * SB, TBP = TB | 1;
  const size_t lds = static_cast<size_t>(4 * a.H) * TBP * 4;
  hipLaunchKernelGGL((rnn_bwd_kernel<CELL, SB>), dim3(static_cast<unsigned>(ceil_div(a.B, TB))), dim3(kBlock), lds, st, a, WT,
                     UT, act, jw, hs, saved, ghs, gx, dA);
  return launch_status();
}

template <int CELL>
static int rnn_wgrad_launch(hipStream_t st, const RnnIn& a, const float* hs, const float* dA, float* part, float* gW, float* gU,
                            float* gb) {
  constexpr int G = CELL == LR_RNN_GRU ? 3 : 4;
  const int GH = G * a.H;
  const int64_t R = a.B * a.L;
  const int nch = rnn_chunks(R, a.D, a.H, GH);
  const int64_t rows_per_chunk = ceil_div(ceil_div(R, nch), kWgRows) * kWgRows;
  const int tiles_k = static_cast<int>(ceil_div((a.D > a.H ? a.D : a.H) + 1, kWgTK));
  const int tiles_c = static_cast<int>(ceil_div(GH, kWgTC));
  hipLaunchKernelGGL((rnn_wgrad_kernel<CELL>), dim3(tiles_k * tiles_c, nch, 2), dim3(kBlock), 0, st, a, hs, dA, rows_per_chunk,
                     part);
  const int64_t n = static_cast<int64_t>(a.D + 1 + a.H + 1) * GH;
  hipLaunchKernelGGL((rnn_reduce_kernel<CELL>), dim3(static_cast<unsigned>(ceil_div(n, kBlock))), dim3(kBlock), 0, st, part, nch,
                     a.D, a.H, gW, gU, gb);
  return launch_status();
}

static bool rnn_args_ok(const RnnIn& a) {
  if (a.B < 0 || a.L < 1 || a.lens == nullptr) return false;
  if (a.x == nullptr && (a.table == nullptr || a.ids == nullptr || a.V < 1)) return false;
  return a.B * a.L < (int64_t{1} << 40);
}

}  // namespace lr

using namespace lr;

extern "C" int lr_rnn_supported(int cell, int D, int H) {
  return (cell == LR_RNN_GRU || cell == LR_RNN_LSTM) && D >= 1 && D <= kRnnMax && H >= 1 && H <= kRnnMax ? 1 : 0;
}

extern "C" size_t lr_rnn_fwd_saved_bytes(int cell, int64_t B, int L, int H) {
  if (B < 0 || L < 1 || H < 1) return 0;
  return static_cast<size_t>(B) * L * (cell == LR_RNN_GRU ? 4 : 5) * H * sizeof(float);
}

extern "C" size_t lr_rnn_bwd_ws_bytes(int cell, int64_t B, int L, int D, int H) {
  if (!lr_rnn_supported(cell, D, H) || B < 0 || L < 1) return 0;
  const int GH = (cell == LR_RNN_GRU ? 3 : 4) * H;
  const size_t dA = rnn_align(static_cast<size_t>(B) * L * 4 * H * 4);
  const size_t wt = rnn_align(static_cast<size_t>(D + H) * GH * 4);
  const size_t part = static_cast<size_t>(rnn_chunks(B * L, D, H, GH)) * (D + 1 + H + 1) * GH * 4;
  return dA + wt + rnn_align(part);
}

extern "C" int lr_rnn_layer_fwd_f32(int cell, int act, const float* x, const float* table, int64_t V, const int32_t* ids,
                                    const int32_t* lens, int64_t B, int L, int D, int H, const float* W, const float* U,
                                    const float* b, const float* in_mask, const float* rec_mask, float* hs, void* saved,
                                    size_t saved_bytes, lr_stream_t stream) {
  if (!lr_rnn_supported(cell, D, H)) return LR_ESHAPE;
  RnnIn a{x, table, V, ids, lens, in_mask, rec_mask, B, L, D, H};
  LR_CHECK_ARG(rnn_args_ok(a));
  if (B == 0) return LR_OK;
  LR_CHECK_ARG(W && U && b && hs && saved);
  if (saved_bytes < lr_rnn_fwd_saved_bytes(cell, B, L, H)) return LR_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const int jw = rnn_group(H);
  float* sv = static_cast<float*>(saved);
  if (rnn_sb(B, jw) == 4) {
    return cell == LR_RNN_GRU ? rnn_fwd_launch<LR_RNN_GRU, 4>(st, a, W, U, b, act, jw, hs, sv)
                              : rnn_fwd_launch<LR_RNN_LSTM, 4>(st, a, W, U, b, act, jw, hs, sv);
  }
  return cell == LR_RNN_GRU ? rnn_fwd_launch<LR_RNN_GRU, 1>(st, a, W, U, b, act, jw, hs, sv)
                            : rnn_fwd_launch<LR_RNN_LSTM, 1>(st, a, W, U, b, act, jw, hs, sv);
}

extern "C" int lr_rnn_layer_bwd_f32(int cell, int act, const float* x, const float* table, int64_t V, const int32_t* ids,
                                    const int32_t* lens, int64_t B, int L, int D, int H, const float* W, const float* U,
                                    const float* in_mask, const float* rec_mask, const float* hs, const void* saved,
                                    const float* ghs, float* gx, float* gW, float* gU, float* gb, void* ws, size_t ws_bytes,
                                    lr_stream_t stream) {
  if (!lr_rnn_supported(cell, D, H)) return LR_ESHAPE;
  RnnIn a{x, table, V, ids, lens, in_mask, rec_mask, B, L, D, H};
  LR_CHECK_ARG(rnn_args_ok(a));
  LR_CHECK_ARG(W && U && gW && gU && gb && ws);
  if (ws_bytes < lr_rnn_bwd_ws_bytes(cell, B, L, D, H)) return LR_EWORKSPACE;
  LR_CHECK_ARG(B == 0 || (hs && saved && ghs && gx));
  hipStream_t st = as_stream(stream);
  const int GH = (cell == LR_RNN_GRU ? 3 : 4) * H;
  char* p = static_cast<char*>(ws);
  float* dA = reinterpret_cast<float*>(p);
  p += rnn_align(static_cast<size_t>(B) * L * 4 * H * 4);
  float* WT = reinterpret_cast<float*>(p);
  float* UT = WT + static_cast<size_t>(D) * GH;
  p += rnn_align(static_cast<size_t>(D + H) * GH * 4);
  float* part = reinterpret_cast<float*>(p);
  const float* sv = static_cast<const float*>(saved);
  if (B > 0) {
    hipLaunchKernelGGL(rnn_transpose_kernel, dim3(grid_for(static_cast<int64_t>(D + H) * GH, kBlock)), dim3(kBlock), 0, st, W, U,
                       D, H, GH, WT, UT);
    const int jw = rnn_group(H);
    int rc;
    if (rnn_sb(B, jw) == 4) {
      rc = cell == LR_RNN_GRU ? rnn_bwd_launch<LR_RNN_GRU, 4>(st, a, WT, UT, act, jw, hs, sv, ghs, gx, dA)
                              : rnn_bwd_launch<LR_RNN_LSTM, 4>(st, a, WT, UT, act, jw, hs, sv, ghs, gx, dA);
    } else {
      rc = cell == LR_RNN_GRU ? rnn_bwd_launch<LR_RNN_GRU, 1>(st, a, WT, UT, act, jw, hs, sv, ghs, gx, dA)
                              : rnn_bwd_launch<LR_RNN_LSTM, 1>(st, a, WT, UT, act, jw, hs, sv, ghs, gx, dA);
    }
    if (rc != LR_OK) return rc;
  }
  return cell == LR_RNN_GRU ? rnn_wgrad_launch<LR_RNN_GRU>(st, a, hs, dA, part, gW, gU, gb)
                            : rnn_wgrad_launch<LR_RNN_LSTM>(st, a, hs, dA, part, gW, gU, gb);
}
