// Alternating least squares (libreco/algorithms/_als.pyx): one half-sweep updates every row m of X against a fixed Y,
//   A_m = G0 + sum_i w_i y_i y_i^T,   b_m = sum_i beta_i y_i,
// implicit (ranking): G0 = Y^T Y + reg I, w = c - 1, beta = c;  explicit (rating): G0 = reg I, w = 1, beta = r,
// solved exactly (Cholesky, `posv`) or by cg_steps conjugate-gradient iterations from the current x.
//
// Rows are independent: every kernel below writes each output once, in a fixed summation order, with no atomics, so two
// runs give identical bits.  All arithmetic is f32 on the VALU.  Rows are split by degree (the plan, built once per fit on
// the host side from the CSR's row lengths, librecommender_amd/ops.py:als_plan):
//   light  (deg <= als_light_cap(K), CG only): one WAVE per row.  The row's y_i are gathered ONCE into the wave's slice of LDS,
//          G0 sits in LDS beside them (shared by the workgroup's four waves), and the residual and every CG step run from LDS:
//          the interactions cross HBM once per half-sweep instead of 1 + cg_steps times as in the reference.  Lane j holds
//          interaction j (dot products y_j . v), lane d holds dimension d (and d + 64) of x, r, p, Ap.  The cap (64 rows for
//          K <= 32, 32 above) keeps a workgroup under 54 KB of LDS at K = 64 so that three workgroups share a CU.
//   medium (cap < deg <= kHeavyDeg, and every non-heavy row of the direct solver): one WORKGROUP per row forms A_m = G0 +
//          Y_m^T diag(w) Y_m and b_m in registers (4 x 4 tiles of A per thread, 32 interactions staged in LDS at a time),
//          writes them to LDS and solves there (Cholesky, or the same CG iteration on the explicit A_m).  deg * K^2 work per
//          row, cheaper than the wave's 2 (1 + cg_steps) deg K once a row no longer fits the wave's LDS.
//   heavy  (deg > kHeavyDeg): under Zipf(1.05) the hottest of 10 M items holds 4.3 M of 200 M distinct pairs, far too many
//          for one workgroup.
//          The row's interactions are cut into kChunk-interaction chunks, each formed into a K x K (+ K) partial slab by its
//          own workgroup; a second kernel sums one row's slabs in chunk order onto G0 and solves as the medium path does.
//          4,096 interactions keep a chunk's slab traffic (17 KB at K = 64) small against its 1 MB of gathered rows.
#include "tile_csr.hpp"   // set_lds

namespace lr {
namespace {

constexpr int kMaxK = 128;
constexpr int kTJ = 32;            // interactions staged in LDS per step of the Gram formation
constexpr int kHeavyDeg = 4096;    // rows above this degree take the chunked path
constexpr int kChunk = 4096;       // interactions per partial slab of a heavy row
constexpr int kLightWaves = 4;     // waves (rows in flight) per workgroup of the light kernel
constexpr int kGramRows = 4096;    // rows of Y per workgroup of the G0 Gram

__host__ __device__ inline int pad4(int K) { return (K + 3) & ~3; }
__host__ __device__ inline int light_cap(int K) { return K <= 32 ? 64 : 32; }

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- workgroup Gram formation --------------------------------------------------------------------------------------
// acc[q][4u+v] += sum_j w_j y_j[4ta+u] y_j[4tb+v] over interactions [s, e) of the CSR (col != nullptr) or over rows [s, e) of
// Y (col == nullptr, w = 1); bacc (threads < Kp) += sum_j beta_j y_j[tid].  mode: 0 = plain Gram, 1 = implicit, 2 = explicit.
// The product w_j y_j[a] is formed first and then fma'd with y_j[b]: the reference's axpy(temp = (c - 1) y[a], y, A[a]).
__device__ void gram_rows(const int32_t* __restrict__ col, const float* __restrict__ val, int64_t s, int64_t e,
                          const float* __restrict__ Y, int K, int Kp, int mode, float* sY, float* sYw, float* sBeta,
                          float (&acc)[4][16], float& bacc) {
  const int tid = threadIdx.x;
  const int TK = Kp / 4;
  const int T = TK * TK;
  for (int64_t t0 = s; t0 < e; t0 += kTJ) {
    const int n = static_cast<int>(e - t0 < kTJ ? e - t0 : kTJ);
    __syncthreads();
    for (int idx = tid; idx < kTJ * Kp; idx += kBlock) {
      const int j = idx / Kp, a = idx - j * Kp;
      float y = 0.f, w = 0.f;
      if (j < n) {
        if (a < K) {
          const int64_t row = col != nullptr ? static_cast<int64_t>(col[t0 + j]) : t0 + j;
          y = Y[row * K + a];
        }
        w = mode == 1 ? val[t0 + j] - 1.f : 1.f;
      }
      sY[idx] = y;
      sYw[idx] = w * y;
    }
    if (tid < kTJ) sBeta[tid] = (mode != 0 && tid < n) ? val[t0 + tid] : 0.f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tile = tid + q * kBlock;
      if (tile < T) {
        const int ta = tile / TK, tb = tile - ta * TK;
        for (int j = 0; j < n; ++j) {
          const float4 ya = ld4(sYw + j * Kp + 4 * ta);
          const float4 yb = ld4(sY + j * Kp + 4 * tb);
          const float av[4] = {ya.x, ya.y, ya.z, ya.w};
          const float bv[4] = {yb.x, yb.y, yb.z, yb.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[q][u * 4 + v] = fmaf(av[u], bv[v], acc[q][u * 4 + v]);
        }
      }
    }
    if (mode != 0 && tid < Kp)
      for (int j = 0; j < n; ++j) bacc = fmaf(sBeta[j], sY[j * Kp + tid], bacc);
  }
}

// ---- workgroup solve of A x = b held in LDS (A: Kp x lda, the K x K block used) -------------------------------------
__device__ float block_sum(float v, float* sRed) {
  v = wave_sum(v);
  const int w = threadIdx.x / kWave;
  __syncthreads();
  if ((threadIdx.x & (kWave - 1)) == 0) sRed[w] = v;
  __syncthreads();
  return ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// CG from x = xrow (the loop of _als.pyx:205-268 on an explicit A): continue when rsold < 1e-10, break when rsnew < 1e-10.
__device__ void solve_cg(const float* sA, int lda, const float* sb, float* sx, float* sp, float* sRed, int K,
                         float* __restrict__ xrow, int cg_steps) {
  const int d = threadIdx.x;
  const bool own = d < K;
  float xd = own ? xrow[d] : 0.f;
  if (d < kMaxK) sx[d] = xd;
  __syncthreads();
  float rd = 0.f;
  if (own) {
    float ax = 0.f;
    for (int e = 0; e < K; ++e) ax = fmaf(sA[d * lda + e], sx[e], ax);
    rd = sb[d] - ax;
  }
  float pd = rd;
  float rsold = block_sum(rd * rd, sRed);
  if (rsold < 1e-10f) return;
  for (int it = 0; it < cg_steps; ++it) {
    __syncthreads();
    if (d < kMaxK) sp[d] = pd;
    __syncthreads();
    float apd = 0.f;
    if (own)
      for (int e = 0; e < K; ++e) apd = fmaf(sA[d * lda + e], sp[e], apd);
    const float pap = block_sum(pd * apd, sRed);
    const float ak = rsold / pap;
    xd = fmaf(ak, pd, xd);
    rd = fmaf(-ak, apd, rd);
    const float rsnew = block_sum(rd * rd, sRed);
    if (rsnew < 1e-10f) break;
    pd = fmaf(1.f, rd, (rsnew / rsold) * pd);
    rsold = rsnew;
  }
  if (own) xrow[d] = xd;
}

// Cholesky A = L L^T in place (lower triangle), then L y = b, L^T x = y (`posv`, _als.pyx:152-164).  A pivot that is not
// positive (or NaN) marks the row in `fail` and leaves x as it was — the reference raises there.
__device__ void solve_chol(float* sA, int lda, float* sb, float* sRed, int K, float* __restrict__ xrow, int32_t* fail_word) {
  const int tid = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    const float piv = sA[k * lda + k];
    if (!(piv > 0.f)) {
      if (tid == 0) *fail_word = k + 1;
      return;                                  // uniform: every thread read the same pivot
    }
    const float l = sqrtf(piv);
    __syncthreads();
    for (int i = k + 1 + tid; i < K; i += kBlock) sA[i * lda + k] = sA[i * lda + k] / l;
    if (tid == 0) sA[k * lda + k] = l;
    __syncthreads();
    const int m = K - k - 1;
    for (int idx = tid; idx < m * m; idx += kBlock) {
      const int i = k + 1 + idx / m, j = k + 1 + idx % m;
      if (j <= i) sA[i * lda + j] = fmaf(-sA[i * lda + k], sA[j * lda + k], sA[i * lda + j]);
    }
  }
  for (int k = 0; k < K; ++k) {              // forward: L y = b
    __syncthreads();
    const float yk = sb[k] / sA[k * lda + k];
    __syncthreads();
    for (int i = k + 1 + tid; i < K; i += kBlock) sb[i] = fmaf(-sA[i * lda + k], yk, sb[i]);
    if (tid == 0) sb[k] = yk;
  }
  for (int k = K - 1; k >= 0; --k) {         // backward: L^T x = y
    __syncthreads();
    const float xk = sb[k] / sA[k * lda + k];
    __syncthreads();
    for (int i = tid; i < k; i += kBlock) sb[i] = fmaf(-sA[k * lda + i], xk, sb[i]);
    if (tid == 0) sb[k] = xk;
  }
  __syncthreads();
  if (tid < K) xrow[tid] = sb[tid];
  (void)sRed;
}

struct SolveLds {
  float *sY, *sYw, *sBeta, *sA, *sb, *sx, *sp, *sRed;
  int lda;
};
__host__ __device__ inline size_t solve_lds_floats(int Kp) {
  return 2 * kTJ * Kp + kTJ + static_cast<size_t>(Kp) * (Kp + 1) + 3 * kMaxK + 8;
}
__device__ SolveLds carve(float* smem, int Kp) {
  SolveLds L;
  L.lda = Kp + 1;
  L.sY = smem;
  L.sYw = L.sY + kTJ * Kp;
  L.sBeta = L.sYw + kTJ * Kp;
  L.sA = L.sBeta + kTJ;
  L.sb = L.sA + Kp * L.lda;
  L.sx = L.sb + kMaxK;
  L.sp = L.sx + kMaxK;
  L.sRed = L.sp + kMaxK;
  return L;
}

// ---- kernels -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void als_gram_partial_kernel(const float* __restrict__ Y, int64_t N, int K,
                                                                   float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = pad4(K);
  SolveLds L = carve(smem, Kp);
  const int64_t P = gridDim.x;
  const int64_t s = N * blockIdx.x / P, e = N * (blockIdx.x + 1) / P;
  float acc[4][16];
  float bacc = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[q][u] = 0.f;
  gram_rows(nullptr, nullptr, s, e, Y, K, Kp, 0, L.sY, L.sYw, L.sBeta, acc, bacc);
  const int TK = Kp / 4;
  float* out = partial + static_cast<int64_t>(blockIdx.x) * K * K;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tile = threadIdx.x + q * kBlock;
    if (tile < TK * TK) {
      const int ta = tile / TK, tb = tile - ta * TK;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int a = 4 * ta + u, b = 4 * tb + v;
          if (a < K && b < K) out[a * K + b] = acc[q][u * 4 + v];
        }
    }
  }
}

// G0[c] = sum_p partial[p][c] in p order (+ reg on the diagonal); nblk == 0: G0 = reg I (explicit task).
__global__ __launch_bounds__(kBlock) void als_gram_finish_kernel(const float* __restrict__ partial, int nblk, int K,
                                                                  float reg, float* __restrict__ G0) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= K * K) return;
  float v = 0.f;
  for (int p = 0; p < nblk; ++p) v += partial[static_cast<int64_t>(p) * K * K + c];
  if (c / K == c % K) v += reg;
  G0[c] = v;
}

// Light rows (CG): one wave per row, everything from LDS.
__global__ __launch_bounds__(kBlock) void als_light_cg_kernel(const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const float* __restrict__ val, float* __restrict__ X,
                                                               const float* __restrict__ Y, int K,
                                                               const float* __restrict__ G0, int implicit, int cg_steps,
                                                               const int32_t* __restrict__ rows, int64_t n_rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = pad4(K), cap = light_cap(K), ldy = Kp + 1;
  float* sG = smem;                                               // Kp x Kp (zero padded)
  const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
  float* sYl = sG + Kp * Kp + wave * (cap * ldy + Kp + cap);      // cap x ldy
  float* sv = sYl + cap * ldy;                                     // Kp
  float* scoef = sv + Kp;                                          // cap
  for (int idx = threadIdx.x; idx < Kp * Kp; idx += kBlock) {
    const int a = idx / Kp, b = idx - a * Kp;
    sG[idx] = (a < K && b < K) ? G0[a * K + b] : 0.f;
  }
  __syncthreads();
  const bool own0 = lane < K, own1 = lane + kWave < K;
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kLightWaves;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * kLightWaves + wave; w < n_rows; w += nwaves) {
    const int64_t m = rows[w];
    const int64_t s = rowptr[m];
    const int n = static_cast<int>(rowptr[m + 1] - s);
    if (n > cap) continue;                                         // the plan never lists such a row here
    wave_sync();
    for (int idx = lane; idx < n * K; idx += kWave) {
      const int j = idx / K, a = idx - j * K;
      sYl[j * ldy + a] = Y[static_cast<int64_t>(col[s + j]) * K + a];
    }
    wave_sync();
    const float cj = lane < n ? val[s + lane] : 0.f;
    const float wj = implicit ? cj - 1.f : 1.f;
    float* xrow = X + m * K;
    float x0 = own0 ? xrow[lane] : 0.f, x1 = own1 ? xrow[lane + kWave] : 0.f;

    // out = G v (gout) and sum_j coef(y_j . v) y_j (sout)
    auto apply = [&](float v0, float v1, bool resid, float& g0, float& g1, float& s0, float& s1) {
      // v goes through LDS: a broadcast read per step (a readlane form, v_readlane into a scalar register per step, measured
      // slower: 144 vs 112 ms for cfg 5's light rows)
      if (lane < Kp) sv[lane] = v0;
      if (lane + kWave < Kp) sv[lane + kWave] = v1;
      wave_sync();
      if (lane < n) {
        float dj = 0.f;
        for (int d = 0; d < K; ++d) dj = fmaf(sYl[lane * ldy + d], sv[d], dj);
        scoef[lane] = resid ? fmaf(-wj, dj, cj) : wj * dj;
      }
      g0 = 0.f, g1 = 0.f;
      for (int e = 0; e < K; ++e) {
        const float ve = sv[e];
        if (own0) g0 = fmaf(sG[e * Kp + lane], ve, g0);
        if (own1) g1 = fmaf(sG[e * Kp + lane + kWave], ve, g1);
      }
      wave_sync();
      s0 = 0.f, s1 = 0.f;
      for (int j = 0; j < n; ++j) {
        const float c = scoef[j];
        if (own0) s0 = fmaf(c, sYl[j * ldy + lane], s0);
        if (own1) s1 = fmaf(c, sYl[j * ldy + lane + kWave], s1);
      }
      wave_sync();
    };

    float g0, g1, t0, t1;
    apply(x0, x1, true, g0, g1, t0, t1);
    float r0 = own0 ? t0 - g0 : 0.f, r1 = own1 ? t1 - g1 : 0.f;    // r = b - A x
    float p0 = r0, p1 = r1;
    float rsold = wave_sum(fmaf(r0, r0, r1 * r1));
    if (rsold < 1e-10f) continue;
    for (int it = 0; it < cg_steps; ++it) {
      apply(p0, p1, false, g0, g1, t0, t1);
      const float ap0 = own0 ? g0 + t0 : 0.f, ap1 = own1 ? g1 + t1 : 0.f;
      const float pap = wave_sum(fmaf(p0, ap0, p1 * ap1));
      const float ak = rsold / pap;
      x0 = fmaf(ak, p0, x0);
      x1 = fmaf(ak, p1, x1);
      r0 = fmaf(-ak, ap0, r0);
      r1 = fmaf(-ak, ap1, r1);
      const float rsnew = wave_sum(fmaf(r0, r0, r1 * r1));
      if (rsnew < 1e-10f) break;
      const float beta = rsnew / rsold;
      p0 = fmaf(1.f, r0, beta * p0);
      p1 = fmaf(1.f, r1, beta * p1);
      rsold = rsnew;
    }
    if (own0) xrow[lane] = x0;
    if (own1) xrow[lane + kWave] = x1;
  }
}

__device__ inline void init_acc_from_g0(float (&acc)[4][16], const float* __restrict__ G0, int K, int Kp) {
  const int TK = Kp / 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tile = threadIdx.x + q * kBlock;
    const int ta = tile / TK, tb = tile - ta * TK;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int a = 4 * ta + u, b = 4 * tb + v;
        acc[q][u * 4 + v] = (G0 != nullptr && tile < TK * TK && a < K && b < K) ? G0[a * K + b] : 0.f;
      }
  }
}

// Medium rows: one workgroup forms A_m, b_m from its row and solves in LDS.
__global__ __launch_bounds__(kBlock) void als_row_solve_kernel(const int64_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const float* __restrict__ val, float* __restrict__ X,
                                                                const float* __restrict__ Y, int K,
                                                                const float* __restrict__ G0, int implicit, int use_cg,
                                                                int cg_steps, const int32_t* __restrict__ rows,
                                                                int64_t n_rows, int32_t* __restrict__ fail) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = pad4(K), TK = Kp / 4;
  SolveLds L = carve(smem, Kp);
  for (int64_t w = blockIdx.x; w < n_rows; w += gridDim.x) {
    const int64_t m = rows[w];
    float acc[4][16];
    float bacc = 0.f;
    init_acc_from_g0(acc, G0, K, Kp);
    gram_rows(col, val, rowptr[m], rowptr[m + 1], Y, K, Kp, implicit ? 1 : 2, L.sY, L.sYw, L.sBeta, acc, bacc);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tile = threadIdx.x + q * kBlock;
      if (tile < TK * TK) {
        const int ta = tile / TK, tb = tile - ta * TK;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) L.sA[(4 * ta + u) * L.lda + 4 * tb + v] = acc[q][u * 4 + v];
      }
    }
    if (threadIdx.x < Kp) L.sb[threadIdx.x] = bacc;
    __syncthreads();
    if (use_cg) solve_cg(L.sA, L.lda, L.sb, L.sx, L.sp, L.sRed, K, X + m * K, cg_steps);
    else solve_chol(L.sA, L.lda, L.sb, L.sRed, K, X + m * K, fail + m);
  }
}

// Heavy rows, step 1: chunk c of heavy row h = chunk_row[c] covers interactions [rowptr[m] + (c - chunk_begin[h]) * kChunk, ...)
// of row m = heavy[h]; its partial A (Kp x Kp) and b (Kp) go to slab c.
__global__ __launch_bounds__(kBlock) void als_heavy_chunk_kernel(const int64_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ col,
                                                                  const float* __restrict__ val,
                                                                  const float* __restrict__ Y, int K, int implicit,
                                                                  const int32_t* __restrict__ heavy,
                                                                  const int32_t* __restrict__ chunk_begin,
                                                                  const int32_t* __restrict__ chunk_row,
                                                                  int64_t n_chunks, float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = pad4(K), TK = Kp / 4;
  SolveLds L = carve(smem, Kp);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int h = chunk_row[c];
    const int64_t m = heavy[h];
    const int64_t r0 = rowptr[m], r1 = rowptr[m + 1];
    const int64_t s = r0 + (c - chunk_begin[h]) * static_cast<int64_t>(kChunk);
    const int64_t e = s + kChunk < r1 ? s + kChunk : r1;
    float acc[4][16];
    float bacc = 0.f;
    init_acc_from_g0(acc, nullptr, K, Kp);
    gram_rows(col, val, s, e, Y, K, Kp, implicit ? 1 : 2, L.sY, L.sYw, L.sBeta, acc, bacc);
    float* slab = slabs + c * (static_cast<int64_t>(Kp) * Kp + Kp);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int tile = threadIdx.x + q * kBlock;
      if (tile < TK * TK) {
        const int ta = tile / TK, tb = tile - ta * TK;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) slab[(4 * ta + u) * Kp + 4 * tb + v] = acc[q][u * 4 + v];
      }
    }
    if (threadIdx.x < Kp) slab[Kp * Kp + threadIdx.x] = bacc;
  }
}

// Heavy rows, step 2: A = G0 + the row's slabs in chunk order, b likewise; solve.
__global__ __launch_bounds__(kBlock) void als_heavy_solve_kernel(float* __restrict__ X, int K,
                                                                  const float* __restrict__ G0, int use_cg,
                                                                  int cg_steps, const int32_t* __restrict__ heavy,
                                                                  const int32_t* __restrict__ chunk_begin,
                                                                  int64_t n_heavy, const float* __restrict__ slabs,
                                                                  int32_t* __restrict__ fail) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Kp = pad4(K);
  SolveLds L = carve(smem, Kp);
  const int64_t slab_floats = static_cast<int64_t>(Kp) * Kp + Kp;
  for (int64_t h = blockIdx.x; h < n_heavy; h += gridDim.x) {
    const int64_t m = heavy[h];
    const int c0 = chunk_begin[h], c1 = chunk_begin[h + 1];
    __syncthreads();
    for (int idx = threadIdx.x; idx < Kp * Kp + Kp; idx += kBlock) {
      const int a = idx / Kp, b = idx - a * Kp;      // a == Kp: the b vector
      float v = (a < K && b < K) ? G0[a * K + b] : 0.f;
      for (int c = c0; c < c1; ++c) v += slabs[c * slab_floats + idx];
      if (a < Kp) L.sA[a * L.lda + b] = v;
      else L.sb[b] = v;
    }
    __syncthreads();
    if (use_cg) solve_cg(L.sA, L.lda, L.sb, L.sx, L.sp, L.sRed, K, X + m * K, cg_steps);
    else solve_chol(L.sA, L.lda, L.sb, L.sRed, K, X + m * K, fail + m);
  }
}

size_t light_lds_bytes(int K) {
  const int Kp = pad4(K), cap = light_cap(K);
  return sizeof(float) * (static_cast<size_t>(Kp) * Kp + kLightWaves * (static_cast<size_t>(cap) * (Kp + 1) + Kp + cap));
}

int gram_blocks(int64_t N) {
  int64_t p = ceil_div(N, kGramRows);
  return static_cast<int>(p < 1 ? 1 : (p > 512 ? 512 : p));
}

}  // namespace
}  // namespace lr

using namespace lr;

extern "C" int lr_als_supported(int K) { return (K >= 1 && K <= kMaxK) ? 1 : 0; }

extern "C" int lr_als_plan_params(int K, int32_t* out3) {
  if (!lr_als_supported(K) || out3 == nullptr) return LR_EINVAL;
  out3[0] = light_cap(K);
  out3[1] = kHeavyDeg;
  out3[2] = kChunk;
  return LR_OK;
}

extern "C" size_t lr_als_ws_bytes(int64_t n_chunks, int K) {
  if (!lr_als_supported(K) || n_chunks < 0) return 0;
  const int64_t Kp = pad4(K);
  const int64_t b = n_chunks * (Kp * Kp + Kp) * static_cast<int64_t>(sizeof(float));
  return static_cast<size_t>(b > 256 ? b : 256);
}

extern "C" size_t lr_als_gram_ws_bytes(int64_t N, int K) {
  if (!lr_als_supported(K) || N < 0) return 0;
  return static_cast<size_t>(gram_blocks(N)) * K * K * sizeof(float);
}

extern "C" int lr_als_gram_f32(const float* Y, int64_t N, int K, float reg, int implicit, float* G0, void* ws,
                               size_t ws_bytes, lr_stream_t stream) {
  if (!lr_als_supported(K) || N < 0 || G0 == nullptr || (implicit && N > 0 && Y == nullptr)) return LR_EINVAL;
  hipStream_t s = as_stream(stream);
  const int fin_grid = static_cast<int>(ceil_div(static_cast<int64_t>(K) * K, kBlock));
  if (!implicit || N == 0) {
    hipLaunchKernelGGL(als_gram_finish_kernel, dim3(fin_grid), dim3(kBlock), 0, s, nullptr, 0, K, reg, G0);
    return launch_status();
  }
  const int P = gram_blocks(N);
  if (ws == nullptr || ws_bytes < lr_als_gram_ws_bytes(N, K)) return LR_EWORKSPACE;
  const size_t lds = solve_lds_floats(pad4(K)) * sizeof(float);
  int rc = set_lds(als_gram_partial_kernel, lds);
  if (rc != LR_OK) return rc;
  float* partial = static_cast<float*>(ws);
  hipLaunchKernelGGL(als_gram_partial_kernel, dim3(P), dim3(kBlock), lds, s, Y, N, K, partial);
  hipLaunchKernelGGL(als_gram_finish_kernel, dim3(fin_grid), dim3(kBlock), 0, s, partial, P, K, reg, G0);
  return launch_status();
}

extern "C" int lr_als_half_sweep_f32(const int64_t* rowptr, const int32_t* col, const float* val, int64_t rows,
                                     float* X, const float* Y, int K, const float* G0, int implicit, int use_cg,
                                     int cg_steps, const int32_t* plan, int64_t n_light, int64_t n_medium,
                                     int64_t n_heavy, int64_t n_chunks, int32_t* fail, void* ws, size_t ws_bytes,
                                     int stage_mask, lr_stream_t stream) {
  if (!lr_als_supported(K) || rows < 0 || n_light < 0 || n_medium < 0 || n_heavy < 0 || n_chunks < 0 ||
      n_light + n_medium + n_heavy != rows || cg_steps < 0 || (n_heavy > 0) != (n_chunks > 0))
    return LR_EINVAL;
  if (rows == 0) return LR_OK;
  if (rowptr == nullptr || X == nullptr || G0 == nullptr || plan == nullptr || (!use_cg && fail == nullptr))
    return LR_EINVAL;
  if (n_chunks > 0 && (ws == nullptr || ws_bytes < lr_als_ws_bytes(n_chunks, K))) return LR_EWORKSPACE;
  hipStream_t s = as_stream(stream);
  const int32_t* light = plan;
  const int32_t* medium = light + n_light;
  const int32_t* heavy = medium + n_medium;
  const int32_t* chunk_begin = heavy + n_heavy;
  const int32_t* chunk_row = chunk_begin + n_heavy + 1;
  const size_t wg_lds = solve_lds_floats(pad4(K)) * sizeof(float);
  int rc;
  if ((rc = set_lds(als_row_solve_kernel, wg_lds)) != LR_OK) return rc;
  if ((stage_mask & 1) && n_light > 0) {
    if (use_cg) {
      const size_t lds = light_lds_bytes(K);
      if ((rc = set_lds(als_light_cg_kernel, lds)) != LR_OK) return rc;
      hipLaunchKernelGGL(als_light_cg_kernel, dim3(grid_for(n_light, kLightWaves, 4096)), dim3(kBlock), lds, s, rowptr,
                         col, val, X, Y, K, G0, implicit, cg_steps, light, n_light);
    } else {
      hipLaunchKernelGGL(als_row_solve_kernel, dim3(grid_for(n_light, 1, 8192)), dim3(kBlock), wg_lds, s, rowptr, col,
                         val, X, Y, K, G0, implicit, 0, cg_steps, light, n_light, fail);
    }
  }
  if ((stage_mask & 2) && n_medium > 0)
    hipLaunchKernelGGL(als_row_solve_kernel, dim3(grid_for(n_medium, 1, 8192)), dim3(kBlock), wg_lds, s, rowptr, col,
                       val, X, Y, K, G0, implicit, use_cg, cg_steps, medium, n_medium, fail);
  if ((stage_mask & 4) && n_chunks > 0) {
    if ((rc = set_lds(als_heavy_chunk_kernel, wg_lds)) != LR_OK) return rc;
    hipLaunchKernelGGL(als_heavy_chunk_kernel, dim3(grid_for(n_chunks, 1, 8192)), dim3(kBlock), wg_lds, s, rowptr, col,
                       val, Y, K, implicit, heavy, chunk_begin, chunk_row, n_chunks, static_cast<float*>(ws));
  }
  if ((stage_mask & 8) && n_heavy > 0) {
    if ((rc = set_lds(als_heavy_solve_kernel, wg_lds)) != LR_OK) return rc;
    hipLaunchKernelGGL(als_heavy_solve_kernel, dim3(grid_for(n_heavy, 1, 8192)), dim3(kBlock), wg_lds, s, X, K, G0,
                       use_cg, cg_steps, heavy, chunk_begin, n_heavy, static_cast<const float*>(ws), fail);
  }
  return launch_status();
}
