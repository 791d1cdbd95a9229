// FTRL-proximal on scalar rows (the wide side of Wide & Deep): TF1's ApplyFtrl / SparseApplyFtrl with lr_power = -0.5 and
// no l2 shrinkage (tensorflow/core/kernels/training_ops.cc, FtrlCompute), per element with gradient g:
//   new_accum = accum + g*g
//   linear   += g - (sqrt(new_accum) - sqrt(accum)) / lr * var
//   var       = |linear| > l1 ? (sign(linear)*l1 - linear) / (sqrt(new_accum)/lr + 2*l2) : 0
// sqrt(new_accum) - sqrt(accum) is formed as g*g / (sqrt(new_accum) + sqrt(accum)): the same quantity without the
// cancellation of two nearly equal f32 roots (a gradient of 1e-3 at accum 0.1 loses two digits in the subtracted form).
//
// Row form (lr_ftrl_rows_f32): TF de-duplicates IndexedSlices before the sparse apply, so a row's gradient is the sum over
// its run of the segments and var / accum / linear of the row are read and written exactly once.  The rows are scalars, so
// the work decomposition of embed_scatter.hip (K/4 lanes per row) has nothing to spread over lanes: here
//   * a run of at most kFtrlLongRun positions is walked by ONE lane, four gathers in flight, added in ascending order;
//   * a longer run is cut into chunks of kFtrlChunk positions, ONE WAVE per chunk: lane l adds positions l, l + 64, ... of
//     the chunk in ascending order, the 64 lane sums are folded by the xor butterfly (a fixed tree), and one wave per run
//     then folds the run's chunk partials the same way (lane l takes chunks l, l + 64, ...) and applies the update.
// Every order is fixed by (run, chunk, lane) alone, never by the grid: no float atomics, run-to-run identical bits.
// Workspace (lr_ftrl_rows_ws_bytes), the layout of LongWs in embed_scatter.hip with one float per chunk:
//   int32 long_count | int32 chunk_count | pad to 256 B | long_seg[NL] | long_base[NL] | chunk_slot[NC] | partial[NC]
// Its contents are arbitrary on entry; the two counters are zeroed by a kernel on the launch stream.
#include "common.hpp"

namespace lr {

constexpr int kFtrlLongRun = 32;     // runs longer than this are summed by waves (tests read both constants from here)
constexpr int kFtrlChunk = 256;      // positions per wave: four independent gathers per lane

struct FtrlCoef {
  float lr, l1, two_l2;
};

// one FTRL-proximal update of a single element; returns the new weight
__device__ __forceinline__ float ftrl_elem(float w, float g, float& accum, float& linear, const FtrlCoef& c) {
  const float gg = g * g;
  const float na = accum + gg;
  const float sa = sqrtf(accum), sna = sqrtf(na);
  const float den = sna + sa;
  const float dsq = den > 0.f ? gg / den : 0.f;      // sqrt(new_accum) - sqrt(accum)
  const float z = linear + (g - dsq / c.lr * w);
  const float quad = sna / c.lr + c.two_l2;
  accum = na;
  linear = z;
  return fabsf(z) > c.l1 ? (copysignf(c.l1, z) - z) / quad : 0.f;
}

struct FtrlWs {
  int32_t* counts;      // [0] = long runs, [1] = chunks
  int32_t* long_seg; int32_t* long_base; int32_t* chunk_slot; float* partial;
  int n_long_max, n_chunk_max;
};

static inline size_t ftrl_align(size_t x) { return (x + 255) / 256 * 256; }
static inline int ftrl_long_max(int64_t n) { return static_cast<int>(n / (kFtrlLongRun + 1) + 1); }
// a long run of len positions has ceil(len / chunk) <= len / chunk + 1 chunks
static inline int ftrl_chunk_max(int64_t n) { return static_cast<int>(n / kFtrlChunk + ftrl_long_max(n) + 1); }
static inline size_t ftrl_ws_bytes(int64_t n) {
  return 256 + 2 * ftrl_align(static_cast<size_t>(ftrl_long_max(n)) * 4) +
         2 * ftrl_align(static_cast<size_t>(ftrl_chunk_max(n)) * 4);
}
static FtrlWs make_ftrl_ws(void* ws, int64_t n) {
  FtrlWs w;
  char* p = static_cast<char*>(ws);
  w.n_long_max = ftrl_long_max(n);
  w.n_chunk_max = ftrl_chunk_max(n);
  w.counts = reinterpret_cast<int32_t*>(p); p += 256;
  w.long_seg = reinterpret_cast<int32_t*>(p); p += ftrl_align(static_cast<size_t>(w.n_long_max) * 4);
  w.long_base = reinterpret_cast<int32_t*>(p); p += ftrl_align(static_cast<size_t>(w.n_long_max) * 4);
  w.chunk_slot = reinterpret_cast<int32_t*>(p); p += ftrl_align(static_cast<size_t>(w.n_chunk_max) * 4);
  w.partial = reinterpret_cast<float*>(p);
  return w;
}

// One lane per run.  Short runs are summed and applied here; with a workspace (`use_long`) a long run is only listed:
// the slot order of the list depends on the atomics, the sums do not (a run's chunks are consecutive from its base).
__global__ __launch_bounds__(kBlock) void ftrl_rows_short_kernel(
    float* __restrict__ var, float* __restrict__ accum, float* __restrict__ linear, const float* __restrict__ grad,
    const int32_t* __restrict__ seg_pos, const int32_t* __restrict__ seg_rows, const int32_t* __restrict__ seg_start,
    const int32_t* __restrict__ n_seg_ptr, FtrlCoef c, int use_long, FtrlWs w) {
  const int n_seg = *n_seg_ptr;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; s < n_seg; s += stride) {
    const int p0 = seg_start[s], p1 = seg_start[s + 1];
    const int len = p1 - p0;
    if (use_long && len > kFtrlLongRun) {
      const int nch = (len + kFtrlChunk - 1) / kFtrlChunk;
      const int slot = atomicAdd(&w.counts[0], 1);
      const int base = atomicAdd(&w.counts[1], nch);
      if (slot < w.n_long_max && base + nch <= w.n_chunk_max) {      // holds by the sizing; never write past the lists
        w.long_seg[slot] = static_cast<int32_t>(s);
        w.long_base[slot] = base;
        for (int j = 0; j < nch; ++j) w.chunk_slot[base + j] = slot;
      }
      continue;
    }
    float g = 0.f;
    int p = p0;
    for (; p + 4 <= p1; p += 4) {       // four gathers in flight, added in ascending order
      const int32_t q0 = seg_pos[p], q1 = seg_pos[p + 1], q2 = seg_pos[p + 2], q3 = seg_pos[p + 3];
      const float a = grad[q0], b = grad[q1], c2 = grad[q2], d = grad[q3];
      g = (((g + a) + b) + c2) + d;
    }
    for (; p < p1; ++p) g += grad[seg_pos[p]];
    const int32_t row = seg_rows[s];
    float a = accum[row], z = linear[row];
    var[row] = ftrl_elem(var[row], g, a, z, c);
    accum[row] = a;
    linear[row] = z;
  }
}

// One wave per chunk of a long run.
__global__ __launch_bounds__(kBlock) void ftrl_rows_chunk_kernel(const float* __restrict__ grad,
                                                                 const int32_t* __restrict__ seg_pos,
                                                                 const int32_t* __restrict__ seg_start, FtrlWs w) {
  constexpr int kWaves = kBlock / kWave;
  const int lane = threadIdx.x % kWave;
  int n_chunks = w.counts[1];
  if (n_chunks > w.n_chunk_max) n_chunks = w.n_chunk_max;
  const int wstride = gridDim.x * kWaves;
  for (int c = blockIdx.x * kWaves + threadIdx.x / kWave; c < n_chunks; c += wstride) {      // uniform per wave
    const int slot = w.chunk_slot[c];
    const int s = w.long_seg[slot];
    const int j = c - w.long_base[slot];
    const int p0 = seg_start[s] + j * kFtrlChunk;
    const int pe = seg_start[s + 1];
    const int p1 = (p0 + kFtrlChunk) < pe ? (p0 + kFtrlChunk) : pe;
    float x[kFtrlChunk / kWave];
#pragma unroll
    for (int u = 0; u < kFtrlChunk / kWave; ++u) {
      const int p = p0 + lane + u * kWave;
      x[u] = p < p1 ? grad[seg_pos[p]] : 0.f;
    }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < kFtrlChunk / kWave; ++u) acc += x[u];
    acc = wave_sum(acc);
    if (lane == 0) w.partial[c] = acc;
  }
}

// One wave per long run: the chunk partials folded in a fixed order, then the update.
__global__ __launch_bounds__(kBlock) void ftrl_rows_finish_kernel(float* __restrict__ var, float* __restrict__ accum,
                                                                  float* __restrict__ linear,
                                                                  const int32_t* __restrict__ seg_rows,
                                                                  const int32_t* __restrict__ seg_start, FtrlCoef c,
                                                                  FtrlWs w) {
  constexpr int kWaves = kBlock / kWave;
  const int lane = threadIdx.x % kWave;
  int n_long = w.counts[0];
  if (n_long > w.n_long_max) n_long = w.n_long_max;
  const int wstride = gridDim.x * kWaves;
  for (int q = blockIdx.x * kWaves + threadIdx.x / kWave; q < n_long; q += wstride) {
    const int s = w.long_seg[q];
    const int base = w.long_base[q];
    const int nch = (seg_start[s + 1] - seg_start[s] + kFtrlChunk - 1) / kFtrlChunk;
    float g = 0.f;
    for (int j = lane; j < nch; j += kWave) g += w.partial[base + j];
    g = wave_sum(g);
    if (lane == 0) {
      const int32_t row = seg_rows[s];
      float a = accum[row], z = linear[row];
      var[row] = ftrl_elem(var[row], g, a, z, c);
      accum[row] = a;
      linear[row] = z;
    }
  }
}

// The same update on every element of a flat range, g = grad[i] + l2_grad_coef * var[i].
template <bool VEC>
__global__ __launch_bounds__(kBlock) void ftrl_dense_kernel(float* __restrict__ var, float* __restrict__ accum,
                                                            float* __restrict__ linear, int64_t n,
                                                            const float* __restrict__ grad, float l2_grad_coef,
                                                            FtrlCoef c) {
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kBlock;
  int64_t tail0 = 0;
  if constexpr (VEC) {
    const int64_t nq = n / 4;
    tail0 = nq * 4;
    for (int64_t q = tid; q < nq; q += stride) {
      const float4 w = ld4(var + q * 4), g0 = ld4(grad + q * 4);
      float4 a = ld4(accum + q * 4), z = ld4(linear + q * 4), r;
      r.x = ftrl_elem(w.x, fmaf(l2_grad_coef, w.x, g0.x), a.x, z.x, c);
      r.y = ftrl_elem(w.y, fmaf(l2_grad_coef, w.y, g0.y), a.y, z.y, c);
      r.z = ftrl_elem(w.z, fmaf(l2_grad_coef, w.z, g0.z), a.z, z.z, c);
      r.w = ftrl_elem(w.w, fmaf(l2_grad_coef, w.w, g0.w), a.w, z.w, c);
      st4(var + q * 4, r);
      st4(accum + q * 4, a);
      st4(linear + q * 4, z);
    }
  }
  for (int64_t i = tail0 + tid; i < n; i += stride) {
    const float w = var[i];
    float a = accum[i], z = linear[i];
    var[i] = ftrl_elem(w, fmaf(l2_grad_coef, w, grad[i]), a, z, c);
    accum[i] = a;
    linear[i] = z;
  }
}

static inline bool ftrl_hp_ok(double lr, double l1, double l2) { return lr > 0.0 && l1 >= 0.0 && l2 >= 0.0; }
static inline FtrlCoef make_ftrl_coef(double lr, double l1, double l2) {
  return FtrlCoef{static_cast<float>(lr), static_cast<float>(l1), static_cast<float>(2.0 * l2)};
}

}  // namespace lr

using namespace lr;

extern "C" size_t lr_ftrl_rows_ws_bytes(int64_t n_max) {
  if (n_max < 0 || n_max >= (int64_t(1) << 31) - 1) return 0;
  return ftrl_ws_bytes(n_max);
}

extern "C" int lr_ftrl_rows_f32(float* var, float* accum, float* linear, int64_t V, const float* grad,
                                const int32_t* seg_pos, const int32_t* seg_rows, const int32_t* seg_start,
                                const int32_t* n_seg, int64_t n, double lr, double l1, double l2, void* ws,
                                size_t ws_bytes, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && V >= 0 && ftrl_hp_ok(lr, l1, l2));
  if (n >= (int64_t(1) << 31) - 1) return LR_ESHAPE;
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(var && accum && linear && grad && seg_pos && seg_rows && seg_start && n_seg);
  if (ws != nullptr && ws_bytes < ftrl_ws_bytes(n)) return LR_EWORKSPACE;
  const bool use_long = ws != nullptr && n > kFtrlLongRun;
  const FtrlCoef c = make_ftrl_coef(lr, l1, l2);
  hipStream_t s = as_stream(stream);
  FtrlWs w{};
  if (use_long) {
    w = make_ftrl_ws(ws, n);
    zero_words_async(w.counts, 2, s);
  }
  hipLaunchKernelGGL(ftrl_rows_short_kernel, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, var, accum, linear, grad, seg_pos,
                     seg_rows, seg_start, n_seg, c, use_long ? 1 : 0, w);
  if (use_long) {
    constexpr int kWaves = kBlock / kWave;
    hipLaunchKernelGGL(ftrl_rows_chunk_kernel, dim3(grid_for(w.n_chunk_max, kWaves)), dim3(kBlock), 0, s, grad, seg_pos,
                       seg_start, w);
    hipLaunchKernelGGL(ftrl_rows_finish_kernel, dim3(grid_for(w.n_long_max, kWaves)), dim3(kBlock), 0, s, var, accum, linear,
                       seg_rows, seg_start, c, w);
  }
  return launch_status();
}

extern "C" int lr_ftrl_dense_f32(float* var, float* accum, float* linear, int64_t n, const float* grad,
                                 double l2_grad_coef, double lr, double l1, double l2, lr_stream_t stream) {
  LR_CHECK_ARG(n >= 0 && ftrl_hp_ok(lr, l1, l2));
  const float gc = static_cast<float>(l2_grad_coef);
  if (n == 0) return LR_OK;
  LR_CHECK_ARG(var && accum && linear && grad);
  const FtrlCoef c = make_ftrl_coef(lr, l1, l2);
  hipStream_t s = as_stream(stream);
  const bool vec = (reinterpret_cast<uintptr_t>(var) | reinterpret_cast<uintptr_t>(accum) |
                    reinterpret_cast<uintptr_t>(linear) | reinterpret_cast<uintptr_t>(grad)) % 16 == 0 && n >= 4;
  if (vec)
    hipLaunchKernelGGL(ftrl_dense_kernel<true>, dim3(grid_for(n / 4 + 3, kBlock)), dim3(kBlock), 0, s, var, accum, linear, n,
                       grad, gc, c);
  else
    hipLaunchKernelGGL(ftrl_dense_kernel<false>, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, var, accum, linear, n, grad,
                       gc, c);
  return launch_status();
}
