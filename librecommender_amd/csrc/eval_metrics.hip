// Evaluation metrics on the device (include/libreco_hip.h, "Evaluation metrics"): sort keys, rank statistics over the sorted
// order (ROC AUC as exact integers, GAUC, PR AUC), pointwise sums, listwise metrics per user and catalogue coverage.
//
// Rank statistics are a segmented scan over tie runs (equal key) and groups (equal high word) in the three-launch form: a
// tile reduce, a scan of the tile summaries by one workgroup, a finish.  No workgroup waits for another inside a launch, so
// nothing depends on dispatch order or residency, and every sum has one fixed order: two calls give the same bits.  The scan
// runs twice, because the second level (the per-group sum of the runs' terms) needs the first level's result at every run
// end: reduce 1, scan 1, reduce 2, scan 2, finish, final sums — six launches, all memory-bound or launch-bound.
//
// No floating-point atomics.  The only atomics are integer adds (NaN count, flag count) onto words a kernel of the same call
// zeroes first.  Every output element is written on every call.
#include "common.hpp"

namespace {

using lr::as_stream;
using lr::launch_status;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;                        // consecutive rows per thread of the scan
constexpr int kScanTile = kThreads * kItems;     // 2,048 rows per workgroup == ops.EVAL_SCAN_TILE
constexpr int kPointItems = 16;
constexpr int kPointTile = kThreads * kPointItems;   // 4,096 rows per workgroup == ops.EVAL_POINT_TILE
constexpr int kMaxK = 1024;

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// ---- scan states ---------------------------------------------------------------------------------------------------------
// Level 1: counts since the last run start (R) and the last group start (G), and since row 0 (A).  `fl` bit 0: a run starts
// inside the summarised range, bit 1: a group starts inside it.  Counts stay below 2^31 (n < 2^31).
struct S1 {
  int fl, posR, cntR, posG, cntG, posA;
};
// Level 2: the sum of the runs' terms since the last group start.
struct S2 {
  int fl, pad;
  long long term;
};

__device__ __forceinline__ S1 identity(const S1*) { return S1{0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ S2 identity(const S2*) { return S2{0, 0, 0ll}; }

__device__ __forceinline__ S1 combine(const S1& a, const S1& b) {
  S1 r;
  r.fl = a.fl | b.fl;
  r.posR = (b.fl & 1) ? b.posR : a.posR + b.posR;
  r.cntR = (b.fl & 1) ? b.cntR : a.cntR + b.cntR;
  r.posG = (b.fl & 2) ? b.posG : a.posG + b.posG;
  r.cntG = (b.fl & 2) ? b.cntG : a.cntG + b.cntG;
  r.posA = a.posA + b.posA;
  return r;
}
__device__ __forceinline__ S2 combine(const S2& a, const S2& b) {
  S2 r;
  r.fl = a.fl | b.fl;
  r.pad = 0;
  r.term = b.fl ? b.term : a.term + b.term;
  return r;
}
__device__ __forceinline__ S1 shfl_up(const S1& s, int d) {
  return S1{__shfl_up(s.fl, d), __shfl_up(s.posR, d), __shfl_up(s.cntR, d), __shfl_up(s.posG, d), __shfl_up(s.cntG, d),
            __shfl_up(s.posA, d)};
}
__device__ __forceinline__ S2 shfl_up(const S2& s, int d) { return S2{__shfl_up(s.fl, d), 0, __shfl_up(s.term, d)}; }

// Exclusive scan of one summary per thread over the workgroup; *total = the combination of all of them.
template <class S>
__device__ __forceinline__ S block_scan_exclusive(const S& agg, S* lds /* [kWaves] */, S* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  S inc = agg;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const S o = shfl_up(inc, d);
    if (lane >= d) inc = combine(o, inc);
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  S before = identity(static_cast<const S*>(nullptr)), tot = before;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const S x = lds[w];
    if (w < wave) before = combine(before, x);
    tot = combine(tot, x);
  }
  __syncthreads();
  const S prev = shfl_up(inc, 1);
  *total = tot;
  return lane == 0 ? before : combine(before, prev);
}

template <class T>
__device__ __forceinline__ T block_sum(T v, T* lds /* [kWaves] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r += lds[w];
  __syncthreads();
  return r;
}

// ---- the rows of one thread ------------------------------------------------------------------------------------------------
struct Rows {
  long long key[kItems + 2];   // key[0]: the row before the first, key[kItems + 1]: the row after the last
  int lab[kItems];
  int64_t first;
  int cnt;
};

__device__ __forceinline__ int hi_word(long long k) { return static_cast<int>(k >> 32); }

__device__ __forceinline__ void load_rows(const long long* __restrict__ key, const uint8_t* __restrict__ label, int64_t n,
                                          Rows& r) {
  r.first = static_cast<int64_t>(blockIdx.x) * kScanTile + static_cast<int64_t>(threadIdx.x) * kItems;
  const int64_t left = n - r.first;
  r.cnt = left <= 0 ? 0 : (left < kItems ? static_cast<int>(left) : kItems);
  r.key[0] = (r.cnt > 0 && r.first > 0) ? key[r.first - 1] : 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const bool ok = j < r.cnt;
    r.key[j + 1] = ok ? key[r.first + j] : 0;
    r.lab[j] = ok ? (label[r.first + j] != 0) : 0;
  }
  r.key[kItems + 1] = (r.cnt == kItems && r.first + kItems < n) ? key[r.first + kItems] : 0;
}

// Row j of the thread: the flags of its place in the order.
struct Place {
  bool run_start, group_start, run_end, group_end;
};
__device__ __forceinline__ Place place_of(const Rows& r, int j, int64_t n) {
  const int64_t i = r.first + j;
  const long long k = r.key[j + 1];
  Place p;
  p.run_start = i == 0 || k != r.key[j];
  p.group_start = i == 0 || hi_word(k) != hi_word(r.key[j]);
  const bool last = i == n - 1;
  // the next row's key: key[j + 2] is loaded for j + 1 < cnt, and for j == kItems - 1 when a next row exists; a thread with
  // fewer than kItems rows holds the last row of all, where `last` decides
  const long long nk = r.key[j + 2];
  p.run_end = last || nk != k;
  p.group_end = last || hi_word(nk) != hi_word(k);
  return p;
}
__device__ __forceinline__ S1 element1(const Place& p, int lab) {
  return S1{(p.run_start ? 1 : 0) | (p.group_start ? 2 : 0), lab, 1, lab, 1, lab};
}
// The term of the run that ends at a row whose inclusive state is `st`:
// pos_run * (2 * neg_below + neg_run), neg_below = the group's negatives before the run.
__device__ __forceinline__ long long run_term(const S1& st) {
  const long long neg_run = st.cntR - st.posR, neg_grp = st.cntG - st.posG;
  return static_cast<long long>(st.posR) * (2 * neg_grp - neg_run);
}

// The thread's level-1 summary.
__device__ __forceinline__ S1 fold1(const Rows& r, int64_t n) {
  S1 agg = identity(static_cast<const S1*>(nullptr));
#pragma unroll
  for (int j = 0; j < kItems; ++j)
    if (j < r.cnt) agg = combine(agg, element1(place_of(r, j, n), r.lab[j]));
  return agg;
}

__global__ void __launch_bounds__(kThreads) rank_reduce1_kernel(const long long* __restrict__ key,
                                                                const uint8_t* __restrict__ label, int64_t n,
                                                                S1* __restrict__ tiles) {
  __shared__ S1 lds[kWaves];
  Rows r;
  load_rows(key, label, n, r);
  S1 total;
  block_scan_exclusive(fold1(r, n), lds, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// One workgroup: tiles[t] <- the combination of tiles[0 .. t), *total <- the combination of all.
template <class S>
__global__ void __launch_bounds__(kThreads) rank_scan_tiles_kernel(S* __restrict__ tiles, int n_tiles, S* __restrict__ total) {
  __shared__ S lds[kWaves];
  S carry = identity(static_cast<const S*>(nullptr));
  for (int base = 0; base < n_tiles; base += kThreads) {
    const int t = base + static_cast<int>(threadIdx.x);
    const S x = t < n_tiles ? tiles[t] : identity(static_cast<const S*>(nullptr));
    S tot;
    const S excl = block_scan_exclusive(x, lds, &tot);
    if (t < n_tiles) tiles[t] = combine(carry, excl);
    carry = combine(carry, tot);
  }
  if (threadIdx.x == 0) *total = carry;
}

// Level 1 again with the tile's incoming state; the terms of the thread's rows and its level-2 summary.
__device__ __forceinline__ S2 fold2(const Rows& r, int64_t n, const S1& excl1, long long* term /* [kItems] */) {
  S1 st = excl1;
  S2 agg = identity(static_cast<const S2*>(nullptr));
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    term[j] = 0;
    if (j < r.cnt) {
      const Place p = place_of(r, j, n);
      st = combine(st, element1(p, r.lab[j]));
      if (p.run_end) term[j] = run_term(st);
      agg = combine(agg, S2{p.group_start ? 1 : 0, 0, term[j]});
    }
  }
  return agg;
}

__global__ void __launch_bounds__(kThreads) rank_reduce2_kernel(const long long* __restrict__ key,
                                                                const uint8_t* __restrict__ label, int64_t n,
                                                                const S1* __restrict__ tiles1, S2* __restrict__ tiles2) {
  __shared__ S1 lds1[kWaves];
  __shared__ S2 lds2[kWaves];
  Rows r;
  load_rows(key, label, n, r);
  S1 tot1;
  const S1 excl1 = combine(tiles1[blockIdx.x], block_scan_exclusive(fold1(r, n), lds1, &tot1));
  long long term[kItems];
  S2 tot2;
  block_scan_exclusive(fold2(r, n, excl1, term), lds2, &tot2);
  if (threadIdx.x == 0) tiles2[blockIdx.x] = tot2;
}

__global__ void __launch_bounds__(kThreads) rank_finish_kernel(const long long* __restrict__ key,
                                                               const uint8_t* __restrict__ label, int64_t n,
                                                               const S1* __restrict__ tiles1, const S1* __restrict__ total1,
                                                               const S2* __restrict__ tiles2, double* __restrict__ part_gauc,
                                                               double* __restrict__ part_pr, long long* __restrict__ part_num2) {
  __shared__ S1 lds1[kWaves];
  __shared__ S2 lds2[kWaves];
  __shared__ double ldsd[kWaves];
  __shared__ long long ldsl[kWaves];
  Rows r;
  load_rows(key, label, n, r);
  S1 tot1;
  const S1 excl1 = combine(tiles1[blockIdx.x], block_scan_exclusive(fold1(r, n), lds1, &tot1));
  long long term[kItems];
  S2 tot2;
  const S2 excl2 = combine(tiles2[blockIdx.x], block_scan_exclusive(fold2(r, n, excl1, term), lds2, &tot2));
  const double P = static_cast<double>(total1->posA), N = static_cast<double>(n);
  S1 st = excl1;
  S2 st2 = excl2;
  double gauc = 0.0, pr = 0.0;
  long long num2 = 0;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    if (j < r.cnt) {
      const Place p = place_of(r, j, n);
      const int64_t i = r.first + j;
      st = combine(st, element1(p, r.lab[j]));
      st2 = combine(st2, S2{p.group_start ? 1 : 0, 0, term[j]});
      num2 += term[j];
      if (p.run_end) {
        // the trapezoid between this run's threshold and the next higher one (or the curve's last point, recall 0 and
        // precision 1): sklearn's precision_recall_curve + auc, whose x runs downwards
        const double tp = P - static_cast<double>(st.posA - st.posR), ps = N - static_cast<double>(i + 1 - st.cntR);
        const double rec = P > 0.0 ? tp / P : 1.0, prec = tp / ps;
        double rec_n = 0.0, prec_n = 1.0;
        if (i != n - 1) {
          const double tp_n = P - static_cast<double>(st.posA), ps_n = N - static_cast<double>(i + 1);
          rec_n = P > 0.0 ? tp_n / P : 1.0;
          prec_n = tp_n / ps_n;
        }
        pr += (rec_n - rec) * (prec_n + prec) / 2.0;
      }
      if (p.group_end) {
        const long long Pg = st.posG, Ng = st.cntG - st.posG;
        if (Pg > 0 && Ng > 0)
          gauc += static_cast<double>(st2.term) / static_cast<double>(2 * Pg * Ng) * static_cast<double>(st.cntG);
      }
    }
  }
  gauc = block_sum(gauc, ldsd);
  pr = block_sum(pr, ldsd);
  num2 = block_sum(num2, ldsl);
  if (threadIdx.x == 0) {
    part_gauc[blockIdx.x] = gauc;
    part_pr[blockIdx.x] = pr;
    part_num2[blockIdx.x] = num2;
  }
}

__global__ void __launch_bounds__(kThreads) rank_final_kernel(const double* __restrict__ part_gauc,
                                                              const double* __restrict__ part_pr,
                                                              const long long* __restrict__ part_num2, int n_tiles,
                                                              const S1* __restrict__ total1, int64_t n,
                                                              long long* __restrict__ out_i64, double* __restrict__ out_f64) {
  __shared__ double ldsd[kWaves];
  __shared__ long long ldsl[kWaves];
  double gauc = 0.0, pr = 0.0;
  long long num2 = 0;
  for (int t = threadIdx.x; t < n_tiles; t += kThreads) {
    gauc += part_gauc[t];
    pr += part_pr[t];
    num2 += part_num2[t];
  }
  gauc = block_sum(gauc, ldsd);
  pr = block_sum(pr, ldsd);
  num2 = block_sum(num2, ldsl);
  if (threadIdx.x == 0) {
    const long long P = total1->posA;
    out_i64[0] = num2;
    out_i64[1] = P;
    out_i64[2] = static_cast<long long>(n) - P;
    out_f64[0] = gauc / static_cast<double>(n);
    out_f64[1] = -pr;
  }
}

struct RankWs {
  size_t tiles1, total1, tiles2, total2, gauc, pr, num2, bytes;
};
inline RankWs rank_ws(int64_t n) {
  const size_t t = static_cast<size_t>(lr::ceil_div(n < 1 ? 1 : n, kScanTile));
  RankWs w;
  size_t o = 0;
  w.tiles1 = o, o += align256(t * sizeof(S1));
  w.total1 = o, o += 256;
  w.tiles2 = o, o += align256(t * sizeof(S2));
  w.total2 = o, o += 256;
  w.gauc = o, o += align256(t * 8);
  w.pr = o, o += align256(t * 8);
  w.num2 = o, o += align256(t * 8);
  w.bytes = o;
  return w;
}

// ---- sort keys ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) keys_kernel(const float* __restrict__ score, const int32_t* __restrict__ group,
                                                        int64_t n, long long* __restrict__ key, int* __restrict__ bad) {
  __shared__ int lds[kWaves];
  int nan = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const float s = score[i];
    uint32_t u = __float_as_uint(s);
    nan += (s != s) ? 1 : 0;
    if (u == 0x80000000u) u = 0u;                                   // -0.0 ties with +0.0
    u ^= (u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u;             // ascending as unsigned; subnormals keep their place
    const uint64_t g = group ? static_cast<uint32_t>(group[i]) : 0u;
    key[i] = static_cast<long long>((g << 32) | u);
  }
  nan = block_sum(nan, lds);
  if (threadIdx.x == 0 && nan) atomicAdd(bad, nan);
}

// ---- pointwise sums ------------------------------------------------------------------------------------------------------
constexpr int kPointF = 5, kPointI = 4;

__device__ __forceinline__ double clip_eps(double x) {
  const double eps = 1.1920928955078125e-07;                         // 2^-23, the eps of float32
  return x < eps ? eps : (x > 1.0 - eps ? 1.0 - eps : x);
}

__global__ void __launch_bounds__(kThreads) point_partial_kernel(const float* __restrict__ pred, const float* __restrict__ label,
                                                                 int64_t n, double mean, double* __restrict__ part_f,
                                                                 long long* __restrict__ part_i) {
  __shared__ double ldsd[kWaves];
  __shared__ long long ldsl[kWaves];
  double f[kPointF] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long c[kPointI] = {0, 0, 0, 0};
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kPointTile;
#pragma unroll 4
  for (int j = 0; j < kPointItems; ++j) {
    const int64_t i = base + static_cast<int64_t>(j) * kThreads + threadIdx.x;
    if (i < n) {
      const float pf = pred[i], yf = label[i];
      const double p = pf, y = yf;
      const double d = y - p, dm = y - mean;
      f[0] += d * d;
      f[1] += fabs(d);
      f[2] += y;
      f[3] += dm * dm;
      // sklearn's log_loss on float32 input: the columns are [1 - p, p] with 1 - p formed in float32, both clipped to
      // [eps, 1 - eps] with the eps of float32, and the logarithms taken in double
      f[4] -= (yf != 0.f) ? log(clip_eps(p)) : log(clip_eps(static_cast<double>(1.0f - pf)));
      const bool one = rintf(pf) == 1.0f, zero = rintf(pf) == 0.0f;     // half to even: 0.5 is class 0
      c[0] += (yf == 1.f && one) ? 1 : 0;
      c[1] += (yf == 0.f && zero) ? 1 : 0;
      c[2] += (yf == 1.f) ? 1 : 0;
      c[3] += (yf == 0.f) ? 1 : 0;
    }
  }
#pragma unroll
  for (int q = 0; q < kPointF; ++q) {
    const double s = block_sum(f[q], ldsd);
    if (threadIdx.x == 0) part_f[static_cast<int64_t>(blockIdx.x) * kPointF + q] = s;
  }
#pragma unroll
  for (int q = 0; q < kPointI; ++q) {
    const long long s = block_sum(c[q], ldsl);
    if (threadIdx.x == 0) part_i[static_cast<int64_t>(blockIdx.x) * kPointI + q] = s;
  }
}

__global__ void __launch_bounds__(kThreads) point_final_kernel(const double* __restrict__ part_f,
                                                               const long long* __restrict__ part_i, int n_blocks,
                                                               double* __restrict__ out_f, long long* __restrict__ out_i) {
  __shared__ double ldsd[kWaves];
  __shared__ long long ldsl[kWaves];
  double f[kPointF] = {0.0, 0.0, 0.0, 0.0, 0.0};
  long long c[kPointI] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < n_blocks; b += kThreads) {
#pragma unroll
    for (int q = 0; q < kPointF; ++q) f[q] += part_f[static_cast<int64_t>(b) * kPointF + q];
#pragma unroll
    for (int q = 0; q < kPointI; ++q) c[q] += part_i[static_cast<int64_t>(b) * kPointI + q];
  }
#pragma unroll
  for (int q = 0; q < kPointF; ++q) {
    const double s = block_sum(f[q], ldsd);
    if (threadIdx.x == 0) out_f[q] = s;
  }
#pragma unroll
  for (int q = 0; q < kPointI; ++q) {
    const long long s = block_sum(c[q], ldsl);
    if (threadIdx.x == 0) out_i[q] = s;
  }
}

// ---- listwise metrics: one wave per user -------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(kThreads) listwise_kernel(const int32_t* __restrict__ reco, const int64_t* __restrict__ truth_ptr,
                                                            const int32_t* __restrict__ truth_items,
                                                            const int32_t* __restrict__ truth_len, const double* __restrict__ disc,
                                                            int64_t U, int k, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t u = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (u >= U) return;                                               // whole waves leave: no barrier below
  const int64_t lo0 = truth_ptr[u], hi0 = truth_ptr[u + 1];
  const int32_t* row = reco + u * k;
  int hits = 0;
  double ap = 0.0, dcg = 0.0;
  for (int c = 0; c < k; c += 64) {
    const int j = c + lane;
    const int id = j < k ? row[j] : -1;
    bool hit = false;
    if (id >= 0) {
      int64_t lo = lo0, hi = hi0;                                    // first position with truth_items[pos] >= id
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (truth_items[mid] < id) lo = mid + 1; else hi = mid;
      }
      hit = lo < hi0 && truth_items[lo] == id;
    }
    const unsigned long long mask = __ballot(hit);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    const double cum = static_cast<double>(hits + before + 1);
    ap += wave_sum_f64(hit ? cum / static_cast<double>(j + 1) : 0.0);
    dcg += wave_sum_f64(hit ? disc[j] : 0.0);
    hits += __popcll(mask);
  }
  double idcg = 0.0;
  for (int c = 0; c < hits; c += 64) idcg += wave_sum_f64(c + lane < hits ? disc[c + lane] : 0.0);
  if (lane == 0) {
    const double h = static_cast<double>(hits);
    out[u] = h / static_cast<double>(k);
    out[U + u] = h / static_cast<double>(truth_len[u]);
    out[2 * U + u] = hits ? ap / h : 0.0;
    out[3 * U + u] = hits ? dcg / idcg : 0.0;
  }
}

// ---- coverage ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) coverage_clear_kernel(int32_t* __restrict__ flags, int64_t n_items,
                                                                  unsigned long long* __restrict__ count) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n_items; i += stride) flags[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0ull;
}
__global__ void __launch_bounds__(kThreads) coverage_mark_kernel(const int32_t* __restrict__ reco, int64_t n, int64_t n_items,
                                                                 int32_t* __restrict__ flags) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const int id = reco[i];
    if (id >= 0 && id < n_items) flags[id] = 1;                     // concurrent stores of the same value
  }
}
__global__ void __launch_bounds__(kThreads) coverage_count_kernel(const int32_t* __restrict__ flags, int64_t n_items,
                                                                  unsigned long long* __restrict__ count) {
  __shared__ long long lds[kWaves];
  long long c = 0;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n_items; i += stride) c += flags[i] != 0;
  c = block_sum(c, lds);
  if (threadIdx.x == 0 && c) atomicAdd(count, static_cast<unsigned long long>(c));
}

}  // namespace

extern "C" {

size_t lr_eval_rank_ws_bytes(int64_t n) { return n < 1 || n >= (1ll << 31) ? 0 : rank_ws(n).bytes; }

size_t lr_eval_point_ws_bytes(int64_t n) {
  if (n < 1 || n >= (1ll << 31)) return 0;
  return align256(static_cast<size_t>(lr::ceil_div(n, kPointTile)) * (kPointF + kPointI) * 8);
}

int lr_eval_keys_f32(const float* score, const int32_t* group, int64_t n, int64_t* key, int32_t* bad, lr_stream_t stream) {
  if (!score || !key || !bad || n < 1) return LR_EINVAL;
  hipStream_t s = as_stream(stream);
  lr::zero_words_async(bad, 1, s);
  hipLaunchKernelGGL(keys_kernel, dim3(lr::grid_for(n, kThreads)), dim3(kThreads), 0, s, score, group, n,
                     reinterpret_cast<long long*>(key), bad);
  return launch_status();
}

int lr_eval_rank_stats(const int64_t* key_sorted, const uint8_t* label_sorted, int64_t n, int64_t* out_i64, double* out_f64,
                       void* ws, size_t ws_bytes, lr_stream_t stream) {
  if (!key_sorted || !label_sorted || !out_i64 || !out_f64 || !ws || n < 1) return LR_EINVAL;
  if (n >= (1ll << 31)) return LR_ESHAPE;
  const RankWs w = rank_ws(n);
  if (ws_bytes < w.bytes) return LR_EWORKSPACE;
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  S1* tiles1 = reinterpret_cast<S1*>(base + w.tiles1);
  S1* total1 = reinterpret_cast<S1*>(base + w.total1);
  S2* tiles2 = reinterpret_cast<S2*>(base + w.tiles2);
  S2* total2 = reinterpret_cast<S2*>(base + w.total2);
  double* pg = reinterpret_cast<double*>(base + w.gauc);
  double* pp = reinterpret_cast<double*>(base + w.pr);
  long long* pn = reinterpret_cast<long long*>(base + w.num2);
  const long long* key = reinterpret_cast<const long long*>(key_sorted);
  const int n_tiles = static_cast<int>(lr::ceil_div(n, kScanTile));
  const dim3 grid(n_tiles), block(kThreads);
  hipLaunchKernelGGL(rank_reduce1_kernel, grid, block, 0, s, key, label_sorted, n, tiles1);
  hipLaunchKernelGGL(rank_scan_tiles_kernel<S1>, dim3(1), block, 0, s, tiles1, n_tiles, total1);
  hipLaunchKernelGGL(rank_reduce2_kernel, grid, block, 0, s, key, label_sorted, n, tiles1, tiles2);
  hipLaunchKernelGGL(rank_scan_tiles_kernel<S2>, dim3(1), block, 0, s, tiles2, n_tiles, total2);
  hipLaunchKernelGGL(rank_finish_kernel, grid, block, 0, s, key, label_sorted, n, tiles1, total1, tiles2, pg, pp, pn);
  hipLaunchKernelGGL(rank_final_kernel, dim3(1), block, 0, s, pg, pp, pn, n_tiles, total1, n,
                     reinterpret_cast<long long*>(out_i64), out_f64);
  return launch_status();
}

int lr_eval_point_sums_f32(const float* pred, const float* label, int64_t n, double mean, double* out_f64, int64_t* out_i64,
                           void* ws, size_t ws_bytes, lr_stream_t stream) {
  if (!pred || !label || !out_f64 || !out_i64 || !ws || n < 1) return LR_EINVAL;
  if (n >= (1ll << 31)) return LR_ESHAPE;
  if (ws_bytes < lr_eval_point_ws_bytes(n)) return LR_EWORKSPACE;
  hipStream_t s = as_stream(stream);
  const int n_blocks = static_cast<int>(lr::ceil_div(n, kPointTile));
  double* pf = static_cast<double*>(ws);
  long long* pi = reinterpret_cast<long long*>(pf + static_cast<size_t>(n_blocks) * kPointF);
  hipLaunchKernelGGL(point_partial_kernel, dim3(n_blocks), dim3(kThreads), 0, s, pred, label, n, mean, pf, pi);
  hipLaunchKernelGGL(point_final_kernel, dim3(1), dim3(kThreads), 0, s, pf, pi, n_blocks, out_f64,
                     reinterpret_cast<long long*>(out_i64));
  return launch_status();
}

int lr_eval_listwise(const int32_t* reco, const int64_t* truth_ptr, const int32_t* truth_items, const int32_t* truth_len,
                     const double* disc, int64_t U, int k, double* out, lr_stream_t stream) {
  if (!reco || !truth_ptr || !truth_len || !disc || !out || U < 1) return LR_EINVAL;
  if (k < 1 || k > kMaxK || U >= (1ll << 31)) return LR_ESHAPE;
  hipLaunchKernelGGL(listwise_kernel, dim3(static_cast<unsigned>(lr::ceil_div(U, kWaves))), dim3(kThreads), 0, as_stream(stream),
                     reco, truth_ptr, truth_items, truth_len, disc, U, k, out);
  return launch_status();
}

int lr_eval_coverage_i32(const int32_t* reco, int64_t n, int64_t n_items, int32_t* flags, int64_t* count, lr_stream_t stream) {
  if (!reco || !flags || !count || n < 1 || n_items < 1) return LR_EINVAL;
  hipStream_t s = as_stream(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
  hipLaunchKernelGGL(coverage_clear_kernel, dim3(lr::grid_for(n_items, kThreads)), dim3(kThreads), 0, s, flags, n_items, cnt);
  hipLaunchKernelGGL(coverage_mark_kernel, dim3(lr::grid_for(n, kThreads)), dim3(kThreads), 0, s, reco, n, n_items, flags);
  hipLaunchKernelGGL(coverage_count_kernel, dim3(lr::grid_for(n_items, kThreads)), dim3(kThreads), 0, s, flags, n_items, cnt);
  return launch_status();
}

}  // extern "C"
