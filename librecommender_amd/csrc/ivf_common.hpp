// The inverted-file search, whatever the lists hold (ivf.hip: f32 rows; ivf_sq8.hip: int8 codes).  Here: the work plan, the
// 16-lane DPP sum, a wave's running top-k over a stream of keys, the scan kernel as a template over a row scorer, and the one
// search driver (coarse top-nprobe, plan, scan, merge).  The plan and merge kernels live in ivf.hip behind ivf_launch_plan /
// ivf_launch_merge and work on 64-bit keys only, whatever produced them.
//
// A list format supplies a row scorer and passes it to ivf_search through a callable that picks the instantiation:
//   struct Scorer {                                  // passed to the kernel by value: pointers and widths only
//     static constexpr int RPW;                      // rows of one wave-load; kWave / RPW consecutive lanes share a row
//     static constexpr int PUSHES;                   // wave-loads pushed between two looks at the candidate list's room: 1 or 4
//     struct Query;                                  // the lane's slice of the query, in registers
//     Query load_query(const float* queries, int64_t q, int j) const;      // j: the lane's place within its row's lane group
//     float score(const Query&, int64_t row, bool in_range, int j) const;  // the row's score, valid on the group's lane j == 0;
//   };                                                                     // !in_range: nothing is loaded
#pragma once
#include "common.hpp"
#include "topk_keys.hpp"

namespace lr {

constexpr int kIvfMinCL = 64;              // shortest chunk of a list one search work item takes
constexpr int64_t kIvfSpread = int64_t(1) << 17;   // a whole-catalogue list is cut into about this many chunks (over all queries)
constexpr size_t kIvfMaxPartBytes = size_t(4) << 30;   // partial top-k keys the search may ask for

static inline size_t ivf_al(size_t x) { return (x + 255) / 256 * 256; }

template <int CTRL>
__device__ __forceinline__ float ivf_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row, the same bits on each of them (every step adds a pair in both orders)
__device__ __forceinline__ float row16_sum(float v) {
  v = ivf_dpp_add<0xB1>(v);    // quad_perm [1,0,3,2]
  v = ivf_dpp_add<0x4E>(v);    // quad_perm [2,3,0,1]
  v = ivf_dpp_add<0x141>(v);   // row_half_mirror
  v = ivf_dpp_add<0x140>(v);   // row_mirror
  return v;
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float p) {
  p = fmaf(a.x, b.x, p);
  p = fmaf(a.y, b.y, p);
  p = fmaf(a.z, b.z, p);
  return fmaf(a.w, b.w, p);
}

struct IvfPlan {
  bool ok;
  int CL;            // rows per work item
  int C;             // candidate-list capacity of a wave (keys in LDS)
  int K2;            // ivf_pow2(k): the final sort
  int64_t P;         // B * nprobe (query, probed list) pairs
  int64_t Wmax;      // work items at most
  size_t off_cs, off_ci, off_pref, off_cnt, off_keys, off_coarse, coarse_bytes, total;
};

static IvfPlan ivf_plan(int64_t B, int64_t N, int D, int k, int nprobe, int nlist) {
  IvfPlan p{};
  p.ok = false;
  if (B < 1 || N < 1 || N >= (int64_t(1) << 31) || D < 4 || D > 256 || (D % 4) != 0 || k < 1 || k > 1024 || nlist < 1 ||
      nlist > 65536 || nprobe < 1 || nprobe > nlist || nlist > N)
    return p;
  p.coarse_bytes = lr_score_topk_ws_bytes(B, nlist, D, nprobe);      // the coarse kernel's own envelope (nprobe <= 4096)
  if (p.coarse_bytes == 0) return p;
  const int64_t cl = ceil_div(N * B, kIvfSpread);
  p.CL = static_cast<int>(ceil_div(cl < kIvfMinCL ? kIvfMinCL : cl, 64) * 64);
  p.K2 = ivf_pow2(k);
  const int c = static_cast<int>(ceil_div(k + 256, 64) * 64);
  p.C = c > p.K2 ? c : p.K2;
  p.P = B * nprobe;
  p.Wmax = B * (nprobe + ceil_div(N, p.CL));      // per query: sum of ceil(len / CL) over distinct lists <= nprobe + N / CL
  if (p.P + 1 >= (int64_t(1) << 31) || p.Wmax >= (int64_t(1) << 31)) return p;
  const size_t key_bytes = static_cast<size_t>(p.Wmax) * k * sizeof(uint64_t);
  if (key_bytes > kIvfMaxPartBytes) return p;
  size_t o = 0;
  p.off_cs = o; o += ivf_al(static_cast<size_t>(p.P) * sizeof(float));
  p.off_ci = o; o += ivf_al(static_cast<size_t>(p.P) * sizeof(int64_t));
  p.off_pref = o; o += ivf_al(static_cast<size_t>(p.P + 1) * sizeof(int32_t));
  p.off_cnt = o; o += ivf_al(static_cast<size_t>(p.Wmax) * sizeof(int32_t));
  p.off_keys = o; o += ivf_al(key_bytes);
  p.off_coarse = o; o += ivf_al(p.coarse_bytes);
  p.total = o;
  p.ok = true;
  return p;
}

// one wave's running top-k over a stream of keys: L[0..cnt) in LDS, T the threshold below which nothing can enter any more
struct WaveTopk {
  uint64_t* L;
  int cnt, k, C, lane;
  uint64_t T;
  __device__ __forceinline__ void shrink() {
    T = wave_select_kth(L, cnt, k, lane);
    cnt = wave_compact(L, cnt, T, lane);
    if (cnt > k) cnt = k;      // keys are distinct for a well-formed index: only duplicate ids could leave more
  }
  // every lane calls; at most `room` lanes pass per call and cnt + room <= C holds on entry
  __device__ __forceinline__ void push(bool pass, uint64_t key) {
    const uint64_t mask = __ballot(pass);
    if (pass) L[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = key;
    cnt += __popcll(mask);
  }
};

// LDS of a scan workgroup (four waves' candidate lists); the merge workgroup takes 64 bytes more for its counts
static inline size_t ivf_scan_lds(const IvfPlan& p) { return static_cast<size_t>(4) * p.C * sizeof(uint64_t); }

// ---- scan ---------------------------------------------------------------------------------------------------------------------
struct IvfScanArgs {
  const float* queries;
  const int64_t* coarse_ids;      // [P] the probed lists
  int nprobe;
  int64_t P;
  const int32_t* pref;            // [P + 1] work items before each pair
  const int64_t* list_ptr;
  const int32_t* list_ids;
  const int64_t* consumed_ptr;
  const int32_t* consumed_idx;
  const uint8_t* filter_flag;
  int k, C, CL;
  int64_t Wmax;
  uint64_t* part_keys;            // [Wmax, k]
  int32_t* part_cnt;              // [Wmax]
};

// A persistent grid of waves, one work item (CL rows of one probed list of one query) per wave at a time.  The scorer's rows
// stream four wave-loads per trip; survivors of the running threshold and of the consumed filter enter the wave's candidate list
// as 64-bit keys, and the list is cut back to its k best whenever the next PUSHES wave-loads might not fit (cnt + PUSHES * RPW
// <= C holds before each such group).  Every work item leaves <= k keys.
template <class Scorer>
__global__ __launch_bounds__(kBlock) void ivf_scan_kernel(IvfScanArgs a, Scorer s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RPW = Scorer::RPW, LPR = kWave / RPW, PUSHES = Scorer::PUSHES;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6, j = lane & (LPR - 1), g = lane / LPR;
  const int k = a.k, C = a.C;
  WaveTopk tk;
  tk.L = reinterpret_cast<uint64_t*>(smem) + static_cast<size_t>(wid) * C;
  tk.k = k;
  tk.C = C;
  tk.lane = lane;
  const int64_t total = a.pref[a.P] < a.Wmax ? a.pref[a.P] : a.Wmax;      // (Wmax bounds it for every well-formed index)
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + wid; w < total; w += static_cast<int64_t>(gridDim.x) * 4) {
    int64_t lo = 0, hi = a.P - 1;      // the pair of work item w: pref[pair] <= w < pref[pair + 1]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (a.pref[mid + 1] > w) hi = mid; else lo = mid + 1;
    }
    const int64_t pair = lo, q = pair / a.nprobe, l = a.coarse_ids[pair];
    const int64_t r0 = a.list_ptr[l] + (w - a.pref[pair]) * a.CL;
    const int64_t r1 = a.list_ptr[l + 1] < r0 + a.CL ? a.list_ptr[l + 1] : r0 + a.CL;
    const typename Scorer::Query qv = s.load_query(a.queries, q, j);
    const bool flt = a.consumed_ptr != nullptr && (a.filter_flag == nullptr || a.filter_flag[q] != 0);
    const int64_t clo = flt ? a.consumed_ptr[q] : 0, chi = flt ? a.consumed_ptr[q + 1] : 0;
    tk.cnt = 0;
    tk.T = 0ull;
    for (int64_t r = r0; r < r1; r += 4 * RPW) {
      float sc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t row = r + u * RPW + g;
        sc[u] = s.score(qv, row, row < r1, j);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t row = r + u * RPW + g;
        const bool ok = j == 0 && row < r1 && sc[u] == sc[u];      // NaN scores are dropped
        const int32_t id = ok ? a.list_ids[row] : 0;
        const uint64_t key = make_key(sc[u], static_cast<uint32_t>(id));
        bool pass = ok && key > tk.T;
        if (pass && flt) pass = !is_consumed(a.consumed_idx, clo, chi, id);
        tk.push(pass, key);      // at most RPW lanes pass
        if ((u + 1) % PUSHES == 0 && tk.cnt + PUSHES * RPW > C) tk.shrink();
      }
    }
    if (tk.cnt > k) tk.shrink();
    for (int i = lane; i < tk.cnt; i += kWave) a.part_keys[w * k + i] = tk.L[i];
    if (lane == 0) a.part_cnt[w] = tk.cnt;
  }
}

// ivf.hip.  plan: pref[i] = work items before (query, probed list) pair i, pref[P] = their total.  merge: one workgroup per query
// folds its work items' keys (part_keys [Wmax, k], part_cnt [Wmax]) into out_scores / out_ids [B, k], sorted, -inf / -1 beyond.
void ivf_launch_plan(const IvfPlan& p, const int64_t* coarse_ids, const int64_t* list_ptr, int nlist, int32_t* pref, hipStream_t s);
void ivf_launch_merge(const IvfPlan& p, int64_t B, int nprobe, int k, const int32_t* pref, const uint64_t* part_keys,
                      const int32_t* part_cnt, float* out_scores, int64_t* out_ids, hipStream_t s);

// ---- driver -------------------------------------------------------------------------------------------------------------------
// The whole search but the format's own part: `lists_shape_ok` / `lists_ptrs_ok` are the caller's checks of its list payload
// (LR_ESHAPE / LR_EINVAL, in the place of the common ones), and `with_scorer(launch)` calls `launch(scorer)` once, with the scorer
// instantiation that fits the row width.
template <class WithScorer>
int ivf_search(const float* queries, int64_t B, const float* centroids, int nlist, const int64_t* list_ptr, const int32_t* list_ids,
               int64_t N, int D, const int64_t* consumed_ptr, const int32_t* consumed_idx, const uint8_t* filter_flag, int k,
               int nprobe, float* out_scores, int64_t* out_ids, void* ws, size_t ws_bytes, lr_stream_t stream, bool lists_shape_ok,
               bool lists_ptrs_ok, WithScorer with_scorer) {
  LR_CHECK_ARG(B >= 0);
  if (B == 0) return LR_OK;
  const IvfPlan p = ivf_plan(B, N, D, k, nprobe, nlist);
  if (!p.ok || !lists_shape_ok) return LR_ESHAPE;
  LR_CHECK_ARG(queries && centroids && list_ptr && list_ids && out_scores && out_ids && lists_ptrs_ok);
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(queries) % 16 == 0 && reinterpret_cast<uintptr_t>(centroids) % 16 == 0);
  if (ws == nullptr || ws_bytes < p.total) return LR_EWORKSPACE;
  LR_CHECK_ARG(reinterpret_cast<uintptr_t>(ws) % 256 == 0);
  hipStream_t s = as_stream(stream);
  char* w = static_cast<char*>(ws);
  float* cs = reinterpret_cast<float*>(w + p.off_cs);
  int64_t* ci = reinterpret_cast<int64_t*>(w + p.off_ci);
  int32_t* pref = reinterpret_cast<int32_t*>(w + p.off_pref);
  int32_t* cnt = reinterpret_cast<int32_t*>(w + p.off_cnt);
  uint64_t* keys = reinterpret_cast<uint64_t*>(w + p.off_keys);
  const int rc = lr_score_topk_f32(queries, B, centroids, nlist, D, nullptr, nullptr, nullptr, nprobe, 0, cs, ci, w + p.off_coarse,
                                   p.coarse_bytes, stream);
  if (rc != LR_OK) return rc;
  ivf_launch_plan(p, ci, list_ptr, nlist, pref, s);
  const IvfScanArgs sa{queries, ci, nprobe, p.P, pref, list_ptr, list_ids, consumed_ptr, consumed_idx, filter_flag, k, p.C, p.CL,
                       p.Wmax, keys, cnt};
  with_scorer([&](auto scorer) {
    hipLaunchKernelGGL(ivf_scan_kernel<decltype(scorer)>, dim3(grid_for(p.Wmax, 4)), dim3(kBlock), ivf_scan_lds(p), s, sa, scorer);
  });
  ivf_launch_merge(p, B, nprobe, k, pref, keys, cnt, out_scores, out_ids, s);
  return launch_status();
}

// is the list payload a non-null, 16-byte aligned pointer
static inline bool ivf_rows_ptr_ok(const void* p) { return p != nullptr && reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace lr
