// What the two inverted-file searches share (ivf.hip: f32 lists; ivf_sq8.hip: int8 lists): the work plan of a search, the
// 16-lane DPP sum, a wave's running top-k over a stream of keys, and the launchers of the plan and merge kernels, which live in
// ivf.hip and work on 64-bit keys only, whatever produced them.
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
  int K2;            // next_pow2(k): the final sort
  int64_t P;         // B * nprobe (query, probed list) pairs
  int64_t Wmax;      // work items at most
  size_t off_cs, off_ci, off_pref, off_cnt, off_keys, off_coarse, coarse_bytes, total;
};

static inline int ivf_pow2(int x) {
  int p = 2;
  while (p < x) p <<= 1;
  return p;
}

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

// ivf.hip.  plan: pref[i] = work items before (query, probed list) pair i, pref[P] = their total.  merge: one workgroup per query
// folds its work items' keys (part_keys [Wmax, k], part_cnt [Wmax]) into out_scores / out_ids [B, k], sorted, -inf / -1 beyond.
void ivf_launch_plan(const IvfPlan& p, const int64_t* coarse_ids, const int64_t* list_ptr, int nlist, int32_t* pref, hipStream_t s);
void ivf_launch_merge(const IvfPlan& p, int64_t B, int nprobe, int k, const int32_t* pref, const uint64_t* part_keys,
                      const int32_t* part_cnt, float* out_scores, int64_t* out_ids, hipStream_t s);

}  // namespace lr
