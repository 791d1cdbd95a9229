"""Swing at the MovieLens-1M shape: `fit`'s score computation on 6,040 users x 3,706 items x 1,000,209 distinct Zipf pairs
from `bench_workloads.distinct_interactions`.  Prints one JSON line: ms per stage (the pair table's plan, count, scan and
fill; the pattern's count + scan + fill; the score kernel; the top-k), the user pairs the reference visits
(sum_i deg(i) (deg(i) - 1) / 2), the entries of the pair table and of the result, the (entry, user pair) look-ups of the
score kernel (sum over entries i < j of C(|U_i ^ U_j|, 2)) and their rate, the bytes the design must move (look-ups x 4 B of
pair values + the pair table and the result once) against 8 TB/s, and `recommend` for 1,024 users at n_rec = 10.

    python scripts/swing_bench.py [--reps 2] [--alpha 1.0]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_workloads import HBM_PEAK_GBS, distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.bases import cf_base  # noqa: E402

SHAPE = (6_040, 3_706, 1_000_209)


def ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=1.0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    n_users, n_items, nnz = SHAPE
    u, i = distinct_interactions(nnz, n_users, n_items, gen, dev)
    key = torch.sort(u.to(torch.int64) * n_items + i.to(torch.int64)).values
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(torch.div(key, n_items, rounding_mode="floor"), minlength=n_users), 0)
    user = cf_base._DeviceCsr(ptr, (key % n_items).to(torch.int32).contiguous(),
                              torch.ones(nnz, dtype=torch.float32, device=dev), (n_users, n_items))
    item = user.transpose()
    deg_i = (item.ptr[1:] - item.ptr[:-1]).to(torch.float64)
    pair_visits = int((deg_i * (deg_i - 1) / 2).sum())
    # look-ups: sum over user pairs of C(c_uv, 2), from the dense co-occurrence counts (exact in f32 at this shape)
    B = torch.zeros((n_users, n_items), dtype=torch.float32, device=dev)
    B[u.long(), i.long()] = 1.0
    C = (B @ B.T).to(torch.float64)
    C.fill_diagonal_(0)
    lookups = int((C * (C - 1) / 2).sum() / 2)
    del B, C
    run = lambda st=None: ops.swing_scores(user.ptr, user.col, item.ptr, item.col, a.alpha, stages=st)  # noqa: E731
    run()                                   # warm-up
    total_ms, stages = [], []
    for _ in range(a.reps):
        (s_ptr, s_col, s_val), t = ms(run)
        total_ms.append(t)
    for _ in range(a.reps):
        st = {}
        run(st)
        stages.append(st)
    best = min(stages, key=lambda d: sum(d.values()))
    p_ptr, p_col, _ = ops.swing_pair_table(user.ptr, user.col, item.ptr, item.col, a.alpha)
    tk, topk_ms = ms(lambda: ops.cf_topk(s_ptr, s_col, s_val, 20))
    users = torch.randint(0, n_users, (1024,), generator=gen, device=dev).to(torch.int32)
    ul = users.long()
    cons_ptr = torch.zeros(1025, dtype=torch.int64, device=dev)
    cons_ptr[1:] = torch.cumsum(user.ptr[ul + 1] - user.ptr[ul], 0)
    idx = torch.cat([user.col[int(b):int(e)] for b, e in zip(user.ptr[ul].tolist(), user.ptr[ul + 1].tolist())])
    rec = lambda: ops.cf_recommend(users, False, user.ptr, user.col, user.val, *tk, n_items, cons_ptr, idx, True, 10)  # noqa: E731
    rec()
    _, rec_ms = ms(rec)
    n_pairs, n_entries = int(p_col.numel()), int(s_col.numel())
    moved = lookups * 4 + n_pairs * 8 * 2 + n_entries * 8 * 2
    score_ms = best.get("scores", 0.0)
    fit_ms = min(total_ms)
    out = {"bench": "swing", "device": torch.cuda.get_device_name(dev), "shape": list(SHAPE), "alpha": a.alpha,
           "fit_scores_ms": round(fit_ms, 2), "fit_scores_ms_all": [round(x, 2) for x in total_ms],
           "stage_ms": {k: round(v, 3) for k, v in best.items()},
           "user_pairs_visited_by_reference": pair_visits, "pair_table_entries": n_pairs, "result_entries": n_entries,
           "lookups": lookups, "lookups_per_s": round(lookups / (score_ms * 1e-3), 1) if score_ms else None,
           "bytes_moved_formula": "lookups * 4 + pair_table_entries * 16 + result_entries * 16", "bytes_moved": moved,
           "floor_ms_at_8TBs": round(moved / (HBM_PEAK_GBS * 1e9) * 1e3, 3),
           "fraction_of_floor": round(moved / (HBM_PEAK_GBS * 1e9) * 1e3 / fit_ms, 4),
           "topk20_ms": round(topk_ms, 2), "recommend_1024_users_n_rec10_ms": round(rec_ms, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
