"""UserCF / ItemCF at MovieLens shapes: the ItemCF fit at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263
distinct Zipf pairs from `bench_workloads.distinct_interactions`, labels in 1..5) and the UserCF fit at the MovieLens-1M
shape (6,040 x 3,706 x 1,000,209).  Prints one JSON line; per leg: ms per stage (host statistics, the similarity's count +
scan + fill, the top-k), W = sum_y deg(y)^2 (the pair visits of one pass), the nnz of the result, pair visits per second,
and the inverted-list bytes the two passes stream (W x 8 B each) against 8 TB/s; plus `recommend` for 1,024 users at
n_rec = 10 and `predict` for 1 M pairs on each leg's model.

    python scripts/cf_bench.py [--legs item20m,user1m] [--sim cosine] [--reps 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_workloads import HBM_PEAK_GBS, distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.algorithms import ItemCF, UserCF  # noqa: E402
from librecommender_amd.bases import cf_base  # noqa: E402

LEGS = {"item20m": ("item_cf", 138_493, 26_744, 20_000_263), "user1m": ("user_cf", 6_040, 3_706, 1_000_209)}


def ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def leg(name, sim_type, reps, gen, dev):
    cf_type, n_users, n_items, nnz = LEGS[name]
    u, i = distinct_interactions(nnz, n_users, n_items, gen, dev)
    lab = torch.randint(1, 6, (nnz,), generator=gen, device=dev).to(torch.float32)
    ui = sp.csr_matrix((lab.cpu().numpy(), (u.cpu().numpy(), i.cpu().numpy())), shape=(n_users, n_items))
    ui.sort_indices()
    user = cf_base._DeviceCsr.from_scipy(ui, dev)
    item = user.transpose()
    X, Y = (item, user) if cf_type == "item_cf" else (user, item)
    x_host = ui.T.tocsr() if cf_type == "item_cf" else ui
    cls = ItemCF if cf_type == "item_cf" else UserCF
    model = cls.__new__(cls)
    model.sim_type, model.min_common = sim_type, 1
    t = time.perf_counter()
    stats = cf_base.row_norm(x_host)
    host_ms = (time.perf_counter() - t) * 1e3
    deg_y = (Y.ptr[1:] - Y.ptr[:-1]).to(torch.float64)
    W = int((deg_y * deg_y).sum())
    model._similarity(x_host, X, Y)        # warm-up
    sim_ms = []
    for _ in range(reps):
        sim, t_ = ms(lambda: model._similarity(x_host, X, Y))
        sim_ms.append(t_)
    _, topk_ms = ms(lambda: ops.cf_topk(sim.ptr, sim.col, sim.val, 20))
    best = min(sim_ms)
    out = {"cf_type": cf_type, "shape": [n_users, n_items, nnz], "sim_type": sim_type, "host_stats_ms": round(host_ms, 1),
           "similarity_ms": round(best, 2), "similarity_ms_all": [round(x, 2) for x in sim_ms],
           "topk20_ms": round(topk_ms, 2), "W_pair_visits_per_pass": W, "sim_nnz": int(sim.col.numel()),
           "pair_visits_per_s": round(2 * W / (best * 1e-3), 1),
           "inverted_list_bytes": 2 * W * 8, "floor_ms_at_8TBs": round(2 * W * 8 / (HBM_PEAK_GBS * 1e9) * 1e3, 2),
           "fraction_of_floor": round(2 * W * 8 / (HBM_PEAK_GBS * 1e9) * 1e3 / best, 3)}
    del stats
    return out, (user, item, sim, n_users, n_items, cf_type)


def serve(state, gen, dev):
    user, item, sim, n_users, n_items, cf_type = state
    tk = ops.cf_topk(sim.ptr, sim.col, sim.val, 20)
    users = torch.randint(0, n_users, (1024,), generator=gen, device=dev).to(torch.int32)
    cons_ptr = torch.zeros(1025, dtype=torch.int64, device=dev)
    lens = (user.ptr[users.long() + 1] - user.ptr[users.long()])
    cons_ptr[1:] = torch.cumsum(lens, 0)
    idx = torch.cat([user.col[int(a):int(b)] for a, b in zip(user.ptr[users.long()].tolist(),
                                                            user.ptr[users.long() + 1].tolist())])
    rec = lambda: ops.cf_recommend(users, cf_type == "user_cf", user.ptr, user.col, user.val, *tk, n_items,  # noqa: E731
                                   cons_ptr, idx, True, 10)
    rec()
    _, rec_ms = ms(rec)
    n = 1_000_000
    pu = torch.randint(0, n_users, (n,), generator=gen, device=dev).to(torch.int32)
    pi = torch.randint(0, n_items, (n,), generator=gen, device=dev).to(torch.int32)
    s_rows, i_rows, inter = (pi, pu, user) if cf_type == "item_cf" else (pu, pi, item)
    pred = lambda: ops.cf_predict(s_rows, i_rows, sim.ptr, sim.col, sim.val, inter.ptr, inter.col, inter.val, 20,  # noqa: E731
                                  True, 1.0, 5.0, 3.5)
    pred()
    _, pred_ms = ms(pred)
    return {"recommend_1024_users_n_rec10_ms": round(rec_ms, 2), "predict_1M_pairs_ms": round(pred_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="item20m,user1m")
    ap.add_argument("--sim", default="cosine")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"bench": "cf", "device": torch.cuda.get_device_name(dev)}
    for name in a.legs.split(","):
        out, state = leg(name, a.sim, a.reps, gen, dev)
        out.update(serve(state, gen, dev))
        res[name] = out
        del state
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
