"""RsItemCF at the MovieLens-20M shape of scripts/cf_bench.py (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs,
labels in 1..5): what a refresh of a neighbourhood model costs with and without the incremental state.

For a delta of 1 % and of 10 % of the interactions (chosen at random; the base is the rest) the script times, on the device
calls that `RsCfBase.fit` makes, every leg after one warm-up pass and `--reps` times, alternating the legs, and keeps the
best and all times (a host clock around work that ends in a device synchronise):

  fit        the from-scratch fit on the base: sums of squares, pair state, update of the empty state, top-k;
  update     the update with the delta, by stage: sums of squares, delta pairs (`ops.cf_pair_state`), merge and refresh
             (`ops.cf_state_update`), top-k over all rows (`ops.cf_topk`);
  refit      `ItemCF(sim_type="cosine")`'s similarity (host row norms + `ops.cf_similarity`) and top-k on the union: the
             only way to refresh a neighbourhood model without the state.

It also reports the entries of the state, the device memory it holds (16 B per entry + rowptr + sumsq), the bytes the merge
streams (old state in, new state out) against 8 TB/s, and the entries of the refit's similarity (more than the state's: an
update does not cross a user's old interactions with the same user's new ones, as in the reference).  Prints one JSON line.

    python scripts/rs_cf_bench.py [--deltas 0.01,0.1] [--reps 3] [--out profiles/rs_cf.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_workloads import HBM_PEAK_GBS, distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.algorithms import ItemCF  # noqa: E402
from librecommender_amd.bases import cf_base  # noqa: E402

N_USERS, N_ITEMS, NNZ, K_SIM = 138_493, 26_744, 20_000_263, 20


def ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def sides(ui, dev):
    """(X, Y) = (item-major, user-major) device CSRs of a user x item host CSR."""
    user = cf_base._DeviceCsr.from_scipy(ui, dev)
    return user.transpose(), user


def fit(X, Y, dev):
    sumsq = torch.zeros(X.shape[0], dtype=torch.float32, device=dev)
    ops.cf_sumsq(X.ptr, X.val, out=sumsq)
    delta = ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val)
    state = ops.cf_state_update(ops.cf_state_empty(X.shape[0], dev), delta, sumsq)
    del delta
    return state, sumsq, ops.cf_topk(state.ptr, state.col, state.sim, K_SIM)


def update(state, sumsq, X, Y, stages):
    def stage(name, fn):
        out, t = ms(fn)
        stages[name] = t
        return out

    new_sumsq = stage("sumsq", lambda: ops.cf_sumsq(X.ptr, X.val, out=sumsq.clone()))
    delta = stage("delta_pairs", lambda: ops.cf_pair_state(X.ptr, X.col, X.val, Y.ptr, Y.col, Y.val))
    new = stage("merge_refresh", lambda: ops.cf_state_update(state, delta, new_sumsq))
    stage("topk", lambda: ops.cf_topk(new.ptr, new.col, new.sim, K_SIM))
    stages["delta_entries"] = int(delta[1].numel())
    return new


def refit(model, x_host, X, Y):
    sim = model._similarity(x_host, X, Y)
    return sim, ops.cf_topk(sim.ptr, sim.col, sim.val, K_SIM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deltas", default="0.01,0.1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="n_users,n_items,nnz (a rehearsal at a small size)")
    a = ap.parse_args()
    n_users, n_items, nnz = (int(v) for v in a.shape.split(",")) if a.shape else (N_USERS, N_ITEMS, NNZ)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    u, i = distinct_interactions(nnz, n_users, n_items, gen, dev)
    lab = torch.randint(1, 6, (nnz,), generator=gen, device=dev).to(torch.float32)
    u, i, lab = u.cpu().numpy(), i.cpu().numpy(), lab.cpu().numpy()
    pick = np.random.default_rng(0).permutation(nnz)
    csr = lambda sel: sp.csr_matrix((lab[sel], (u[sel], i[sel])), shape=(n_users, n_items))  # noqa: E731
    union = csr(slice(None))
    union.sort_indices()
    UX, UY = sides(union, dev)
    union_items = union.T.tocsr()
    model = ItemCF.__new__(ItemCF)
    model.sim_type, model.min_common = "cosine", 1
    res = {"bench": "rs_cf", "device": torch.cuda.get_device_name(dev), "shape": [n_users, n_items, nnz], "k_sim": K_SIM,
           "reps": a.reps, "legs": {}}
    for frac in (float(f) for f in a.deltas.split(",")):
        n_delta = int(round(nnz * frac))
        BX, BY = sides(csr(pick[n_delta:]), dev)
        DX, DY = sides(csr(pick[:n_delta]), dev)
        times = {"fit": [], "update": [], "refit": []}
        stages_all = []
        for rep in range(a.reps + 1):                  # the first pass warms every shape up and is not kept
            (state, sumsq, _), t_fit = ms(lambda: fit(BX, BY, dev))
            stages = {}
            new, t_upd = ms(lambda: update(state, sumsq, DX, DY, stages))
            (sim, _), t_ref = ms(lambda: refit(model, union_items, UX, UY))
            if rep:
                times["fit"].append(t_fit)
                times["update"].append(t_upd)
                times["refit"].append(t_ref)
                stages_all.append(stages)
            entries, base_entries = int(new.col.numel()), int(state.col.numel())
            # the refit sees more pairs: an update does not cross a user's old interactions with the same user's new ones
            refit_entries = int(sim.col.numel())
            del state, sumsq, new, sim
            torch.cuda.empty_cache()
        best = {k: min(v) for k, v in times.items()}
        stage_best = {k: round(min(s[k] for s in stages_all), 2) for k in ("sumsq", "delta_pairs", "merge_refresh", "topk")}
        state_bytes = entries * ops.CF_STATE_ENTRY_BYTES + (n_items + 1) * 8 + n_items * 4
        streamed = (base_entries + entries) * ops.CF_STATE_ENTRY_BYTES
        res["legs"][f"delta_{frac:g}"] = {
            "delta_interactions": n_delta, "delta_entries": stages_all[0]["delta_entries"], "base_entries": base_entries,
            "state_entries": entries, "state_bytes": state_bytes, "refit_entries": refit_entries,
            "fit_ms": round(best["fit"], 2), "update_ms": round(best["update"], 2), "refit_ms": round(best["refit"], 2),
            "all_ms": {k: [round(x, 2) for x in v] for k, v in times.items()}, "update_stage_ms": stage_best,
            "update_over_refit": round(best["update"] / best["refit"], 3),
            "merge_streamed_bytes": streamed,
            "merge_floor_ms_at_8TBs": round(streamed / (HBM_PEAK_GBS * 1e9) * 1e3, 2)}
        del BX, BY, DX, DY
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
