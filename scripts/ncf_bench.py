"""NCF on the device: the fused training step against the autograd composition, the one-launch inference tower
(`ops.ncf_score`, csrc/ncf.hip) against the torch inference composition, and full-catalogue ranking.  Writes `<out>/ncf.json`
and `<out>/ncf.md` and prints the JSON.

(a) the step: `NCFNet` at the MovieLens-20M id shape (138,493 users x 26,744 items, Zipf ids), embed 16, hidden (128, 64, 32),
    cross entropy, row-wise Adam, against the same net built with `fused=False`, at batch 512 (the default 256 with one
    negative) and 8,192.
(b) the tower: `net.forward` on 2^18 pairs with `ops.ncf_score` and with the torch composition (gather + BatchNorm + `addmm` ...),
    for (128, 64, 32) and for (64, 64, 64, 16); the two are compared on the same pairs before they are timed.
(c) ranking: the scores of 1,024 users over a 100,000-item catalogue and their top 10 (`NCFCatalogScorer.scores` + `topk`, what
    `recommend_user` runs per block of users): the `ops.pair_mlp` branch (default stack), the chunked `ops.ncf_score` branch
    (four-layer stack), and the chunked torch composition on 64 of the users.

Every variant is warmed up, then timed in alternating rounds with a HIP-event pair around `reps` back-to-back calls per round;
median [min, max] over the rounds.

    python scripts/ncf_bench.py [--out profiles] [--rounds 7] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd.nets import NCFNet  # noqa: E402
from librecommender_amd.recommendation.ncf_catalog import NCFCatalogScorer  # noqa: E402

N_USERS, N_ITEMS = 138_493, 26_744


def zipf_ids(n, rows, gen, dev):
    w = 1.0 / torch.arange(1, rows + 1, device=dev, dtype=torch.float64)
    return torch.multinomial(w, n, replacement=True, generator=gen).to(torch.int32)


def event_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(variants, rounds, reps, warm=5):
    """{name: fn} -> {name: (median us, min, max)} over `rounds` alternating rounds."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(event_us(fn, reps))
    return {k: (round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)) for k, v in t.items()}


def trained(net, gen, dev, steps=3, B=512):
    """A few steps, so that the BatchNorm averages and affines are not the initial ones."""
    for _ in range(steps):
        net.train_step(zipf_ids(B, net.tables.n_users, gen, dev), zipf_ids(B, net.tables.n_items, gen, dev),
                       torch.randint(0, 2, (B,), device=dev, generator=gen).float())
    return net


def step_rows(rounds, reps, dev):
    out, gen = [], torch.Generator(device=dev)
    gen.manual_seed(1)
    for B in (512, 8192):
        users, items = zipf_ids(B, N_USERS, gen, dev), zipf_ids(B, N_ITEMS, gen, dev)
        labels = (torch.arange(B, device=dev) % 2).float()
        nets = {name: NCFNet(N_USERS, N_ITEMS, 16, (128, 64, 32), True, None, 0.01, 1e-5, 0, dev, fused=name == "fused")
                for name in ("fused", "composition")}
        assert nets["fused"].fused and not nets["composition"].fused
        la, lb = (float(n.train_step(users, items, labels)) for n in nets.values())
        res = alternate({k: (lambda n_=n_: n_.train_step(users, items, labels)) for k, n_ in nets.items()}, rounds, reps)
        out.append({"batch": B, "first_step_loss_fused_composition": [la, lb], "us_per_step_median_min_max": res,
                    "tail_form": "one launch" if nets["fused"]._blk[B]["tail"].fused else "chain",
                    "composition_over_fused": round(res["composition"][0] / res["fused"][0], 3)})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def score_rows(rounds, reps, dev, n=1 << 18):
    out, gen = [], torch.Generator(device=dev)
    gen.manual_seed(2)
    for hidden in ((128, 64, 32), (64, 64, 64, 16)):
        net = trained(NCFNet(N_USERS, N_ITEMS, 16, hidden, True, None, 0.01, 1e-5, 0, dev), gen, dev)
        assert net.score_kernel
        users, items = zipf_ids(n, N_USERS, gen, dev), zipf_ids(n, N_ITEMS, gen, dev)

        def composed():
            net.score_kernel = False
            try:
                return net.forward(users, items)
            finally:
                net.score_kernel = True

        diff = float((net.forward(users, items) - composed()).abs().max())
        res = alternate({"ncf_score": lambda: net.forward(users, items), "torch": composed}, rounds, reps)
        out.append({"hidden": list(hidden), "pairs": n, "max_abs_diff": diff, "us_per_call_median_min_max": res,
                    "torch_over_ncf_score": round(res["torch"][0] / res["ncf_score"][0], 2),
                    "pairs_per_s_ncf_score": round(n / res["ncf_score"][0] * 1e6)})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def rank_rows(rounds, reps, dev, n_users=1024, n_items=100_000, k=10):
    out, gen = [], torch.Generator(device=dev)
    gen.manual_seed(3)
    uids = torch.randperm(20_000, device=dev, generator=gen)[:n_users].tolist()
    for hidden in ((128, 64, 32), (64, 64, 64, 16)):
        net = trained(NCFNet(20_000, n_items, 16, hidden, True, None, 0.01, 1e-5, 0, dev), gen, dev)
        sc = NCFCatalogScorer(SimpleNamespace(net=net, device=dev, n_items=n_items))
        fold = sc._item_side()[0]
        branch = "pair_mlp" if sc._fused_tail(fold[2], fold[3]) is not None else "ncf_score"
        rank = lambda ids=uids: torch.topk(sc.scores(ids), k, dim=1, sorted=True).indices        # noqa: E731
        variants = {branch: rank}
        sub = uids[:64]
        ref = torch.stack([net.forward(torch.full((n_items,), u, dtype=torch.int32, device=dev),
                                       torch.arange(n_items, dtype=torch.int32, device=dev)) for u in sub[:4]])
        diff = float((sc.scores(sub[:4]) - ref).abs().max())
        if branch == "ncf_score":           # the same chunked forward from torch ops, on 64 of the users
            def composed():
                net.score_kernel = False
                try:
                    return rank(sub)
                finally:
                    net.score_kernel = True
            variants["torch_64_users"] = composed
        res = alternate(variants, rounds, max(2, reps // 10), warm=2)
        out.append({"hidden": list(hidden), "users": n_users, "items": n_items, "k": k, "branch": branch,
                    "max_abs_diff_vs_forward": diff, "us_per_call_median_min_max": res,
                    "users_per_s": round(n_users / res[branch][0] * 1e6)})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def markdown(res):
    fmt = lambda t: f"{t[0]} [{t[1]}, {t[2]}]"  # noqa: E731
    L = ["# NCF: training step, one-launch inference tower, catalogue ranking", "",
         f"Measured on {res['device']} by `scripts/ncf_bench.py` ({res['rounds']} alternating rounds, HIP events; median [min, max]",
         "over the rounds, in us).  Everything below is measured; nothing here is extrapolated.", "",
         "## (a) the training step, embed 16, hidden (128, 64, 32), MovieLens-20M id shape", "",
         "| batch | fused step | autograd composition (`fused=False`) | composition / fused | tail form |", "|---|---|---|---|---|"]
    for r in res["step"]:
        u = r["us_per_step_median_min_max"]
        L.append(f"| {r['batch']} | {fmt(u['fused'])} | {fmt(u['composition'])} | {r['composition_over_fused']} | {r['tail_form']} |")
    L += ["", "## (b) `ops.ncf_score` against the torch inference composition, 2^18 pairs, embed 16", "",
          "| hidden | ncf_score | torch | torch / ncf_score | pairs / s (ncf_score) | largest difference between the two |",
          "|---|---|---|---|---|---|"]
    for r in res["score"]:
        u = r["us_per_call_median_min_max"]
        L.append(f"| {tuple(r['hidden'])} | {fmt(u['ncf_score'])} | {fmt(u['torch'])} | {r['torch_over_ncf_score']} | "
                 f"{r['pairs_per_s_ncf_score']:,} | {r['max_abs_diff']:.2e} |")
    L += ["", "## (c) scores of 1,024 users over 100,000 items and their top 10", "",
          "| hidden | branch | per call | users / s | the same from torch ops, 64 users | largest difference from `net.forward` |",
          "|---|---|---|---|---|---|"]
    for r in res["rank"]:
        u = r["us_per_call_median_min_max"]
        t64 = fmt(u["torch_64_users"]) if "torch_64_users" in u else "not measured"
        L.append(f"| {tuple(r['hidden'])} | {r['branch']} | {fmt(u[r['branch']])} | {r['users_per_s']:,} | {t64} | "
                 f"{r['max_abs_diff_vs_forward']:.2e} |")
    L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"bench": "ncf", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "reps": a.reps,
           "step": step_rows(a.rounds, a.reps, dev), "score": score_rows(a.rounds, a.reps, dev),
           "rank": rank_rows(a.rounds, a.reps, dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ncf.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, "ncf.md"), "w") as f:
        f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
