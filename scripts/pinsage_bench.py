"""PinSage at a MovieLens-20M-like shape (138,493 users x 26,744 items, `--nnz` skewed interactions drawn from a seed; both
CSRs are built on the device, as in scripts/graphsage_bench.py): one training step of `PinSageNet` on the fused kernels of
csrc/pinsage.hip against the same net composed from torch ops under autograd (`fused=False`: same sampled ids and weights, same
optimiser), and the sampling on its own.  Two configurations: i2i at the reference's defaults (256 start nodes, 10 walks of 5
steps for the pairs; 2 layers x 3 neighbours from 10 walks of at most 2 steps with termination probability 0.5, embed_size 16,
max margin) and u2i at batch 8,192 (bpr).  No item features (T = 1).

The two nets are timed in alternating rounds inside one process (HIP events around every step, after warm-up steps of every
shape); the table holds the median and the minimum over rounds of the mean step time.  Prints one JSON line.

    python scripts/pinsage_bench.py [--steps 30] [--rounds 5] [--nnz 2000000]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd.nets.pinsage_net import PinSageNet  # noqa: E402
from scripts.graphsage_bench import N_ITEMS, N_USERS, SEED, events, make_graph, sample_i2i, sample_u2i  # noqa: E402


def bench(paradigm, B, graph, users, items, steps, rounds, dev):
    loss = "max_margin" if paradigm == "i2i" else "bpr"
    nets = {name: PinSageNet(paradigm, N_USERS, N_ITEMS, 16, 2, 3, 0.0, dev, graph, seed=SEED, fused=name == "fused")
            for name in ("fused", "composed")}
    draw = (lambda net: sample_i2i(net, B, net.step + 1)) if paradigm == "i2i" else (
        lambda net: sample_u2i(net, B, net.step + 1, users, items))

    def step(net):
        q, pos, neg = draw(net)
        return net.train_step(loss, q, pos, neg)

    def tower_only(net):
        q, pos, neg = draw(net)
        net.step += 1
        ids = torch.cat([q, pos, neg] if paradigm == "i2i" else [pos, neg]).contiguous()
        t = net.item_tower(ids, net.step, True)
        t.backward(torch.ones_like(t.repr))
        return ids.numel()

    for net in nets.values():                       # warm-up of every shape
        for _ in range(3):
            step(net)
            tower_only(net)
    torch.cuda.synchronize()
    times = {k: [] for k in ("fused", "composed", "fused_tower", "composed_tower", "sampling", "neighbors")}
    trees = 0
    for _ in range(rounds):                         # alternating rounds in one process
        for name, net in nets.items():
            times[name].append(events(lambda: step(net), steps))
            times[name + "_tower"].append(events(lambda: tower_only(net), steps))
        net = nets["fused"]
        times["sampling"].append(events(lambda: draw(net), steps))
        q, pos, neg = draw(net)
        ids = torch.cat([q, pos, neg] if paradigm == "i2i" else [pos, neg]).contiguous()
        trees = ids.numel()
        times["neighbors"].append(events(lambda: net.tree(ids, 1), steps))
    row = {"paradigm": paradigm, "batch": B, "loss": loss, "num_layers": 2, "num_neighbors": 3, "embed_size": 16, "num_walks": 10,
           "neighbor_walk_len": 2, "termination_prob": 0.5, "item_trees_per_step": trees, "fused_path_used": nets["fused"].item_fused}
    for k, v in times.items():
        row[k + "_ms_median"], row[k + "_ms_min"] = round(statistics.median(v), 4), round(min(v), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nnz", type=int, default=2_000_000)
    a = ap.parse_args()
    dev = torch.device("cuda")
    graph, users, items = make_graph(a.nnz, dev)
    perm = torch.randperm(users.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    users, items = users[perm].contiguous(), items[perm].contiguous()
    res = {"bench": "pinsage", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, a.nnz],
           "steps_per_round": a.steps, "rounds": a.rounds, "rows": []}
    for paradigm, B in (("i2i", 256), ("u2i", 8192)):
        res["rows"].append(bench(paradigm, B, graph, users, items, a.steps, a.rounds, dev))
        print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
