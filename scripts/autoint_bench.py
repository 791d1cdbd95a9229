"""AutoInt's training step and inference forward, the fused path (csrc/autoint.hip) against the composed path of the SAME net
(`FeatAutoIntNet(fused=False)`: `seq_nets.multi_head_attention` + `TFDense` under autograd), which is what a user had before
the kernels.  Both paths share everything around the stack: the gathers of `FeatEmbedding`, the loss in torch, the segment
build and the row-wise Adam of the tables, the dense Adam launch.

Data: 100,000 users x 20,000 items and T - 2 plain sparse columns of 1,000 values each, uniform ids, labels alternating 1 / 0;
embed_size 16, att_embed_size (8, 8, 8), 2 heads, residual, cross entropy, row-wise Adam.  Per shape the two nets are timed in
`--rounds` alternating rounds of `--steps` consecutive steps (HIP events around every step, and a host timer around one
synchronisation), so the spread between rounds stands next to the difference between the paths.  The kernel columns are
HIP-event times per call of `lr_autoint_fwd_f32` (one launch) and `lr_autoint_bwd_f32` (two launches) from a pass of their own.
Prints one JSON line.

    python scripts/autoint_bench.py [--configs 256x8,256x39,8192x8,8192x39] [--steps 50] [--rounds 3] [--infer 262144x8]
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

from librecommender_amd import ops  # noqa: E402
from librecommender_amd.nets import FeatSpec  # noqa: E402
from librecommender_amd.nets.autoint_net import FeatAutoIntNet  # noqa: E402

N_USERS, N_ITEMS, COL_VALUES, K, HEAD_DIMS, HEADS = 100_000, 20_000, 1_000, 16, (8, 8, 8), 2
KERNELS = ("lr_autoint_fwd_f32", "lr_autoint_bwd_f32")


def timed(step, n_steps):
    torch.cuda.synchronize()
    evs = []
    t = time.perf_counter()
    for s in range(n_steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(s)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3 / n_steps
    return round(wall, 4), round(sum(a.elapsed_time(b) for a, b in evs) / n_steps, 4)


def make(T, dev, fused):
    n_sp = T - 2
    spec = FeatSpec(N_USERS, N_ITEMS, n_sp, n_sp * COL_VALUES + 1)
    return FeatAutoIntNet(spec, K, HEAD_DIMS, HEADS, True, 1e-3, 1e-5, 0, dev, fused=fused)


def batches(B, T, n, dev, gen):
    users = torch.randint(0, N_USERS, (n, B), device=dev, generator=gen, dtype=torch.int32)
    items = torch.randint(0, N_ITEMS, (n, B), device=dev, generator=gen, dtype=torch.int32)
    sparse = torch.randint(0, COL_VALUES, (n, B, T - 2), device=dev, generator=gen, dtype=torch.int32)
    sparse += torch.arange(T - 2, device=dev, dtype=torch.int32)[None, None, :] * COL_VALUES
    labels = (torch.arange(B, device=dev) % 2 == 0).float()
    return users, items, sparse, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="256x8,256x39,8192x8,8192x39")
    ap.add_argument("--infer", default="262144x8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"bench": "autoint", "device": torch.cuda.get_device_name(dev), "embed_size": K, "att_embed_size": list(HEAD_DIMS),
           "num_heads": HEADS, "steps_per_round": a.steps, "rounds": a.rounds, "train": [], "infer": []}
    for cfg in a.configs.split(","):
        B, T = map(int, cfg.split("x"))
        users, items, sparse, labels = batches(B, T, a.steps, dev, gen)
        nets = {"fused": make(T, dev, True), "composed": make(T, dev, False)}
        assert nets["fused"].fused and not nets["composed"].fused
        steps = {k: (lambda s, net=net: net.train_step(users[s], items[s], labels, sparse=sparse[s])) for k, net in nets.items()}
        for step in steps.values():
            for s in range(5):
                step(s)
        row = {"batch": B, "fields": T, "fused_event_ms": [], "composed_event_ms": [], "fused_wall_ms": [], "composed_wall_ms": []}
        for _ in range(a.rounds):
            for k in ("fused", "composed"):
                wall, ev = timed(steps[k], a.steps)
                row[f"{k}_wall_ms"].append(wall)
                row[f"{k}_event_ms"].append(ev)
        ops.TIMER.enable(*KERNELS)
        for s in range(min(a.steps, 20)):
            steps["fused"](s)
        torch.cuda.synchronize()
        row["kernel_us_per_call"] = {k[11:14]: round(sum(x.elapsed_time(y) for x, y in v) * 1e3 / len(v), 2)
                                     for k, v in ops.TIMER.events.items()}
        ops.TIMER.disable()
        row["composed_over_fused"] = round(min(row["composed_event_ms"]) / min(row["fused_event_ms"]), 3)
        res["train"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    for cfg in filter(None, a.infer.split(",")):
        B, T = map(int, cfg.split("x"))
        users, items, sparse, _ = batches(B, T, 1, dev, gen)
        nets = {"fused": make(T, dev, True), "composed": make(T, dev, False)}
        fwd = {k: (lambda s, net=net: net.forward(users[0], items[0], sparse=sparse[0])) for k, net in nets.items()}
        for f in fwd.values():
            for s in range(3):
                f(s)
        row = {"batch": B, "fields": T, "fused_event_ms": [], "composed_event_ms": []}
        for _ in range(a.rounds):
            for k in ("fused", "composed"):
                row[f"{k}_event_ms"].append(timed(fwd[k], 20)[1])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fwd["fused"](0)
        row["fused_peak_extra_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        torch.cuda.reset_peak_memory_stats()
        fwd["composed"](0)
        row["composed_peak_extra_mb"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
        row["composed_over_fused"] = round(min(row["composed_event_ms"]) / min(row["fused_event_ms"]), 3)
        res["infer"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
