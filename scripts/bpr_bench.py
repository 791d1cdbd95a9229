"""BPR at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs from
`bench_workloads.distinct_interactions`, shuffled): the engine (`use_tf=False`) for each optimiser at windows 256, 8,192 and
65,536 and the mini-batch mode at batch 8,192, for K = 16 and 64.  Prints one JSON line; per configuration: wall ms per
window over `--windows` consecutive windows and what that makes per epoch (ms, samples / s), the mean time of every kernel
launch of a window from HIP events in a pass of its own (triple score, the two segment builds, the two ordered updates),
the mean and the largest longest-chain length of the measured windows, and — named as what it is, not as a bound the
kernels are expected to meet — the time to move the bytes the algorithm must move over 8 TB/s: per sample three rows read
for the score, three rows and their optimiser state read and written for the update.  The tables are 9 MB (K = 16) to
43 MB (K = 64) and cache resident; the honest bounds are the longest chain and the launch count.  Negatives come from the
device sampler's "random" rule (not the positive): the consumed CSR plays no part in what is timed.

    python scripts/bpr_bench.py [--ks 16,64] [--windows 200] [--opts sgd,momentum,adam] [--sizes 256,8192,65536]
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
from librecommender_amd.algorithms import BPR  # noqa: E402
from librecommender_amd.algorithms.bpr import N_STATES, BprNet  # noqa: E402

N_USERS, N_ITEMS, NNZ = 138_493, 26_744, 20_000_263
KERNELS = ("lr_bpr_triple_score_f32", "lr_segments_build", "lr_bpr_row_update_f32")


class _Info:
    user_consumed, global_mean, min_max_rating = {}, 0.0, (0, 1)
    n_users, n_items = N_USERS, N_ITEMS


def engine(K, opt, W, n_win, users, pos, neg, dev):
    m = BPR("ranking", _Info(), embed_size=K, lr=0.01, batch_size=W, use_tf=False, optimizer=opt)
    m.build_model()
    m._state = m._new_state()
    n = min(users.numel(), W * n_win)
    u, p, q = users[:n], pos[:n], neg[:n]
    m.engine_epoch(u[: 2 * W], p[: 2 * W], q[: 2 * W], 1)          # warm-up
    torch.cuda.synchronize()
    t = time.perf_counter()
    m.engine_epoch(u, p, q, 1)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    windows = -(-n // W)
    ops.TIMER.enable(*KERNELS)
    m.engine_epoch(u[: W * min(windows, 50)], p[: W * min(windows, 50)], q[: W * min(windows, 50)], 1)
    torch.cuda.synchronize()
    ev = {k: [x.elapsed_time(y) * 1e3 for x, y in v] for k, v in ops.TIMER.events.items()}
    ops.TIMER.disable()
    mean = lambda xs: round(sum(xs) / max(len(xs), 1), 2)  # noqa: E731
    # per window the launches alternate: item segments, user segments; item update, user update
    per_launch = {"triple_score": mean(ev[KERNELS[0]]), "segments_items": mean(ev[KERNELS[1]][0::2]),
                  "segments_users": mean(ev[KERNELS[1]][1::2]), "update_items": mean(ev[KERNELS[2]][0::2]),
                  "update_users": mean(ev[KERNELS[2]][1::2])}
    items2 = torch.stack([p, q], 1).reshape(-1)
    chains = [int(torch.bincount(items2[2 * a:2 * (a + W)].long()).max()) for a in range(0, n, W)]
    epoch_windows = -(-NNZ // W)
    D = K + 1
    bytes_per_sample = 3 * D * 4 + 3 * D * 4 * 2 * (1 + N_STATES[opt])
    per_win = wall / windows
    return {"K": K, "optimizer": opt, "window": W, "windows_measured": windows, "wall_ms_per_window": round(per_win, 4),
            "epoch_ms": round(per_win * epoch_windows, 1), "samples_per_s": round(W / (per_win * 1e-3), 1),
            "kernel_us_per_launch": per_launch, "longest_item_chain_mean": round(sum(chains) / len(chains), 1),
            "longest_item_chain_max": max(chains), "bytes_per_sample": bytes_per_sample,
            "epoch_ms_to_move_those_bytes_at_8TBs": round(NNZ * bytes_per_sample / (HBM_PEAK_GBS * 1e9) * 1e3, 3)}


def minibatch(K, B, n_steps, users, pos, neg, dev):
    net = BprNet(N_USERS, N_ITEMS, K, 1e-3, 1e-5, None, False, False, 0, dev)
    step = lambda s: net.train_step(users[s * B:(s + 1) * B], pos[s * B:(s + 1) * B], neg[s * B:(s + 1) * B])  # noqa: E731
    step(0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for s in range(n_steps):
        step(s)
    torch.cuda.synchronize()
    per = (time.perf_counter() - t) * 1e3 / n_steps
    bytes_per_sample = 3 * K * 4 + 3 * K * 4 * 2 * 3
    return {"K": K, "batch": B, "steps_measured": n_steps, "wall_ms_per_step": round(per, 4),
            "epoch_ms": round(per * -(-NNZ // B), 1), "samples_per_s": round(B / (per * 1e-3), 1),
            "bytes_per_sample": bytes_per_sample,
            "epoch_ms_to_move_those_bytes_at_8TBs": round(NNZ * bytes_per_sample / (HBM_PEAK_GBS * 1e9) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--opts", default="sgd,momentum,adam")
    ap.add_argument("--sizes", default="256,8192,65536")
    ap.add_argument("--windows", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    u, i = distinct_interactions(NNZ, N_USERS, N_ITEMS, gen, dev)
    perm = torch.randperm(NNZ, generator=gen, device=dev)
    users, pos = u[perm].contiguous(), i[perm].contiguous()
    neg = ops.sample_negatives(pos, 1, N_ITEMS, 1)
    res = {"bench": "bpr", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, NNZ], "engine": [], "minibatch": []}
    for K in map(int, a.ks.split(",")):
        for opt in a.opts.split(","):
            for W in map(int, a.sizes.split(",")):
                res["engine"].append(engine(K, opt, W, a.windows, users, pos, neg, dev))
        res["minibatch"].append(minibatch(K, 8192, a.windows, users, pos, neg, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
