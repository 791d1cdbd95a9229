"""SVD and SVD++ at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs from
`bench_workloads.distinct_interactions`, shuffled; labels 1 / 0 alternating, `recent_num` = 30: a user's history is the
last 30 of their pairs in generation order), K = 16 and 64, batch 256 and 8,192, cross entropy, row-wise Adam.  Prints one
JSON line; per configuration: ms per step over `--steps` consecutive steps, host-timed around one synchronisation and as the
mean of a HIP-event pair around every step, the mean HIP-event time per launch of the three kernels of csrc/svd.hip (history pool, score, y gradient) from a pass of its own, the mean number of distinct users,
history entries and touched y rows per step, the time to move the bytes the step must move over 8 TB/s (named as that, not
as a bound the kernels are expected to meet: the tables are cache resident), and beside them the same step composed from
torch ops on the same GPU (`index_select` forward, for SVD++ `embedding_bag(mode="sum")` over the padded [B, 30] bags,
autograd, `index_add_` of the row gradients into gradient tables; no optimiser step, so it is a lower bound of what a
user would have without these kernels).

    python scripts/svd_bench.py [--ks 16,64] [--batches 256,8192] [--steps 100]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_workloads import HBM_PEAK_GBS, distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.algorithms.svd import SvdNet  # noqa: E402

N_USERS, N_ITEMS, NNZ, RECENT = 138_493, 26_744, 20_000_263, 30
KERNELS = ("lr_svdpp_pool_f32", "lr_mf_score_f32", "lr_svdpp_hist_grad_f32")


def histories(u, i):
    """CSR of the last RECENT items of every user, on the device."""
    order = torch.argsort(u, stable=True)
    us, it = u[order].long(), i[order]
    counts = torch.bincount(us, minlength=N_USERS)
    end = torch.cumsum(counts, 0)
    rank = torch.arange(us.numel(), device=u.device) - (end - counts)[us]
    keep = rank >= (counts[us] - RECENT)
    lens = counts.clamp(max=RECENT)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=u.device), torch.cumsum(lens, 0)])
    return ptr.contiguous(), it[keep].to(torch.int32).contiguous()


def timed(step, n_steps):
    """(host-timed ms per step around one synchronisation, mean HIP-event ms of a step) over `n_steps` consecutive steps.  The
    event pair of a step spans whatever the stream waits for inside it, host reads included."""
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
    return wall, sum(a.elapsed_time(b) for a, b in evs) / n_steps


def ours(model, K, B, n_steps, users, items, labels, hist, dev):
    net = SvdNet(N_USERS, N_ITEMS, K, 1e-3, 1e-5, None, False, False, 0, dev, "cross_entropy", with_history=model == "svdpp")
    if model == "svdpp":
        net.hist_ptr, net.hist_idx = hist
    step = lambda s: net.train_step(users[s * B:(s + 1) * B], items[s * B:(s + 1) * B], labels[s * B:(s + 1) * B])  # noqa: E731
    step(0)
    per, per_ev = timed(step, n_steps)
    ops.TIMER.enable(*KERNELS)
    for s in range(min(n_steps, 50)):
        step(s)
    torch.cuda.synchronize()
    mean = lambda xs: round(sum(xs) / len(xs), 2) if xs else None  # noqa: E731
    ev = {k: mean([x.elapsed_time(y) * 1e3 for x, y in v]) for k, v in ops.TIMER.events.items()}
    ops.TIMER.disable()
    # what a step touches, from the first ten steps
    nd = ent = touched = 0.0
    n_stat = min(n_steps, 10)
    for s in range(n_stat):
        du = torch.unique(users[s * B:(s + 1) * B].long())
        nd += du.numel() / n_stat
        if model == "svdpp":
            ptr, idx = hist
            lens = ptr[du + 1] - ptr[du]
            ent += float(lens.sum()) / n_stat
            pos = torch.repeat_interleave(ptr[du], lens) + (torch.arange(int(lens.sum()), device=dev)
                                                            - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens))
            touched += torch.unique(idx[pos]).numel() / n_stat
    entries_ms = None
    if model == "svdpp":      # the entry list of a step alone (torch index ops and the step's one host read)
        seg = net.adam.segments("user", users[:B].contiguous(), N_USERS, want_slots=True)
        net._entries(seg, B)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(n_steps):
            net._entries(seg, B)
        torch.cuda.synchronize()
        entries_ms = round((time.perf_counter() - t) * 1e3 / n_steps, 4)
    row = K * 4
    # score: two rows read, two gradient rows written per sample; row-wise Adam of p / q: gradient row read, (w, m, v) read and
    # written per distinct row (items counted as B: an upper bound); pool: entries + p read, z written; y side: G read per entry,
    # (w, m, v) read and written per touched row
    bytes_step = B * 4 * row + B * row * 2 + (nd + B) * 6 * row
    if model == "svdpp":
        bytes_step += (ent + 2 * nd) * row + ent * row + touched * 6 * row
    return {"model": model, "K": K, "batch": B, "steps_measured": n_steps, "wall_ms_per_step": round(per, 4),
            "event_ms_per_step": round(per_ev, 4), "entry_list_ms_per_step": entries_ms,
            "samples_per_s": round(B / (per * 1e-3), 1),
            "kernel_us_per_launch": {"pool": ev[KERNELS[0]], "score": ev[KERNELS[1]], "hist_grad": ev[KERNELS[2]]},
            "distinct_users": round(nd, 1), "history_entries": round(ent, 1), "touched_y_rows": round(touched, 1),
            "bytes_per_step": int(bytes_step), "us_to_move_those_bytes_at_8TBs": round(bytes_step / (HBM_PEAK_GBS * 1e9) * 1e6, 3)}


def torch_composed(model, K, B, n_steps, users, items, labels, hist, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    P, Q = (torch.randn((n, K), device=dev, generator=gen) * 0.05 for n in (N_USERS, N_ITEMS))
    bu, bi = torch.zeros(N_USERS, device=dev), torch.zeros(N_ITEMS, device=dev)
    grads = {"P": torch.zeros_like(P), "Q": torch.zeros_like(Q), "bu": torch.zeros_like(bu), "bi": torch.zeros_like(bi)}
    if model == "svdpp":
        Y = torch.cat([torch.randn((N_ITEMS, K), device=dev, generator=gen) * 0.05, torch.zeros((1, K), device=dev)]).requires_grad_(True)
        grads["Y"] = torch.zeros_like(Y)
        ptr, idx = hist
        lens = ptr[1:] - ptr[:-1]
        pad = torch.full((N_USERS, RECENT), N_ITEMS, dtype=torch.int64, device=dev)       # row N_ITEMS of Y is zero
        col = torch.arange(idx.numel(), device=dev) - torch.repeat_interleave(ptr[:-1], lens)
        pad[torch.repeat_interleave(torch.arange(N_USERS, device=dev), lens), col] = idx.long()
        scale = torch.where(lens > 0, lens.float().rsqrt(), torch.zeros_like(lens, dtype=torch.float32))

    def step(s):
        u, i = users[s * B:(s + 1) * B].long(), items[s * B:(s + 1) * B].long()
        y = labels[s * B:(s + 1) * B]
        pr, qr = P.index_select(0, u).requires_grad_(True), Q.index_select(0, i).requires_grad_(True)
        bur, bir = bu.index_select(0, u).requires_grad_(True), bi.index_select(0, i).requires_grad_(True)
        leaves = [pr, qr, bur, bir]
        x = pr
        if model == "svdpp":
            h = pad.index_select(0, u)                       # [B, 30] bags, padded with the zero row
            leaves.append(Y)
            x = pr + scale.index_select(0, u)[:, None] * F.embedding_bag(h, Y, mode="sum", padding_idx=N_ITEMS)
        loss = F.binary_cross_entropy_with_logits(bur + bir + (x * qr).sum(1), y)
        g = torch.autograd.grad(loss, leaves)
        grads["P"].index_add_(0, u, g[0])
        grads["Q"].index_add_(0, i, g[1])
        grads["bu"].index_add_(0, u, g[2])
        grads["bi"].index_add_(0, i, g[3])
        if model == "svdpp":
            grads["Y"].add_(g[4])                          # embedding_bag's backward already is the index_add_, into a dense table
        return loss

    step(0)
    wall, ev = timed(step, n_steps)
    return round(wall, 4), round(ev, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,64")
    ap.add_argument("--batches", default="256,8192")
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    u, i = distinct_interactions(NNZ, N_USERS, N_ITEMS, gen, dev)
    hist = histories(u, i)
    perm = torch.randperm(NNZ, generator=gen, device=dev)
    users, items = u[perm].to(torch.int32).contiguous(), i[perm].to(torch.int32).contiguous()
    labels = (torch.arange(NNZ, device=dev) % 2 == 0).float()
    items = torch.where(labels > 0, items, torch.roll(items, 1))          # label 0: some other sample's item
    res = {"bench": "svd", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, NNZ], "recent_num": RECENT,
           "longest_history": int((hist[0][1:] - hist[0][:-1]).max()), "rows": []}
    for model in ("svd", "svdpp"):
        for K in map(int, a.ks.split(",")):
            for B in map(int, a.batches.split(",")):
                row = ours(model, K, B, a.steps, users, items, labels, hist, dev)
                row["torch_composed_ms_per_step"], row["torch_composed_event_ms_per_step"] = torch_composed(
                    model, K, B, a.steps, users, items, labels, hist, dev)
                res["rows"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
