"""WaveNet at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs from
`bench_workloads.distinct_interactions`; a user's history is their pairs in generation order, a sample's window the up to L
items before it, padded with the pad id), one block of four dilated layers, embed_size 16, cross entropy with labels 1 / 0
alternating, row-wise Adam.  Prints one JSON line; per configuration (batch, L, filters): ms per training step over `--steps`
consecutive steps (host-timed around one synchronisation, and the mean of a HIP-event pair around every step), the mean
HIP-event time of the forward and the backward call of csrc/wavenet.hip from a pass of its own, and beside them the same
step with the user side composed from torch ops under autograd on the same GPU (`index_select` of the window rows, `F.pad` +
`F.conv1d` + `relu` per layer, `max`, autograd, `index_add_` of the row gradients into gradient tables; no optimiser step, so
it is a lower bound of what a user would have without these kernels).

    python scripts/wavenet_bench.py [--configs 512x10x16,...] [--steps 50]
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

from bench_workloads import distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.nets.wavenet_net import WaveNetNet  # noqa: E402

N_USERS, N_ITEMS, NNZ, K = 138_493, 26_744, 20_000_263, 16
N_BLOCKS, N_PER_BLOCK = 1, 4
KERNELS = ("lr_wavenet_fwd_f32", "lr_wavenet_bwd_f32")
CONFIGS = "512x10x16,512x10x64,512x50x16,512x50x64,8192x10x16,8192x10x64,8192x50x16,8192x50x64"


def windows(u, i, n, L, gen):
    """n samples drawn from the pairs: (users, seqs int32 [n, L] left-aligned and padded with N_ITEMS, items, mean length)."""
    dev = u.device
    order = torch.argsort(u, stable=True)
    us, it = u[order].long(), i[order].long()
    counts = torch.bincount(us, minlength=N_USERS)
    start = torch.cumsum(counts, 0) - counts
    pick = torch.randint(0, us.numel(), (n,), device=dev, generator=gen)
    pos = pick - start[us[pick]]                                  # the sample's position in its user's history
    length = pos.clamp(max=L)
    t = torch.arange(L, device=dev)[None, :]
    src = (pick - length)[:, None] + t
    valid = t < length[:, None]
    seqs = torch.where(valid, it[src.clamp(max=us.numel() - 1)], torch.full_like(src, N_ITEMS))
    return (us[pick].to(torch.int32).contiguous(), seqs.to(torch.int32).contiguous(), it[pick].to(torch.int32).contiguous(),
            float(length.float().mean()))


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
    return wall, sum(a.elapsed_time(b) for a, b in evs) / n_steps


def ours(B, L, nF, n_steps, users, seqs, items, labels, dev):
    net = WaveNetNet(N_USERS, N_ITEMS, K, nF, N_BLOCKS, N_PER_BLOCK, False, L, 1e-3, 1e-5, 0, dev, False, "cross_entropy")
    sl = lambda x, s: x[s * B:(s + 1) * B]  # noqa: E731
    step = lambda s: net.train_step(sl(users, s), sl(seqs, s), sl(items, s), sl(labels, s))  # noqa: E731
    for s in range(3):
        step(s)
    wall, ev = timed(step, n_steps)
    ops.TIMER.enable(*KERNELS)
    for s in range(min(n_steps, 20)):
        step(s)
    torch.cuda.synchronize()
    mean = lambda xs: round(sum(xs) / len(xs), 2) if xs else None  # noqa: E731
    k_us = {k: mean([x.elapsed_time(y) * 1e3 for x, y in v]) for k, v in ops.TIMER.events.items()}
    ops.TIMER.disable()
    return wall, ev, k_us


def torch_composed(B, L, nF, n_steps, users, seqs, items, labels, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen) * 0.05  # noqa: E731
    Uv, S, Q, bi = rnd(N_USERS + 1, K), rnd(N_ITEMS + 1, K), rnd(N_ITEMS, 2 * K), torch.zeros(N_ITEMS, device=dev)
    n = N_BLOCKS * N_PER_BLOCK
    # torch's conv1d layout [F, C, k]
    Ws = [rnd(nF, K if j == 0 else nF, 2).requires_grad_(True) for j in range(n)] + [rnd(nF, nF, 1).requires_grad_(True)]
    bs = [torch.zeros(nF, device=dev, requires_grad=True) for _ in range(n + 1)]
    Wd, bd = rnd(nF, K).requires_grad_(True), torch.zeros(K, device=dev, requires_grad=True)
    grads = {"U": torch.zeros_like(Uv), "S": torch.zeros_like(S), "Q": torch.zeros_like(Q), "bi": torch.zeros_like(bi)}
    sl = lambda x, s: x[s * B:(s + 1) * B]  # noqa: E731

    def step(s):
        us, ids, it, y = sl(users, s).long(), sl(seqs, s).long(), sl(items, s).long(), sl(labels, s)
        x = S.index_select(0, ids.reshape(-1)).view(B, L, K).requires_grad_(True)
        ur = Uv.index_select(0, us).requires_grad_(True)
        qr, br = Q.index_select(0, it).requires_grad_(True), bi.index_select(0, it).requires_grad_(True)
        a = x.transpose(1, 2)
        for j in range(n):
            d = 2 ** (j % N_PER_BLOCK)
            a = torch.relu(F.conv1d(F.pad(a, (d, 0)), Ws[j], bs[j], dilation=d))
        a = torch.relu(F.conv1d(a, Ws[n], bs[n]))
        uvec = torch.cat([ur, torch.addmm(bd, a.max(dim=2).values, Wd)], dim=1)
        loss = F.binary_cross_entropy_with_logits((uvec * qr).sum(1) + br, y)
        g = torch.autograd.grad(loss, [x, ur, qr, br, Wd, bd, *Ws, *bs])
        grads["S"].index_add_(0, ids.reshape(-1), g[0].reshape(-1, K))
        grads["U"].index_add_(0, us, g[1])
        grads["Q"].index_add_(0, it, g[2])
        grads["bi"].index_add_(0, it, g[3])
        return loss

    for s in range(3):
        step(s)
    return timed(step, n_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=CONFIGS)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    u, i = distinct_interactions(NNZ, N_USERS, N_ITEMS, gen, dev)
    res = {"bench": "wavenet", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, NNZ], "embed_size": K,
           "n_blocks": N_BLOCKS, "n_layers_per_block": N_PER_BLOCK, "steps_measured": a.steps, "rows": []}
    for cfg in a.configs.split(","):
        B, L, nF = map(int, cfg.split("x"))
        users, seqs, items, mean_len = windows(u, i, B * a.steps, L, gen)
        labels = (torch.arange(B * a.steps, device=dev) % 2 == 0).float()
        items = torch.where(labels > 0, items, torch.roll(items, 1))      # label 0: some other sample's item
        wall, ev, k_us = ours(B, L, nF, a.steps, users, seqs, items, labels, dev)
        t_wall, t_ev = torch_composed(B, L, nF, a.steps, users, seqs, items, labels, dev)
        res["rows"].append({"batch": B, "L": L, "filters": nF, "mean_len": round(mean_len, 2),
                            "wall_ms_per_step": round(wall, 4), "event_ms_per_step": round(ev, 4),
                            "samples_per_s": round(B / (wall * 1e-3), 1),
                            "kernel_us_per_call": {"fwd": k_us[KERNELS[0]], "bwd": k_us[KERNELS[1]]},
                            "torch_composed_ms_per_step": round(t_wall, 4),
                            "torch_composed_event_ms_per_step": round(t_ev, 4)})
        print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
