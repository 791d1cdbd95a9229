"""RNN4Rec at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs from
`bench_workloads.distinct_interactions`; a user's history is their pairs in generation order, a sample's window the up to L
items before it, at least the one-step sequence [pad]), GRU and LSTM, one layer, embed_size 16, cross entropy with labels
1 / 0 alternating, row-wise Adam.  Prints one JSON line; per configuration (batch, L, units): ms per training step over
`--steps` consecutive steps (host-timed around one synchronisation, and the mean of a HIP-event pair around every step), the
mean HIP-event time per launch of the forward and the backward layer call of csrc/rnn.hip from a pass of its own, and beside
them the same step with the recurrent layer composed from torch ops, one cell per time step under autograd, on the same GPU
(`index_select` of the window rows, `torch.where` for the sequence mask, autograd, `index_add_` of the row gradients into
gradient tables; no optimiser step, so it is a lower bound of what a user would have without these kernels).

    python scripts/rnn_bench.py [--configs 512x10x16,8192x10x64,8192x50x64] [--cells gru,lstm] [--steps 50]
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
from librecommender_amd.nets.rnn_nets import RNN4RecNet  # noqa: E402

N_USERS, N_ITEMS, NNZ, K = 138_493, 26_744, 20_000_263, 16
KERNELS = ("lr_rnn_layer_fwd_f32", "lr_rnn_layer_bwd_f32")


def windows(u, i, n, L, gen):
    """n samples drawn from the pairs: (seqs int32 [n, L] left-aligned and padded with N_ITEMS, lens >= 1, items)."""
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
    return seqs.to(torch.int32).contiguous(), length.clamp(min=1).to(torch.int32).contiguous(), it[pick].to(torch.int32).contiguous()


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


def ours(cell, B, L, H, n_steps, seqs, lens, items, labels, dev):
    net = RNN4RecNet(N_ITEMS, K, (H,), cell, False, 0.0, False, L, 1e-3, 1e-5, 0, dev, False, "cross_entropy")
    sl = lambda x, s: x[s * B:(s + 1) * B]  # noqa: E731
    step = lambda s: net.train_step(sl(seqs, s), sl(lens, s), items=sl(items, s), labels=sl(labels, s))  # noqa: E731
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


def torch_composed(cell, B, L, H, n_steps, seqs, lens, items, labels, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    G = 3 if cell == "gru" else 4
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen) * 0.05  # noqa: E731
    S, Q, bi = rnd(N_ITEMS + 1, H), rnd(N_ITEMS, K), torch.zeros(N_ITEMS, device=dev)
    W, U, b = rnd(H, G * H).requires_grad_(True), rnd(H, G * H).requires_grad_(True), torch.zeros((2, G * H), device=dev, requires_grad=True)
    Wd, bd = rnd(H, K).requires_grad_(True), torch.zeros(K, device=dev, requires_grad=True)
    grads = {"S": torch.zeros_like(S), "Q": torch.zeros_like(Q), "bi": torch.zeros_like(bi)}
    sl = lambda x, s: x[s * B:(s + 1) * B]  # noqa: E731

    def step(s):
        ids, ln, it, y = sl(seqs, s).long(), sl(lens, s), sl(items, s).long(), sl(labels, s)
        x = S.index_select(0, ids.reshape(-1)).view(B, L, H).requires_grad_(True)
        qr, br = Q.index_select(0, it).requires_grad_(True), bi.index_select(0, it).requires_grad_(True)
        h = torch.zeros((B, H), device=dev)
        c = torch.zeros((B, H), device=dev)
        for t in range(L):
            v = (ln > t)[:, None]
            if cell == "gru":
                mx, mh = torch.addmm(b[0], x[:, t], W), torch.addmm(b[1], h, U)
                z, r = torch.sigmoid(mx[:, :H] + mh[:, :H]), torch.sigmoid(mx[:, H:2 * H] + mh[:, H:2 * H])
                hn = torch.lerp(torch.tanh(mx[:, 2 * H:] + r * mh[:, 2 * H:]), h, z)
            else:
                a = torch.addmm(b[0], x[:, t], W) + h @ U
                cn = torch.sigmoid(a[:, H:2 * H]) * c + torch.sigmoid(a[:, :H]) * torch.tanh(a[:, 2 * H:3 * H])
                hn = torch.sigmoid(a[:, 3 * H:]) * torch.tanh(cn)
                c = torch.where(v, cn, c)
            h = torch.where(v, hn, h)
        uvec = torch.addmm(bd, h, Wd)
        loss = F.binary_cross_entropy_with_logits((uvec * qr).sum(1) + br, y)
        g = torch.autograd.grad(loss, [x, qr, br, W, U, b, Wd, bd])
        grads["S"].index_add_(0, ids.reshape(-1), g[0].reshape(-1, H))
        grads["Q"].index_add_(0, it, g[1])
        grads["bi"].index_add_(0, it, g[2])
        return loss

    for s in range(3):
        step(s)
    return timed(step, n_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="512x10x16,8192x10x64,8192x50x64")
    ap.add_argument("--cells", default="gru,lstm")
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    u, i = distinct_interactions(NNZ, N_USERS, N_ITEMS, gen, dev)
    res = {"bench": "rnn4rec", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, NNZ], "embed_size": K,
           "steps_measured": a.steps, "rows": []}
    for cfg in a.configs.split(","):
        B, L, H = map(int, cfg.split("x"))
        seqs, lens, items = windows(u, i, B * a.steps, L, gen)
        labels = (torch.arange(B * a.steps, device=dev) % 2 == 0).float()
        items = torch.where(labels > 0, items, torch.roll(items, 1))      # label 0: some other sample's item
        for cell in a.cells.split(","):
            wall, ev, k_us = ours(cell, B, L, H, a.steps, seqs, lens, items, labels, dev)
            t_wall, t_ev = torch_composed(cell, B, L, H, a.steps, seqs, lens, items, labels, dev)
            res["rows"].append({"cell": cell, "batch": B, "L": L, "units": H, "mean_len": round(float(lens.float().mean()), 2),
                                "wall_ms_per_step": round(wall, 4), "event_ms_per_step": round(ev, 4),
                                "samples_per_s": round(B / (wall * 1e-3), 1),
                                "kernel_us_per_launch": {"layer_fwd": k_us[KERNELS[0]], "layer_bwd": k_us[KERNELS[1]]},
                                "torch_composed_ms_per_step": round(t_wall, 4),
                                "torch_composed_event_ms_per_step": round(t_ev, 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
