"""Caser at the MovieLens-20M shape (138,493 users x 26,744 items, 20,000,263 distinct Zipf pairs from
`bench_workloads.distinct_interactions`; a user's history is their pairs in generation order, a sample's window the up to L
items before it, padded with the pad id), cross entropy with labels 1 / 0 alternating, row-wise Adam.  Prints one JSON line;
per configuration (batch x L x embed_size x nh x nv): ms per training step over `--steps` consecutive steps (host-timed around
one synchronisation, and the mean of a HIP-event pair around every step), the mean HIP-event time of the forward and the
backward call of csrc/caser.hip from a pass of its own, and beside them, at the same parameter shapes on the same GPU, the user
side composed from torch ops under autograd (`index_select` of the window rows, L + 1 `F.conv1d` + `relu`, L `amax`, autograd,
`index_add_` of the row gradients into gradient tables): its forward + backward alone, to set against the two kernels, and the
whole step without an optimiser step, a lower bound of what a user would have without these kernels.  The wide shape is in
the default list at batch 256 only: at 8192x50x64x16x8 the composed side did not finish 13 steps within five minutes on the
MI355X it was tried on (150 convolution shapes new to MIOpen), so that configuration is measured on request only; the fused side is timed
first and printed to stderr as soon as it is known.

    python scripts/caser_bench.py [--configs 256x10x16x2x4,...] [--steps 50]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_workloads import distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.nets.caser_net import CaserNet  # noqa: E402
from wavenet_bench import N_ITEMS, N_USERS, NNZ, timed, windows  # noqa: E402

KERNELS = ("lr_caser_fwd_f32", "lr_caser_bwd_f32")
CONFIGS = "256x10x16x2x4,8192x10x16x2x4,256x50x64x16x8"


def ours(B, L, K, nh, nv, n_steps, users, seqs, items, labels, dev):
    net = CaserNet(N_USERS, N_ITEMS, K, nh, nv, False, L, 1e-3, 1e-5, 0, dev, False, "cross_entropy")
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


def torch_composed(B, L, K, nh, nv, n_steps, users, seqs, items, labels, dev):
    """-> ((wall, event) ms of the whole step, (wall, event) ms of the convolutions' forward + backward alone)."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen) * 0.05  # noqa: E731
    Uv, S, Q, bi = rnd(N_USERS + 1, K), rnd(N_ITEMS + 1, K), rnd(N_ITEMS, 2 * K), torch.zeros(N_ITEMS, device=dev)
    # torch's conv1d layout [F, C, k]
    Ws = [rnd(nh, K, i).requires_grad_(True) for i in range(1, L + 1)] + [rnd(nv, L, 1).requires_grad_(True)]
    bs = [torch.zeros(nh, device=dev, requires_grad=True) for _ in range(L)] + [torch.zeros(nv, device=dev, requires_grad=True)]
    width = L * nh + K * nv
    Wd, bd = rnd(width, K).requires_grad_(True), torch.zeros(K, device=dev, requires_grad=True)
    grads = {"U": torch.zeros_like(Uv), "S": torch.zeros_like(S), "Q": torch.zeros_like(Q), "bi": torch.zeros_like(bi)}
    gfeat = rnd(B, width)
    sl = lambda x, s: x[s * B:(s + 1) * B]  # noqa: E731

    def features(x):
        xt = x.transpose(1, 2)
        out = [torch.relu(F.conv1d(xt, Ws[i], bs[i])).amax(dim=2) for i in range(L)]
        out.append(torch.relu(F.conv1d(x, Ws[L], bs[L])).transpose(1, 2).reshape(B, -1))
        return torch.cat(out, dim=1)

    def convs(s):
        ids = sl(seqs, s).long()
        x = S.index_select(0, ids.reshape(-1)).view(B, L, K).requires_grad_(True)
        return torch.autograd.grad(features(x), [x, *Ws, *bs], gfeat)

    def step(s):
        us, ids, it, y = sl(users, s).long(), sl(seqs, s).long(), sl(items, s).long(), sl(labels, s)
        x = S.index_select(0, ids.reshape(-1)).view(B, L, K).requires_grad_(True)
        ur = Uv.index_select(0, us).requires_grad_(True)
        qr, br = Q.index_select(0, it).requires_grad_(True), bi.index_select(0, it).requires_grad_(True)
        uvec = torch.cat([ur, torch.relu(torch.addmm(bd, features(x), Wd))], dim=1)
        loss = F.binary_cross_entropy_with_logits((uvec * qr).sum(1) + br, y)
        g = torch.autograd.grad(loss, [x, ur, qr, br, Wd, bd, *Ws, *bs])
        grads["S"].index_add_(0, ids.reshape(-1), g[0].reshape(-1, K))
        grads["U"].index_add_(0, us, g[1])
        grads["Q"].index_add_(0, it, g[2])
        grads["bi"].index_add_(0, it, g[3])
        return loss

    for s in range(3):
        step(s)
        convs(s)
    return timed(step, n_steps), timed(convs, n_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=CONFIGS)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    t0 = time.perf_counter()
    u, i = distinct_interactions(NNZ, N_USERS, N_ITEMS, gen, dev)
    torch.cuda.synchronize()
    print(f"pairs drawn in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    res = {"bench": "caser", "device": torch.cuda.get_device_name(dev), "shape": [N_USERS, N_ITEMS, NNZ], "steps_measured": a.steps,
           "rows": []}
    for cfg in a.configs.split(","):
        B, L, K, nh, nv = map(int, cfg.split("x"))
        users, seqs, items, mean_len = windows(u, i, B * a.steps, L, gen)
        labels = (torch.arange(B * a.steps, device=dev) % 2 == 0).float()
        items = torch.where(labels > 0, items, torch.roll(items, 1))      # label 0: some other sample's item
        wall, ev, k_us = ours(B, L, K, nh, nv, a.steps, users, seqs, items, labels, dev)
        print(f"{cfg}: fused {wall:.3f} ms per step, kernels {k_us}", file=sys.stderr, flush=True)
        (t_wall, t_ev), (c_wall, c_ev) = torch_composed(B, L, K, nh, nv, a.steps, users, seqs, items, labels, dev)
        res["rows"].append({"batch": B, "L": L, "embed_size": K, "nh": nh, "nv": nv, "mean_len": round(mean_len, 2),
                            "wall_ms_per_step": round(wall, 4), "event_ms_per_step": round(ev, 4),
                            "samples_per_s": round(B / (wall * 1e-3), 1),
                            "kernel_us_per_call": {"fwd": k_us[KERNELS[0]], "bwd": k_us[KERNELS[1]]},
                            "torch_composed_ms_per_step": round(t_wall, 4),
                            "torch_composed_event_ms_per_step": round(t_ev, 4),
                            "torch_composed_convs_fwd_bwd_ms": round(c_wall, 4),
                            "torch_composed_convs_fwd_bwd_event_ms": round(c_ev, 4)})
        print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
