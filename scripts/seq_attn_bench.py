"""The sequence-attention kernels (csrc/seq_attn.hip) against the torch compositions they replace.

(a) the op alone: forward + backward of `ops.seq_attn` against the composition under autograd (the core of
    `seq_nets.multi_head_attention` with its [B, L, L] mask built beforehand, outside the timed region; for the pooling form
    `feat_nets.dot_attention_torch`), B = 512 and 8,192, L = 10 and 50, (heads, head width) = (1, 32), (2, 32), (1, 80), and
    the pooling form (one query, the keys are the values, width 32) at L = 10 and 50.  Lengths are uniform in 1 .. L.
(b) the whole step: `FeatTransformerNet` and `FeatSIMNet` at the MovieLens-20M id shape (138,493 users x 26,744 items, uniform
    ids, no side features) with the reference's defaults (Transformer: embed 16, window 10, one layer, one head; SIM: embed 16,
    long window 100, short window 10, top-k 10, two heads), `fused_attention=True` against `fused_attention=False` of the same
    net.

The two paths are timed in `--rounds` alternating rounds of `--steps` consecutive calls (HIP events around every call), so the
spread between rounds stands next to the difference between the paths.  The kernel columns are HIP-event times per call of
`lr_seq_attn_fwd_f32` and `lr_seq_attn_bwd_f32` (one launch each) from a pass of their own.  Prints one JSON line.

    python scripts/seq_attn_bench.py [--batches 512,8192] [--steps 50] [--rounds 3] [--step-batch 8192]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd import ops  # noqa: E402
from librecommender_amd.nets import FeatSpec  # noqa: E402
from librecommender_amd.nets.feat_nets import dot_attention_torch  # noqa: E402
from librecommender_amd.nets.seq_nets import FeatSIMNet, FeatTransformerNet  # noqa: E402

N_USERS, N_ITEMS = 138_493, 26_744
KERNELS = ("lr_seq_attn_fwd_f32", "lr_seq_attn_bwd_f32")
HEAD_SHAPES = ((1, 32), (2, 32), (1, 80))


def timed(step, n_steps):
    torch.cuda.synchronize()
    evs = []
    for s in range(n_steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(s)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    return round(sum(a.elapsed_time(b) for a, b in evs) / n_steps, 4)


def composed_core(q, k, v, H, mask):
    """The core of `seq_nets.multi_head_attention` (its lines between the projections)."""
    B, Tq, M = q.shape
    Tk, hd = k.shape[1], M // H
    qh, kh, vh = (x.view(B, x.shape[1], H, hd).transpose(1, 2) for x in (q, k, v))
    s = (qh * (1.0 / math.sqrt(hd))) @ kh.transpose(2, 3)
    s = s - 1e9 * (~mask[:, None, :, :]).to(s.dtype)
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, Tq, M)


def alternate(steps, rounds, n_steps, row):
    for step in steps.values():
        for s in range(5):
            step(s)
    for k in steps:
        row[f"{k}_event_ms"] = []
    for _ in range(rounds):
        for k, step in steps.items():
            row[f"{k}_event_ms"].append(timed(step, n_steps))
    ops.TIMER.enable(*KERNELS)
    for s in range(min(n_steps, 20)):
        steps["fused"](s)
    torch.cuda.synchronize()
    row["kernel_us_per_call"] = {k[12:15]: round(sum(x.elapsed_time(y) for x, y in v) * 1e3 / len(v), 2)
                                 for k, v in ops.TIMER.events.items() if v}
    row["kernel_calls_per_step"] = {k[12:15]: len(v) // min(n_steps, 20) for k, v in ops.TIMER.events.items() if v}
    ops.TIMER.disable()
    row["composed_over_fused"] = round(min(row["composed_event_ms"]) / min(row["fused_event_ms"]), 3)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def op_row(B, L, H, hd, pooled, dev, gen, a):
    M, Tq = H * hd, 1 if pooled else L
    q = torch.randn((B, Tq, M), device=dev, generator=gen).requires_grad_(True)
    k = torch.randn((B, L, M), device=dev, generator=gen).requires_grad_(True)
    v = k if pooled else torch.randn((B, L, M), device=dev, generator=gen).requires_grad_(True)
    gout = torch.randn((B, Tq, M), device=dev, generator=gen)
    lens = torch.randint(1, L + 1, (B,), device=dev, generator=gen, dtype=torch.int32)
    mask = (torch.arange(L, device=dev)[None, :] < lens[:, None])[:, None, :].expand(-1, Tq, -1)
    scale = 1.0 if pooled else 1.0 / math.sqrt(hd)

    def run(f):
        def step(_):
            q.grad = k.grad = v.grad = None
            f().backward(gout)
        return step

    if pooled:
        composed = lambda: dot_attention_torch(q[:, 0], k, lens)[:, None, :]
    else:
        composed = lambda: composed_core(q, k, v, H, mask)
    steps = {"fused": run(lambda: ops.seq_attn(q, k, v, H, scale, lens=lens)), "composed": run(composed)}
    # what the kernels must move at the least: q, k, v, out once forward; q, k, v, gout, gq, gk, gv once backward
    n_q, n_k = B * Tq * M * 4, B * L * M * 4
    row = {"batch": B, "L": L, "heads": H, "head_dim": hd, "pooled": pooled,
           "min_bytes": {"fwd": 2 * n_q + (1 if pooled else 2) * n_k, "bwd": 3 * n_q + (3 if pooled else 4) * n_k}}
    return alternate(steps, a.rounds, a.steps, row)


def step_row(kind, B, dev, gen, a):
    spec = FeatSpec(N_USERS, N_ITEMS, 0, 0, 0)
    if kind == "transformer":
        n_seq = 10
        make = lambda fused: FeatTransformerNet(spec, 16, (128, 64, 32), max_seq_len=10, num_heads=1, num_tfm_layers=1, lr=1e-3,
                                                device=dev, fused_attention=fused)
    else:
        n_seq = 110
        make = lambda fused: FeatSIMNet(spec, 16, (200, 80), search_topk=10, long_max_len=100, short_max_len=10, num_heads=2,
                                        lr=1e-3, device=dev, fused_attention=fused)
    n = a.steps
    users = torch.randint(0, N_USERS, (n, B), device=dev, generator=gen, dtype=torch.int32)
    items = torch.randint(0, N_ITEMS, (n, B), device=dev, generator=gen, dtype=torch.int32)
    seqs = torch.randint(0, N_ITEMS, (n, B, n_seq), device=dev, generator=gen, dtype=torch.int32)
    if kind == "transformer":
        lens = torch.randint(1, 11, (n, B), device=dev, generator=gen, dtype=torch.int32)
        seqs = torch.where(torch.arange(10, device=dev)[None, None, :] < lens[:, :, None], seqs, N_ITEMS)
    else:
        lens = torch.stack([torch.randint(1, 101, (n, B), device=dev, generator=gen, dtype=torch.int32),
                            torch.randint(1, 11, (n, B), device=dev, generator=gen, dtype=torch.int32)], dim=2)
        pos = torch.arange(110, device=dev)[None, None, :]
        valid = torch.where(pos < 100, pos < lens[:, :, :1], pos - 100 < lens[:, :, 1:])
        seqs = torch.where(valid, seqs, N_ITEMS)
    labels = (torch.arange(B, device=dev) % 2 == 0).float()
    nets = {"fused": make(True), "composed": make(False)}
    steps = {k: (lambda s, net=net: net.train_step(users[s], items[s], labels, seqs=seqs[s], seq_lens=lens[s]))
             for k, net in nets.items()}
    return alternate(steps, a.rounds, n, {"model": kind, "batch": B})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="512,8192")
    ap.add_argument("--step-batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    res = {"bench": "seq_attn", "device": torch.cuda.get_device_name(dev), "steps_per_round": a.steps, "rounds": a.rounds,
           "op": [], "step": []}
    for B in map(int, filter(None, a.batches.split(","))):
        for L in (10, 50):
            for H, hd in HEAD_SHAPES:
                res["op"].append(op_row(B, L, H, hd, False, dev, gen, a))
            res["op"].append(op_row(B, L, 1, 32, True, dev, gen, a))
    if a.step_batch > 0:
        for kind in ("transformer", "sim"):
            res["step"].append(step_row(kind, a.step_batch, dev, gen, a))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
