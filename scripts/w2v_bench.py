"""Item2Vec's training epoch on the device (csrc/word2vec.hip) at the MovieLens-1M and MovieLens-20M shapes, and the same window
composed from torch ops (gathers, `index_add_`), which is what a user could write without the kernels.  No gensim number
exists here (gensim is no dependency of this package), so none is claimed.

Data: synthetic consumed lists with the shapes' user, item and interaction counts, item popularity ~ 1 / rank, list lengths
equal.  embed_size 16, window_size 5, 5 negatives.  Per shape and window (`batch_size`, in pairs):
  * `pairs_ms`: keep flags, compaction, count / scan / emit of the epoch's pair list, one call;
  * `targets_ms`: the targets of the first chunk of up to 2^20 pairs;
  * `window_ms`: the mean over `--windows` consecutive windows of score + two segment builds + two ordered updates, in
    `--rounds` rounds (a HIP-event pair around each round), fused and composed alternating, from the same tables;
  * `kernel_us`: HIP-event time per call of the window's entry points, from a pass of their own;
  * `epoch_s_estimated` = pairs + targets per chunk + windows x window_ms, and `epoch_s_measured` where the whole epoch was run
    (`--full-epoch-below` pairs / window count), with pairs per second from it.
Prints one JSON line.

    python scripts/w2v_bench.py [--shapes ml1m,ml20m] [--windows 200] [--rounds 3] [--batch-sizes 256,4096]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd import ops  # noqa: E402
from librecommender_amd.algorithms import Item2Vec  # noqa: E402

SHAPES = {"ml1m": (6040, 3706, 1_000_209), "ml20m": (138_493, 26_744, 20_000_263)}
KERNELS = ("lr_w2v_score_f32", "lr_segments_build", "lr_w2v_out_update_f32")
D = 16


class Info:
    """The least a model needs of a `DataInfo` when the corpus is given as consumed lists."""
    global_mean, min_max_rating = 0.0, (0, 1)

    def __init__(self, n_users, n_items, n_inter, seed=0):
        rng = np.random.default_rng(seed)
        p = 1.0 / np.arange(1, n_items + 1)
        items = rng.choice(n_items, size=n_inter, p=p / p.sum()).astype(np.int32)
        cuts = np.linspace(0, n_inter, n_users + 1).astype(np.int64)
        self.n_users, self.n_items = n_users, n_items
        self.user_consumed = {u: items[cuts[u]:cuts[u + 1]] for u in range(n_users)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composed_window(syn0, syn1, ins, centre, rows, labels, pair_of, pos0, inv_total):
    """The window of DESIGN §7.9 from torch ops, negatives only (six slots per pair; `rows` / `labels` are the window's
    slices, `pair_of` the pair of every slot).  `index_add_` adds with float atomics: the same sums in no fixed order."""
    W = ins.numel()
    slot_in = ins.long()[pair_of]
    r = rows.long()
    live = (r >= 0) & (slot_in >= 0) & (slot_in < syn0.shape[0])
    rc, ic = r.clamp(min=0), slot_in.clamp(0, syn0.shape[0] - 1)
    v, w = syn0[ic], syn1[rc]
    f = (v * w).sum(1)
    progress = (pos0 + centre.double()) * inv_total
    alpha = torch.clamp(0.025 - (0.025 - 1e-4) * progress, min=1e-4).float()[pair_of]
    g = (labels.float() - torch.sigmoid(f)) * alpha
    g = torch.where(live & (f.abs() < 6), g, torch.zeros_like(g))
    stash = torch.zeros((W, syn0.shape[1]), device=ins.device).index_add_(0, pair_of, g[:, None] * w)
    syn1.index_add_(0, rc, g[:, None] * v)
    syn0.index_add_(0, ins.long().clamp(0, syn0.shape[0] - 1), stash)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,ml20m")
    ap.add_argument("--batch-sizes", default="256,4096")
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--full-epoch-below", type=int, default=20_000, help="run the whole epoch when it has fewer windows")
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"bench": "word2vec", "device": torch.cuda.get_device_name(dev), "embed_size": D, "window_size": 5, "rows": []}
    for shape in a.shapes.split(","):
        nu, ni, nt = SHAPES[shape]
        info = Info(nu, ni, nt)
        for W in map(int, a.batch_sizes.split(",")):
            m = Item2Vec("ranking", info, embed_size=D, n_epochs=5, batch_size=W, seed=1)
            m.build_model()
            W = m.window_pairs()
            ins, pred, centre = m.epoch_pairs(1)                    # warm-up of the corpus path
            torch.cuda.synchronize()
            t = time.perf_counter()
            ins, pred, centre = m.epoch_pairs(1)
            torch.cuda.synchronize()
            pairs_ms = (time.perf_counter() - t) * 1e3
            n = ins.numel()
            c1 = min(n, max(W, (1 << 20) // W * W))
            tg = {}
            targets_ms = event_ms(lambda: tg.update(ops.w2v_targets(ins[:c1], pred[:c1], m._cum, m.seed, 1)))
            n_win = min(a.windows, c1 // W)
            pos0, inv_total = 0.0, 1.0 / (m.n_epochs * m.total_words)
            bufs = {"g": torch.empty(tg["rows"].numel(), dtype=torch.float32, device=dev),
                    "stash": torch.empty((W, D), dtype=torch.float32, device=dev),
                    "seg_out": ops.SegmentBuilder(6 * W, ni, dev), "seg_in": ops.SegmentBuilder(W, ni, dev)}
            start = (m.syn0.clone(), m.syn1.clone())
            pair_of = torch.arange(W, device=dev).repeat_interleave(6)

            def fused():
                for k in range(n_win):
                    m.engine_window(ins, centre, tg, 6 * W * k, 6 * W * (k + 1), W * k, W * (k + 1), pos0, inv_total, bufs, False)

            def composed():
                for k in range(n_win):
                    s, t6 = slice(W * k, W * (k + 1)), slice(6 * W * k, 6 * W * (k + 1))
                    composed_window(m.syn0, m.syn1, ins[s], centre[s], tg["rows"][t6], tg["labels"][t6], pair_of, pos0, inv_total)

            row = {"shape": shape, "users": nu, "items": ni, "tokens": nt, "batch_size": W, "pairs": n, "windows_per_epoch": -(-n // W),
                   "timed_windows": n_win, "pairs_ms": round(pairs_ms, 2), "targets_ms": round(targets_ms, 3),
                   "fused_window_ms": [], "composed_window_ms": []}
            for name, fn in (("fused", fused), ("composed", composed)):      # warm-up
                fn()
            for _ in range(a.rounds):
                for name, fn in (("fused", fused), ("composed", composed)):
                    m.syn0.copy_(start[0])
                    m.syn1.copy_(start[1])
                    row[f"{name}_window_ms"].append(round(event_ms(fn) / n_win, 4))
            ops.TIMER.enable(*KERNELS)
            fused()
            torch.cuda.synchronize()
            row["kernel_us"] = {k: [len(v), round(sum(x.elapsed_time(y) for x, y in v) * 1e3 / max(len(v), 1), 2)]
                                for k, v in ops.TIMER.events.items()}
            ops.TIMER.disable()
            n_chunks = -(-n // max(c1, 1))
            row["epoch_s_estimated"] = round((pairs_ms + n_chunks * targets_ms + row["windows_per_epoch"] * min(row["fused_window_ms"])) / 1e3, 3)
            row["composed_over_fused"] = round(min(row["composed_window_ms"]) / min(row["fused_window_ms"]), 2)
            if row["windows_per_epoch"] < a.full_epoch_below:
                m.syn0.copy_(start[0])
                m.syn1.copy_(start[1])
                torch.cuda.synchronize()
                t = time.perf_counter()
                m.engine_epoch(1)
                torch.cuda.synchronize()
                row["epoch_s_measured"] = round(time.perf_counter() - t, 3)
                row["pairs_per_s_measured"] = round(n / row["epoch_s_measured"])
            row["pairs_per_s_estimated"] = round(n / row["epoch_s_estimated"])
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
