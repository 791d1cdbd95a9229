"""IVF-Flat index (`recommendation/ivf.py`, csrc/ivf.hip) against the exact scan (`ops.score_topk`) on a clustered catalogue.

The catalogue is a mixture of Gaussians with a fixed seed (`--components` centres drawn from N(0, I), rows = centre + `--sigma`
x N(0, I)); uniform random vectors have no list structure and would show only the worst case.  Queries come from the same
mixture.  For every N of `--sizes` (D = 128, nlist = round(4 sqrt(N))) the script reports

  build      `IVFFlatIndex.train_add` split into train (k-means on <= 256 nlist rows), assign (all rows) and permute (list build
             + row permutation), HIP events around each leg;
  search     for B in `--batches`, k = 100, nprobe in `--nprobes`: the time of `index.search` and of `ops.score_topk` on the same
             inputs, measured in ALTERNATING rounds in the same session (a host clock around work that ends in a device
             synchronise; best of `--reps` and all times kept), the device time of the index's C call alone (HIP events around
             `lr_ivf_search_f32`: its six launches without the wrapper), recall@k of the index against the exact ids, the rows the fine
             scan reads (sum over queries of the probed lists' lengths) and their bytes as a fraction of 8 TB/s over the search
             time.

Prints one JSON line; `--out` also writes it indented.

    python scripts/ivf_bench.py [--sizes 1000000,10000000] [--batches 1,64,1024] [--nprobes 1,8,32,128] [--reps 5] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_workloads import HBM_PEAK_GBS  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.recommendation.ivf import IVFFlatIndex  # noqa: E402

D, K = 128, 100


def ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def mixture(n, centres, sigma, gen, dev, chunk=1 << 20):
    out = torch.empty((n, D), dtype=torch.float32, device=dev)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        c = torch.randint(0, centres.shape[0], (b - a,), generator=gen, device=dev)
        out[a:b] = centres[c] + sigma * torch.randn((b - a, D), generator=gen, device=dev)
    return out


def probed_rows(index, queries, nprobe):
    """Rows the fine scan reads: per query the lengths of its nprobe best lists (the coarse step restated with torch)."""
    lens = (index.list_ptr[1:] - index.list_ptr[:-1]).to(torch.float64)
    total = 0.0
    for a in range(0, queries.shape[0], 256):
        top = (queries[a:a + 256] @ index.centroids.T).topk(nprobe, dim=1).indices
        total += float(lens[top].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--components", type=int, default=2048)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"bench": "ivf", "device": torch.cuda.get_device_name(dev), "d": D, "k": K, "components": a.components, "sigma": a.sigma,
           "niter": a.niter, "reps": a.reps, "exact_arith": ops.TOPK_ARITH, "sizes": {}}
    for N in (int(s) for s in a.sizes.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        centres = torch.randn((a.components, D), generator=gen, device=dev)
        rows = mixture(N, centres, a.sigma, gen, dev)
        nlist = int(round(4 * math.sqrt(N)))
        index, t_build = ms(lambda: IVFFlatIndex.train_add(rows, nlist, niter=a.niter, timings=True))
        lens = (index.list_ptr[1:] - index.list_ptr[:-1])
        leg = {"nlist": nlist, "n_train": min(N, 256 * nlist), "build_ms": {k: round(v, 1) for k, v in index.timings.items()},
               "build_total_ms": round(t_build, 1), "list_len": {"max": int(lens.max()), "mean": round(N / nlist, 1),
                                                                 "empty": int((lens == 0).sum())}, "search": []}
        for B in (int(s) for s in a.batches.split(",")):
            queries = mixture(B, centres, a.sigma, gen, dev)
            exact_ids = ops.score_topk(queries, rows, K)[1]
            for nprobe in (int(s) for s in a.nprobes.split(",")):
                if nprobe > nlist:
                    continue
                ids = index.search(queries, K, nprobe)[1]                      # warm-up of both shapes, and the recall
                hit = (ids.unsqueeze(2) == exact_ids.unsqueeze(1)).any(dim=2).sum().item()
                t_ivf, t_exact = [], []
                for _ in range(a.reps):                                        # alternating rounds
                    t_ivf.append(ms(lambda: index.search(queries, K, nprobe))[1])
                    t_exact.append(ms(lambda: ops.score_topk(queries, rows, K))[1])
                ops.TIMER.enable("lr_ivf_search_f32")                          # HIP events around the C call: its launches alone
                for _ in range(a.reps):
                    index.search(queries, K, nprobe)
                torch.cuda.synchronize()
                t_dev = min(x.elapsed_time(y) for x, y in ops.TIMER.events["lr_ivf_search_f32"])
                ops.TIMER.disable()
                scanned = probed_rows(index, queries, nprobe)
                leg["search"].append({
                    "B": B, "nprobe": nprobe, "nprobe_over_nlist": round(nprobe / nlist, 5), "recall_at_k": round(hit / (B * K), 4),
                    "ivf_ms": round(min(t_ivf), 4), "ivf_device_ms": round(t_dev, 4), "exact_ms": round(min(t_exact), 4),
                    "ivf_all_ms": [round(t, 4) for t in t_ivf],
                    "exact_all_ms": [round(t, 4) for t in t_exact], "exact_over_ivf": round(min(t_exact) / min(t_ivf), 2),
                    "scanned_rows": int(scanned), "scan_fraction_of_hbm_peak":
                        round(scanned * D * 4 / (min(t_ivf) * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)})
        res["sizes"][str(N)] = leg
        del rows, index
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
