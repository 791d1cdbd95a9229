"""IVF-SQ8 index (`recommendation/ivf_sq8.py`, csrc/ivf_sq8.hip) against the IVF-Flat index and the exact scan
(`ops.score_topk`), on the clustered catalogues of `scripts/ivf_bench.py` (same mixture, same seed, D = 128, k = 100,
nlist = round(4 sqrt(N))).

For every N of `--sizes` the script reports

  build      `IVFSQ8Index.train_add` and `IVFFlatIndex.train_add`, each split into its legs (HIP events), and the device bytes
             of both indexes (SQ8: codes, scales, ids, ptr, centroids; Flat: the same with f32 list rows in place of codes and
             scales); the two indexes' centroids and lists are checked to be equal;
  search     for B in `--batches`, nprobe in `--nprobes`, refine in `--refines`: the time of `IVFSQ8Index.search`, of
             `IVFFlatIndex.search` and of `ops.score_topk` on the same inputs, in ALTERNATING rounds in the same session (a host
             clock around work that ends in a device synchronise; best of `--reps`, all times kept), the device time of
             `lr_ivf_sq8_search_f32` alone (HIP events), recall@k of each against the exact ids, the probed rows, and the
             roofline of the scan: bytes of probed codes (rows x code stride) over 8 TB/s, as a time and as a fraction of the
             SQ8 search time.

Prints one JSON line; `--out` also writes it indented.

    python scripts/ivf_sq8_bench.py [--sizes 1000000,10000000] [--batches 1,64,1024] [--nprobes 1,8,32,128] [--refines 0,1,4]
                                    [--reps 5] [--out f.json]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_workloads import HBM_PEAK_GBS  # noqa: E402
from ivf_bench import D, K, mixture, ms, probed_rows  # noqa: E402
from librecommender_amd import ops  # noqa: E402
from librecommender_amd.recommendation.ivf import IVFFlatIndex  # noqa: E402
from librecommender_amd.recommendation.ivf_sq8 import IVFSQ8Index  # noqa: E402


def recall(ids, exact_ids):
    return round((ids.unsqueeze(2) == exact_ids.unsqueeze(1)).any(dim=2).sum().item() / exact_ids.numel(), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--batches", default="1,64,1024")
    ap.add_argument("--nprobes", default="1,8,32,128")
    ap.add_argument("--refines", default="0,1,4")
    ap.add_argument("--components", type=int, default=2048)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    refines = [int(s) for s in a.refines.split(",")]
    res = {"bench": "ivf_sq8", "device": torch.cuda.get_device_name(dev), "d": D, "k": K, "components": a.components,
           "sigma": a.sigma, "niter": a.niter, "reps": a.reps, "exact_arith": ops.TOPK_ARITH, "sizes": {}}
    for N in (int(s) for s in a.sizes.split(",")):
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        centres = torch.randn((a.components, D), generator=gen, device=dev)
        rows = mixture(N, centres, a.sigma, gen, dev)
        nlist = int(round(4 * math.sqrt(N)))
        sq8, t_sq8 = ms(lambda: IVFSQ8Index.train_add(rows, nlist, niter=a.niter, timings=True))
        flat, t_flat = ms(lambda: IVFFlatIndex.train_add(rows, nlist, niter=a.niter, timings=True))
        same_lists = bool(torch.equal(sq8.centroids, flat.centroids) and torch.equal(sq8.list_ptr, flat.list_ptr)
                          and torch.equal(sq8.list_ids, flat.list_ids))
        flat_bytes = sum(t.numel() * t.element_size() for t in (flat.list_rows, flat.list_ids, flat.list_ptr, flat.centroids))
        stride = sq8.codes.shape[1]
        leg = {"nlist": nlist, "same_centroids_and_lists": same_lists,
               "sq8_build_ms": {k: round(v, 1) for k, v in sq8.timings.items()}, "sq8_build_total_ms": round(t_sq8, 1),
               "flat_build_ms": {k: round(v, 1) for k, v in flat.timings.items()}, "flat_build_total_ms": round(t_flat, 1),
               "sq8_bytes": sq8.nbytes, "flat_bytes": flat_bytes, "table_bytes": rows.numel() * 4, "code_stride": stride, "search": []}
        for B in (int(s) for s in a.batches.split(",")):
            queries = mixture(B, centres, a.sigma, gen, dev)
            exact_ids = ops.score_topk(queries, rows, K)[1]
            for nprobe in (int(s) for s in a.nprobes.split(",")):
                if nprobe > nlist:
                    continue
                rec = {"B": B, "nprobe": nprobe, "flat_recall": recall(flat.search(queries, K, nprobe)[1], exact_ids)}
                rec["sq8_recall"] = {str(r): recall(sq8.search(queries, K, nprobe, refine=r)[1], exact_ids) for r in refines}   # + warm-up
                t = {"flat": [], "exact": [], **{f"sq8_r{r}": [] for r in refines}}
                for _ in range(a.reps):                                        # alternating rounds
                    for r in refines:
                        t[f"sq8_r{r}"].append(ms(lambda: sq8.search(queries, K, nprobe, refine=r))[1])
                    t["flat"].append(ms(lambda: flat.search(queries, K, nprobe))[1])
                    t["exact"].append(ms(lambda: ops.score_topk(queries, rows, K))[1])
                rec["ms"] = {k: round(min(v), 4) for k, v in t.items()}
                rec["all_ms"] = {k: [round(x, 4) for x in v] for k, v in t.items()}
                dev_ms = {}
                for r in refines:                                              # HIP events around the stage-1 C call alone
                    ops.TIMER.enable("lr_ivf_sq8_search_f32")
                    for _ in range(a.reps):
                        sq8.search(queries, K, nprobe, refine=r)
                    torch.cuda.synchronize()
                    dev_ms[str(r)] = round(min(x.elapsed_time(y) for x, y in ops.TIMER.events["lr_ivf_sq8_search_f32"]), 4)
                    ops.TIMER.disable()
                rec["sq8_stage1_device_ms"] = dev_ms
                scanned = probed_rows(flat, queries, nprobe)
                roof_ms = scanned * stride / (HBM_PEAK_GBS * 1e9) * 1e3
                rec.update({"scanned_rows": int(scanned), "code_bytes": int(scanned * stride), "roofline_ms": round(roof_ms, 5),
                            "roofline_over_sq8": {str(r): round(roof_ms / rec["ms"][f"sq8_r{r}"], 4) for r in refines}})
                leg["search"].append(rec)
                print(f"N={N} B={B} nprobe={nprobe}: {rec['ms']}", file=sys.stderr, flush=True)
        res["sizes"][str(N)] = leg
        del rows, sq8, flat
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
