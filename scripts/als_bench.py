"""ALS half-sweeps at the scale of BASELINE cfg 5's interaction matrix: 10 M users x 10 M items, 200 M distinct Zipf(1.05)
pairs (`bench_workloads.distinct_interactions`), K = 64, implicit (confidence alpha r + 1 with r = 1), CG (3 steps) and the
direct solver.  Prints one JSON line: ms per half-sweep and per epoch (HIP events, after warm-up), each kernel's time (the
sweep's stages launched one at a time), the algorithmic bytes nnz (4 + 4 + 4K) + the row reads and writes of X against
8 TB/s, the Gram flops of the workgroup paths (medium + heavy rows, 2 deg K^2 per row) against the f32 MFMA peak, and the
plan-build time.

    python scripts/als_bench.py [--users N] [--items N] [--nnz N] [--K 64] [--epochs 2] [--warmup 1] [--solvers cg,direct]
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

from bench_workloads import HBM_PEAK_GBS, MFMA_F32_PEAK_TF, distinct_interactions  # noqa: E402
from librecommender_amd import ops  # noqa: E402


def csr(rows_of, cols_of, n_rows, dev):
    order = torch.argsort(rows_of.to(torch.int64) * (int(cols_of.max()) + 1) + cols_of)
    col = cols_of[order].to(torch.int32).contiguous()
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(rows_of.to(torch.int64), minlength=n_rows), 0)
    return rowptr, col


def timed(fn, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=10_000_000)
    ap.add_argument("--items", type=int, default=10_000_000)
    ap.add_argument("--nnz", type=int, default=200_000_000)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--solvers", default="cg,direct")
    ap.add_argument("--alpha", type=float, default=10.0)
    ap.add_argument("--reg", type=float, default=0.1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = args.K
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    eu, ei = distinct_interactions(args.nnz, args.users, args.items, gen, dev)
    val = torch.full((args.nnz,), 1.0 * args.alpha + 1.0, dtype=torch.float32, device=dev)   # implicit, r = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u_rp, u_col = csr(eu, ei, args.users, dev)
    i_rp, i_col = csr(ei, eu, args.items, dev)
    torch.cuda.synchronize()
    t_csr = (time.perf_counter() - t0) * 1e3
    del eu, ei
    t0 = time.perf_counter()
    u_plan, i_plan = ops.als_plan(u_rp, K), ops.als_plan(i_rp, K)
    torch.cuda.synchronize()
    t_plan = (time.perf_counter() - t0) * 1e3
    X = torch.randn((args.users, K), generator=gen, device=dev) * 0.03
    Y = torch.randn((args.items, K), generator=gen, device=dev) * 0.03
    sides = {"user": ((u_rp, u_col, val), u_plan, X, Y), "item": ((i_rp, i_col, val), i_plan, Y, X)}

    def side_stats(rp, plan):
        deg = rp[1:] - rp[:-1]
        light = deg <= plan.light_cap
        heavy = deg > plan.heavy_deg
        wg = deg[~light].to(torch.float64)
        return {"rows": plan.rows, "light_rows": plan.n_light, "medium_rows": plan.n_medium, "heavy_rows": plan.n_heavy,
                "heavy_chunks": plan.n_chunks, "nnz_light": int(deg[light].sum()), "nnz_heavy": int(deg[heavy].sum()),
                "max_degree": int(deg.max()), "wg_gram_flop": float((2.0 * wg * K * K).sum())}

    stats = {s: side_stats(v[0][0], v[1]) for s, v in sides.items()}
    out = {"workload": "als_cfg5", "users": args.users, "items": args.items, "nnz": args.nnz, "K": K,
           "alpha": args.alpha, "reg": args.reg, "csr_build_ms": round(t_csr, 1), "plan_build_ms": round(t_plan, 1),
           "plan": stats, "solvers": {}}
    for solver in args.solvers.split(","):
        use_cg = solver == "cg"
        res = {}

        def sweep(side, mask=15):
            c, plan, A, B = sides[side]
            G0 = ops.als_gram(B, args.reg, True)
            ops.als_half_sweep(*c, A, B, G0, True, use_cg, plan, 3, stage_mask=mask)

        for _ in range(args.warmup):
            sweep("user")
            sweep("item")
        torch.cuda.synchronize()
        hs = {s: timed(lambda s=s: sweep(s), args.epochs) for s in ("user", "item")}
        ep = timed(lambda: (sweep("user"), sweep("item")), args.epochs)
        kern = {}
        for s in ("user", "item"):
            c, plan, A, B = sides[s]
            kern[f"{s}.gram"] = timed(lambda B=B: ops.als_gram(B, args.reg, True))
            G0 = ops.als_gram(B, args.reg, True)
            for name, mask in (("light", 1), ("medium", 2), ("heavy_slabs", 4), ("heavy_solve", 8)):
                if mask == 8 and plan.n_heavy:
                    ops.als_half_sweep(*c, A, B, G0, True, use_cg, plan, 3, stage_mask=4)
                kern[f"{s}.{name}"] = timed(lambda c=c, plan=plan, A=A, B=B, G0=G0, mask=mask:
                                            ops.als_half_sweep(*c, A, B, G0, True, use_cg, plan, 3, stage_mask=mask))
        for s in ("user", "item"):
            st = stats[s]
            nbytes = args.nnz * (4 + 4 + 4 * K) + 2 * st["rows"] * K * 4
            res[f"{s}_half_sweep_ms"] = round(hs[s], 3)
            res[f"{s}_bytes_GB"] = round(nbytes / 1e9, 2)
            res[f"{s}_hbm_fraction"] = round(nbytes / (hs[s] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
            gram_ms = kern[f"{s}.medium"] + kern[f"{s}.heavy_slabs"] + (kern[f"{s}.light"] if not use_cg else 0.0)
            flop = st["wg_gram_flop"] + (2.0 * st["nnz_light"] * K * K if not use_cg else 0.0)
            res[f"{s}_wg_gram_TFLOP"] = round(flop / 1e12, 3)
            res[f"{s}_wg_gram_fraction_of_f32_mfma_peak"] = round(flop / max(gram_ms, 1e-9) / 1e9 / MFMA_F32_PEAK_TF, 4)
        res["epoch_ms"] = round(ep, 3)
        res["kernels_ms"] = {k: round(v, 3) for k, v in kern.items()}
        out["solvers"][solver] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
