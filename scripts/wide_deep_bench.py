"""Wide & Deep's FTRL wide-row update (csrc/ftrl.hip) against the same update composed from torch ops, and the whole training
step with either.  Writes `<out>/wide_deep.json` and `<out>/wide_deep.md` and prints the JSON.

(a) the kernel: one stream of B x F' positions (batch 256 and 8,192; 8 and 39 fields), field 0 two-valued (two runs of about
    B / 2 positions: the long-run path), the other fields Zipf ids over 1,000 rows each.  Three variants, timed in alternating
    rounds with a HIP-event pair around `--reps` back-to-back calls per round, median and range over the rounds:
      rows       `ops.ftrl_rows` on segments that exist already (in the net the deep update builds them anyway);
      seg+rows   `SegmentBuilder.build` + `ops.ftrl_rows`: what a caller without segments pays;
      torch      `torch.unique(return_inverse)` + `index_add_` + the elementwise update + three indexed stores.
    Before timing, the variants are compared on the same inputs.
(b) the step: `WideDeepNet` at the MovieLens-20M id shape (138,493 users x 26,744 items) with six sparse columns (one
    two-valued, five Zipf over 1,000 rows) = 8 fields, embed 16, hidden (128, 64, 32), against the same net whose wide table
    update is the torch composition; and the share of a step spent in the wide forward (`lin` gather + Dense(1)).

    python scripts/wide_deep_bench.py [--out profiles] [--rounds 7] [--reps 50]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd import ops  # noqa: E402
from librecommender_amd.nets import FeatSpec, WideDeepNet  # noqa: E402

N_USERS, N_ITEMS = 138_493, 26_744
FIELD_ROWS, LR, L1 = 1000, 0.01, 1e-3


def zipf_ids(n, rows, gen, dev):
    """ids in [0, rows) with P(r) ~ 1 / (r + 1)."""
    w = 1.0 / torch.arange(1, rows + 1, device=dev, dtype=torch.float64)
    return torch.multinomial(w, n, replacement=True, generator=gen).to(torch.int32)


def stream(B, F, gen, dev):
    cols = [torch.randint(0, 2, (B,), device=dev, generator=gen, dtype=torch.int32)]
    cols += [2 + (f - 1) * FIELD_ROWS + zipf_ids(B, FIELD_ROWS, gen, dev) for f in range(1, F)]
    return torch.stack(cols, dim=1).reshape(-1).contiguous(), 2 + (F - 1) * FIELD_ROWS


def torch_ftrl_rows(var, accum, linear, grad, ids, lr=LR, l1=L1):
    rows, inv = torch.unique(ids.long(), return_inverse=True)
    g = torch.zeros(rows.numel(), device=var.device).index_add_(0, inv, grad)
    w, a, z = var[rows], accum[rows], linear[rows]
    na = a + g * g
    sna = na.sqrt()
    z = z + g - (sna - a.sqrt()) / lr * w
    var[rows] = torch.where(z.abs() > l1, (torch.sign(z) * l1 - z) / (sna / lr), torch.zeros_like(z))
    accum[rows] = na
    linear[rows] = z


def event_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(variants, rounds, reps):
    """{name: fn} -> {name: (median us, min, max)} over `rounds` alternating rounds."""
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(event_us(fn, reps))
    return {k: (round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)) for k, v in t.items()}


def kernel_rows(rounds, reps, dev):
    out = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    for B in (256, 8192):
        for F in (8, 39):
            ids, V = stream(B, F, gen, dev)
            n = ids.numel()
            grad = torch.randn(n, device=dev, generator=gen) * 0.1
            mk = lambda: (torch.rand(V, device=dev, generator=gen) - 0.5, torch.full((V,), 0.1, device=dev), torch.zeros(V, device=dev))  # noqa: E731
            builder = ops.SegmentBuilder(n, V, dev)
            seg = builder.build(ids)
            # same inputs, both variants, before any timing
            a, b = mk(), None
            b = tuple(x.clone() for x in a)
            ops.ftrl_rows(*a, grad, seg, LR, L1)
            torch_ftrl_rows(*b, grad, ids)
            diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
            s = mk()
            runs = torch.bincount(ids.long(), minlength=V)
            res = alternate({"rows": lambda: ops.ftrl_rows(*s, grad, seg, LR, L1),
                             "seg+rows": lambda: ops.ftrl_rows(*s, grad, builder.build(ids), LR, L1),
                             "torch": lambda: torch_ftrl_rows(*s, grad, ids)}, rounds, reps)
            out.append({"batch": B, "fields": F, "positions": n, "distinct_rows": int((runs > 0).sum()),
                        "longest_run": int(runs.max()), "runs_over_32": int((runs > ops.FTRL_LONG_RUN).sum()),
                        "max_abs_diff_vs_torch": diff, "us_per_call_median_min_max": res,
                        "torch_over_rows": round(res["torch"][0] / res["rows"][0], 2),
                        "torch_over_seg_rows": round(res["torch"][0] / res["seg+rows"][0], 2)})
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


class ComposedWideNet(WideDeepNet):
    """The same net with the wide table updated by the torch composition."""

    def _wide_rows(self, seg, gl):
        t = self.tables
        ids = torch.cat([self._last_ctx.idx_plain.reshape(-1)] + [fi.reshape(-1) for fi in self._last_ctx.pooled_idx])
        torch_ftrl_rows(t.lin.view(-1), t.lin_m.view(-1), t.lin_v.view(-1), gl.view(-1), ids, self.lr["wide"])


def step_rows(rounds, reps, dev):
    out = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    n_cols = 6
    spec = FeatSpec(N_USERS, N_ITEMS, n_cols, 2 + (n_cols - 1) * FIELD_ROWS)
    for B in (256, 8192):
        users = torch.multinomial(1.0 / torch.arange(1, N_USERS + 1, device=dev, dtype=torch.float64), B, True, generator=gen).to(torch.int32)
        items = zipf_ids(B, N_ITEMS, gen, dev)
        sparse = stream(B, n_cols, gen, dev)[0].view(B, n_cols)
        labels = (torch.arange(B, device=dev) % 2).float()
        nets = {}
        for name, cls in (("kernel", WideDeepNet), ("torch", ComposedWideNet)):
            net = cls(spec, 16, (128, 64, 32), True, None, {"wide": LR, "deep": 1e-3}, 1e-5, 0, dev)
            if name == "torch":          # the composed update needs the step's ids: keep the context of the last forward
                fwd = net.emb.forward
                def keep(*a, _net=net, _fwd=fwd, **kw):
                    r = _fwd(*a, **kw)
                    _net._last_ctx = r[0]
                    return r
                net.emb.forward = keep
            nets[name] = net
        res = alternate({k: (lambda n_=n_: n_.train_step(users, items, labels, sparse=sparse)) for k, n_ in nets.items()},
                        rounds, max(5, reps // 5))
        t, net = nets["kernel"].tables, nets["kernel"]
        idx = torch.cat([users.view(-1, 1) + t.user_off, items.view(-1, 1) + t.item_off, sparse + t.sparse_off], dim=1).contiguous()
        with torch.no_grad():
            wide_fwd = alternate({"wide_fwd": lambda: net.wide_term(ops.embed_gather(t.lin, idx).view(idx.shape))}, rounds, reps)
        out.append({"batch": B, "fields": spec.n_fields, "us_per_step_median_min_max": res,
                    "torch_over_kernel": round(res["torch"][0] / res["kernel"][0], 3),
                    "wide_forward_us_median_min_max": wide_fwd["wide_fwd"],
                    "wide_forward_share_of_step": round(wide_fwd["wide_fwd"][0] / res["kernel"][0], 4)})
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def markdown(res):
    L = ["# Wide & Deep: FTRL wide-row update and training step", "",
         f"Measured on {res['device']} by `scripts/wide_deep_bench.py` ({res['rounds']} alternating rounds, HIP events; median",
         "[min, max] over the rounds).  Everything below is measured; nothing here is extrapolated.", "",
         "## (a) `ops.ftrl_rows` against torch ops (`unique` + `index_add_` + elementwise), us per call", "",
         "| batch | fields | positions | distinct rows | longest run | rows | seg + rows | torch | torch / rows | torch / (seg + rows) |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    fmt = lambda t: f"{t[0]} [{t[1]}, {t[2]}]"  # noqa: E731
    for r in res["kernel"]:
        u = r["us_per_call_median_min_max"]
        L.append(f"| {r['batch']} | {r['fields']} | {r['positions']} | {r['distinct_rows']} | {r['longest_run']} | {fmt(u['rows'])} | "
                 f"{fmt(u['seg+rows'])} | {fmt(u['torch'])} | {r['torch_over_rows']} | {r['torch_over_seg_rows']} |")
    L += ["", "`rows`: segments exist already (the deep update of the step builds them); `seg + rows`: the segment build is paid too.",
          "Largest |difference| between the two variants' results on the same inputs (absolute, on `linear` values that reach a few "
          "hundred where a run sums thousands of gradients): "
          f"{max(r['max_abs_diff_vs_torch'] for r in res['kernel']):.2e}.", "",
          "## (b) the whole step, 8 fields at the MovieLens-20M id shape, us per step", "",
          "| batch | kernel | wide update from torch ops | torch / kernel | wide forward (`lin` gather + Dense(1)) | its share of the step |",
          "|---|---|---|---|---|---|"]
    for r in res["step"]:
        u = r["us_per_step_median_min_max"]
        L.append(f"| {r['batch']} | {fmt(u['kernel'])} | {fmt(u['torch'])} | {r['torch_over_kernel']} | "
                 f"{fmt(r['wide_forward_us_median_min_max'])} | {100 * r['wide_forward_share_of_step']:.1f} % |")
    L += ["", "Open candidate, not built: a fused wide-term forward that gathers `lin`, multiplies by the `wide_term` kernel and writes",
          "[B] in one launch; the last two columns are what it could remove at most.  Merging the long-run finish into the chunk",
          "kernel (one launch less) is the other one.", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"bench": "wide_deep", "device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "reps": a.reps,
           "kernel": kernel_rows(a.rounds, a.reps, dev), "step": step_rows(a.rounds, a.reps, dev)}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "wide_deep.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(a.out, "wide_deep.md"), "w") as f:
        f.write(markdown(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
