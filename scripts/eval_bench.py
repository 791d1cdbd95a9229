"""`evaluate()` on the host (sklearn / numpy / Python sets) against `evaluate(on_device=True)` (csrc/eval_metrics.hip) at the
ML-20M shape: 138,493 users x 26,744 items, an eval set of `--positives` positives and as many sampled negatives.

The model is a stub: `predict` is a hash of (user, item) in float32 (about 1,000,003 distinct values: ties occur), and
`recommend_user` returns k ids per user from a hash as well.  Both paths call the same stub through the same batching, so the
difference between them is the metric computation and, on the device path, the upload of the predictions.

Legs, each timed in ALTERNATING rounds (host, device, host, device, ...) in one session, a host clock around a call that
ends in a device synchronise, every time kept and the best reported:

  point     roc_auc + pr_auc + log_loss
  gauc      roc_gauc (one sklearn call per user on the host: minutes per round, so `--gauc-rounds` host rounds only)
  list2048  precision / recall / map / ndcg / coverage at k = 10 for 2,048 sampled users
  listall   the same for every user of the eval set

and, with HIP events on the device path's own stages at the same size: the prediction upload, `ops.eval_keys`, `torch.sort`,
the label gather, `ops.eval_rank_stats` and `ops.eval_point_sums`, which gives the share of `torch.sort` in the device time of
the rank metrics.  The values of the two paths are compared too (max absolute difference per leg).

Prints one JSON line; `--out` also writes it indented.

    python scripts/eval_bench.py [--positives 2000000] [--rounds 3] [--gauc-rounds 1] [--skip-host-gauc] [--out f.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from librecommender_amd import ops  # noqa: E402
from librecommender_amd.data import TransformedEvalSet  # noqa: E402
from librecommender_amd.evaluation import evaluate  # noqa: E402

N_USERS, N_ITEMS, K = 138_493, 26_744, 10


class StubModel:
    task = "ranking"
    n_users, n_items = N_USERS, N_ITEMS
    eval_user_batch = 8192

    def __init__(self, dev):
        self.device = dev

    def predict(self, user, item, inner_id=True):
        h = (np.asarray(user, dtype=np.int64) * 2654435761 + np.asarray(item, dtype=np.int64) * 40503) % 1000003
        return (h / 1000003.0).astype(np.float32)

    def recommend_user(self, user, n_rec, **kw):
        u = np.asarray(user, dtype=np.int64)
        ids = (u[:, None] * 7919 + np.arange(n_rec)[None, :] * 104729) % N_ITEMS
        return {int(a): row for a, row in zip(u.tolist(), ids)}


def eval_set(n_pos, seed):
    rng = np.random.default_rng(seed)
    users = np.repeat(rng.integers(0, N_USERS, n_pos), 2)
    items = rng.integers(0, N_ITEMS, 2 * n_pos)
    labels = np.zeros(2 * n_pos, dtype=np.float32)
    labels[::2] = 1.0
    return TransformedEvalSet(users, items, labels)


def timed(fn):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return out, time.perf_counter() - t


def leg(model, data, metrics, rounds, sample_user_num=None, host_rounds=None):
    kw = dict(neg_sampling=False, metrics=metrics, k=K, sample_user_num=sample_user_num, seed=42)
    host_rounds = rounds if host_rounds is None else host_rounds
    host = host_rounds > 0
    times = {"host": [], "device": []}
    vals = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        evaluate(model, data, on_device=True, **kw)                 # warm-up: code objects, the cached uploads
        for r in range(rounds):
            if r < host_rounds:
                vals["host"], t = timed(lambda: evaluate(model, data, on_device=False, **kw))
                times["host"].append(t)
            vals["device"], t = timed(lambda: evaluate(model, data, on_device=True, **kw))
            times["device"].append(t)
    res = {"metrics": metrics, "device_s": times["device"], "device_best_s": min(times["device"]), "device_values": vals["device"]}
    if host:
        res.update(host_s=times["host"], host_best_s=min(times["host"]), host_values=vals["host"],
                   speedup=min(times["host"]) / min(times["device"]),
                   max_abs_diff=max(abs(vals["host"][m] - vals["device"][m]) for m in vals["host"]))
    else:
        res["host_s"] = "not measured"
    return res


def event_ms(fn, reps):
    out = None
    best = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b))
    return out, min(best)


def stages(model, data, dev, reps):
    """HIP-event times (ms, best of `reps`) of the device path's own stages."""
    from librecommender_amd.evaluation import device_metrics as D

    c = D._cache(data, dev)
    pred, t_pred = timed(lambda: D.predict_all(model, data, 8192, dev))
    out = {"rows": int(pred.numel()), "predict_and_upload_s": t_pred}
    for name, group in (("global", None), ("by_user", c["users"])):
        (key, _), t_keys = event_ms(lambda: ops.eval_keys(pred, group), reps)
        (skey, order), t_sort = event_ms(lambda: torch.sort(key), reps)
        lab, t_gather = event_ms(lambda: c["labels_u8"].index_select(0, order), reps)
        _, t_rank = event_ms(lambda: ops.eval_rank_stats(skey, lab), reps)
        total = t_keys + t_sort + t_gather + t_rank
        out[name] = {"keys_ms": t_keys, "sort_ms": t_sort, "gather_ms": t_gather, "rank_stats_ms": t_rank, "total_ms": total,
                     "sort_share": t_sort / total}
    _, out["point_sums_ms"] = event_ms(lambda: ops.eval_point_sums(pred, c["labels"]), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positives", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gauc-rounds", type=int, default=1, help="host rounds of the roc_gauc leg (minutes each)")
    ap.add_argument("--skip-host-gauc", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on an MI355X: no HIP device here")
    dev = torch.device("cuda:0")
    model = StubModel(dev)
    data, t_build = timed(lambda: eval_set(a.positives, 0))
    res = {"shape": {"users": N_USERS, "items": N_ITEMS, "rows": len(data), "eval_users": len(data.positive_consumed), "k": K},
           "eval_set_build_s": t_build}
    res["point"] = leg(model, data, ["roc_auc", "pr_auc", "log_loss"], a.rounds)
    print("point done", file=sys.stderr, flush=True)
    lists = ["precision", "recall", "map", "ndcg", "coverage"]
    res["list2048"] = leg(model, data, lists, a.rounds, sample_user_num=2048)
    res["listall"] = leg(model, data, lists, a.rounds)
    print("lists done", file=sys.stderr, flush=True)
    res["stages"] = stages(model, data, dev, a.reps)
    res["gauc"] = leg(model, data, ["roc_gauc"], a.rounds, host_rounds=0 if a.skip_host_gauc else a.gauc_rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
