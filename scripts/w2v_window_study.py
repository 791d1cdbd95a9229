"""How large may the word2vec window (`batch_size`, in pairs) be?  Runs the CPU oracle (tests/w2v_oracle.py, f64) on the
planted-cluster case and on a Zipf-head case at windows 1, 4, 16, ... and several seeds, and prints the final mean loss per
pair of every run, the run-to-run spread of window 1 and the largest window of the list inside it.  No device needed.

    python scripts/w2v_window_study.py [--seeds 3] [--json out.json]

The results this project's default was chosen from are recorded in profiles/word2vec.md."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import w2v_oracle as O  # noqa: E402

WINDOWS = (1, 4, 16, 64, 256, 1024, 4096, 16384)


def zipf_lists(n_users, n_items, list_len, seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_items + 1)
    p /= p.sum()
    return [[int(x) for x in rng.choice(n_items, size=list_len, replace=False, p=p)] for _ in range(n_users)]


def run_case(name, lists, n_items, D, window_size, n_epochs, hs, seeds, windows):
    tokens, sptr = O.flatten_sentences(lists)
    out = {}
    for W in windows:
        vals = []
        for seed in seeds:
            t0 = time.perf_counter()
            _, _, losses = O.train(lambda p: (tokens, sptr), n_items, D, window_size, n_epochs, seed, W, hs=hs)
            vals.append(losses[-1])
            print(f"{name} hs={int(hs)} W={W} seed={seed} final_loss={losses[-1]:.5f} first_loss={losses[0]:.5f} "
                  f"({time.perf_counter() - t0:.1f}s)", flush=True)
        out[W] = vals
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--windows", default=",".join(map(str, WINDOWS)))
    a = ap.parse_args()
    seeds = list(range(1, a.seeds + 1))
    windows = [int(w) for w in a.windows.split(",")]
    cases = {}
    lists, _ = O.planted_clusters(200, 4, 10, 10, 0)
    cases["planted_40_items"] = (lists, 40, 16, 5, 40)
    cases["zipf_500_items"] = (zipf_lists(2000, 500, 10, 0), 500, 16, 5, 10)
    res = {}
    for name, (lists, n_items, D, ws, ne) in cases.items():
        for hs in (False, True):
            r = run_case(name, lists, n_items, D, ws, ne, hs, seeds, windows)
            base = r[windows[0]]
            spread = max(base) - min(base)
            ok = [W for W in windows if abs(np.mean(r[W]) - np.mean(base)) <= spread]
            largest = windows[0]
            for W in windows:          # the largest window such that every smaller one is inside the spread too
                if W in ok:
                    largest = W
                else:
                    break
            print(f"== {name} hs={int(hs)}: window-1 mean {np.mean(base):.5f} spread {spread:.5f}; means "
                  + ", ".join(f"W={W}: {np.mean(r[W]):.5f}" for W in windows) + f"; largest inside the spread: {largest}",
                  flush=True)
            res[f"{name}_hs{int(hs)}"] = {"n_items": n_items, "losses": {str(W): v for W, v in r.items()}, "spread_w1": spread,
                                          "largest_inside": largest}
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
