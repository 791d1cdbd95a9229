"""numpy / Python-int restatements of what csrc/eval_metrics.hip computes (include/libreco_hip.h, "Evaluation metrics").

Counts are int64 / Python ints and exact; everything else is fp64.  tests/test_eval_cpu.py checks these functions against
sklearn and the host functions of `librecommender_amd.evaluation.metrics`; tests/test_eval_gpu.py checks the kernels against
them.  The summation ORDER of the fp64 sums is numpy's, not the kernels': the two agree within the bounds below, not bit
for bit.

Bounds (derived, not tuned):
* `RANK_ATOL(n)` = n * 2^-52: ROC AUC, GAUC and PR AUC are sums of at most n fp64 terms bounded by 1 in total, each with a
  few roundings of its own; any order of summation stays within n * 2^-53 of the exact sum, and so do two of them apart.
* `LIST_RTOL(k)` = 4 k 2^-53: AP and NDCG are sums of at most k positive terms (relative error of any order at most
  (k - 1) 2^-53 each side), with one division per term and one at the end.
* `point_rtol(n)` = (n + 8) 2^-52 relative to the sum of the terms' magnitudes: an fp64 sum of n terms in any order
  ((n - 1) 2^-53 each side) whose terms carry up to two roundings, or one logarithm good to an ulp or two, on each side."""
import numpy as np

EPS32 = 2.0 ** -23


def RANK_ATOL(n):
    return n * 2.0 ** -52


def LIST_RTOL(k):
    return 4 * k * 2.0 ** -53


def point_rtol(n):
    return (n + 8) * 2.0 ** -52


# ---- sort keys ------------------------------------------------------------------------------------------------------------
def float_image(score):
    """uint32: ascending as unsigned exactly where the floats ascend; -0.0 is +0.0 first; subnormals keep their place."""
    u = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u >> 31).astype(bool)
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def keys(score, group=None):
    """(int64 keys, number of NaN scores)."""
    score = np.asarray(score, dtype=np.float32)
    g = np.zeros(len(score), np.uint64) if group is None else np.asarray(group).astype(np.uint32).astype(np.uint64)
    key = ((g << np.uint64(32)) | float_image(score).astype(np.uint64)).view(np.int64)
    return key, int(np.isnan(score).sum())


def sort_by_key(key, label):
    order = np.argsort(key, kind="stable")
    return key[order], (np.asarray(label)[order] != 0).astype(np.uint8)


# ---- rank statistics over the sorted order -----------------------------------------------------------------------------------
def _starts(changed):
    return np.flatnonzero(np.r_[True, changed])


def rank_stats(key_sorted, label_sorted):
    """(num2, P, Nneg) as Python ints, gauc and pr_auc as floats, from keys sorted ascending and their 0/1 labels."""
    key = np.asarray(key_sorted, dtype=np.int64)
    pos = (np.asarray(label_sorted) != 0).astype(np.int64)
    n = len(key)
    run_start = _starts(key[1:] != key[:-1])
    pos_run = np.add.reduceat(pos, run_start)
    cnt_run = np.diff(np.r_[run_start, n])
    neg_run = cnt_run - pos_run
    hi = key >> 32
    grp_of_run = hi[run_start]
    grp_start = _starts(grp_of_run[1:] != grp_of_run[:-1])          # index into the runs
    neg_before = np.cumsum(neg_run) - neg_run                        # negatives in earlier runs, all groups
    first_of_group = np.repeat(grp_start, np.diff(np.r_[grp_start, len(run_start)]))
    neg_below = neg_before - neg_before[first_of_group]              # ... of the run's own group
    term = pos_run * (2 * neg_below + neg_run)                       # < 2^63 for n < 2^31
    num2_g = np.add.reduceat(term, grp_start)
    P_g = np.add.reduceat(pos_run, grp_start)
    n_g = np.add.reduceat(cnt_run, grp_start)
    total = 0.0
    for t, p, m in zip(num2_g.tolist(), P_g.tolist(), n_g.tolist()):
        if p > 0 and m - p > 0:
            total += t / (2 * p * (m - p)) * m
    P = int(pos.sum())
    return (sum(num2_g.tolist()), P, n - P), total / n, pr_auc_of_runs(pos_run, cnt_run, P)


def pr_auc_of_runs(pos_run, cnt_run, P):
    """sklearn's `auc(*precision_recall_curve(y, s)[1::-1])`: thresholds are the runs, highest score first; tp and tp + fp
    accumulate from the top; the curve ends at (recall 0, precision 1); trapezoids over recall."""
    tps = np.cumsum(pos_run[::-1]).astype(np.float64)
    ps = np.cumsum(cnt_run[::-1]).astype(np.float64)
    precision = tps / ps
    recall = tps / P if P > 0 else np.ones_like(tps)
    p = np.r_[precision[::-1], 1.0]
    r = np.r_[recall[::-1], 0.0]
    return float(-np.sum(np.diff(r) * (p[1:] + p[:-1]) / 2.0))


def roc_auc(num2, P, Nneg):
    return num2 / (2 * P * Nneg)


# ---- pointwise sums ----------------------------------------------------------------------------------------------------------
def point_sums(pred, label, mean=0.0):
    """({sq, abs, y, tot, logloss} fp64 sums, (TP, TN, P, N) ints) of float32 predictions and labels."""
    pf, yf = np.asarray(pred, dtype=np.float32), np.asarray(label, dtype=np.float32)
    p, y = pf.astype(np.float64), yf.astype(np.float64)
    d = y - p
    clip = lambda x: np.clip(x, EPS32, 1.0 - EPS32)
    q = (np.float32(1.0) - pf).astype(np.float64)                    # sklearn forms the other column in float32
    with np.errstate(invalid="ignore", divide="ignore"):
        ll = -np.where(yf != 0, np.log(clip(p)), np.log(clip(q)))
    cls = np.rint(pf)                                                # half to even
    sums = {"sq": float(np.sum(d * d)), "abs": float(np.sum(np.abs(d))), "y": float(np.sum(y)),
            "tot": float(np.sum((y - mean) ** 2)), "logloss": float(np.sum(ll)), "abs_logloss": float(np.sum(np.abs(ll)))}
    counts = (int(np.sum((yf == 1) & (cls == 1))), int(np.sum((yf == 0) & (cls == 0))), int(np.sum(yf == 1)), int(np.sum(yf == 0)))
    return sums, counts


def balanced_accuracy(TP, TN, P, N):
    """sklearn's balanced_accuracy_score for labels in {0, 1}: the mean recall of the classes that occur in y_true."""
    rec = [c / s for c, s in ((TP, P), (TN, N)) if s > 0]
    return sum(rec) / len(rec)


def r2(ss_res, ss_tot):
    """sklearn's r2_score with force_finite: 1 - SSres / SStot; with SStot = 0, 1.0 for a perfect fit and 0.0 otherwise."""
    if ss_tot != 0:
        return 1.0 - ss_res / ss_tot
    return 1.0 if ss_res == 0 else 0.0


# ---- listwise ------------------------------------------------------------------------------------------------------------------
def discounts(k):
    return 1.0 / np.log2(np.arange(2, k + 2))


def listwise(reco, truths, truth_len, k):
    """f64 [4, U]: precision, recall, AP, NDCG at k.  `reco` int [U, k] padded with -1, `truths` one collection of ids per
    user, `truth_len` the divisor of recall."""
    reco = np.asarray(reco)
    U = reco.shape[0]
    disc = discounts(k)
    out = np.zeros((4, U), dtype=np.float64)
    for u in range(U):
        hit = (reco[u] >= 0) & np.isin(reco[u], np.asarray(list(truths[u]), dtype=np.int64))
        h = int(hit.sum())
        out[0, u] = h / k
        out[1, u] = h / int(truth_len[u])
        if h:
            cum = np.cumsum(hit).astype(np.float64)
            out[2, u] = float(np.sum((cum / np.arange(1, k + 1))[hit]) / h)
            out[3, u] = float(np.sum(disc[hit]) / np.sum(disc[:h]))
    return out


def truth_csr(truths):
    """(ptr int64 [U + 1], items int32 ascending and distinct per user, len int32 [U] = len(truths[u]) with duplicates)."""
    lists = [np.unique(np.asarray(list(t), dtype=np.int32)) for t in truths]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    items = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, items, np.array([len(t) for t in truths], dtype=np.int32)


def coverage(reco, n_items):
    ids = np.asarray(reco).reshape(-1)
    return int(len(np.unique(ids[(ids >= 0) & (ids < n_items)])))
