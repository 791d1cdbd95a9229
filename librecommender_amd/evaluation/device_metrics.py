"""The device path of `evaluate` (`on_device=True`): the values of `libreco/evaluation/evaluate.py:62-193` and
`metrics.py` computed by the kernels of csrc/eval_metrics.hip instead of sklearn, numpy and Python sets.

Predictions are uploaded batch by batch into one f32 buffer (every `predict` of this package returns numpy); labels, user
indices and the truth lists are uploaded once per eval set and kept on it (`_device_cache`).  The sort of the 64-bit keys is
`torch.sort`; everything that reads the sorted rows is one `ops.eval_rank_stats` call.  What comes back to the host is a
handful of sums.

Values equal the host path's up to fp64 summation order, with two exceptions that are the host's own float32 arithmetic:
`mae` and `r2` are float32 sums there (numpy / sklearn keep the input dtype) and fp64 sums here."""
import math
import warnings

import numpy as np
import torch

from .. import ops

RANK_METRICS = ("roc_auc", "pr_auc")
POINT_METRICS = ("loss", "log_loss", "balanced_accuracy")


def model_device(model) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate(on_device=True) needs an MI355X device (there is no CPU fallback for the metric kernels)")
    dev = getattr(model, "device", None)
    if isinstance(dev, torch.device) and dev.type == "cuda":
        return dev
    return torch.device("cuda", torch.cuda.current_device())


def _cache(data, dev):
    """Per eval set: labels (f32 and u8) and user indices on the device, uploaded once; the truth CSRs by user sample."""
    tag = (str(dev), len(data), bool(data.has_sampled))
    c = getattr(data, "_device_cache", None)
    if c is None or c["tag"] != tag:
        labels = np.ascontiguousarray(data.labels, dtype=np.float32)
        c = {"tag": tag,
             "labels": torch.from_numpy(labels).to(dev),
             "labels_u8": torch.from_numpy((labels != 0).astype(np.uint8)).to(dev),
             "users": torch.from_numpy(np.ascontiguousarray(data.user_indices, dtype=np.int32)).to(dev),
             "truth": {}, "disc": {}}
        data._device_cache = c
    return c


def predict_all(model, data, batch_size, dev) -> torch.Tensor:
    """f32 [N] on the device: `model.predict` batch by batch, each batch uploaded once into the one buffer."""
    out = torch.empty(len(data), dtype=torch.float32, device=dev)
    for s in range(0, len(data), batch_size):
        u, i, _ = data[s:s + batch_size]
        p = torch.from_numpy(np.ascontiguousarray(np.atleast_1d(model.predict(u, i, inner_id=True)), dtype=np.float32))
        out[s:s + p.numel()].copy_(p.reshape(-1))
    return out


def _nan_error():
    return ValueError("Input contains NaN.")


def _rank(pred, labels_u8, group=None):
    """(num2, P, Nneg, gauc, pr_auc) of one keyed sort."""
    key, bad = ops.eval_keys(pred, group)
    key, order = torch.sort(key)
    ints, flts = ops.eval_rank_stats(key, labels_u8.index_select(0, order))
    if int(bad.item()) > 0:
        raise _nan_error()
    return (*ints.tolist(), *flts.tolist())


def _single_class_warning(what):
    from sklearn.exceptions import UndefinedMetricWarning

    warnings.warn(f"Only one class is present in y_true. {what} is not defined in that case.", UndefinedMetricWarning)


def pointwise(model, data, metrics, batch_size, dev, out):
    c = _cache(data, dev)
    pred = predict_all(model, data, batch_size, dev)
    n = pred.numel()
    want = set(metrics)
    if want & set(RANK_METRICS):                                     # the global order: one sort for both
        num2, P, Nneg, _, pr = _rank(pred, c["labels_u8"])
    if "roc_gauc" in want:                                           # the (user, score) order does not serve the global metrics
        gauc = _rank(pred, c["labels_u8"], c["users"])[3]
    if want & set(POINT_METRICS):
        f, cnt = ops.eval_point_sums(pred, c["labels"])
        f, cnt = f.tolist(), cnt.tolist()
        if math.isnan(f[4]):
            raise _nan_error()
    for m in metrics:
        if m in ("log_loss", "loss"):
            out[m] = f[4] / n
        elif m == "balanced_accuracy":
            TP, TN, Pc, Nc = cnt
            rec = [a / b for a, b in ((TP, Pc), (TN, Nc)) if b > 0]
            out[m] = sum(rec) / len(rec)
        elif m == "roc_auc":
            if P == 0 or Nneg == 0:                                  # sklearn: nan and a warning
                _single_class_warning("ROC AUC score")
                out[m] = float("nan")
            else:
                out[m] = num2 / (2 * P * Nneg)
        elif m == "roc_gauc":
            out[m] = gauc
        elif m == "pr_auc":
            out[m] = pr


def rating(model, data, metrics, batch_size, dev, out):
    c = _cache(data, dev)
    pred = predict_all(model, data, batch_size, dev)
    n = pred.numel()
    f = ops.eval_point_sums(pred, c["labels"])[0].tolist()
    if any(math.isnan(x) for x in f[:3]):
        raise _nan_error()
    for m in metrics:
        if m in ("rmse", "loss"):
            out[m] = math.sqrt(f[0] / n)
        elif m == "mae":
            out[m] = f[1] / n
        elif m == "r2":
            if n < 2:                                                # sklearn: not defined, nan and a warning
                warnings.warn("R^2 score is not well-defined with less than two samples.")
                out[m] = float("nan")
                continue
            tot = ops.eval_point_sums(pred, c["labels"], mean=f[2] / n)[0][3].item()
            if tot != 0:
                out[m] = 1.0 - f[0] / tot
            else:                                                    # sklearn's force_finite
                out[m] = 1.0 if f[0] == 0 else 0.0


def truth_csr(data, users, dev, key):
    """The truth lists of `users` as a CSR on the device, built once per (eval set, user sample)."""
    c = _cache(data, dev)
    hit = c["truth"].get(key)
    if hit is None:
        lists = [np.unique(np.asarray(data.positive_consumed[u], dtype=np.int32)) for u in users]
        ptr = np.zeros(len(users) + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        items = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        lens = np.array([len(data.positive_consumed[u]) for u in users], dtype=np.int32)
        hit = c["truth"][key] = (torch.from_numpy(ptr).to(dev), torch.from_numpy(items.astype(np.int32)).to(dev),
                                 torch.from_numpy(lens).to(dev))
    return hit


def listwise(model, data, metrics, users, recos, k, dev, out, cache_key):
    c = _cache(data, dev)
    k = int(k)
    reco = np.full((len(users), max(k, 0)), -1, dtype=np.int32)
    for r, u in enumerate(users):
        ids = np.asarray(recos[u]).reshape(-1)[:k]
        reco[r, :len(ids)] = ids
    reco = torch.from_numpy(reco).to(dev)
    if set(metrics) & {"precision", "recall", "map", "ndcg"}:
        ptr, items, lens = truth_csr(data, users, dev, cache_key)
        disc = c["disc"].get(k)
        if disc is None:                                             # k outside 1 .. 1024: `ops.eval_listwise` raises before it reads this
            disc = c["disc"][k] = torch.from_numpy(1.0 / np.log2(np.arange(2, max(k, 0) + 2))).to(dev)
        per_user = ops.eval_listwise(reco, ptr, items, lens, disc)
        means = (per_user.sum(dim=1) / len(users)).tolist()
    row = {"precision": 0, "recall": 1, "map": 2, "ndcg": 3}
    for m in metrics:
        if m == "coverage":
            out[m] = int(ops.eval_coverage(reco, model.n_items).item()) / model.n_items * 100
        elif m in row:
            out[m] = means[row[m]]
