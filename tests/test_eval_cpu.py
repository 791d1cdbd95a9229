"""tests/eval_oracle.py (the restatement the metric kernels are tested against) checked against sklearn and the host functions
of `librecommender_amd.evaluation.metrics`: integer quantities exactly, fp64 quantities within the derived bounds of the oracle's
docstring.  Also the host-side contract of the new keyword: the default takes the old path and touches no `ops.eval_*`."""
import warnings

import numpy as np
import pytest
from sklearn.metrics import auc, balanced_accuracy_score, log_loss, precision_recall_curve, r2_score, roc_auc_score

from librecommender_amd.evaluation import metrics as M

from . import eval_oracle as O

N_BIG = 1 << 18


def _scores(rng, n, kind):
    if kind == "random":
        return rng.random(n).astype(np.float32)
    if kind == "tied":                                               # rounded to 1/4: five distinct values
        return (np.round(rng.random(n) * 4) / 4).astype(np.float32)
    if kind == "zeros":                                              # -0.0 and +0.0 tie, between a negative and a positive value
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], dtype=np.float32), n)
    raise ValueError(kind)


def _rank(score, label, group=None):
    key, bad = O.keys(score, group)
    assert bad == 0
    return O.rank_stats(*O.sort_by_key(key, label))


@pytest.mark.parametrize("kind", ["random", "tied", "zeros"])
@pytest.mark.parametrize("n", [2, 1000, N_BIG])
def test_auc_and_pr_auc_equal_sklearn(kind, n):
    rng = np.random.default_rng(n + len(kind))
    s = _scores(rng, n, kind)
    y = (rng.random(n) < 0.3).astype(np.float32)
    y[0], y[-1] = 1, 0
    (num2, P, Nneg), gauc, pr = _rank(s, y)
    assert (P, Nneg) == (int(y.sum()), n - int(y.sum()))
    assert abs(O.roc_auc(num2, P, Nneg) - roc_auc_score(y, s)) <= O.RANK_ATOL(n)
    assert abs(gauc - roc_auc_score(y, s)) <= O.RANK_ATOL(n)         # one group: GAUC is the AUC
    p, r, _ = precision_recall_curve(y, s)
    assert abs(pr - auc(r, p)) <= O.RANK_ATOL(n)


def test_key_image_orders_like_the_floats_and_ties_the_zeros():
    tiny = np.float32(1e-45)                                         # the smallest subnormal
    vals = np.array([-np.inf, -3.5, -tiny, -0.0, 0.0, tiny, 2.0 ** -126, 1.0, np.inf], dtype=np.float32)
    img = O.float_image(vals).astype(np.int64)
    assert img[3] == img[4]                                          # -0.0 == +0.0
    d = np.diff(img)
    assert (np.delete(d, 3) > 0).all() and d[3] == 0
    key, bad = O.keys(np.array([0.5, np.nan, 1.0, np.nan], np.float32), np.array([0, 1, 2 ** 31 - 1, 0]))
    assert bad == 2 and (key >= 0).all() and key[2] >> 32 == 2 ** 31 - 1
    # the host path ties the zeros too
    y = np.array([1, 0, 1, 0], np.float32)
    s = np.array([-0.0, 0.0, 0.0, -0.0], np.float32)
    (num2, P, Nneg), _, _ = _rank(s, y)
    assert O.roc_auc(num2, P, Nneg) == roc_auc_score(y, s) == 0.5


@pytest.mark.parametrize("kind", ["random", "tied"])
def test_gauc_equals_the_host_function(kind):
    rng = np.random.default_rng(5)
    n = 20000
    users = rng.integers(0, 700, n)
    users[users == 3] = 4                                            # an absent id
    s = _scores(rng, n, kind)
    y = (rng.random(n) < 0.4).astype(np.float32)
    y[users == 10] = 1                                               # single-class users, both kinds
    y[users == 11] = 0
    _, gauc, _ = _rank(s, y, users)
    assert abs(gauc - M.roc_gauc(y, s, users)) <= O.RANK_ATOL(n)


def test_single_class_labels_on_the_host_path():
    """What the host path returns for one class, which the device path repeats: roc_auc is nan with a warning, pr_auc the area
    of a curve whose recall is all ones (no positives) or whose precision is all ones (no negatives)."""
    s = np.array([.1, .2, .2, .4, .5, .9], np.float32)
    for y, area in ((np.zeros(6, np.float32), 0.5), (np.ones(6, np.float32), 1.0)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.isnan(roc_auc_score(y, s))
            p, r, _ = precision_recall_curve(y, s)
            assert auc(r, p) == area
        (num2, P, Nneg), gauc, pr = _rank(s, y)
        assert P * Nneg == 0 and gauc == 0.0 and pr == area


@pytest.mark.parametrize("n", [1, 7, 4096, N_BIG])
def test_point_sums_equal_sklearn_and_numpy(n):
    rng = np.random.default_rng(n)
    p = rng.random(n).astype(np.float32)
    p[: min(n, 5)] = np.array([0.0, 1.0, 0.5, 1e-10, 1 - 1e-7], np.float32)[: min(n, 5)]
    y = (rng.random(n) < 0.4).astype(np.float32)
    if n > 1:
        y[0], y[1] = 1, 0
    sums, (TP, TN, P, N) = O.point_sums(p, y, mean=float(y.astype(np.float64).mean()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if n > 1:
            assert abs(sums["logloss"] / n - log_loss(y, p)) <= O.point_rtol(n) * sums["abs_logloss"] / n
            assert O.balanced_accuracy(TP, TN, P, N) == balanced_accuracy_score(y, np.round(p))
    assert (P, N) == (int(y.sum()), n - int(y.sum()))
    assert abs(np.sqrt(sums["sq"] / n) - M.rmse(y, p)) <= O.point_rtol(n) * M.rmse(y, p)
    d = y.astype(np.float64) - p.astype(np.float64)
    assert abs(sums["abs"] - np.abs(d).sum()) <= O.point_rtol(n) * np.abs(d).sum()
    if n > 1:
        ref = r2_score(y.astype(np.float64), p.astype(np.float64))
        assert abs(O.r2(sums["sq"], sums["tot"]) - ref) <= O.point_rtol(n) * (1 + abs(ref))


def test_half_rounds_to_even_and_constant_labels():
    p = np.array([0.5, 0.5, 0.50000006, 0.49999997, 1.0, 0.0], np.float32)
    y = np.array([1, 0, 1, 0, 1, 0], np.float32)
    _, (TP, TN, P, N) = O.point_sums(p, y)
    assert (TP, TN, P, N) == (2, 3, 3, 3)                            # the 0.5 of a positive row is class 0
    assert O.balanced_accuracy(TP, TN, P, N) == balanced_accuracy_score(y, np.round(p))
    ones = np.ones(8, np.float32)
    for pred in (ones, np.zeros(8, np.float32)):                    # SStot = 0: 1.0 for a perfect fit, else 0.0
        sums, _ = O.point_sums(pred, ones, mean=1.0)
        assert sums["tot"] == 0 and O.r2(sums["sq"], sums["tot"]) == r2_score(ones, pred)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, c = O.point_sums(p, np.zeros(6, np.float32))
        assert O.balanced_accuracy(*c) == balanced_accuracy_score(np.zeros(6), np.round(p))


def _listwise_case(rng, U, k, n_items=400):
    truths, recos = [], []
    for u in range(U):
        t = rng.choice(n_items, size=int(rng.integers(1, 30)), replace=False).tolist()
        if u % 3 == 0:
            t = t + t[:2]                                            # duplicates: len(y_true) counts them, the match does not
        pool = rng.choice(n_items, size=k, replace=False)
        if u % 4 == 1:
            pool = np.setdiff1d(pool, t)                             # a user without hits
        if u % 4 == 2:
            pool = pool[: max(1, k // 2)]                            # a list shorter than k
        if u % 4 == 3:                                               # the first position hits; ids stay distinct
            pool = np.r_[t[0], pool[pool != t[0]]][:k]
        truths.append(t)
        recos.append(pool.astype(np.int32))
    return truths, recos


@pytest.mark.parametrize("k", [1, 10, 64, 65])
def test_listwise_equals_the_host_functions(k):
    rng = np.random.default_rng(k)
    U = 40
    truths, recos = _listwise_case(rng, U, k)
    reco = np.full((U, k), -1, np.int32)
    for u, r in enumerate(recos):
        reco[u, :len(r)] = r
    ptr, items, lens = O.truth_csr(truths)
    assert all((np.diff(items[ptr[u]:ptr[u + 1]]) > 0).all() for u in range(U))
    assert lens[0] == len(truths[0]) > ptr[1] - ptr[0]               # duplicates stay in the divisor
    got = O.listwise(reco, truths, lens, k)
    fns = (M.precision_at_k, M.recall_at_k, M.average_precision_at_k, M.ndcg_at_k)
    for row, fn in enumerate(fns):
        ref = np.array([fn(truths[u], recos[u], k) for u in range(U)], dtype=np.float64)
        assert (np.abs(got[row] - ref) <= O.LIST_RTOL(k) * np.abs(ref)).all(), fn.__name__
    assert (got[:, 1::4] == 0).all() or k == 1
    y_recos = {u: recos[u] for u in range(U)}
    assert O.coverage(reco, 400) / 400 * 100 == M.coverage(y_recos, range(U), 400)


# ---- the keyword --------------------------------------------------------------------------------------------------------------
class _Model:
    task = "ranking"
    n_users, n_items = 5, 7

    def predict(self, u, i, inner_id=False):
        return ((np.asarray(u) * 7 + np.asarray(i)) % 10 / 10).astype(np.float32)


def _counted(monkeypatch):
    from librecommender_amd import ops

    calls = []
    for name in ("eval_keys", "eval_rank_stats", "eval_point_sums", "eval_listwise", "eval_coverage"):
        def fail(*a, _n=name, **kw):
            calls.append(_n)
            raise AssertionError(f"ops.{_n} called")
        monkeypatch.setattr(ops, name, fail)
    return calls


def test_default_arguments_take_the_host_path(monkeypatch):
    from librecommender_amd import evaluation as E
    from librecommender_amd.data import TransformedEvalSet

    assert E.ON_DEVICE is False
    calls = _counted(monkeypatch)
    data = TransformedEvalSet(np.arange(20) % 5, np.arange(20) % 7, (np.arange(20) % 2).astype(np.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = E.evaluate(_Model(), data, neg_sampling=False, metrics=["loss", "roc_auc", "pr_auc", "roc_gauc", "balanced_accuracy"])
        res2 = E.evaluate(_Model(), data, neg_sampling=False, metrics=["loss", "roc_auc"], on_device=False)
    assert calls == [] and list(res) == ["loss", "roc_auc", "pr_auc", "roc_gauc", "balanced_accuracy"]
    assert all(type(v) is float for v in res.values()) and res2["roc_auc"] == res["roc_auc"]


def test_set_device_metrics_switches_the_default(monkeypatch):
    from librecommender_amd import evaluation as E
    from librecommender_amd.data import TransformedEvalSet
    from librecommender_amd.evaluation import device_metrics as D

    seen = []
    monkeypatch.setattr(D, "model_device", lambda model: seen.append("device") or (_ for _ in ()).throw(RuntimeError("stop")))
    data = TransformedEvalSet(np.arange(20) % 5, np.arange(20) % 7, (np.arange(20) % 2).astype(np.float32))
    assert E.set_device_metrics(True) is False
    try:
        assert E.ON_DEVICE is True
        with pytest.raises(RuntimeError, match="stop"):
            E.evaluate(_Model(), data, neg_sampling=False, metrics=["roc_auc"])
        with pytest.raises(ValueError, match="not suitable"):          # names are checked before the path is chosen
            E.evaluate(_Model(), data, neg_sampling=False, metrics=["rmse"])
        E.evaluate(_Model(), data, neg_sampling=False, metrics=["roc_auc"], on_device=False)      # the keyword wins
    finally:
        assert E.set_device_metrics(False) is True
    assert seen == ["device"] and E.ON_DEVICE is False
