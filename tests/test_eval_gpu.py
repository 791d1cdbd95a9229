"""The metric kernels (csrc/eval_metrics.hip) through `ops.eval_*` against tests/eval_oracle.py, and `evaluate(on_device=True)`
against the host path of the same call.

Integer outputs (keys, NaN count, num2 / P / Nneg, TP / TN / P / N, coverage) must equal the oracle's exactly; fp64 outputs
stay within the oracle's derived bounds (`RANK_ATOL`, `LIST_RTOL`, `point_rtol`: its docstring).  The kernels' summation order
is not restated in the oracle, so no fp64 output is compared bit for bit with it; two runs of a kernel are.

The kernel-level functions take `dev` and their parameters only: tests/test_guarded_eval_gpu.py runs them again on poisoned,
guarded allocations."""
import os
import re
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import _lib, ops

from . import eval_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(__file__)
DATA = os.path.join(HERE, "golden", "sample_movielens_rating.dat")
T = ops.EVAL_SCAN_TILE
PT = ops.EVAL_POINT_TILE


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_exported_tiles_are_the_kernels():
    """The workspace queries step where a new tile begins: 24 B and 16 B of tile summaries and 72 B of partial sums per tile,
    each region rounded to 256 B."""
    lib = _lib.load()
    assert lib.lr_eval_rank_ws_bytes(9 * T + 1) == lib.lr_eval_rank_ws_bytes(10 * T) < lib.lr_eval_rank_ws_bytes(10 * T + 1)
    assert lib.lr_eval_point_ws_bytes(2 * PT + 1) == lib.lr_eval_point_ws_bytes(3 * PT) < lib.lr_eval_point_ws_bytes(3 * PT + 1)
    assert lib.lr_eval_rank_ws_bytes(0) == lib.lr_eval_rank_ws_bytes(2 ** 31) == 0 < lib.lr_eval_rank_ws_bytes(2 ** 31 - 1)


# ---- keys ---------------------------------------------------------------------------------------------------------------
def test_keys(dev):
    tiny = np.float32(1e-45)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 2.0 ** -126, -(2.0 ** -127), np.nan, 1.0, -1.0, np.nan, 0.5],
                    dtype=np.float32)
    score = np.tile(vals, 41)                                        # 533 rows: more than one workgroup
    group = np.tile(np.array([0, 2 ** 31 - 1, 5], dtype=np.int32), len(score))[: len(score)]
    for g in (None, group):
        exp, bad = O.keys(score, g)
        key, nbad = ops.eval_keys(_dev(score, dev), None if g is None else _dev(g, dev))
        assert key.dtype == torch.int64 and nbad.dtype == torch.int32
        assert np.array_equal(key.cpu().numpy(), exp) and int(nbad.item()) == bad == 82
        assert (key >= 0).all()
    one = ops.eval_keys(_dev(np.array([-0.0], np.float32), dev))
    assert int(one[0].item()) == 0x80000000 and int(one[1].item()) == 0
    with pytest.raises(ValueError, match="shape not supported"):
        ops.eval_keys(torch.zeros(0, device=dev))


# ---- rank statistics ------------------------------------------------------------------------------------------------------
NS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 7]
PATTERNS = ["equal", "distinct", "four", "span3", "own_group", "single_class_groups", "edge_groups_single", "all_pos_but_one"]


def _pattern(rng, n, pattern):
    """(score f32 [n], label f32 [n], group int32 [n] or None)."""
    four = rng.choice(np.array([-0.0, 0.0, 0.25, -1.5, 3.0], dtype=np.float32), n)      # the zeros tie: four distinct values
    label = (rng.random(n) < 0.4).astype(np.float32)
    group = None
    if pattern == "equal":                                           # one run across every tile
        score = np.full(n, 0.25, np.float32)
    elif pattern == "distinct":
        score = rng.permutation(n).astype(np.float32) - n / 2
    elif pattern == "four":
        score = four
    elif pattern == "span3":                                         # one group over three tiles (the whole input where smaller)
        score = four
        small = np.repeat(np.arange(n // 50 + 1), 50)[:n]
        big = min(n, 2 * T + 100)
        start = min(T - 50, n - big)
        group = small.copy()
        group[start:start + big] = small[start]
        group[start + big:] += 1
        group = rng.permutation(group)                               # the sort brings them together
    elif pattern == "own_group":                                     # every row its own group, up to the largest id
        score = four
        group = rng.permutation(np.arange(n) + (2 ** 31 - n))
    elif pattern == "single_class_groups":
        score = four
        group = np.repeat(np.arange(n // 7 + 1), 7)[:n]
        label[group % 2 == 0] = (group[group % 2 == 0] // 2) % 2
        group = group * 3                                            # gaps between the ids
    elif pattern == "edge_groups_single":
        score = four
        group = np.repeat(np.arange(5), n // 5 + 1)[:n]
        label[group == group.min()] = 1
        label[group == group.max()] = 0
    elif pattern == "all_pos_but_one":
        score = four
        label[:] = 1
        label[int(rng.integers(0, n))] = 0
    else:
        raise ValueError(pattern)
    return score, label, None if group is None else group.astype(np.int32)


def _rank_stats(dev, score, label, group):
    key, bad = ops.eval_keys(_dev(score, dev), None if group is None else _dev(group, dev))
    key, order = torch.sort(key)
    lab = _dev((label != 0).astype(np.uint8), dev).index_select(0, order)
    ints, flts = ops.eval_rank_stats(key, lab)
    return key, lab, ints, flts, bad


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_rank_stats(dev, n, pattern):
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n)
    score, label, group = _pattern(rng, n, pattern)
    key, lab, ints, flts, bad = _rank_stats(dev, score, label, group)
    exp_key, exp_bad = O.keys(score, group)
    exp_key, exp_lab = O.sort_by_key(exp_key, label)
    assert int(bad.item()) == exp_bad == 0
    assert np.array_equal(key.cpu().numpy(), exp_key)
    (num2, P, Nneg), gauc, pr = O.rank_stats(exp_key, exp_lab)       # the labels of equal keys may come in another order: the
    assert ints.tolist() == [num2, P, Nneg]                          # statistics do not depend on it
    got_gauc, got_pr = flts.tolist()
    print(f"EVAL-FIGURE rank n={n} {pattern} gauc_err={abs(got_gauc - gauc):.3e} pr_err={abs(got_pr - pr):.3e} bound={O.RANK_ATOL(n):.3e}")
    assert abs(got_gauc - gauc) <= O.RANK_ATOL(n)
    assert abs(got_pr - pr) <= O.RANK_ATOL(n)
    if pattern == "own_group":
        assert got_gauc == 0.0 and num2 == 0
    if group is None and P and Nneg:                                 # one group: GAUC is the AUC
        assert abs(got_gauc - num2 / (2 * P * Nneg)) <= O.RANK_ATOL(n)


def test_rank_stats_argument_errors(dev):
    key = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        ops.eval_rank_stats(key, torch.zeros(3, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError):
        ops.eval_rank_stats(key, torch.zeros(4, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="shape not supported"):
        ops.eval_rank_stats(key[:0], torch.zeros(0, dtype=torch.uint8, device=dev))


# ---- pointwise sums -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["binary", "ones", "ratings"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, PT - 1, PT, PT + 1, 3 * PT + 5])
def test_point_sums(dev, n, labels):
    rng = np.random.default_rng(n + len(labels))
    if labels == "ratings":
        y = rng.integers(1, 6, n).astype(np.float32)
        p = (y + rng.standard_normal(n)).astype(np.float32)
    else:
        y = (rng.random(n) < 0.4).astype(np.float32) if labels == "binary" else np.ones(n, np.float32)
        p = rng.random(n).astype(np.float32)
        special = np.array([0.0, 1.0, 0.5, 0.5, 1e-10, 1 - 1e-7, 0.50000006, 0.49999997], np.float32)
        p[: min(n, 8)] = special[: min(n, 8)]
        if n >= 4 and labels == "binary":
            y[2], y[3] = 1, 0                                        # 0.5 under both labels
    mean = float(y.astype(np.float64).sum() / n)
    f, c = ops.eval_point_sums(_dev(p, dev), _dev(y, dev), mean=mean)
    sums, counts = O.point_sums(p, y, mean)
    assert c.tolist() == list(counts)
    got = dict(zip(("sq", "abs", "y", "tot", "logloss"), f.tolist()))
    assert got["y"] == sums["y"]                                     # small integers: exact in any order
    for name in ("sq", "abs", "tot"):
        assert abs(got[name] - sums[name]) <= O.point_rtol(n) * sums[name], name
    if labels != "ratings":
        assert abs(got["logloss"] - sums["logloss"]) <= O.point_rtol(n) * sums["abs_logloss"]
    if labels == "ones":                                             # SStot = 0 exactly: r2 takes sklearn's finite value
        assert got["tot"] == 0.0 and O.r2(got["sq"], got["tot"]) == 0.0
        f2, _ = ops.eval_point_sums(_dev(y, dev), _dev(y, dev), mean=mean)
        assert f2.tolist()[:2] == [0.0, 0.0] and O.r2(*[f2.tolist()[i] for i in (0, 3)]) == 1.0


def test_point_sums_nan_prediction_poisons_the_log_loss(dev):
    p = np.array([0.2, np.nan, 0.7], np.float32)
    f, _ = ops.eval_point_sums(_dev(p, dev), _dev(np.array([1, 0, 1], np.float32), dev))
    assert np.isnan(f.tolist()[4])


# ---- listwise ---------------------------------------------------------------------------------------------------------------
N_ITEMS = 20011                                                      # a prime: id = (start + stride * j) mod it never repeats in a row


def _listwise_case(rng, U, k):
    truths, reco = [], np.zeros((U, k), dtype=np.int64)
    j = np.arange(k)
    for u in range(U):
        size = (1, 5000, int(rng.integers(2, 40)))[u % 3]
        t = np.sort(rng.choice(N_ITEMS, size=size, replace=False))
        row = (int(rng.integers(0, N_ITEMS)) + int(rng.integers(1, N_ITEMS)) * j) % N_ITEMS
        if u % 2 == 0 and size >= 2 and k >= 2:                     # the first and the last truth item are recommended
            row[(row == t[0]) | (row == t[-1])] = -1
            row[0], row[k - 1] = t[-1], t[0]
        elif u % 4 == 1:
            row[row == t[0]] = -1
            row[k // 2] = t[0]
        if u % 5 == 4:
            row[k - k // 3:] = -1                                    # a list shorter than k
        if u % 7 == 3:
            t = np.r_[t, t[:1]]                                      # a duplicate: it counts in the divisor of recall only
        truths.append(t.tolist())
        reco[u] = row
    return truths, reco.astype(np.int32)


@pytest.mark.parametrize("k", [1, 10, 64, 65, 1024])
@pytest.mark.parametrize("U", [1, 63, 64, 65, 1000])
def test_listwise(dev, U, k):
    rng = np.random.default_rng(100 * U + k)
    truths, reco = _listwise_case(rng, U, k)
    ptr, items, lens = O.truth_csr(truths)
    exp = O.listwise(reco, truths, lens, k)
    if U >= 63 and k >= 10:
        assert exp[0].max() > 0 and exp[0].min() == 0                # users with and without hits
    out = ops.eval_listwise(_dev(reco, dev), _dev(ptr, dev), _dev(items, dev), _dev(lens, dev), _dev(O.discounts(k), dev))
    got = out.cpu().numpy()
    assert got.shape == (4, U)
    assert np.array_equal(got[:2], exp[:2])                          # integer over integer: one division, the same on both sides
    err = np.abs(got[2:] - exp[2:])
    print(f"EVAL-FIGURE listwise U={U} k={k} max_rel_err={(err / np.maximum(exp[2:], 1e-300)).max():.3e} bound={O.LIST_RTOL(k):.3e}")
    assert (err <= O.LIST_RTOL(k) * np.abs(exp[2:])).all()


def test_listwise_unsupported_k_raises_and_writes_nothing(dev):
    U = 5
    truths = [[1, 2, 3]] * U
    ptr, items, lens = (_dev(a, dev) for a in O.truth_csr(truths))
    for k in (0, 1025):
        out = torch.full((4, U), 1234.5, dtype=torch.float64, device=dev)
        reco = torch.zeros((U, k), dtype=torch.int32, device=dev)
        disc = torch.ones(max(k, 1), dtype=torch.float64, device=dev)[:k]
        with pytest.raises(ValueError, match="shape not supported"):
            ops.eval_listwise(reco, ptr, items, lens, disc, out=out)
        if k:                                                        # the C entry point itself refuses too
            with pytest.raises(ValueError):
                ops._call("lr_eval_listwise", reco.data_ptr(), ptr.data_ptr(), items.data_ptr(), lens.data_ptr(), disc.data_ptr(),
                          U, k, out.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        assert (out == 1234.5).all()


# ---- coverage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["same", "distinct", "last_id", "random", "padding_only"])
def test_coverage(dev, kind):
    rng = np.random.default_rng(len(kind))
    n_items, U, k = 3001, 70, 10
    if kind == "same":
        reco = np.full((U, k), 17, np.int32)
    elif kind == "distinct":
        reco = rng.permutation(n_items)[: U * k].reshape(U, k).astype(np.int32)
    elif kind == "last_id":
        reco = np.full((U, k), -1, np.int32)
        reco[3, 4] = n_items - 1
        reco[0, 0] = 0
    elif kind == "random":
        reco = rng.integers(-1, n_items, (U, k)).astype(np.int32)
    else:
        reco = np.full((U, k), -1, np.int32)
    exp = O.coverage(reco, n_items)
    assert exp == {"same": 1, "distinct": U * k, "last_id": 2, "padding_only": 0}.get(kind, exp)
    got = ops.eval_coverage(_dev(reco, dev), n_items)
    assert got.dtype == torch.int64 and int(got.item()) == exp


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):
    rng = np.random.default_rng(9)
    n = 5 * T + 13
    score = rng.standard_normal(n).astype(np.float32).round(2)
    label = (rng.random(n) < 0.3).astype(np.float32)
    group = rng.integers(0, 40, n).astype(np.int32)
    pred = rng.random(n).astype(np.float32)
    truths, reco = _listwise_case(rng, 65, 65)
    ptr, items, lens = (_dev(a, dev) for a in O.truth_csr(truths))
    runs = []
    for _ in range(2):
        key, _, ints, flts, bad = _rank_stats(dev, score, label, group)
        f, c = ops.eval_point_sums(_dev(pred, dev), _dev(label, dev), mean=0.3)
        lw = ops.eval_listwise(_dev(reco, dev), ptr, items, lens, _dev(O.discounts(65), dev))
        cov = ops.eval_coverage(_dev(reco, dev), N_ITEMS)
        runs.append((key, ints, flts, bad, f, c, lw, cov))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- model level --------------------------------------------------------------------------------------------------------------
POINT = ["loss", "log_loss", "balanced_accuracy", "roc_auc", "pr_auc", "roc_gauc"]
LIST = ["precision", "recall", "map", "ndcg", "coverage"]


def _frames():
    from librecommender_amd.data import split_by_ratio_chrono

    df = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"]).iloc[:20000]
    return split_by_ratio_chrono(df, test_size=0.2)


@pytest.fixture(scope="module")
def ranking_sets(dev):
    from librecommender_amd.data import DatasetPure

    train, evald = _frames()
    train_data, info = DatasetPure.build_trainset(train)
    return train_data, info, evald


def _compare(model, eval_data, metrics, k, sample_user_num, neg_sampling):
    from librecommender_amd.evaluation import evaluate

    kw = dict(neg_sampling=neg_sampling, metrics=metrics, k=k, sample_user_num=sample_user_num, seed=11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = evaluate(model, eval_data, **kw)                      # samples the negatives into eval_data; both paths read them
        device = evaluate(model, eval_data, on_device=True, **kw)
        again = evaluate(model, eval_data, on_device=True, **kw)     # the cached uploads
    assert list(device) == list(host) and device == again
    assert all(type(v) is float for v in device.values())
    return host, device, len(eval_data)


def _check_ranking(host, device, n, n_users, k):
    for m in host:
        err = abs(device[m] - host[m])
        print(f"EVAL-FIGURE model {m} host={host[m]!r} device={device[m]!r} err={err:.3e}")
        if m in ("roc_auc", "pr_auc", "roc_gauc"):
            assert err <= O.RANK_ATOL(n), m
        elif m in ("loss", "log_loss"):
            assert err <= O.point_rtol(n) * host[m], m               # the terms are all positive
        elif m in ("balanced_accuracy", "coverage"):
            assert err <= 2.0 ** -52 * host[m], m                    # the same integers through the same few operations
        else:                                                        # a mean over the users (any order: U 2^-53 a side) of per-user values
            assert err <= (n_users + 4 * k) * 2.0 ** -52 * host[m], m


@pytest.mark.parametrize("name", ["BPR", "DeepFM"])
def test_evaluate_on_device_equals_the_host_path(dev, ranking_sets, name):
    import librecommender_amd.algorithms as A
    from librecommender_amd.data import DatasetPure

    train_data, info, evald = ranking_sets
    if name == "BPR":
        model = A.BPR("ranking", info, embed_size=16, n_epochs=1, seed=7, use_tf=True)
    else:
        model = A.DeepFM("ranking", info, embed_size=16, n_epochs=1, lr=1e-2, batch_size=512, hidden_units=(32, 16), seed=7)
    model.fit(train_data, neg_sampling=True, verbose=0)
    for k, num in ((10, 200), (7, None)):
        eval_data = DatasetPure.build_evalset(evald)
        host, device, n = _compare(model, eval_data, POINT + LIST, k, num, True)
        n_users = num or len(eval_data.positive_consumed)
        _check_ranking(host, device, n, n_users, k)
        assert hasattr(eval_data, "_device_cache") and len(eval_data._device_cache["truth"]) == 1


def test_rating_metrics_on_device_equal_the_host_path(dev):
    """rmse is fp64 on both sides.  mae and r2 are FLOAT32 sums on the host (numpy's mean and sklearn's r2_score keep the
    input dtype): a pairwise float32 sum of n terms, each rounded once, errs by at most (log2 n + 4) 2^-24 relatively, and r2
    holds two such sums and a float32 mean, in a ratio: 4 (log2 n + 6) 2^-24 (1 + |1 - r2|)."""
    import librecommender_amd.algorithms as A
    from librecommender_amd.data import DatasetPure

    train, evald = _frames()
    train_data, info = DatasetPure.build_trainset(train)
    eval_data = DatasetPure.build_evalset(evald)
    model = A.SVD("rating", info, embed_size=16, n_epochs=1, seed=42)
    model.fit(train_data, neg_sampling=False, verbose=0)
    host, device, n = _compare(model, eval_data, ["loss", "rmse", "mae", "r2"], 10, None, False)
    for m in host:
        print(f"EVAL-FIGURE model {m} host={host[m]!r} device={device[m]!r} err={abs(device[m] - host[m]):.3e}")
    lg = np.log2(n)
    assert abs(device["rmse"] - host["rmse"]) <= O.point_rtol(n) * host["rmse"] and device["loss"] == device["rmse"]
    assert abs(device["mae"] - host["mae"]) <= (lg + 4) * 2.0 ** -24 * host["mae"]
    assert abs(device["r2"] - host["r2"]) <= 4 * (lg + 6) * 2.0 ** -24 * (1 + abs(1 - host["r2"]))


def test_nan_predictions_raise_on_the_device_path(dev, ranking_sets):
    from librecommender_amd.data import TransformedEvalSet
    from librecommender_amd.evaluation import evaluate

    class Model:
        task, n_users, n_items, device = "ranking", 5, 7, dev

        def predict(self, u, i, inner_id=False):
            p = np.linspace(0.1, 0.9, len(u)).astype(np.float32)
            p[1] = np.nan
            return p

    data = TransformedEvalSet(np.arange(20) % 5, np.arange(20) % 7, (np.arange(20) % 2).astype(np.float32))
    for metrics in (["roc_auc"], ["roc_gauc"], ["log_loss"], ["balanced_accuracy"]):
        with pytest.raises(ValueError, match="NaN"):
            evaluate(Model(), data, neg_sampling=False, metrics=metrics, on_device=True)
    with pytest.raises(ValueError, match="not suitable"):
        evaluate(Model(), data, neg_sampling=False, metrics=["rmse"], on_device=True)


def test_fit_prints_the_same_numbers_with_device_metrics(dev, ranking_sets, capsys):
    import librecommender_amd.algorithms as A
    from librecommender_amd import evaluation as E
    from librecommender_amd.data import DatasetPure

    train_data, info, evald = ranking_sets
    printed = []
    for flag in (False, True):
        prev = E.set_device_metrics(flag)
        try:
            model = A.BPR("ranking", info, embed_size=16, n_epochs=1, seed=7, use_tf=True)
            model.fit(train_data, neg_sampling=True, verbose=2, eval_data=DatasetPure.build_evalset(evald), metrics=POINT + LIST,
                      eval_user_num=150)
        finally:
            E.set_device_metrics(prev)
        printed.append(re.findall(r"eval [^\n]*", capsys.readouterr().out))
    assert len(printed[0]) == len(POINT + LIST) and printed[0] == printed[1]
