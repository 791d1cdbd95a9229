"""ALS on the device (csrc/als.hip): the Gram G0, one half-sweep of every task x solver x width against the fp64
restatement of `_als.pyx` (tests/als_oracle.py), determinism, and the model surface on the MovieLens sample."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import ALS
from librecommender_amd.data import DatasetPure, split_by_ratio_chrono
from librecommender_amd.evaluation import evaluate

from . import als_oracle as O

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(__file__), "golden", "sample_movielens_rating.dat")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("K", [1, 8, 16, 20, 64, 128])
def test_gram_against_fp64_and_bitwise_repeatable(dev, K):
    rng = np.random.default_rng(K)
    N = 12_347                                    # not a multiple of any tile
    Y = rng.normal(0, 0.2, (N, K)).astype(np.float32)
    Yd = _dev(Y, dev)
    g = ops.als_gram(Yd, 0.25, True)
    g2 = ops.als_gram(Yd, 0.25, True)
    torch.cuda.synchronize()
    ref = O.gram0(Y, np.float32(0.25), True)
    np.testing.assert_allclose(g.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    assert torch.equal(g, g2)
    e = ops.als_gram(Yd, 0.25, False).cpu().numpy()
    np.testing.assert_array_equal(e, np.float32(0.25) * np.eye(K, dtype=np.float32))


def _sweep_case(K, implicit, seed=0):
    """Rows on both sides of every plan threshold, zero- and one-degree rows, and one row of degree 100 k (heavy path)."""
    import ctypes as C

    from librecommender_amd import _lib

    lim = (C.c_int32 * 3)()
    assert _lib.load().lr_als_plan_params(K, lim) == 0
    cap, heavy, chunk = list(lim)
    degs = [0, 0, 1, 1, 2, 3, cap - 1, cap, cap + 1, cap + 2, 100, heavy - 1, heavy, heavy + 1, chunk * 2 + 5, 100_000]
    degs += list(np.random.default_rng(seed).integers(0, 40, 24))
    rng = np.random.default_rng(seed + 1)
    cols = 120_000
    indptr, indices, val = O.random_csr(rng, len(degs), cols, degs, values=(1.0, 5.0))
    if implicit:
        val = (val * 2 + 1).astype(np.float32)      # confidences
    X = rng.normal(0, 0.1, (len(degs), K)).astype(np.float32)
    Y = rng.normal(0, 0.1, (cols, K)).astype(np.float32)
    return indptr, indices, val, X, Y


@pytest.mark.parametrize("K", [8, 16, 20, 64, 128])
@pytest.mark.parametrize("use_cg", [True, False])
@pytest.mark.parametrize("task", ["rating", "ranking"])
def test_half_sweep_against_fp64(dev, task, use_cg, K):
    implicit = task == "ranking"
    indptr, indices, val, X, Y = _sweep_case(K, implicit)
    reg = 0.1
    rp, col, v = _dev(indptr, dev), _dev(indices, dev), _dev(val, dev)
    Xd, Yd = _dev(X, dev), _dev(Y, dev)
    plan = ops.als_plan(rp, K)
    assert plan.n_light > 0 and plan.n_medium > 0 and plan.n_heavy > 0
    G0 = ops.als_gram(Yd, reg, implicit)
    fail = ops.als_half_sweep(rp, col, v, Xd, Yd, G0, implicit, use_cg, plan)
    X2 = _dev(X, dev)
    ops.als_half_sweep(rp, col, v, X2, Yd, G0, implicit, use_cg, plan)
    got = Xd.cpu().numpy().astype(np.float64)
    assert torch.equal(Xd, X2), "two runs differ"
    if fail is not None:
        assert int(fail.count_nonzero()) == 0
    ref = O.half_sweep(indptr, indices, val, X, Y, np.float32(reg), implicit, use_cg)
    rel = 1e-3 if use_cg else 1e-4
    err = np.linalg.norm(got - ref, axis=1)
    bar = rel * np.linalg.norm(ref, axis=1) + 1e-6
    bad = np.nonzero(err > bar)[0]
    assert bad.size == 0, [(int(m), int(indptr[m + 1] - indptr[m]), float(err[m]), float(bar[m])) for m in bad[:8]]


@pytest.mark.parametrize("task", ["rating", "ranking"])
def test_direct_solver_objective_does_not_increase(dev, task):
    implicit = task == "ranking"
    rng = np.random.default_rng(5)
    nu, ni, K, reg = 300, 200, 16, 0.05
    deg = rng.integers(0, 30, nu)
    indptr, indices, val = O.random_csr(rng, nu, ni, deg)
    if implicit:
        val = (val * 3 + 1).astype(np.float32)
    # the transpose
    rows = np.repeat(np.arange(nu), deg)
    order = np.lexsort((rows, indices))
    tptr = np.zeros(ni + 1, np.int64)
    tptr[1:] = np.cumsum(np.bincount(indices, minlength=ni))
    U = _dev(rng.normal(0, 0.1, (nu, K)).astype(np.float32), dev)
    V = _dev(rng.normal(0, 0.1, (ni, K)).astype(np.float32), dev)
    ucsr = (_dev(indptr, dev), _dev(indices, dev), _dev(val, dev))
    icsr = (_dev(tptr, dev), _dev(rows[order].astype(np.int32), dev), _dev(val[order], dev))
    up, ip = ops.als_plan(ucsr[0], K), ops.als_plan(icsr[0], K)
    prev = None
    for _ in range(4):
        for csr, plan, X, Y in ((ucsr, up, U, V), (icsr, ip, V, U)):
            ops.als_half_sweep(*csr, X, Y, ops.als_gram(Y, reg, implicit), implicit, False, plan)
            f = O.objective(indptr, indices, val, U.cpu().numpy(), V.cpu().numpy(), reg, implicit)
            if prev is not None:
                assert f <= prev * (1 + 1e-5) + 1e-6, (f, prev)
            prev = f


def test_direct_solver_failure_raises_value_error(dev):
    rng = np.random.default_rng(2)
    indptr, indices, val = O.random_csr(rng, 10, 50, [3] * 10)
    val = np.full_like(val, -50.0)                 # w = c - 1 < 0: A is not positive definite
    rp = _dev(indptr, dev)
    X = _dev(rng.normal(0, 1, (10, 8)).astype(np.float32), dev)
    Y = _dev(rng.normal(0, 1, (50, 8)).astype(np.float32), dev)
    X0 = X.clone()
    fail = ops.als_half_sweep(rp, _dev(indices, dev), _dev(val, dev), X, Y, ops.als_gram(Y, 1e-3, True), True, False,
                              ops.als_plan(rp, 8))
    assert int(fail.count_nonzero()) > 0
    bad = fail != 0
    assert torch.equal(X[bad], X0[bad])            # failing rows are left as they were


@pytest.fixture(scope="module")
def movielens():
    df = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    train, evald = split_by_ratio_chrono(df, test_size=0.2)
    train_data, info = DatasetPure.build_trainset(train)
    eval_data = DatasetPure.build_evalset(evald)
    return df, train, evald, train_data, eval_data, info


@pytest.mark.parametrize("task,use_cg", [("rating", True), ("ranking", True), ("ranking", False), ("rating", False)])
def test_model_surface(dev, movielens, tmp_path, task, use_cg):
    df, train, evald, train_data, eval_data, info = movielens
    before = train_data.sparse_interaction.copy()
    model = ALS(task, info, embed_size=16, n_epochs=2, reg=0.1, alpha=10, use_cg=use_cg, seed=42)
    model.fit(train_data, neg_sampling=task == "ranking", verbose=0)
    assert (train_data.sparse_interaction != before).nnz == 0
    assert np.array_equal(train_data.sparse_interaction.data, before.data)
    assert model.user_embeds.shape == (info.n_users + 1, 16) and model.user_embeds.is_cuda
    u, i = train.user.iloc[0], train.item.iloc[0]
    pred = model.predict(user=u, item=i)
    assert np.all(np.isfinite(pred))
    recs = model.recommend_user(user=u, n_rec=7)[u]
    assert len(recs) == 7
    metrics = ["rmse"] if task == "rating" else ["roc_auc", "precision", "ndcg"]
    res = evaluate(model, eval_data, neg_sampling=task == "ranking", metrics=metrics, k=10)
    assert all(np.isfinite(v) for v in res.values())
    if task == "ranking":
        assert res["roc_auc"] > 0.6, res
    else:   # exact ALS at reg = 0.1 overfits the sparse users of this sample: a sanity bar on the 1 - 5 scale
        assert res["rmse"] < 4.0, res
    model.init_knn(approximate=False, sim_type="cosine")
    assert len(model.search_knn_items(i, 5)) == 5
    # full checkpoint
    model.save(str(tmp_path), "als")
    loaded = ALS.load(str(tmp_path), "als", info)
    users = train.user.unique()[:20].tolist()
    a = model.recommend_user(user=users, n_rec=10)
    b = loaded.recommend_user(user=users, n_rec=10)
    assert all(np.array_equal(a[x], b[x]) for x in users)
    # inference-only checkpoint in the reference's layout: {name}.npz + default recs + hyper-parameters
    model.save(str(tmp_path), "als_inf", inference_only=True)
    assert not os.path.exists(os.path.join(tmp_path, "als_inf_variables.npz"))
    with np.load(os.path.join(tmp_path, "als_inf.npz")) as z:
        assert set(z.files) == {"user_embed", "item_embed"} and z["user_embed"].shape == (info.n_users + 1, 16)
    inf = ALS.load(str(tmp_path), "als_inf", info)          # EmbedBase.load: embeddings only
    c = inf.recommend_user(user=users, n_rec=10)
    assert all(np.array_equal(a[x], c[x]) for x in users)


def test_fit_is_deterministic_and_continues(dev, movielens):
    *_, train_data, _, info = movielens
    m1 = ALS("ranking", info, embed_size=32, n_epochs=2, reg=0.1, seed=3)
    m2 = ALS("ranking", info, embed_size=32, n_epochs=2, reg=0.1, seed=3)
    m1.fit(train_data, neg_sampling=True, verbose=0)
    m2.fit(train_data, neg_sampling=True, verbose=0)
    assert torch.equal(m1.user_embeds, m2.user_embeds) and torch.equal(m1.item_embeds, m2.item_embeds)
    # a second fit continues from the current tables (OOV rows dropped, then appended again)
    m3 = ALS("ranking", info, embed_size=32, n_epochs=4, reg=0.1, seed=3)
    m3.fit(train_data, neg_sampling=True, verbose=0)
    m1.fit(train_data, neg_sampling=True, verbose=0)
    assert m1.user_embeds.shape == (info.n_users + 1, 32)
    assert torch.equal(m1.user_embeds, m3.user_embeds)


def test_rebuild_model_keeps_old_rows(dev, movielens, tmp_path):
    df, train, evald, train_data, eval_data, info = movielens
    model = ALS("rating", info, embed_size=16, n_epochs=1, reg=0.1)
    model.fit(train_data, neg_sampling=False, verbose=0)
    model.save(str(tmp_path), "als")
    new = evald.copy()
    new["user"] = new["user"] + 10_000_000           # unseen users
    train2, info2 = DatasetPure.merge_trainset(new, info)
    m2 = ALS("rating", info2, embed_size=16, n_epochs=1, reg=0.1)
    m2.rebuild_model(str(tmp_path), "als")
    old_u = model.user_embeds[: info.n_users]
    assert torch.equal(m2.user_embeds[: info.n_users], old_u)
    assert torch.equal(m2.item_embeds[: info.n_items], model.item_embeds[: info.n_items])
    m2.fit(train2, neg_sampling=False, verbose=0)
    assert m2.user_embeds.shape[0] == info2.n_users + 1


def test_multi_rank_fit_raises(dev, movielens, monkeypatch):
    *_, train_data, _, info = movielens
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        ALS("ranking", info, reg=0.1, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)


def test_embed_size_over_limit(dev, movielens):
    *_, info = movielens
    with pytest.raises(ValueError):
        ALS("ranking", info, embed_size=129, reg=0.1)


@pytest.mark.parametrize("use_cg", [True, False])
def test_zipf_million_scale_rows_against_fp64(dev, use_cg):
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from bench_workloads import distinct_interactions

    n, E, K, reg = 1_000_000, 20_000_000, 64, 0.1
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    eu, ei = distinct_interactions(E, n, n, gen, dev)
    order = torch.argsort(eu.to(torch.int64) * n + ei)
    col = ei[order].contiguous()
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(eu.to(torch.int64), minlength=n), 0)
    del eu, ei, order
    val = torch.rand(E, generator=gen, device=dev) * 4 + 1           # confidences in [1, 5)
    X = torch.randn((n, K), generator=gen, device=dev) * 0.05
    Y = torch.randn((n, K), generator=gen, device=dev) * 0.05
    X0 = X.cpu().numpy()
    plan = ops.als_plan(rowptr, K)
    assert plan.n_heavy > 0
    ops.als_half_sweep(rowptr, col, val, X, Y, ops.als_gram(Y, reg, True), True, use_cg, plan)
    deg = (rowptr[1:] - rowptr[:-1])
    heavy = torch.topk(deg, 32).indices.cpu().numpy()
    rnd = np.random.default_rng(0).choice(n, 1000, replace=False)
    rows = np.unique(np.concatenate([heavy, rnd]))
    ip, ix, iv, Yn = rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy(), Y.cpu().numpy()
    ref = O.half_sweep(ip, ix, iv, X0, Yn, np.float32(reg), True, use_cg, rows=rows)
    got = X.cpu().numpy()[rows].astype(np.float64)
    err = np.linalg.norm(got - ref, axis=1)
    bar = (1e-3 if use_cg else 1e-4) * np.linalg.norm(ref, axis=1) + 1e-6
    bad = np.nonzero(err > bar)[0]
    assert bad.size == 0, [(int(rows[m]), float(err[m]), float(bar[m])) for m in bad[:8]]
