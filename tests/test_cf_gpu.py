"""UserCF / ItemCF on the device against the numpy restatement (tests/cf_oracle.py): the similarity CSR bit for bit,
top-k, recommend and predict, the model surface, `save_knn` and the oversize guard."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import ItemCF, UserCF
from librecommender_amd.bases.cf_base import _DeviceCsr
from librecommender_amd.data import DatasetPure, split_by_ratio_chrono
from librecommender_amd.evaluation import evaluate
from librecommender_amd.serving import save_knn

from . import cf_oracle as O

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(__file__), "golden", "sample_movielens_rating.dat")


def random_csr(n_rows, n_cols, nnz, seed, integer=True, zipf=False):
    rng = np.random.default_rng(seed)
    if zipf:
        r = np.minimum(rng.zipf(1.3, nnz) - 1, n_rows - 1)
        c = np.minimum(rng.zipf(1.3, nnz) - 1, n_cols - 1)
    else:
        r, c = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    key = np.unique(r.astype(np.int64) * n_cols + c)
    v = rng.integers(1, 6, key.size).astype(np.float32) if integer else rng.standard_normal(key.size).astype(np.float32)
    m = sp.csr_matrix((v, (key // n_cols, key % n_cols)), shape=(n_rows, n_cols), dtype=np.float32)
    m.sort_indices()
    return m


def device_sim(x, sim_type, min_common):
    """The model's own path (CfBase._similarity) on a host CSR x: rows are the x side."""
    dev = torch.device("cuda")
    X = _DeviceCsr.from_scipy(x, dev)
    m = UserCF.__new__(UserCF)
    m.sim_type, m.min_common = sim_type, min_common
    s = m._similarity(x, X, X.transpose())
    return s.ptr.cpu().numpy(), s.col.cpu().numpy(), s.val.cpu().numpy()


def assert_sim_equal(x, sim_type, min_common):
    ptr, col, val = device_sim(x, sim_type, min_common)
    ref = O.similarity(x, sim_type, min_common)
    assert np.array_equal(ptr, ref.indptr.astype(np.int64))
    assert np.array_equal(col, ref.indices)
    assert np.array_equal(val.view(np.uint32), ref.data.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("side", ["item_cf", "user_cf"])
@pytest.mark.parametrize("sim_type", ["cosine", "pearson", "jaccard"])
@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("integer", [True, False])
def test_similarity_bitwise(dev, side, sim_type, min_common, integer):
    ui = random_csr(300, 200, 6000, seed=1, integer=integer)
    x = ui if side == "user_cf" else ui.T.tocsr()
    x.sort_indices()
    assert_sim_equal(x, sim_type, min_common)


def test_similarity_explicit_zero_labels_and_empty_rows(dev):
    x = random_csr(150, 90, 2500, seed=2)
    x.data[::7] = 0.0                      # stored zeros still co-occur
    for st in ("cosine", "pearson", "jaccard"):
        assert_sim_equal(x, st, 1)
    rows = np.full(151, 0, dtype=np.int64)
    rows[1:] = np.where(np.arange(150) < 140, np.diff(x.indptr), 0).cumsum()
    keep = np.concatenate([np.arange(x.indptr[r], x.indptr[r + 1]) for r in range(140)])
    x2 = sp.csr_matrix((x.data[keep], x.indices[keep], rows), shape=(150, 90))   # 10 rows of zero degree
    assert_sim_equal(x2, "cosine", 1)


def test_pearson_exact_zero_entries_dropped(dev):
    # rows 0 / 1 share y 0, 1 with centred products +1 and -1: the pair sums to exactly 0 and is dropped
    x = sp.csr_matrix(np.array([[1, 3, 0, 0], [3, 3, 1, 5], [1, 1, 0, 2]], dtype=np.float32))
    ref = O.similarity(x, "pearson")
    ptr, col, val = device_sim(x, "pearson", 1)
    assert np.array_equal(col, ref.indices) and np.array_equal(val, ref.data) and np.array_equal(ptr, ref.indptr)


def test_hard_shapes_sampled_rows(dev):
    T = ops.cf_sim_tile_cols()
    n_x = 2 * T + 1500                      # more than two LDS tiles
    rng = np.random.default_rng(5)
    n_y = 400
    r, c = rng.integers(0, n_x, 60000), rng.integers(0, n_y, 60000)
    r = np.concatenate([r, np.arange(11000)])                            # y 0 gets degree >= 10 K
    c = np.concatenate([c, np.zeros(11000, dtype=np.int64)])
    key = np.unique(r.astype(np.int64) * n_y + c)
    v = rng.integers(1, 6, key.size).astype(np.float32)
    x = sp.csr_matrix((v, (key // n_y, key % n_y)), shape=(n_x + 7, n_y))   # 7 trailing zero-degree rows
    x.sort_indices()
    assert np.diff(x.T.tocsr().indptr).max() >= 10000
    sample = [0, 1, 2, 7, T - 1, T, 2 * T + 3, n_x - 1, n_x + 3] + rng.integers(0, n_x, 12).tolist()
    for st in ("cosine", "pearson", "jaccard"):
        ptr, col, val = device_sim(x, st, 2)
        ref = O.similarity_rows(x, st, 2, rows=sample)
        for r_ in sample:
            c_, v_ = ref[r_]
            got_c = col[ptr[r_]:ptr[r_ + 1]]
            assert np.array_equal(got_c, c_), (st, r_, len(got_c), len(c_), np.setdiff1d(c_, got_c)[:10],
                                               np.setdiff1d(got_c, c_)[:10])
            assert np.array_equal(val[ptr[r_]:ptr[r_ + 1]].view(np.uint32), v_.view(np.uint32)), (st, r_)


def test_similarity_deterministic(dev):
    x = random_csr(500, 300, 20000, seed=9, zipf=True)
    a = device_sim(x, "cosine", 1)
    b = device_sim(x, "cosine", 1)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("k", [1, 20, 10_000])
def test_topk(dev, k):
    x = random_csr(400, 120, 5000, seed=3)
    sim = O.similarity(x, "pearson")          # negative values included
    sim.data[::5] = np.round(sim.data[::5], 1)   # ties
    S = _DeviceCsr.from_scipy(sim, torch.device("cuda"))
    ids, sims, lens = (t.cpu().numpy() for t in ops.cf_topk(S.ptr, S.col, S.val, k))
    ref = O.topk(sim, k)
    for r in range(sim.shape[0]):
        got = None if lens[r] == 0 else list(zip(ids[r, :lens[r]].tolist(), sims[r, :lens[r]].tolist()))
        assert got == ref[r], r


@pytest.fixture(scope="module")
def movielens():
    df = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    train, evald = split_by_ratio_chrono(df, test_size=0.2)
    train_data, info = DatasetPure.build_trainset(train)
    eval_data = DatasetPure.build_evalset(evald)
    return df, train, evald, train_data, eval_data, info


def _check_recs(model, info, n_rec, filter_consumed):
    users = list(range(info.n_users))
    ui = model.user_interaction
    tk = O.topk(model.sim_matrix, model.k_sim)
    got = model._recommend_batch(users, n_rec, filter_consumed, False)
    ids, scs, lens, ncand, fb = (t.cpu().numpy() for t in ops.cf_recommend(
        torch.tensor(users, dtype=torch.int32, device="cuda"), model.cf_type == "user_cf", *[
            getattr(model._device("user"), a) for a in ("ptr", "col", "val")], *model._topk(), info.n_items,
        *model._consumed_csr(users, torch.device("cuda")), filter_consumed, n_rec))
    n_fallback = 0
    for u in users:
        kind, rid, rsc = O.recommend(model.cf_type, ui, tk, u, n_rec, info.user_consumed[u], filter_consumed)
        assert fb[u] == kind, u
        if kind:
            n_fallback += 1
            continue
        gsc = scs[u, :lens[u]]
        assert lens[u] == len(rid)
        assert np.array_equal(gsc.view(np.uint32), rsc.view(np.uint32)), u
        assert np.array_equal(got[u], rid)     # ties broken by ascending id on both sides
    return n_fallback


@pytest.mark.parametrize("cls", [ItemCF, UserCF])
@pytest.mark.parametrize("task", ["rating", "ranking"])
def test_recommend_and_predict(dev, movielens, cls, task):
    df, train, evald, train_data, eval_data, info = movielens
    model = cls(task, info, sim_type="cosine", k_sim=20)
    model.fit(train_data, neg_sampling=task == "ranking", verbose=0)
    x = model.user_interaction if cls is UserCF else model.item_interaction
    ref = O.similarity(x, "cosine")
    assert np.array_equal(model.sim_matrix.indices, ref.indices) and np.array_equal(model.sim_matrix.data, ref.data)
    for filt in (True, False):
        _check_recs(model, info, 10, filt)
    _check_recs(model, info, info.n_items + 5, True)          # n_rec above the candidate count
    # fallback users come from popular_recommendations in order
    recs = model.recommend_user(user=[info.id2user[0], "unknown-user"], n_rec=5)
    assert len(recs["unknown-user"]) == 5
    # predict against the restatement
    rng = np.random.default_rng(0)
    us, its = rng.integers(0, info.n_users, 3000), rng.integers(0, info.n_items, 3000)
    got = model.predict(us, its, inner_id=True)
    sim, inter = model.sim_matrix, (model.item_interaction if cls is UserCF else model.user_interaction)
    n_default = 0
    for q in range(len(us)):
        s_row, i_row = (us[q], its[q]) if cls is UserCF else (its[q], us[q])
        want, none = O.predict(sim, inter, s_row, i_row, model.k_sim, task, model.lower_bound if task == "rating" else 0,
                               model.upper_bound if task == "rating" else 0, model.default_pred)
        n_default += none
        assert np.isclose(got[q], want, rtol=1e-6, atol=0), q
    assert 0 < n_default < len(us)
    unk = model.predict(np.array([info.n_users, 0]), np.array([0, info.n_items]), inner_id=True)
    assert np.all(unk == np.float32(model.default_pred))
    with pytest.raises(ValueError):
        model.predict(np.array([info.n_users]), np.array([0]), inner_id=True, cold_start="average")


@pytest.mark.parametrize("cls", [ItemCF, UserCF])
def test_model_surface(dev, movielens, tmp_path, cls):
    df, train, evald, train_data, eval_data, info = movielens
    model = cls("rating", info, sim_type="pearson", k_sim=15, min_common=2)
    model.fit(train_data, neg_sampling=False, verbose=0)
    res = evaluate(model, eval_data, neg_sampling=False, metrics=["rmse"], k=10)
    assert np.isfinite(res["rmse"]) and res["rmse"] < 2.0, res
    ranker = cls("ranking", info, k_sim=15)
    ranker.fit(train_data, neg_sampling=True, verbose=0)
    res = evaluate(ranker, DatasetPure.build_evalset(evald), neg_sampling=True, metrics=["precision", "ndcg"], k=10)
    assert all(np.isfinite(v) and v > 0 for v in res.values()), res
    model.save(str(tmp_path), "cf")
    x = model.user_interaction if cls is UserCF else model.item_interaction
    ref = O.similarity(x, "pearson", 2)
    loaded_sim = sp.load_npz(os.path.join(tmp_path, "cf_sim_matrix.npz"))
    assert (loaded_sim != ref).nnz == 0 and np.array_equal(loaded_sim.indices, ref.indices)
    ui = train_data.sparse_interaction
    got_ui = sp.load_npz(os.path.join(tmp_path, "cf_user_inter.npz"))
    assert got_ui.shape == (info.n_users, info.n_items)
    assert (got_ui[: ui.shape[0], : ui.shape[1]] != ui).nnz == 0
    assert (sp.load_npz(os.path.join(tmp_path, "cf_item_inter.npz")) != got_ui.T.tocsr()).nnz == 0
    loaded = cls.load(str(tmp_path), "cf", info)
    users = list(range(0, info.n_users, 7))
    info.np_rng = np.random.default_rng(0)
    a = model.recommend_user(user=users, n_rec=10, inner_id=True)
    info.np_rng = np.random.default_rng(0)
    b = loaded.recommend_user(user=users, n_rec=10, inner_id=True)
    assert all(np.array_equal(a[u], b[u]) for u in users)
    us, its = np.arange(info.n_users) % info.n_users, np.arange(info.n_users) % info.n_items
    assert np.array_equal(model.predict(us, its, inner_id=True), loaded.predict(us, its, inner_id=True))
    with pytest.raises(NotImplementedError):
        loaded.rebuild_model(str(tmp_path), "cf")
    # save_knn
    save_knn(str(tmp_path / "knn"), model, 10)
    with open(tmp_path / "knn" / "sim.json") as f:
        assert json.load(f) == O.save_sim_matrix(ref, 10)
    assert os.path.exists(tmp_path / "knn" / "user_consumed.json")


def test_fit_twice_identical_bytes(dev, movielens):
    *_, train_data, _, info = movielens
    a, b = ItemCF("ranking", info), ItemCF("ranking", info)
    a.fit(train_data, neg_sampling=True, verbose=0)
    b.fit(train_data, neg_sampling=True, verbose=0)
    for n in ("indptr", "indices", "data"):
        assert getattr(a.sim_matrix, n).tobytes() == getattr(b.sim_matrix, n).tobytes()


def test_multi_rank_fit_raises(dev, movielens, monkeypatch):
    *_, train_data, _, info = movielens
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        UserCF("ranking", info).fit(train_data, neg_sampling=True, verbose=0)


def test_oversize_result_raises_before_allocating(dev, movielens, monkeypatch):
    *_, train_data, _, info = movielens
    monkeypatch.setattr(ops, "CF_SIM_MAX_BYTES", 4096)
    with pytest.raises(MemoryError, match="similarity matrix"):
        ItemCF("ranking", info).fit(train_data, neg_sampling=True, verbose=0)
