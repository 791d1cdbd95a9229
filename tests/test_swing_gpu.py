"""Swing on the device against the numpy restatement (tests/swing_oracle.py): the score CSR (exact pattern, every entry
within (P + 16) * 2^-24 relative of the fp64 sum of its P pairs, bit-symmetric, bit-identical run to run), top-k, recommend
and predict on the device's own scores, the model surface with save / load, the retrain flow and the oversize guard.

The bound is derived, not measured: all terms are positive, so an f32 sum of P terms in any order is within (P - 1) * 2^-24
relative to first order, and each term carries at most eight correctly rounded operations (two sqrt, two reciprocals, one
add, one reciprocal, two products); 16 instead of 8 covers the second-order terms.
"""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import Swing
from librecommender_amd.bases.cf_base import _DeviceCsr
from librecommender_amd.data import DataInfo, DatasetPure, split_by_ratio_chrono
from librecommender_amd.evaluation import evaluate

from . import swing_oracle as O

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(__file__), "golden", "sample_movielens_rating.dat")
EPS = 2.0 ** -24


def random_csr(n_rows, n_cols, nnz, seed, zipf=False):
    rng = np.random.default_rng(seed)
    if zipf:
        r = np.minimum(rng.zipf(1.3, nnz) - 1, n_rows - 1)
        c = np.minimum(rng.zipf(1.3, nnz) - 1, n_cols - 1)
    else:
        r, c = rng.integers(0, n_rows, nnz), rng.integers(0, n_cols, nnz)
    key = np.unique(r.astype(np.int64) * n_cols + c)
    v = rng.integers(1, 6, key.size).astype(np.float32)
    m = sp.csr_matrix((v, (key // n_cols, key % n_cols)), shape=(n_rows, n_cols), dtype=np.float32)
    m.sort_indices()
    return m


def _with_rows(base, extra_rows):
    m = sp.vstack([base] + [sp.csr_matrix((np.ones(len(c), dtype=np.float32), (np.zeros(len(c), dtype=np.int64), c)),
                                          shape=(1, base.shape[1])) for c in extra_rows]).tocsr()
    m.sort_indices()
    return m


def _heavy_user():
    rng = np.random.default_rng(5)
    return _with_rows(random_csr(200, 12000, 6000, seed=5), [rng.choice(12000, 10500, replace=False)])


def _heavy_items():
    rng = np.random.default_rng(6)
    base = random_csr(40, 5000, 3000, seed=6).tolil()
    base[0, rng.choice(5000, 4500, replace=False)] = 1.0       # two items that share more users than a wave keeps in LDS
    base[1, rng.choice(5000, 4200, replace=False)] = 1.0
    m = base.tocsr().T.tocsr()
    m.sort_indices()
    return m


CASES = {
    "uniform": lambda: random_csr(300, 200, 6000, seed=1),
    "uniform_small": lambda: random_csr(150, 90, 2500, seed=2),
    "zipf": lambda: random_csr(500, 300, 20000, seed=9, zipf=True),
    "three_user_tiles": lambda: random_csr(17000, 120, 40000, seed=3),      # users beyond two 8,192-column tiles
    "three_item_tiles": lambda: random_csr(300, 17000, 30000, seed=4),      # items beyond two 8,192-column tiles
    "user_with_10k_items": _heavy_user,
    "items_with_4k_users": _heavy_items,
}


def device_scores(A, alpha, prev=None):
    dev = torch.device("cuda")
    U = _DeviceCsr.from_scipy(A, dev)
    I = U.transpose()
    p = None
    if prev is not None:
        P = _DeviceCsr.from_scipy(sp.csr_matrix(prev, dtype=np.float32), dev)
        p = (P.ptr, P.col, P.val)
    ptr, col, val = ops.swing_scores(U.ptr, U.col, I.ptr, I.col, alpha, prev=p)
    n = A.shape[1]
    return sp.csr_matrix((val.cpu().numpy(), col.cpu().numpy(), ptr.cpu().numpy()), shape=(n, n))


def assert_scores(S, A, alpha, prev=None, extra_terms=0):
    ref = O.scores64(A, alpha, prev=prev)
    assert np.array_equal(S.indptr, ref.indptr) and np.array_equal(S.indices, ref.indices)     # the exact pattern
    assert S.dtype == np.float32
    P = O.pairs(A)
    if prev is None:
        assert np.array_equal(P.indptr, ref.indptr) and np.array_equal(P.indices, ref.indices)
    # the pairs of every entry of the result (none for an entry that only the previous scores hold)
    rows = np.repeat(np.arange(ref.shape[0]), np.diff(ref.indptr))
    P = sp.csr_matrix((np.asarray(P[rows, ref.indices]).ravel(), ref.indices, ref.indptr), shape=ref.shape)
    assert prev is not None or P.data.min(initial=1) >= 1
    err = np.abs(S.data.astype(np.float64) - ref.data)
    bound = (P.data + extra_terms + 16) * EPS * ref.data
    worst = float((err / bound).max()) if ref.nnz else 0.0
    print(f"entries {ref.nnz}, largest P {P.data.max() if ref.nnz else 0:.0f}, largest error / bound {worst:.3f}")
    assert np.all(err <= bound), (worst, int(np.argmax(err / bound)))     # every entry
    T = S.T.tocsr()
    T.sort_indices()
    assert np.array_equal(T.indices, S.indices) and T.data.tobytes() == S.data.tobytes()       # s == s.T bit for bit


@pytest.mark.parametrize("alpha", [1.0, 0.7, 5.0])
@pytest.mark.parametrize("case", ["uniform", "uniform_small", "zipf"])
def test_scores(dev, case, alpha):
    A = CASES[case]()
    assert_scores(device_scores(A, alpha), A, alpha)


@pytest.mark.parametrize("case", ["three_user_tiles", "three_item_tiles", "user_with_10k_items", "items_with_4k_users"])
def test_scores_large_shapes(dev, case):
    A = CASES[case]()
    if case == "user_with_10k_items":
        assert np.diff(A.indptr).max() >= 10000
    if case == "items_with_4k_users":
        deg = np.sort(np.diff(A.T.tocsr().indptr))
        assert deg[-2] >= 4000 and (A.T @ A).tocsr()[0, 1] > ops._lib.load().lr_swing_lds_users()
    assert_scores(device_scores(A, 0.7), A, 0.7)


def test_known_answer(dev):
    A = sp.csr_matrix(np.array([[1, 1, 1, 1, 0], [1, 1, 0, 1, 0], [1, 0, 1, 1, 1]], dtype=np.float32))
    S = device_scores(A, 1.0)
    R, P = O.scores32_ref(A, 1.0), O.pairs(A).toarray()
    assert np.array_equal(S.toarray()[P <= 2], R[P <= 2])        # one or two pairs: no order to differ in
    assert np.allclose(S.toarray(), R, rtol=4 * EPS, atol=0)     # three pairs: (a + c) + b against (a + b) + c
    assert_scores(S, A, 1.0)


def test_edge_shapes(dev):
    # an empty user, users with one item (alpha + 0), items with one user, ids beyond the last one seen
    A = sp.csr_matrix(np.array([[1, 1, 0, 0, 0, 0, 0],
                                [0, 0, 0, 0, 0, 0, 0],
                                [1, 1, 1, 0, 0, 0, 0],
                                [0, 0, 0, 1, 0, 0, 0],
                                [1, 0, 0, 0, 1, 0, 0],
                                [0, 0, 0, 0, 0, 0, 0],
                                [0, 0, 0, 0, 0, 0, 0]], dtype=np.float32))
    S = device_scores(A, 0.7)
    assert_scores(S, A, 0.7)
    assert S[3].nnz == 0 and S[5].nnz == 0 and S[0, 1] > 0 and S[0, 2] == 0
    B = sp.csr_matrix(np.array([[1, 1], [1, 1], [1, 1]], dtype=np.float32))     # c_uv = 2 for every pair
    assert_scores(device_scores(B, 0.25), B, 0.25)
    empty = sp.csr_matrix((4, 6), dtype=np.float32)
    assert device_scores(empty, 1.0).nnz == 0
    single = sp.csr_matrix(np.eye(5, dtype=np.float32))                          # no pair at all
    assert device_scores(single, 1.0).nnz == 0


def test_deterministic(dev):
    A = CASES["zipf"]()
    a, b = device_scores(A, 1.0), device_scores(A, 1.0)
    for n in ("indptr", "indices", "data"):
        assert getattr(a, n).tobytes() == getattr(b, n).tobytes()


def test_previous_scores_are_added(dev):
    A = CASES["uniform_small"]()
    first = A.copy()
    first.data[first.indptr[75]:] = 0
    first.eliminate_zeros()
    second = A.copy()
    second.data[: second.indptr[75]] = 0
    second.eliminate_zeros()
    prev = device_scores(first[:, :80], 1.0)                    # fewer items than the new data
    S = device_scores(second, 1.0, prev=prev)
    assert_scores(S, second, 1.0, prev=prev, extra_terms=1)


@pytest.fixture(scope="module")
def movielens():
    df = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    train, evald = split_by_ratio_chrono(df, test_size=0.2)
    train_data, info = DatasetPure.build_trainset(train)
    eval_data = DatasetPure.build_evalset(evald)
    return df, train, evald, train_data, eval_data, info


@pytest.fixture(scope="module")
def fitted(movielens):
    *_, train_data, eval_data, info = movielens
    model = Swing("ranking", info, top_k=20, alpha=1.0)
    model.fit(train_data, neg_sampling=True, verbose=2, eval_data=eval_data, metrics=["roc_auc", "precision", "ndcg"],
              k=10, eval_user_num=200)
    return model


def test_model_scores(dev, movielens, fitted):
    *_, train_data, _, info = movielens
    A = fitted.user_interaction
    assert A.shape == (info.n_users, info.n_items)
    assert_scores(fitted.sim_matrix, A, 1.0)
    again = Swing("ranking", info)
    again.fit(train_data, neg_sampling=True, verbose=0)
    assert again.sim_matrix.data.tobytes() == fitted.sim_matrix.data.tobytes()


@pytest.mark.parametrize("k", [1, 20, 10_000])
def test_topk_on_device_scores(dev, fitted, k):
    S = fitted.sim_matrix
    D = fitted._device("sim")
    ids, sims, lens = (t.cpu().numpy() for t in ops.cf_topk(D.ptr, D.col, D.val, k))
    ref = O.topk(S, k)
    ties = 0
    for r in range(S.shape[0]):
        got = list(zip(ids[r, :lens[r]].tolist(), sims[r, :lens[r]]))
        assert [g[0] for g in got] == [w[0] for w in ref[r]], r
        assert all(g[1] == w[1] for g, w in zip(got, ref[r])), r
        ties += len({w[1] for w in ref[r]}) < len(ref[r])
    assert k == 1 or ties > 0                                    # ties are common in Swing: the order by id is exercised


@pytest.mark.parametrize("filter_consumed", [True, False])
@pytest.mark.parametrize("n_rec", [10, 4000])
def test_recommend_on_device_scores(dev, movielens, fitted, filter_consumed, n_rec):
    info = movielens[-1]
    S, A = fitted.sim_matrix, fitted.user_interaction
    tk = O.topk(S, fitted.top_k)
    users = list(range(0, info.n_users, 3))
    got = fitted._recommend_batch(users, n_rec, filter_consumed, False)
    popular = {info.item2id[i] for i in info.popular_items}
    padded = 0
    for u, rec in zip(users, got):
        want, pad, _ = O.recommend(S, A, info.user_consumed[u], u, n_rec, fitted.top_k, filter_consumed, tk=tk)
        assert len(rec) == n_rec
        assert rec[: len(want)].tolist() == want, u             # (score descending, id ascending) on both sides
        assert set(rec[len(want):].tolist()) <= popular          # the shortfall comes from the popular items
        padded += pad > 0
    assert n_rec != 4000 or padded > 0


def test_predict_on_device_scores(dev, movielens, fitted):
    info = movielens[-1]
    S, A = fitted.sim_matrix, fitted.user_interaction
    rng = np.random.default_rng(0)
    us, its = rng.integers(0, info.n_users, 3000), rng.integers(0, info.n_items, 3000)
    heavy = np.argsort(-np.diff(A.indptr))[:20]                 # users with many items meet the top-k cut
    us[:600] = np.repeat(heavy, 30)
    got = fitted.predict(us, its, inner_id=True)
    n_default = 0
    for q in range(len(us)):
        want = O.predict(S, A, us[q], its[q], fitted.top_k, fitted.default_pred)
        n_default += want == 0
        assert np.isclose(got[q], want, rtol=1e-6, atol=0), q
    assert 0 < n_default < len(us)
    # the cut to top_k comes before the intersection: with the whole row some of these would differ
    full = [O.predict(S, A, us[q], its[q], 10 ** 9) for q in range(600)]
    assert any(not np.isclose(f, g, rtol=1e-6) for f, g in zip(full, got[:600]))
    unk = fitted.predict(np.array([info.n_users, 0]), np.array([0, info.n_items]), inner_id=True)
    assert np.all(unk == np.float32(fitted.default_pred))
    assert isinstance(float(fitted.predict(0, 0, inner_id=True)), float)


def test_model_surface(dev, movielens, fitted, tmp_path):
    df, train, evald, train_data, eval_data, info = movielens
    res = evaluate(fitted, eval_data, neg_sampling=True, metrics=["roc_auc", "precision", "ndcg"], k=10, seed=2222)
    assert all(np.isfinite(v) and v > 0 for v in res.values()), res
    user, item = df.user.iloc[0], df.item.iloc[0]
    assert fitted.predict(user=user, item=item) >= 0
    assert np.allclose(fitted.predict(user="cold user2", item="cold item2", cold_start="popular"), fitted.default_pred)
    assert fitted.predict(user="cold user1", item="cold item2") == fitted.predict(user="cold user2", item="cold item2")
    with pytest.raises(ValueError):
        fitted.predict(user="cold user1", item="cold item2", cold_start="other")
    recs = fitted.recommend_user(user=[user, "cold user1"], n_rec=7)
    assert len(recs[user]) == 7 and len(recs["cold user1"]) == 7
    assert set(recs["cold user1"]) <= set(info.popular_items)
    with pytest.raises(ValueError):
        fitted.recommend_user(user="cold user1", n_rec=7, cold_start="other")
    with pytest.raises(TypeError):
        fitted.recommend_user(1, 7, seq=[1, 2, 3])
    rnd = fitted.recommend_user(user, 10, random_rec=True)[user]
    all_cand = O.recommend(fitted.sim_matrix, fitted.user_interaction, info.user_consumed[info.user2id[user]],
                           info.user2id[user], 10, fitted.top_k)[2]
    assert len(rnd) == 10 and len(set(rnd)) == 10 and {info.item2id[i] for i in rnd} <= set(all_cand)
    # save / load
    fitted.save(str(tmp_path / "new_folder"), "swing")
    for part in ("hyper_parameters.json", "swing_scores.npz", "user_inter.npz", "item_inter.npz"):
        assert os.path.exists(tmp_path / "new_folder" / f"swing_{part}")
    loaded = Swing.load(str(tmp_path / "new_folder"), "swing", info)
    assert (loaded.top_k, loaded.alpha) == (fitted.top_k, fitted.alpha)
    users = list(range(0, info.n_users, 7))
    info.np_rng = np.random.default_rng(0)
    a = fitted.recommend_user(user=users, n_rec=10, inner_id=True)
    info.np_rng = np.random.default_rng(0)
    b = loaded.recommend_user(user=users, n_rec=10, inner_id=True)
    assert all(np.array_equal(a[u], b[u]) for u in users)
    us, its = np.arange(info.n_users) % info.n_users, np.arange(info.n_users) % info.n_items
    assert np.array_equal(fitted.predict(us, its, inner_id=True), loaded.predict(us, its, inner_id=True))


def test_all_consumed_and_cold_start(dev, movielens):
    *_, train_data, _, info = movielens
    model = Swing("ranking", info)
    model.fit(train_data, neg_sampling=True, verbose=0)
    u = 1
    saved = info.user_consumed[u]
    try:
        info.user_consumed[u] = list(range(info.n_items))
        model._consumed_index = None
        recos = model.recommend_user(user=u, n_rec=7, inner_id=True)
    finally:
        info.user_consumed[u] = saved
        model._consumed_index = None
    assert len(recos[u]) == 7 and np.all(np.isin(recos[u], [info.item2id[i] for i in info.popular_items]))


def test_retrain(dev, tmp_path):
    all_data = pd.read_csv(DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    first_half = all_data[: len(all_data) // 2]
    train, evald = split_by_ratio_chrono(first_half, test_size=0.2)
    train_data, info = DatasetPure.build_trainset(train)
    eval_data = DatasetPure.build_evalset(evald)
    model = Swing("ranking", info, top_k=20, alpha=1.0, num_threads=2)
    model.fit(train_data, neg_sampling=True, verbose=2, eval_data=eval_data, metrics=["roc_auc", "precision"])
    first = evaluate(model, eval_data, neg_sampling=True, metrics=["roc_auc", "precision"], k=10, seed=2222)
    info.save(str(tmp_path), "swing_model")
    model.save(str(tmp_path), "swing_model")
    old_scores, old_user = model.sim_matrix.copy(), model.user_interaction.copy()

    new_info = DataInfo.load(str(tmp_path), "swing_model")
    second = all_data[len(all_data) // 2: len(all_data) * 3 // 4]
    train2, eval2 = split_by_ratio_chrono(second, test_size=0.2)
    train_data2, new_info = DatasetPure.merge_trainset(train2, new_info, merge_behavior=True)
    eval_data2 = DatasetPure.merge_evalset(eval2, new_info)
    new_model = Swing("ranking", new_info, top_k=20, alpha=1.0)
    new_model.rebuild_model(str(tmp_path), "swing_model")
    assert new_model.incremental and new_model.n_items >= model.n_items
    new_model.fit(train_data2, neg_sampling=True, verbose=2, eval_data=eval_data2, metrics=["roc_auc", "precision"])

    shape = (new_info.n_users, new_info.n_items)
    new_inter = sp.csr_matrix(train_data2.sparse_interaction)
    new_inter.resize(shape)
    assert_scores(new_model.sim_matrix, new_inter, 1.0, prev=old_scores, extra_terms=1)
    merged = O.merge(old_user, new_inter)
    merged.resize(shape)
    assert (new_model.user_interaction != merged).nnz == 0
    assert (new_model.item_interaction != merged.T.tocsr()).nnz == 0
    lonely = np.flatnonzero(np.diff(new_inter.T.tocsr().indptr)[: old_scores.shape[0]] == 0)
    assert len(lonely)                                           # items without new users keep their rows
    for i in lonely[:50]:
        assert np.array_equal(new_model.sim_matrix[i].indices, old_scores[i].indices)
        assert np.array_equal(new_model.sim_matrix[i].data, old_scores[i].data)
    user, item = second.user.iloc[0], second.item.iloc[0]
    assert new_model.predict(user=user, item=item) >= 0
    assert len(new_model.recommend_user(user=user, n_rec=7)[user]) == 7
    again = evaluate(new_model, eval_data2, neg_sampling=True, metrics=["roc_auc", "precision"], k=10, seed=2222)
    assert again["roc_auc"] != first["roc_auc"]
    new_model.save(str(tmp_path), "swing_model")
    assert (Swing.load(str(tmp_path), "swing_model", new_info).sim_matrix != new_model.sim_matrix).nnz == 0


def test_multi_rank_fit_raises(dev, movielens, monkeypatch):
    *_, train_data, _, info = movielens
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        Swing("ranking", info).fit(train_data, neg_sampling=True, verbose=0)


@pytest.mark.parametrize("cap, what", [(4096, "user-pair table"), (20_000_000, "similarity matrix")])
def test_oversize_raises_before_allocating(dev, movielens, monkeypatch, cap, what):
    *_, train_data, _, info = movielens
    monkeypatch.setattr(ops, "SWING_MAX_BYTES", cap)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(MemoryError, match=what):
        Swing("ranking", info).fit(train_data, neg_sampling=True, verbose=0)
    assert torch.cuda.max_memory_allocated() - before < cap + 16 * 2 ** 20     # plans and counts only, never the table
