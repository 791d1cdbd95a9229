"""UserCF / ItemCF without a GPU: the numpy restatement (tests/cf_oracle.py) against hand-computed answers and, where
the reference checkout exists, against the reference's own statistics and pure-Python top-k / recommend / predict; the
constructor's warnings and checks; the C-ABI's host-side queries."""
import inspect
import sys

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

from librecommender_amd import _lib
from librecommender_amd.algorithms import ItemCF, UserCF
from librecommender_amd.bases import cf_base
from librecommender_amd.data import DatasetPure
from oracle import ref_loader

from . import cf_oracle as O

needs_ref = pytest.mark.skipif(not ref_loader.available(), reason="reference checkout absent")


@pytest.fixture
def ref():
    saved = list(sys.path)
    ref_loader.load()
    yield
    sys.path[:] = saved


def small(n=400, seed=0, n_users=40, n_items=60):
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"user": rng.integers(0, n_users, n), "item": rng.integers(0, n_items, n),
                       "label": rng.integers(1, 6, n).astype(np.float32)})
    return DatasetPure.build_trainset(df)


X = sp.csr_matrix(np.array([[1, 2, 0, 0], [2, 0, 3, 0], [0, 4, 1, 1], [0, 0, 0, 0]], dtype=np.float32))


def test_known_answers_cosine_jaccard_pearson():
    s = O.similarity(X, "cosine").toarray()
    n = np.sqrt(np.array([5, 13, 18], dtype=np.float64)).astype(np.float32)
    assert s[0, 1] == np.float32(2) / (n[0] * n[1]) and s[0, 1] == s[1, 0]
    assert s[0, 2] == np.float32(8) / (n[0] * n[2]) and s[1, 2] == np.float32(3) / (n[1] * n[2])
    assert np.all(np.diag(s) == 0) and not s[3].any()
    j = O.similarity(X, "jaccard").toarray()
    assert j[0, 1] == np.float32(1) / np.float32(3) and j[1, 2] == np.float32(1) / np.float32(4)
    p = O.similarity(X, "pearson")
    # row 0: mean 1.5, centred (-.5, .5); row 1 (-.5, .5); shared y 0: .25; centred norms sqrt(.5)
    assert p[0, 1] == np.float32(0.25) / (np.float32(np.sqrt(0.5)) * np.float32(np.sqrt(0.5)))


def test_min_common_and_zero_dropping():
    assert O.similarity(X, "cosine", 2).nnz == 0
    z = sp.csr_matrix(np.array([[1, -1], [1, 1]], dtype=np.float32))     # prods 1 - 1 = 0: the pair is dropped
    assert O.similarity(z, "cosine").nnz == 0
    assert O.similarity(z, "jaccard").nnz == 2


def test_explicit_zero_labels_count():
    z = sp.csr_matrix((np.array([0, 2, 0, 3], dtype=np.float32), np.array([0, 1, 0, 1]), np.array([0, 2, 4])),
                      shape=(2, 2))
    j = O.similarity(z, "jaccard").toarray()
    assert j[0, 1] == 1.0
    c = O.similarity(z, "cosine").toarray()
    assert c[0, 1] == np.float32(6) / (np.float32(2) * np.float32(3))


def test_statistics_match_restatement():
    x = small()[0].sparse_interaction
    assert np.array_equal(cf_base.row_norm(x), O.stat_norm(x))
    assert np.array_equal(cf_base.row_mean(x), O.stat_mean(x), equal_nan=True)
    assert np.array_equal(cf_base.row_centred_norm(x), O.stat_centred_norm(x))


def test_constructor_warnings(capsys):
    _, info = small()
    ItemCF("ranking", info, sim_type="pearson")
    assert "pearson is not suitable for implicit data" in capsys.readouterr().out
    UserCF("rating", info, sim_type="jaccard")
    assert "jaccard is not suitable for explicit data" in capsys.readouterr().out


@pytest.mark.parametrize("cls", [ItemCF, UserCF])
@pytest.mark.parametrize("kw", [{"sim_type": "euclid"}, {"mode": "sideways"}])
def test_bad_sim_type_or_mode_raises_before_device_work(cls, kw):
    train, info = small()
    with pytest.raises(ValueError):
        cls("rating", info, **kw).fit(train, neg_sampling=False, verbose=0)


def test_rebuild_raises():
    _, info = small()
    with pytest.raises(NotImplementedError):
        ItemCF("rating", info).rebuild_model("x", "y")


def test_cabi_host_queries():
    lib = _lib.load()
    T = lib.lr_cf_sim_tile_cols()
    assert T >= 1024 and T & (T - 1) == 0
    assert lib.lr_cf_sim_ws_bytes() >= 4
    assert lib.lr_cf_select_max() >= 256
    assert lib.lr_cf_recommend_ws_bytes(3, 100) >= 3 * 100 * 5
    assert lib.lr_cf_recommend_ws_bytes(-1, 100) == 0
    for name in ("lr_cf_sim_f32", "lr_cf_topk_f32", "lr_cf_recommend_f32", "lr_cf_predict_f32"):
        assert name in _lib.SIGNATURES
    assert lib.lr_cf_topk_f32(None, None, None, 4, 0, None, None, None, None) == -1      # k < 1
    assert lib.lr_cf_sim_f32(*([None] * 6), 5, None, None, 7, 1, None, None, None, 1, 0, None, None, None, None,
                             None, 0, None) == -1                                          # bad sim_type


# ---- against the reference checkout -----------------------------------------------------------------------------------
@needs_ref
def test_statistics_bitwise_equal_reference(ref):
    from libreco.utils import similarities as S

    for seed in range(3):
        x = small(2000, seed)[0].sparse_interaction
        for m in (x, x.T.tocsr()):
            assert np.array_equal(S.compute_sparse_norm(m), O.stat_norm(m))
            assert np.array_equal(S.compute_sparse_mean(m), O.stat_mean(m), equal_nan=True)
            assert np.array_equal(S.compute_sparse_mean_centered_norm(m), O.stat_centred_norm(m))
            assert np.array_equal(S.compute_sparse_count(m), O.stat_count(m))


def _ref_model(name, task, info_ref, sim, user_inter, k_sim):
    import importlib

    mod = importlib.import_module(f"libreco.algorithms.{name.lower().replace('cf', '_cf')}")
    m = getattr(mod, name)(task, info_ref, k_sim=k_sim)
    m.sim_matrix = sim
    m.user_interaction = user_inter
    m.item_interaction = user_inter.T.tocsr()
    m.compute_top_k()
    return m


@needs_ref
@pytest.mark.parametrize("name", ["ItemCF", "UserCF"])
@pytest.mark.parametrize("task", ["rating", "ranking"])
def test_restatement_equals_reference_model(ref, name, task):
    from libreco.data import DatasetPure as RefDataset

    rng = np.random.default_rng(4)
    df = pd.DataFrame({"user": rng.integers(0, 50, 700), "item": rng.integers(0, 70, 700),
                       "label": rng.integers(1, 6, 700).astype(np.float32)})
    df = df.drop_duplicates(["user", "item"], keep="last")
    train, info = RefDataset.build_trainset(df)
    ui = train.sparse_interaction.tocsr()
    ui.sort_indices()
    x = ui if name == "UserCF" else ui.T.tocsr()
    sim = O.similarity(x, "cosine", 1)
    k_sim = 7
    m = _ref_model(name, task, info, sim, ui, k_sim)
    tk = O.topk(sim, k_sim)
    assert all(m.topk_sim[i] == tk[i] for i in tk)
    cf_type = "user_cf" if name == "UserCF" else "item_cf"
    seed_state = np.random.default_rng(11)
    info.np_rng = np.random.default_rng(11)
    for u in range(info.n_users):
        for filt in (True, False):
            got = m.recommend_one(u, 10, filt, False)
            kind, ids, scores = O.recommend(cf_type, ui, tk, u, 10, info.user_consumed[u], filt)
            if kind:
                want = np.array([info.item2id[i] for i in seed_state.choice(info.popular_items, 10)])
                assert np.array_equal(got, want)
                continue
            sc = O.recommend_scores(cf_type, ui, tk, u)
            ref_scores = np.array([sc[i] for i in got], dtype=np.float32)
            assert np.array_equal(np.sort(ref_scores)[::-1], ref_scores)         # the reference's order by score
            assert np.array_equal(np.sort(got), np.sort(ids)) or len(got) == 10
            assert np.array_equal(ref_scores, scores)
    rng = np.random.default_rng(1)
    us, its = rng.integers(0, info.n_users, 300), rng.integers(0, info.n_items, 300)
    preds = m.predict(us, its, inner_id=True)
    inter = ui if name == "ItemCF" else ui.T.tocsr()
    lo, hi = (info.min_max_rating if task == "rating" else (0, 0))
    for q in range(len(us)):
        s_row, i_row = (its[q], us[q]) if name == "ItemCF" else (us[q], its[q])
        want, _ = O.predict(sim, inter, s_row, i_row, k_sim, task, lo, hi, m.default_pred)
        assert np.float32(preds[q]) == np.float32(want)


@needs_ref
@pytest.mark.parametrize("name", ["ItemCF", "UserCF"])
def test_signatures_match_reference(ref, name):
    import importlib

    mine = {"ItemCF": ItemCF, "UserCF": UserCF}[name]
    theirs = getattr(importlib.import_module(f"libreco.algorithms.{name.lower().replace('cf', '_cf')}"), name)
    for meth in ("__init__", "fit", "predict", "recommend_user", "save", "load", "rebuild_model"):
        a, b = inspect.signature(getattr(mine, meth)), inspect.signature(getattr(theirs, meth))
        assert list(a.parameters) == list(b.parameters), meth
        assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()], meth
