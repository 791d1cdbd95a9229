"""`DynEmbedBase` (bases/dyn_embed_base.py) on a stub `data_info`: the four models derive from it and own neither the id
conversion nor the dynamic branch of `recommend_user`; `convert_array_id`; the sequence window under the three fallbacks; the
rejection of `user_feats` by the models without user features; and `DenseParams.take_over` on the CPU device.  No device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from librecommender_amd.algorithms import RNN4Rec, TwoTower, WaveNet, YouTubeRetrieval
from librecommender_amd.bases import DynEmbedBase, EmbedBase
from librecommender_amd.layers.dense import DenseParams

L, N = 4, 6
_NO_COLS = SimpleNamespace(name=[], index=[])


class _Info:
    global_mean, min_max_rating = 3.0, (1, 5)
    n_users, n_items = 3, N
    user_consumed = {0: [0, 1, 2, 3, 4, 5], 1: [3], 2: []}
    user2id = {"a": 0, "b": 1, "c": 2}
    item2id = {10 * (i + 1): i for i in range(N)}            # raw 10, 20, .. 60 -> 0 .. 5
    item_col = []
    user_sparse_col = user_dense_col = item_sparse_col = item_dense_col = _NO_COLS
    user_sparse_unique = user_dense_unique = None


MODELS = {"RNN4Rec": lambda: RNN4Rec("ranking", _Info(), recent_num=L),
          "WaveNet": lambda: WaveNet("ranking", _Info(), recent_num=L),
          "YouTubeRetrieval": lambda: YouTubeRetrieval("ranking", _Info(), recent_num=L),
          "TwoTower": lambda: TwoTower("ranking", _Info())}
WINDOWED = ("RNN4Rec", "WaveNet", "YouTubeRetrieval")


# ---- class structure ------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [RNN4Rec, WaveNet, YouTubeRetrieval, TwoTower], ids=lambda c: c.__name__)
def test_models_derive_from_the_base_and_own_no_copy(cls):
    assert issubclass(cls, DynEmbedBase) and issubclass(DynEmbedBase, EmbedBase)
    assert "convert_array_id" not in vars(cls)
    assert "recommend_user" not in vars(cls)
    assert cls.convert_array_id is DynEmbedBase.convert_array_id
    assert cls.recommend_user is DynEmbedBase.recommend_user
    assert "dyn_user_embedding" in vars(cls)                  # the model's one call into its net


def test_only_the_models_without_user_features_reject_them():
    flags = {name: type(make()).__dict__.get("takes_user_feats", DynEmbedBase.takes_user_feats) for name, make in MODELS.items()}
    assert flags == {"RNN4Rec": False, "WaveNet": False, "YouTubeRetrieval": True, "TwoTower": True}


# ---- convert_array_id -----------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_convert_array_id(name):
    m = MODELS[name]()
    n = m.n_users
    np.testing.assert_array_equal(m.convert_array_id("b", False), [1])
    np.testing.assert_array_equal(m.convert_array_id("nobody", False), [n])
    np.testing.assert_array_equal(m.convert_array_id(2, True), [2])
    np.testing.assert_array_equal(m.convert_array_id(np.int64(0), True), [0])
    for inner in (-1, n, n + 5):
        np.testing.assert_array_equal(m.convert_array_id(inner, True), [n])
    with pytest.raises(ValueError, match="`inner id` user must be int"):
        m.convert_array_id("b", True)
    with pytest.raises(ValueError, match="`inner id` user must be int"):
        m.convert_array_id(1.0, True)
    with pytest.raises(AssertionError, match="must be scalar"):
        m.convert_array_id([0, 1], False)


# ---- the window -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", WINDOWED)
def test_window_of_a_given_sequence(name):
    m = MODELS[name]()
    assert m.max_seq_len == L and m.n_items == N
    cases = [
        ([10, 20, 30, 40, 50, 60], False, [[2, 3, 4, 5]]),     # longer than L: the last four
        ([0, 1, 2, 3, 4], True, [[1, 2, 3, 4]]),
        ([30, 10], False, [[2, 0, N, N]]),                     # shorter: pad-filled
        ([5], True, [[5, N, N, N]]),
        ([10, 999, 20], False, [[0, N, 1, N]]),                # an unknown raw item keeps its slot as the pad id
        ([1, -1, 6, 2], True, [[1, N, N, 2]]),                 # inner ids outside [0, n_items)
        (np.array([3, 4]), True, [[3, 4, N, N]]),
    ]
    for seq, inner_id, want in cases:
        got = m._window(0, seq, inner_id)
        assert got.shape == (1, L) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {seq}")


@pytest.mark.parametrize("seq", [None, []], ids=["none", "empty"])
@pytest.mark.parametrize("name", WINDOWED)
def test_window_fallbacks(name, seq):
    """No `seq`: the cached recent window (RNN4Rec, WaveNet) or the tail of the consumed list (YouTubeRetrieval); the three
    agree on known users, and the OOV user's window is all pad."""
    m = MODELS[name]()
    want = {0: [[2, 3, 4, 5]], 1: [[3, N, N, N]], 2: [[N, N, N, N]], m.n_users: [[N, N, N, N]]}
    for uid, w in want.items():
        got = m._window(uid, seq, False)
        assert got.shape == (1, L) and got.dtype == np.int32
        np.testing.assert_array_equal(got, w, err_msg=f"{name} user {uid}")
    if name != "YouTubeRetrieval":
        np.testing.assert_array_equal(m._window(1, seq, True), m.recent_seqs[[1]])


def test_rnn_window_length():
    m = MODELS["RNN4Rec"]()
    for seq, want in (([10, 20, 30, 40, 50, 60], 4), ([30, 10], 2), ([999], 1), (np.array([1, 2, 3]), 3)):
        np.testing.assert_array_equal(m._window_len(0, seq), [want])
    # no sequence: the cached length, which is 1 for a user without history and for the OOV user (the one-step [pad])
    for seq in (None, []):
        assert [int(m._window_len(u, seq)[0]) for u in (0, 1, 2, m.n_users)] == [4, 1, 0, 1]
    assert m.recent_seq_lens.tolist() == [4, 1, 0, 1]


# ---- user features --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["RNN4Rec", "WaveNet"])
@pytest.mark.parametrize("seq", [None, [10, 20]], ids=["no-seq", "seq"])
def test_user_feats_are_rejected_by_name(name, seq):
    m = MODELS[name]()
    for call in (lambda: m.recommend_user("a", 3, user_feats={"age": 1}, seq=seq),
                 lambda: m.dyn_user_embedding("a", user_feats={"age": 1}, seq=seq)):
        with pytest.raises(ValueError, match=f"`{name}` has no user features: `user_feats`"):
            call()


@pytest.mark.parametrize("name", ["YouTubeRetrieval", "TwoTower"])
def test_user_feature_rows(name):
    m = MODELS[name]()
    assert m._user_feature_rows(1, None) == (None, None) and m._user_feature_rows(1, {"age": 3}) == (None, None)
    info = m.data_info
    info.user_sparse_unique = np.arange(8).reshape(4, 2)
    info.user_dense_unique = np.arange(4, dtype=np.float32).reshape(4, 1)
    sp, de = m._user_feature_rows(2, None)
    np.testing.assert_array_equal(sp, [[4, 5]])
    np.testing.assert_array_equal(de, [[2.0]])


# ---- DenseParams.take_over ------------------------------------------------------------------
def _params(seed, shapes=((3, 5), (5,))):
    P = DenseParams(torch.device("cpu"), seed)
    P.add("w", shapes[0], "glorot_uniform")
    P.add("b", shapes[1], "ones")
    P.finalize()
    return P


def _saved(prefix=""):
    rng = np.random.default_rng(5)
    P = _params(1)
    return {f"{prefix}w": rng.standard_normal((3, 5)).astype(np.float32), f"{prefix}b": rng.standard_normal(5).astype(np.float32),
            "opt::dense_m": rng.standard_normal(P.m.shape).astype(np.float32),
            "opt::dense_v": rng.random(P.v.shape).astype(np.float32)}


def test_take_over_all_shapes_equal(capsys):
    P, a = _params(2), _saved()
    assert P.take_over(a, True) is True
    np.testing.assert_array_equal(P["w"].detach().numpy(), a["w"])
    np.testing.assert_array_equal(P["b"].detach().numpy(), a["b"])
    np.testing.assert_array_equal(P.m.numpy(), a["opt::dense_m"])
    np.testing.assert_array_equal(P.v.numpy(), a["opt::dense_v"])
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("how", ["shape", "missing"])
def test_take_over_skips_one_parameter_and_the_moments(how, capsys):
    P, a = _params(2), _saved()
    fresh = P["w"].detach().clone()
    if how == "shape":
        a["w"] = np.zeros((4, 5), dtype=np.float32)
    else:
        del a["w"]
    assert P.take_over(a, True) is False
    np.testing.assert_array_equal(P["w"].detach().numpy(), fresh.numpy())
    np.testing.assert_array_equal(P["b"].detach().numpy(), a["b"])
    assert not P.m.any() and not P.v.any()
    out = capsys.readouterr().out
    assert out.count("will be skipped") == 1 and '"w"' in out


def test_take_over_leaves_moments_of_another_layout(capsys):
    P, a = _params(2), _saved()
    a["opt::dense_m"], a["opt::dense_v"] = a["opt::dense_m"][:-4], a["opt::dense_v"][:-4]
    assert P.take_over(a, True) is True
    np.testing.assert_array_equal(P["w"].detach().numpy(), a["w"])
    assert not P.m.any() and not P.v.any()


def test_take_over_without_full_assign_leaves_the_moments():
    P, a = _params(2), _saved()
    P.m.fill_(0.25)
    P.v.fill_(0.5)
    assert P.take_over(a, False) is True
    np.testing.assert_array_equal(P["b"].detach().numpy(), a["b"])
    assert (P.m == 0.25).all() and (P.v == 0.5).all()


def test_take_over_through_a_key_prefix(capsys):
    P, a = _params(2), _saved("dense::")
    assert P.take_over(a, True, name_of=lambda k: f"dense::{k}") is True
    np.testing.assert_array_equal(P["w"].detach().numpy(), a["dense::w"])
    np.testing.assert_array_equal(P.m.numpy(), a["opt::dense_m"])
    Q = _params(3)
    fresh = Q["b"].detach().clone()
    assert Q.take_over(a, True) is False                      # without the prefix nothing is found
    np.testing.assert_array_equal(Q["b"].detach().numpy(), fresh.numpy())
    assert not Q.m.any() and capsys.readouterr().out.count("will be skipped") == 2
