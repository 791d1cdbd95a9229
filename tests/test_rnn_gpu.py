"""The recurrent layers and RNN4Rec on the device (csrc/rnn.hip, layers/recurrent.py, nets/rnn_nets.py,
algorithms/rnn4rec.py) against the CPU oracle (tests/rnn_oracle.py, f64 variant).  tests/test_rnn_cpu.py shows that the oracle
equals torch's own cells and autograd and that the oracle's f32 arithmetic passes every tolerance used here."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import RNN4Rec
from librecommender_amd.data import DatasetPure
from librecommender_amd.nets.rnn_nets import RNN4RecNet

from . import rnn_oracle as O

pytestmark = pytest.mark.gpu

CELLS = ("gru", "lstm")


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _shape_id(s):
    return "x".join(map(str, s))


def _run(dev, cell, c, act, form="table", ids=None, lens=None):
    """Forward + backward of one case on the device -> five torch tensors (hs, gx, gW, gU, gb)."""
    ids = c["ids"] if ids is None else ids
    lens = c["lens"] if lens is None else lens
    W, U, b, ghs, im, rm = (_dev(c[k], dev) for k in ("W", "U", "b", "ghs", "in_mask", "rec_mask"))
    if form == "table":
        src = dict(table=_dev(c["table"], dev), ids=_dev(ids, dev))
    else:
        src = dict(x=_dev(c["table"][ids], dev))
    hs, saved = ops.rnn_layer_fwd(cell, W, U, b, _dev(lens, dev), in_mask=im, rec_mask=rm, act=act, **src)
    gx, gW, gU, gb = ops.rnn_layer_bwd(cell, W, U, _dev(lens, dev), hs, saved, ghs, in_mask=im, rec_mask=rm, act=act, **src)
    return hs, gx, gW, gU, gb


def _np(outs):
    return tuple(o.cpu().numpy() for o in outs)


# ---- 1. one layer, forward and backward ----------------------------------------------------
@pytest.mark.parametrize("shape", O.LAYER_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("act", [True, False], ids=["tanh", "identity"])
@pytest.mark.parametrize("cell", CELLS)
def test_layer(dev, cell, act, shape):
    """Both forms against the f64 oracle by the delta rule; lens 0, 1, L - 1 and L in every batch, Zipf ids with repeats;
    the x form and the table form give equal bits."""
    c = O.layer_case(cell, *shape)
    table = _run(dev, cell, c, act, "table")
    O.check_layer(_np(table), cell, c, act, f"{cell} act={act} {_shape_id(shape)}")
    x = _run(dev, cell, c, act, "x")
    for name, a, b in zip(O.OUTPUTS, table, x):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", O.WIDE_SHAPES, ids=_shape_id)
@pytest.mark.parametrize("cell", CELLS)
def test_layer_wide_batches(dev, cell, shape):
    """Batches past the threshold at which a lane owns four samples instead of one: the same checks as `test_layer`."""
    test_layer(dev, cell, True, shape)


# ---- 2. masked steps -----------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
def test_masked_steps(dev, cell):
    """The pad row is NaN and every masked id names it: everything finite, gx exactly 0 there; other valid ids at the masked
    steps, and lens beyond [0, L], give the same bits."""
    B, L = 37, 10
    c = O.layer_case(cell, B, L, 16, 16)
    valid = O.valid_steps(c["lens"], L)
    pad = c["V"] - 1
    assert np.isnan(c["table"][pad]).all()
    ids = np.where(valid, c["ids"], pad).astype(np.int32)
    got = _run(dev, cell, c, True, "table", ids=ids)
    O.check_layer(_np(got), cell, c, True, f"masked {cell}", ids=ids)
    assert not got[1].cpu().numpy()[~valid].any()
    for name, a, b in zip(O.OUTPUTS, got, _run(dev, cell, c, True, "table")):      # the case's own ids at the masked steps
        assert torch.equal(a, b), name
    wild = c["lens"].copy()
    wild[c["lens"] == L] = L + 3
    wild[c["lens"] == 0] = -2
    for name, a, b in zip(O.OUTPUTS, got, _run(dev, cell, c, True, "table", ids=ids, lens=wild)):
        assert torch.equal(a, b), name
    hs = got[0].cpu().numpy()
    assert not hs[c["lens"] == 0].any()                                            # len 0: every output is 0
    one = np.flatnonzero(c["lens"] == 1)[0]
    assert (hs[one] == hs[one, 0]).all()                                           # the carried state is repeated


@pytest.mark.parametrize("cell", CELLS)
def test_bad_ids(dev, cell):
    """An id of -1 or V + 5 at a valid step is a masked step; the other samples keep their bits."""
    B, L = 37, 10
    c = O.layer_case(cell, B, L, 16, 16)
    c["lens"][5], c["lens"][6] = L, L
    clean = _run(dev, cell, c, True, "table")
    ids = c["ids"].copy()
    ids[5, 0], ids[6, 3], ids[6, L - 1] = -1, c["V"] + 5, -1
    got = _run(dev, cell, c, True, "table", ids=ids)
    O.check_layer(_np(got), cell, c, True, f"bad-ids {cell}", ids=ids)
    others = np.setdiff1d(np.arange(B), [5, 6])
    for a, b in zip(got[:2], clean[:2]):
        assert np.array_equal(a.cpu().numpy()[others], b.cpu().numpy()[others])
    assert not got[1].cpu().numpy()[5, 0].any() and not got[1].cpu().numpy()[6, 3].any()
    hs = got[0].cpu().numpy()
    assert not hs[5, 0].any() and np.array_equal(hs[6, 3], hs[6, 2]) and np.array_equal(hs[6, L - 1], hs[6, L - 2])


# ---- 3. determinism ------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
def test_two_runs_give_the_same_bits(dev, cell):
    c = O.layer_case(cell, 300, 10, 20, 16)
    a, b = _run(dev, cell, c, True), _run(dev, cell, c, True)
    for name, p, q in zip(O.OUTPUTS, a, b):
        assert torch.equal(p, q), name


# ---- 4. dropout masks ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 10, 16, 16), (300, 7, 16, 128)], ids=_shape_id)
@pytest.mark.parametrize("cell", CELLS)
def test_dropout_masks(dev, cell, shape):
    c = O.layer_case(cell, *shape, dropout=0.5)
    assert (c["in_mask"] == 0).any() and (c["rec_mask"] == 2).any()
    for act in (True, False):
        O.check_layer(_np(_run(dev, cell, c, act)), cell, c, act, f"dropout {cell} act={act} {_shape_id(shape)}")


def test_unsupported_shapes(dev):
    assert ops.rnn_supported("gru", 1, 1) and ops.rnn_supported("lstm", 128, 128)
    assert not ops.rnn_supported("gru", 129, 16) and not ops.rnn_supported("lstm", 16, 129) and not ops.rnn_supported("gru", 0, 4)
    W, U, b = (torch.zeros(s, device=dev) for s in ((16, 3 * 129), (129, 3 * 129), (2, 3 * 129)))
    with pytest.raises(ValueError):
        ops.rnn_layer_fwd("gru", W, U, b, torch.ones(2, dtype=torch.int32, device=dev), x=torch.zeros((2, 3, 16), device=dev))


# ---- 5. three consecutive training steps ---------------------------------------------------
def _cfg_id(cfg):
    return "-".join("x".join(map(str, x)) if isinstance(x, tuple) else str(x) for x in cfg)


def _check_net(net, twin, what):
    for k, ref in twin.w.items():
        got = net.vars[k] if k in net.vars else net.P[k]
        np.testing.assert_allclose(got.detach().cpu().numpy().reshape(ref.shape), ref.numpy(), rtol=1e-4, atol=5e-5,
                                   err_msg=f"{k} {what}")


def _stepped(dev, cell, hidden, ln, loss, dense, reg, norm_embed=False):
    S = O.STEP_SHAPE
    net = RNN4RecNet(S["n_items"], S["K"], hidden, cell, ln, 0.0, norm_embed, S["L"], S["lr"], 1e-5, 11, dev, dense, loss, reg)
    w = O.step_weights(cell, hidden, ln)
    assert set(w) == set(net.vars) | set(net.P.params)
    with torch.no_grad():
        for k, val in w.items():
            dst = net.vars[k] if k in net.vars else net.P[k]
            dst.copy_(_dev(val, dev).view_as(dst))
    twin = O.NetTwin(w, cell, len(hidden), ln, loss, S["lr"], 1e-5, dense, reg, norm_embed)
    for step, batch in enumerate(O.step_batches(loss), 1):
        want = twin.train_step(**batch)
        got = float(net.train_step(**batch))
        assert abs(got - want) < 1e-5, (step, got, want)
        _check_net(net, twin, f"after step {step}")
    return net


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=_cfg_id)
def test_training_steps(dev, cfg):
    """Loss to 1e-5, every variable to rtol 1e-4 / atol 5e-5 (the figures of the DeepFM step in `smoke()`)."""
    _stepped(dev, *cfg)


@pytest.mark.parametrize("loss", ["cross_entropy", "bpr"])
def test_training_steps_norm_embed(dev, loss):
    _stepped(dev, "gru", (16,), False, loss, False, None, norm_embed=True)


def test_training_step_reg_needs_dense(dev):
    with pytest.raises(ValueError, match="dense_adam=True"):
        RNN4RecNet(5, 8, (8,), "gru", device=dev, reg=0.01)


def test_dropout_step_uses_the_given_masks(dev):
    """A step with dropout masks against the twin given the same masks; the net draws its own when none are given."""
    S, cell, hidden = O.STEP_SHAPE, "lstm", (16, 8)
    net = RNN4RecNet(S["n_items"], S["K"], hidden, cell, False, 0.5, False, S["L"], S["lr"], 1e-5, 11, dev, False, "focal")
    w = O.step_weights(cell, hidden, False)
    with torch.no_grad():
        for k, val in w.items():
            dst = net.vars[k] if k in net.vars else net.P[k]
            dst.copy_(_dev(val, dev).view_as(dst))
    twin = O.NetTwin(w, cell, 2, False, "focal", S["lr"])
    batch = O.step_batches("focal")[0]
    masks = net.rnn.draw_masks(S["B"], net.gen)
    assert [tuple(m.shape) for pair in masks for m in pair] == [(S["B"], 16), (S["B"], 16), (S["B"], 16), (S["B"], 8)]
    want = twin.train_step(**batch, masks=[tuple(m.cpu().numpy() for m in pair) for pair in masks])
    assert abs(float(net.train_step(**batch, masks=masks)) - want) < 1e-5
    _check_net(net, twin, "dropout step")
    assert np.isfinite(float(net.train_step(**batch)))


# ---- 6. the model on the MovieLens sample --------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    df = pd.read_csv(O.DATA, sep="::", engine="python", names=["user", "item", "label", "time"]).iloc[:6000]
    old, new = df.iloc[:5000], df.iloc[5000:]
    train_data, info = DatasetPure.build_trainset(old)
    return old, new, train_data, info


def _fit(info, train_data, losses=None, **kw):
    model = RNN4Rec("ranking", info, **dict(dict(embed_size=8, n_epochs=3, lr=0.01, batch_size=256, hidden_units=16, seed=7), **kw))
    if losses is not None:
        step = model.train_on_batch
        model.train_on_batch = lambda b: losses.append(step(b)) or losses[-1]
    model.fit(train_data, neg_sampling=True, verbose=0)
    return model


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("loss", ["cross_entropy", "focal", "bpr"])
def test_fit_lowers_the_training_loss(dev, sample, loss, cell):
    _, _, train_data, info = sample
    losses = []
    _fit(info, train_data, losses, loss_type=loss, rnn_type=cell)
    per_epoch = torch.stack(losses).view(3, -1).mean(1).tolist()
    print(f"RNN-FIGURE fit loss={loss} cell={cell} epoch means {per_epoch}")
    assert per_epoch[2] < per_epoch[0]


def _is_top(scores, ids):
    """`ids` are distinct, in descending score order, and their scores are the len(ids) largest of `scores`."""
    assert len(set(ids)) == len(ids)
    np.testing.assert_allclose(scores[ids], np.sort(scores)[::-1][:len(ids)], rtol=1e-4, atol=1e-6)


def test_model_surface(dev, sample, tmp_path):
    old, new, train_data, info = sample
    model = _fit(info, train_data, hidden_units=[16, 8], use_layer_norm=True)
    K, nU, nI = 8, info.n_users, info.n_items
    assert model.user_embeds.shape == (nU + 1, K + 1) and model.item_embeds.shape == (nI + 1, K + 1)
    U, I = model.user_embeds_np, model.item_embeds_np
    assert (U[:nU, K] == 1).all() and np.array_equal(I[:nI, K], model.net.vars["item_bias_var"].view(-1).cpu().numpy())
    # predict / recommend are dot products of the exported embeddings
    users, items = old.user.iloc[:40].tolist(), old.item.iloc[:40].tolist()
    uid, iid = [info.user2id[u] for u in users], [info.item2id[i] for i in items]
    raw = (U[uid] * I[iid]).sum(1)
    np.testing.assert_allclose(model.predict(user=users, item=items), 1 / (1 + np.exp(-raw)), rtol=1e-4, atol=1e-6)
    u = users[0]
    recs = model.recommend_user(user=u, n_rec=7)[u]
    consumed = set(info.user_consumed[uid[0]])
    scores = I[:nI] @ U[uid[0]]
    scores[list(consumed)] = -np.inf
    _is_top(scores, [info.item2id[i] for i in recs.tolist()])
    assert not consumed & {info.item2id[i] for i in recs.tolist()}                  # filter_consumed
    kept = model.recommend_user(user=u, n_rec=nI, filter_consumed=False)[u]
    assert consumed <= {info.item2id[i] for i in kept.tolist()}
    cold = model.recommend_user(user=-999, n_rec=7)[-999]                           # cold start
    assert len(cold) == 7 and set(cold.tolist()) <= {info.id2item[j] for j in model.default_recs.tolist()}
    np.testing.assert_allclose(model.predict(user=-999, item=items[0]), 1 / (1 + np.exp(-float(U[nU] @ I[iid[0]]))), rtol=1e-4)
    # dyn_user_embedding(seq=...) is the net on that window
    seq = old.item.iloc[100:104].tolist() + [-12345]                                # an unknown item is the pad id
    window = np.full((1, model.max_seq_len), nI, dtype=np.int32)
    window[0, :5] = [info.item2id[i] for i in seq[:4]] + [nI]
    want = model.net.embed_users(window, np.array([5], dtype=np.int32))[0].cpu().numpy()
    assert np.array_equal(model.dyn_user_embedding(u, seq=seq), want)
    assert np.array_equal(model.dyn_user_embedding(u), U[uid[0], :K])               # no seq: the cached recent window
    with_bias = model.dyn_user_embedding(u, seq=seq, include_bias=True)
    assert with_bias.shape == (K + 1,) and with_bias[K] == 1
    dyn = model.recommend_user(user=u, n_rec=7, seq=seq)[u]
    s2 = I[:nI] @ with_bias
    s2[list(consumed)] = -np.inf
    _is_top(s2, [info.item2id[i] for i in dyn.tolist()])
    with pytest.raises(ValueError, match="user_feats"):
        model.recommend_user(user=u, n_rec=3, user_feats={"sex": "F"})
    with pytest.raises(ValueError, match="user_feats"):
        model.dyn_user_embedding(u, user_feats={"sex": "F"})
    # save -> load, full and inference-only
    some = old.user.unique()[:20].tolist()
    a = model.recommend_user(user=some, n_rec=10)
    model.save(str(tmp_path), "rnn")
    full = RNN4Rec.load(str(tmp_path), "rnn", info)
    assert all(torch.equal(full.net.vars[k], model.net.vars[k]) for k in model.net.vars)
    assert all(torch.equal(full.net.P[k], model.net.P[k]) for k in model.net.P.params)
    b = full.recommend_user(user=some, n_rec=10)
    assert np.array_equal(full.dyn_user_embedding(u, seq=seq), want)
    model.save(str(tmp_path), "rnn_inf", inference_only=True)
    assert not os.path.exists(os.path.join(tmp_path, "rnn_inf_variables.npz"))
    c = RNN4Rec.load(str(tmp_path), "rnn_inf", info).recommend_user(user=some, n_rec=10)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with np.load(os.path.join(tmp_path, "rnn_variables.npz")) as z:
        assert {"embedding/seq_embeds_var", "embedding/item_embeds_var", "embedding/item_bias_var", "gru/gru_cell/kernel",
                "gru_1/gru_cell_1/recurrent_kernel", "layer_normalization_1/gamma", "dense/kernel", "dense/bias"} <= set(z.files)
        assert z["embedding/item_bias_var"].shape == (nI,) and z["gru/gru_cell/bias"].shape == (2, 48)
    # retraining on merged data with added items keeps old rows, moments and the step count; the pad row moves
    train2, info2 = DatasetPure.merge_trainset(new, info)
    assert info2.n_items > nI
    m2 = RNN4Rec("ranking", info2, embed_size=8, n_epochs=1, lr=0.01, hidden_units=[16, 8], use_layer_norm=True, seed=7)
    m2.rebuild_model(str(tmp_path), "rnn", full_assign=True)
    V1, V2 = model.net.vars, m2.net.vars
    for k in V1:
        assert torch.equal(V2[k][:nI], V1[k][:nI]) and torch.equal(m2.net.m[k][:nI], model.net.m[k][:nI]), k
        assert not bool(m2.net.m[k][nI:info2.n_items].any()), k
    assert torch.equal(V2["seq_embeds_var"][info2.n_items], V1["seq_embeds_var"][nI])
    assert torch.equal(m2.net.v["seq_embeds_var"][info2.n_items], model.net.v["seq_embeds_var"][nI])
    assert not torch.equal(V2["seq_embeds_var"][nI], V1["seq_embeds_var"][nI])      # a new item's fresh row, not the old pad
    assert all(torch.equal(m2.net.P[k], model.net.P[k]) for k in model.net.P.params)
    assert torch.equal(m2.net.P.m, model.net.P.m) and m2.net.step == model.net.step > 0
    m3 = RNN4Rec("ranking", info2, embed_size=8, n_epochs=1, hidden_units=[16, 8], use_layer_norm=True)
    m3.rebuild_model(str(tmp_path), "rnn", full_assign=False)
    assert torch.equal(m3.net.vars["item_embeds_var"][:nI], V1["item_embeds_var"]) and m3.net.step == 0
    assert not bool(m3.net.m["item_embeds_var"].any()) and not bool(m3.net.P.m.any())
    m2.fit(train2, neg_sampling=True, verbose=0)
    assert m2.user_embeds.shape[0] == info2.n_users + 1 and m2.net.step > model.net.step


def test_rating_task_and_keras_initialisers(dev, sample):
    old, _, _, info = sample
    train_data, info_r = DatasetPure.build_trainset(old)
    m = RNN4Rec("rating", info_r, rnn_type="lstm", embed_size=8, n_epochs=1, lr=0.01, hidden_units=16, seed=3)
    m.build_model()
    P = m.net.P
    b = P["lstm/lstm_cell/bias"].detach().cpu().numpy()
    assert (b[16:32] == 1).all() and not b[:16].any() and not b[32:].any()          # unit_forget_bias
    U = P["lstm/lstm_cell/recurrent_kernel"].detach().cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(U @ U.T, np.eye(16), atol=1e-5)                       # orthogonal
    lim = np.sqrt(6.0 / (16 + 64))
    Wk = P["lstm/lstm_cell/kernel"].detach().cpu().numpy()
    assert np.abs(Wk).max() <= lim and np.abs(Wk).max() > 0.8 * lim                 # glorot-uniform
    assert m.net.loss == "mse" and m.net.vars["seq_embeds_var"].shape == (info_r.n_items + 1, 16)
    m.model_built = True
    m.fit(train_data, neg_sampling=False, verbose=0)
    p = m.predict(user=old.user.iloc[:5].tolist(), item=old.item.iloc[:5].tolist())
    assert ((np.asarray(p) >= 1) & (np.asarray(p) <= 5)).all()


def test_unsupported_hidden_units_raise_at_build(dev, sample):
    _, _, train_data, info = sample
    with pytest.raises(ValueError, match="1 to 128"):
        RNN4Rec("ranking", info, hidden_units=[16, 256]).build_model()


def test_multi_rank_fit_raises(dev, sample, monkeypatch):
    _, _, train_data, info = sample
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        RNN4Rec("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
