"""AutoInt's stack and AutoInt on the device (csrc/autoint.hip, nets/autoint_net.py, algorithms/autoint.py) against the CPU
oracle (tests/autoint_oracle.py, f64 variant) and against the same net composed from torch ops under autograd.
tests/test_autoint_cpu.py shows that the oracle equals `seq_nets.multi_head_attention` and torch autograd, and that the
oracle's f32 arithmetic passes every tolerance used here."""
import os

import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import AutoInt
from librecommender_amd.data import DatasetFeat
from librecommender_amd.nets import FeatSpec
from librecommender_amd.nets.autoint_net import FeatAutoIntNet
from oracle.make_golden import FEAT_KW, MULTI_KW, synthetic_frame

from . import autoint_oracle as O

pytestmark = pytest.mark.gpu

OUTPUTS = ("acts", "logits", "gx", "gparams")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, c):
    """Forward + backward of one case on the device -> {name: torch tensor}."""
    _, _, _, H, head_dims, residual = c["shape"]
    x, params = _dev(c["x"], dev), _dev(O.pack_params(c["layers"], c["w"], c["c"]), dev)
    logits, acts, saved = ops.autoint_fwd(x, params, H, head_dims, residual)
    gx, gparams = ops.autoint_bwd(x, params, H, head_dims, residual, acts, saved, _dev(c["glogits"], dev))
    return dict(acts=acts, logits=logits, gx=gx, gparams=gparams)


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


# ---- 1. the stack, forward and backward ------------------------------------------------------
@pytest.mark.parametrize("shape", O.SHAPES, ids=O.sid)
def test_stack(dev, shape):
    """Every layer of acts, the logits, gx and every parameter gradient against the f64 oracle by the delta rule."""
    c = O.stack_case(*shape)
    O.check_stack(_np(_run(dev, c)), c, O.sid(shape))


@pytest.mark.parametrize("shape", O.WIDE_SHAPES, ids=O.sid)
def test_stack_wide_batches(dev, shape):
    """Batches at which a workgroup owns several samples and the last tile is not full: the same checks as `test_stack`."""
    test_stack(dev, shape)


def test_softmax_of_one_field(dev):
    """T = 1: P is exactly 1, so a layer is A + (A Wv) Wo whatever the query and key kernels hold."""
    c = O.stack_case(5, 1, 6, 2, (4,), True)
    got = _run(dev, c)
    other = dict(c, layers=[(Wq * 3 + 1, Wk * -2, Wv, Wo) for Wq, Wk, Wv, Wo in c["layers"]])
    again = _run(dev, other)
    assert torch.equal(got["acts"], again["acts"]) and torch.equal(got["logits"], again["logits"])
    g = O.unpack_params(got["gparams"].cpu().numpy(), 1, 6, 2, (4,))[0][0]
    assert not g[0].any() and not g[1].any() and g[2].any() and g[3].any()


def test_saturated_softmax(dev):
    """Scores that reach +-80 and beyond: finite and inside the rule (the row maximum is subtracted before exp)."""
    c = O.saturated_case()
    O.check_stack(_np(_run(dev, c)), c, "saturated")


# ---- 2. inference mode, bits -----------------------------------------------------------------
@pytest.mark.parametrize("shape", [O.SHAPES[3], O.WIDE_SHAPES[1]], ids=O.sid)
def test_inference_mode_and_batch_independence(dev, shape):
    """Without acts only the logits are written, with the training forward's bits; a sample's logit has the same bits alone
    (B = 1), in a small batch and inside the whole one."""
    c = O.stack_case(*shape)
    B, _, _, H, head_dims, residual = shape
    x, params = _dev(c["x"], dev), _dev(O.pack_params(c["layers"], c["w"], c["c"]), dev)
    train, acts, _ = ops.autoint_fwd(x, params, H, head_dims, residual)
    infer, none, saved = ops.autoint_fwd(x, params, H, head_dims, residual, want_acts=False)
    assert none is None and saved is None and torch.equal(train, infer)
    for i in (0, B // 2, B - 1):
        assert torch.equal(ops.autoint_fwd(x[i:i + 1].contiguous(), params, H, head_dims, residual, want_acts=False)[0], infer[i:i + 1])
    part = ops.autoint_fwd(x[3:30].contiguous(), params, H, head_dims, residual)
    assert torch.equal(part[0], infer[3:30]) and torch.equal(part[1], acts[:, 3:30])


def test_two_runs_give_the_same_bits(dev):
    c = O.stack_case(*O.WIDE_SHAPES[1])
    a, b = _run(dev, c), _run(dev, c)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


def test_empty_batch(dev):
    c = O.stack_case(1, 8, 16, 2, (8, 8, 8), True)
    x, params = _dev(c["x"], dev)[:0], _dev(O.pack_params(c["layers"], c["w"], c["c"]), dev)
    logits, acts, saved = ops.autoint_fwd(x, params, 2, (8, 8, 8), True)
    assert logits.shape == (0,) and acts.shape == (3, 0, 8, 16)
    gparams = torch.full_like(params, 7.0)
    gx, out = ops.autoint_bwd(x, params, 2, (8, 8, 8), True, acts, saved, logits.clone(), gparams=gparams)
    assert gx.shape == (0, 8, 16) and out is gparams and not gparams.any()


def test_unsupported_shapes(dev):
    assert ops.autoint_supported(1, 1, 1, (1,)) and ops.autoint_supported(64, 64, 8, (8,) * 8) and ops.autoint_supported(64, 64, 1, (64,))
    x, params = torch.zeros((2, 65, 16), device=dev), torch.zeros(4096, device=dev)
    with pytest.raises(ValueError, match="unsupported AutoInt shape"):
        ops.autoint_fwd(x, params, 2, (8,))
    with pytest.raises(ValueError, match="unsupported AutoInt shape"):
        ops.autoint_fwd(x[:, :8].contiguous(), params, 2, (33,))
    with pytest.raises(ValueError, match="unsupported AutoInt shape"):
        ops.autoint_bwd(x, params, 2, (8,), True, x, params.view(torch.uint8)[:0], params[:2])
    n, hd = ops._head_dims((8,))
    out = torch.zeros(4096, device=dev)
    with pytest.raises(ValueError, match="lr_autoint_fwd_f32"):              # LR_ESHAPE from the entry point itself
        ops._call("lr_autoint_fwd_f32", x.data_ptr(), 2, 65, 16, 2, n, hd, 1, params.data_ptr(), 0, 0, 0, 0, out.data_ptr(), ops._stream())
    with pytest.raises(ValueError, match="lr_autoint_bwd_f32"):
        ops._call("lr_autoint_bwd_f32", x.data_ptr(), 2, 8, 16, 9, n, hd, 1, params.data_ptr(), out.data_ptr(), 0, out.data_ptr(),
                  out.data_ptr(), out.data_ptr(), out.data_ptr(), out.numel() * 4, ops._stream())
    with pytest.raises(ValueError, match="parameter buffer"):
        ops.autoint_fwd(x[:, :8].contiguous(), params, 2, (8,))


# ---- 3. three consecutive training steps: fused against composed -------------------------------
def _frame():
    """The synthetic feature frame with its dense columns standardised: raw `profit` reaches 1e4, where the f32 rounding of a
    logit alone (1e4 x 6e-8) is past the 1e-5 the losses are compared to."""
    df = synthetic_frame()
    for col in ("age", "profit"):
        df[col] = (df[col] - df[col].mean()) / df[col].std()
    return df


@pytest.fixture(scope="module")
def feat_data():
    out = {}
    for tag, kw in (("feat", FEAT_KW), ("multi", MULTI_KW)):
        df = _frame()
        train_data, info = DatasetFeat.build_trainset(df, **kw)
        out[tag] = (df, train_data, info)
    return out


# (data, loss, dense_adam, reg, head_dims, residual)
STEP_CONFIGS = [("multi", "cross_entropy", False, None, (8, 8, 8), True), ("multi", "focal", False, None, (8, 4), True),
                ("feat", "mse", False, None, (8, 8, 8), True), ("multi", "cross_entropy", True, 0.01, (8, 8, 8), True),
                ("feat", "cross_entropy", False, None, (5,), False)]


def _cfg_id(cfg):
    return "-".join(str(v) if not isinstance(v, tuple) else "_".join(map(str, v)) for v in cfg)


@pytest.mark.parametrize("cfg", STEP_CONFIGS, ids=_cfg_id)
def test_training_steps(dev, feat_data, cfg):
    """Two nets from one seed, one on the kernels and one composed from `seq_nets.multi_head_attention` and `TFDense` under
    autograd: the loss to 1e-5, every table and dense parameter to rtol 1e-4 / atol 5e-5 (the figures of tests/test_rnn_gpu.py
    and tests/test_wavenet_gpu.py) over three steps.  Plain, pooled and dense fields; cross entropy, focal, mse, dense Adam
    with `reg`, no residual."""
    tag, loss, dense_adam, reg, head_dims, residual = cfg
    _, ts, info = feat_data[tag]
    spec = FeatSpec.from_data_info(info, "sqrtn" if tag == "multi" else "normal")
    mk = lambda fused: FeatAutoIntNet(spec, 6, head_dims, 2, residual, 0.01, 1e-5, 11, dev, dense_adam, reg, fused=fused)
    fused, composed = mk(True), mk(False)
    assert fused.fused and not composed.fused and torch.equal(fused.P.flat, composed.P.flat)
    assert (tag == "multi") == bool(spec.pooled) and spec.n_dense_cols == 2
    rng = np.random.default_rng(3)
    for step in range(1, 4):
        rows = rng.integers(0, len(ts.user_indices), 48)
        labels = ts.labels[rows].astype(np.float32) if loss == "mse" else rng.integers(0, 2, 48).astype(np.float32)
        batch = dict(users=ts.user_indices[rows], items=ts.item_indices[rows], labels=labels, sparse=ts.sparse_indices[rows],
                     dense=ts.dense_values[rows], loss_type=loss)
        want, got = float(composed.train_step(**batch)), float(fused.train_step(**batch))
        print(f"AUTOINT-FIGURE step {_cfg_id(cfg)} {step}: loss {got:.8f} composed {want:.8f}")
        assert abs(got - want) < 1e-5, (step, got, want)
        for k, ref in composed.P.params.items():
            torch.testing.assert_close(fused.P[k], ref, rtol=1e-4, atol=5e-5, msg=lambda m: f"{k} after step {step}: {m}")
        torch.testing.assert_close(fused.tables.embed, composed.tables.embed, rtol=1e-4, atol=5e-5)
        torch.testing.assert_close(fused.tables.m, composed.tables.m, rtol=1e-4, atol=5e-5)
    torch.testing.assert_close(fused.forward(ts.user_indices[:40], ts.item_indices[:40], sparse=ts.sparse_indices[:40], dense=ts.dense_values[:40]),
                               composed.forward(ts.user_indices[:40], ts.item_indices[:40], sparse=ts.sparse_indices[:40],
                                                dense=ts.dense_values[:40]), rtol=1e-4, atol=5e-5)


# ---- 4. the model ----------------------------------------------------------------------------
def _fit(info, train_data, task="ranking", losses=None, **kw):
    model = AutoInt(task, info, **dict(dict(embed_size=8, n_epochs=3, lr=0.01, batch_size=64, seed=7), **kw))
    if losses is not None:
        step = model.train_on_batch
        model.train_on_batch = lambda b: losses.append(step(b)) or losses[-1]
    model.fit(train_data, neg_sampling=task == "ranking", verbose=0)
    return model


@pytest.mark.parametrize("task,loss", [("ranking", "cross_entropy"), ("ranking", "focal"), ("rating", "cross_entropy")])
def test_fit_lowers_the_training_loss(dev, feat_data, task, loss):
    df, train_data, info = feat_data["multi"]
    losses = []
    model = _fit(info, train_data, task, losses, loss_type=loss)
    assert model.net.fused
    per_epoch = torch.stack(losses).view(3, -1).mean(1).tolist()
    print(f"AUTOINT-FIGURE fit task={task} loss={loss} epoch means {per_epoch}")
    assert per_epoch[2] < per_epoch[0]
    p = np.asarray(model.predict(user=df.user.iloc[:5].tolist(), item=df.item.iloc[:5].tolist()))
    lo, hi = (0, 1) if task == "ranking" else (1, 5)
    assert ((p >= lo) & (p <= hi)).all()


def test_model_surface(dev, feat_data, tmp_path):
    df, train_data, info = feat_data["feat"]
    model = _fit(info, train_data, att_embed_size=(8, 4), use_bn=True, dropout_rate=0.2)
    net = model.net
    assert net.fused and model.att_head_dims == (8, 4) and net.T == 2 + 5 + 2
    assert model._catalog_scorer() is None and not model._batch_norms()               # the chunked forward, no BatchNorm
    u = df.user.iloc[0]
    recs = model.recommend_user(user=u, n_rec=7)[u]
    consumed = {info.id2item[i] for i in info.user_consumed[info.user2id[u]]}
    assert len(recs) == 7 and not consumed & set(recs.tolist())                       # filter_consumed
    unfiltered = model.recommend_user(user=u, n_rec=info.n_items, filter_consumed=False)[u]
    scores = model._scores_all_items(info.user2id[u], None, None).cpu().numpy()
    assert np.array_equal(np.sort(scores)[::-1], scores[[info.item2id[i] for i in unfiltered.tolist()]])
    assert len(model.recommend_user(user=u, n_rec=7, user_feats={"sex": "female", "occupation": "c"})[u]) == 7
    with pytest.raises(ValueError, match="seq"):
        model.recommend_user(user=u, n_rec=3, seq=[1, 2])
    # the chunked scorer over ragged chunks gives the bits of one forward
    model.score_chunk = 17
    assert np.array_equal(model._scores_all_items(info.user2id[u], None, None).cpu().numpy(), scores)
    # save -> load, full and inference-only
    some = df.user.unique()[:10].tolist()
    a = model.recommend_user(user=some, n_rec=5)
    model.save(str(tmp_path), "ai")
    full = AutoInt.load(str(tmp_path), "ai", info)
    assert full.att_head_dims == (8, 4) and torch.equal(full.net.P.flat, net.P.flat) and torch.equal(full.net.tables.embed, net.tables.embed)
    b = full.recommend_user(user=some, n_rec=5)
    model.save(str(tmp_path), "ai_inf", inference_only=True)
    c = AutoInt.load(str(tmp_path), "ai_inf", info).recommend_user(user=some, n_rec=5)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with np.load(os.path.join(tmp_path, "ai_variables.npz")) as z:
        assert z["dense::multi_head_attention/query/kernel"].shape == (8, 2, 8)
        assert z["dense::multi_head_attention_1/attention_output/kernel"].shape == (2, 4, 8)
        assert z["dense::dense/kernel"].shape == (9 * 8, 1) and z["dense::embedding/dense_embeds_var"].shape == (2, 8)


def test_rebuild_keeps_rows_moments_and_step(dev, tmp_path):
    from oracle.make_golden import retrain_frames

    old, new = retrain_frames()
    train0, info0 = DatasetFeat.build_trainset(old, **FEAT_KW)
    kw = dict(embed_size=8, n_epochs=1, lr=0.01, batch_size=64, seed=7)
    m0 = AutoInt("ranking", info0, **kw)
    m0.fit(train0, neg_sampling=True, verbose=0)
    m0.save(str(tmp_path), "m", inference_only=False)
    train1, info1 = DatasetFeat.merge_trainset(new, info0, merge_behavior=True)
    assert info1.n_users > info0.n_users and info1.n_items > info0.n_items
    m1 = AutoInt("ranking", info1, **kw)
    m1.rebuild_model(str(tmp_path), "m", full_assign=True)
    t0, t1 = m0.net.tables, m1.net.tables
    for name, n in (("user_embeds_var", info0.n_users), ("item_embeds_var", info0.n_items)):
        assert torch.equal(t1.variable(name)[:n], t0.variable(name)[:n]), name
    assert torch.equal(t1.m[: info0.n_users], t0.m[: info0.n_users]) and torch.equal(t1.v[: info0.n_users], t0.v[: info0.n_users])
    assert torch.equal(m1.net.P.flat, m0.net.P.flat) and torch.equal(m1.net.P.m, m0.net.P.m) and m1.net.step == m0.net.step > 0
    m2 = AutoInt("ranking", info1, **kw)
    m2.rebuild_model(str(tmp_path), "m", full_assign=False)
    assert m2.net.step == 0 and not bool(m2.net.P.m.any()) and torch.equal(m2.net.P.flat, m0.net.P.flat)
    m1.fit(train1, neg_sampling=True, verbose=0)
    assert m1.net.step > m0.net.step and len(m1.recommend_user(new["user"].iloc[0], 5)[new["user"].iloc[0]]) == 5


def test_keras_fans_of_the_projections(dev, feat_data):
    _, _, info = feat_data["feat"]
    m = AutoInt("ranking", info, embed_size=16, att_embed_size=(8,), num_heads=4, seed=3)
    m.build_model()
    P, K, H, hd = m.net.P, 16, 4, 8
    for name, shape, fans in (("query", (K, H, hd), K * H + K * hd), ("attention_output", (H, hd, K), H * hd + H * K)):
        w = P[f"multi_head_attention/{name}/kernel"].detach()
        lim = np.sqrt(6.0 / fans)
        assert tuple(w.shape) == shape and float(w.abs().max()) <= lim and float(w.abs().max()) > 0.9 * lim, name
    assert not bool(P["dense/bias"].any()) and tuple(P["dense/kernel"].shape) == (9 * 16, 1)


def test_more_fields_than_the_kernels_take(dev):
    """70 fields: the net is composed from torch ops (`fused` is False) and still trains."""
    rng = np.random.default_rng(0)
    spec = FeatSpec(n_users=30, n_items=40, n_sparse_cols=68, sparse_rows=68 * 3 + 1)
    assert spec.n_fields == 70 and not ops.autoint_supported(70, 8, 2, (8,))
    net = FeatAutoIntNet(spec, 8, (8,), 2, True, 0.01, 1e-5, 5, dev)
    assert not net.fused
    users, items = rng.integers(0, 30, 64).astype(np.int32), rng.integers(0, 40, 64).astype(np.int32)
    sparse = (np.arange(68)[None, :] * 3 + rng.integers(0, 3, (64, 68))).astype(np.int32)
    labels = (users % 2).astype(np.float32)
    losses = [float(net.train_step(users, items, labels, sparse=sparse)) for _ in range(30)]
    assert losses[-1] < losses[0]
    assert FeatAutoIntNet(spec, 8, (8,), 2, True, 0.01, 1e-5, 5, dev, fused=False).fused is False


def test_constructor_checks(dev, feat_data):
    _, _, info = feat_data["feat"]
    assert AutoInt("ranking", info, att_embed_size=4).att_head_dims == (4,)
    for bad in (dict(att_embed_size="8"), dict(att_embed_size=8.0), dict(loss_type="bpr"), dict(num_heads=0)):
        with pytest.raises(ValueError):
            AutoInt("ranking", info, **bad)
    assert AutoInt("ranking", info, reg=0.01).dense_adam                              # `reg` selects the dense update


def test_multi_rank_fit_raises(dev, feat_data, monkeypatch):
    _, train_data, info = feat_data["feat"]
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        AutoInt("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
