"""Caser's convolutions and Caser on the device (csrc/caser.hip, nets/caser_net.py, algorithms/caser.py) against the CPU oracle
(tests/caser_oracle.py, f64 variant).  tests/test_caser_cpu.py shows that the oracle equals torch's own conv1d, max and
autograd, that the oracle's f32 arithmetic passes every tolerance used here, and that the seeded step batches stay clear of
ReLU and pool flips."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import Caser
from librecommender_amd.data import DatasetPure
from librecommender_amd.nets.caser_net import CaserNet

from . import caser_oracle as O

pytestmark = pytest.mark.gpu

OUTPUTS = ("feat", "arg", "gx", "gparams")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _shape_id(s):
    return "x".join(map(str, s))


def _run(dev, c, ids=None):
    """Forward + backward of one case on the device -> {name: torch tensor}."""
    _, _, _, nh, nv = c["shape"]
    table, idt = _dev(c["table"], dev), _dev(c["ids"] if ids is None else ids, dev)
    params = _dev(O.pack_params(c["layers"]), dev)
    feat, arg = ops.caser_fwd(table, idt, params, nh, nv)
    gx, gparams = ops.caser_bwd(table, idt, params, nh, nv, feat, arg, _dev(c["gfeat"], dev))
    return dict(feat=feat, arg=arg, gx=gx, gparams=gparams)


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same_bits(a, b):
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


# ---- 1. the convolutions, forward and backward -----------------------------------------------
@pytest.mark.parametrize("shape", O.STACK_SHAPES, ids=_shape_id)
def test_stack(dev, shape):
    """feat and arg against the f64 oracle, gx and every parameter gradient against the f64 backward of the device's own ReLU
    pattern and arg (`check_caser`); windows ending in 0, 1, L - 1 and L pad ids, Zipf ids."""
    c = O.stack_case(*shape)
    O.check_caser(_np(_run(dev, c)), c, _shape_id(shape))


@pytest.mark.parametrize("shape", O.WIDE_SHAPES, ids=_shape_id)
def test_stack_wide_batches(dev, shape):
    """Batches at which a workgroup owns several samples and the slab count is at its cap: the same checks as `test_stack`."""
    test_stack(dev, shape)


# ---- 2. exact ties ---------------------------------------------------------------------------
def test_equal_positions_pool_to_the_first(dev):
    """Windows whose last five ids are the pad row: for kernel size i <= 5 the positions 5 .. 10 - i see only pad rows, have
    one receptive field and must give equal bits; arg is the first position that holds the maximum, so never a later one of
    them.  The pre-pool values stay on the chip, so the equal bits show in the pool: where the all-pad positions hold the
    maximum and lead the mixed positions clearly, arg is 5 (a later one of them with a larger last bit would win otherwise),
    and the value is that of a window of pad rows only, bit for bit."""
    L, nh = 10, 2
    c = O.stack_case(37, L, 16, nh, 4)
    c["custom"] = True
    c["ids"][:, 5:] = c["V"] - 1
    got = _np(_run(dev, c))
    O.check_caser(got, c, "equal positions")
    f64, arg64, zs = O.forward_oracle(c, "f64")
    hit = False
    for i in range(1, 6):
        sl = slice((i - 1) * nh, i * nh)
        a = got["arg"][:, sl]
        assert (a <= 5).all(), i
        tied = zs[i - 1].max(axis=1) == zs[i - 1][:, 5]          # the all-pad positions hold the f64 maximum
        lead = zs[i - 1].max(axis=1) - np.sort(zs[i - 1][:, :5], axis=1)[:, -1] > 1e-3
        assert (a[tied & lead] == 5).all(), i                    # and lead the positions before them clearly: the first of them
        hit = hit or bool((tied & lead).any())
    assert hit
    # a window of pad rows only: every position of every kernel size has one receptive field, so the maximum is at 0 and the
    # value is that of the all-pad positions above, bit for bit
    pads = c["ids"].copy()
    pads[:] = c["V"] - 1
    allpad = _np(_run(dev, c, ids=pads))
    assert not allpad["arg"].any()
    for i in range(1, 6):
        sl = slice((i - 1) * nh, i * nh)
        at5 = got["arg"][:, sl] == 5
        assert np.array_equal(got["feat"][:, sl][at5], allpad["feat"][:, sl][at5]), i


def test_dead_filter(dev):
    """A horizontal and a vertical filter with a bias of -100: feat == 0, arg == 0 and exactly zero gradient through them."""
    shape = (37, 10, 16, 2, 4)
    L, K, nh, nv = shape[1:]
    c = O.stack_case(*shape)
    c["custom"] = True
    i, f, g = 3, 1, 2
    c["layers"][i - 1][1][f] = -100.0
    c["layers"][L][1][g] = -100.0
    got = _np(_run(dev, c))
    O.check_caser(got, c, "dead filter")
    col = (i - 1) * nh + f
    vcols = L * nh + np.arange(K) * nv + g
    assert not got["feat"][:, col].any() and not got["arg"][:, col].any() and not got["feat"][:, vcols].any()
    grads, _ = O.unpack_params(got["gparams"], L, K, nh, nv)
    assert not grads[i - 1][0][:, :, f].any() and grads[i - 1][1][f] == 0
    assert not grads[L][0][:, :, g].any() and grads[L][1][g] == 0
    # nothing else sees the dead units' upstream gradient at all
    c2 = dict(c, gfeat=c["gfeat"].copy())
    c2["gfeat"][:, col] = 1e6
    c2["gfeat"][:, vcols] = 1e6
    again = _np(_run(dev, c2))
    assert np.array_equal(again["gx"], got["gx"]) and np.array_equal(again["gparams"], got["gparams"])


# ---- 3. bad ids ------------------------------------------------------------------------------
def test_bad_ids(dev):
    """An id of -1 or V + 5 is a zero input row and gets a gradient of exactly 0; the other samples keep their bits."""
    B, L = 37, 10
    c = O.stack_case(B, L, 16, 2, 4)
    clean = _run(dev, c)
    ids = c["ids"].copy()
    ids[5, 0], ids[6, 3], ids[6, L - 1] = -1, c["V"] + 5, -1
    got = _run(dev, c, ids=ids)
    g = _np(got)
    O.check_caser(g, c, "bad ids", ids=ids)
    assert not g["gx"][5, 0].any() and not g["gx"][6, 3].any() and not g["gx"][6, L - 1].any()
    assert g["gx"][5, 1].any() and g["gx"][6, 2].any()
    others = np.setdiff1d(np.arange(B), [5, 6])
    for k in ("feat", "arg", "gx"):
        assert np.array_equal(g[k][others], clean[k].cpu().numpy()[others]), k
    # a zero input row is what the bad id is: the same bits as a table row of zeros
    c0 = dict(c, table=np.concatenate([c["table"], np.zeros((1, 16), dtype=np.float32)]))
    zero_ids = np.where((ids < 0) | (ids >= c["V"]), c["V"], ids).astype(np.int32)
    z = _run(dev, c0, ids=zero_ids)
    for k in ("feat", "arg"):
        assert torch.equal(z[k], got[k]), k


# ---- 4. determinism, shapes --------------------------------------------------------------------
def test_batch_of_one_has_the_same_bits(dev):
    """A sample's row of feat and arg (and of gx) is the same alone, in a small batch and in a batch whose workgroups own
    several samples; the inference mode (no arg) gives the same feat."""
    for shape in ((300, 10, 20, 3, 4), (2100, 3, 4, 2, 2)):
        c = O.stack_case(*shape)
        whole = _run(dev, c)
        table, params = _dev(c["table"], dev), _dev(O.pack_params(c["layers"]), dev)
        feat_inf, none = ops.caser_fwd(table, _dev(c["ids"], dev), params, shape[3], shape[4], need_arg=False)
        assert none is None and torch.equal(feat_inf, whole["feat"])
        for b in (0, 3, shape[0] - 1):
            one = dict(c, ids=c["ids"][b:b + 1], gfeat=c["gfeat"][b:b + 1])
            got = _run(dev, one)
            for k in ("feat", "arg", "gx"):
                assert torch.equal(got[k][0], whole[k][b]), (shape, b, k)


def test_two_runs_give_the_same_bits(dev):
    for shape in ((300, 10, 20, 3, 4), (2100, 3, 4, 2, 2)):
        c = O.stack_case(*shape)
        _same_bits(_run(dev, c), _run(dev, c))


def test_unsupported_shapes(dev):
    assert ops.caser_supported(1, 1, 1, 1) and ops.caser_supported(64, 128, 64, 64)
    for bad in ((65, 16, 2, 4), (10, 129, 2, 4), (10, 16, 65, 4), (10, 16, 2, 65), (0, 16, 2, 4), (10, 0, 2, 4), (10, 16, 0, 4),
                (10, 16, 2, 0)):
        assert not ops.caser_supported(*bad), bad
        assert ops.caser_param_floats(*bad) == 0, bad
    table, params = torch.zeros((4, 16), device=dev), torch.zeros(64, device=dev)
    ids = torch.zeros((2, 65), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="unsupported Caser shape"):
        ops.caser_fwd(table, ids, params, 2, 4)
    with pytest.raises(ValueError, match="unsupported Caser shape"):
        ops.caser_fwd(table, ids[:, :10].contiguous(), params, 2, 65)
    out = torch.zeros(4096, device=dev)
    with pytest.raises(ValueError, match="lr_caser_fwd_f32"):          # LR_ESHAPE from the entry point itself
        ops._call("lr_caser_fwd_f32", table.data_ptr(), 4, ids.data_ptr(), 2, 65, 16, 2, 4, params.data_ptr(), out.data_ptr(),
                  ids.data_ptr(), ops._stream())
    with pytest.raises(ValueError, match="lr_caser_bwd_f32"):
        ops._call("lr_caser_bwd_f32", table.data_ptr(), 4, ids.data_ptr(), 2, 10, 16, 65, 4, params.data_ptr(), out.data_ptr(),
                  ids.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.numel() * 4, ops._stream())
    with pytest.raises(ValueError, match="parameter buffer"):
        ops.caser_fwd(table, ids[:, :10].contiguous(), params, 2, 4)
    good = torch.zeros(ops.caser_param_floats(10, 16, 2, 4) + 1, device=dev)
    with pytest.raises(ValueError, match="16-byte"):
        ops.caser_fwd(table, ids[:, :10].contiguous(), good[1:], 2, 4)
    empty = torch.zeros((0, 10), dtype=torch.int32, device=dev)
    feat, arg = ops.caser_fwd(table, empty, good[:-1], 2, 4)                   # B == 0: empties, nothing launched
    assert feat.shape == (0, 84) and arg.shape == (0, 20)
    gx, gp = ops.caser_bwd(table, empty, good[:-1], 2, 4, feat, arg, torch.zeros_like(feat))
    assert gx.shape == (0, 10, 16) and not gp.any()


# ---- 5. consecutive training steps ---------------------------------------------------------
def _cfg_id(cfg):
    return "-".join(map(str, cfg))


def _check_net(net, twin, what):
    for k, ref in twin.w.items():
        got = net.vars[k] if k in net.vars else net.P[k]
        np.testing.assert_allclose(got.detach().cpu().numpy().reshape(ref.shape), ref.numpy(), rtol=1e-4, atol=5e-5,
                                   err_msg=f"{k} {what}")


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=_cfg_id)
def test_training_steps(dev, cfg):
    """Loss to 1e-5, every variable to rtol 1e-4 / atol 5e-5 (the figures of tests/test_wavenet_gpu.py) over two steps: cross
    entropy, focal, mse, dense Adam with `reg`, `norm_embed` and two negatives per sample."""
    loss, dense, reg, norm, num_neg = cfg
    S = O.STEP_SHAPE
    net = CaserNet(S["n_users"], S["n_items"], S["K"], S["nh"], S["nv"], norm, S["L"], S["lr"], 1e-5, 11, dev, dense, loss, reg)
    w = O.step_weights(O.step_seed(cfg))
    assert set(w) == set(net.vars) | set(net.P.params)
    with torch.no_grad():
        for k, val in w.items():
            dst = net.vars[k] if k in net.vars else net.P[k]
            dst.copy_(_dev(val, dev).view_as(dst))
    twin = O.NetTwin(w, S["L"], loss, S["lr"], 1e-5, dense, reg, norm)
    for step, batch in enumerate(O.step_batches(seed=O.step_seed(cfg), num_neg=num_neg), 1):
        want = twin.train_step(**batch)
        got = float(net.train_step(**batch))
        print(f"CASER-FIGURE step {cfg} {step}: loss {got:.8f} twin {want:.8f}")
        assert abs(got - want) < 1e-5, (step, got, want)
        _check_net(net, twin, f"after step {step}")


def test_training_step_reg_needs_dense(dev):
    with pytest.raises(ValueError, match="dense_adam=True"):
        CaserNet(5, 5, 8, device=dev, reg=0.01)


# ---- 6. the model on the MovieLens sample --------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    df = pd.read_csv(O.DATA, sep="::", engine="python", names=["user", "item", "label", "time"]).iloc[:6000]
    old, new = df.iloc[:5000], df.iloc[5000:]
    train_data, info = DatasetPure.build_trainset(old)
    return old, new, train_data, info


def _fit(info, train_data, losses=None, **kw):
    model = Caser("ranking", info, **dict(dict(embed_size=8, n_epochs=3, lr=0.01, batch_size=256, seed=7), **kw))
    if losses is not None:
        step = model.train_on_batch
        model.train_on_batch = lambda b: losses.append(step(b)) or losses[-1]
    model.fit(train_data, neg_sampling=True, verbose=0)
    return model


@pytest.mark.parametrize("loss", ["cross_entropy", "focal"])
def test_fit_lowers_the_training_loss(dev, sample, loss):
    _, _, train_data, info = sample
    losses = []
    _fit(info, train_data, losses, loss_type=loss)
    per_epoch = torch.stack(losses).view(3, -1).mean(1).tolist()
    print(f"CASER-FIGURE fit loss={loss} epoch means {per_epoch}")
    assert per_epoch[2] < per_epoch[0]


def _is_top(scores, ids):
    """`ids` are distinct, in descending score order, and their scores are the len(ids) largest of `scores`."""
    assert len(set(ids)) == len(ids)
    np.testing.assert_allclose(scores[ids], np.sort(scores)[::-1][:len(ids)], rtol=1e-4, atol=1e-6)


def test_model_surface(dev, sample, tmp_path):
    old, new, train_data, info = sample
    model = _fit(info, train_data, nh_filters=3, nv_filters=2, recent_num=6, use_bn=True, dropout_rate=0.2)
    K, nU, nI = 8, info.n_users, info.n_items
    assert model.user_embeds.shape == (nU + 1, 2 * K + 1) and model.item_embeds.shape == (nI + 1, 2 * K + 1)
    U, I = model.user_embeds_np, model.item_embeds_np
    assert (U[:nU, 2 * K] == 1).all() and np.array_equal(I[:nI, 2 * K], model.net.vars["item_bias_var"].view(-1).cpu().numpy())
    uv = model.net.vars["user_embeds_var"]
    assert torch.allclose(uv[nU], uv[:nU].mean(dim=0))                               # the OOV row is the mean user row
    assert np.array_equal(U[:nU, :K], uv[:nU].cpu().numpy())
    assert (U[:nU, K:2 * K] >= 0).all()                                              # relu(Dense(..))
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
    cold = model.recommend_user(user=-999, n_rec=7)[-999]                           # an unknown user: cold start
    assert len(cold) == 7 and set(cold.tolist()) <= {info.id2item[j] for j in model.default_recs.tolist()}
    # dyn_user_embedding(seq=...) is the net on that window and the user's row
    seq = old.item.iloc[100:104].tolist() + [-12345]                                # an unknown item is the pad id
    window = np.full((1, model.max_seq_len), nI, dtype=np.int32)
    window[0, :4] = [info.item2id[i] for i in seq[:4]]
    want = model.net.embed_users(np.array([uid[0]], dtype=np.int32), window)[0].cpu().numpy()
    assert np.array_equal(model.dyn_user_embedding(u, seq=seq), want)
    assert np.array_equal(model.dyn_user_embedding(u), U[uid[0], :2 * K])           # no seq: the cached recent window
    oov = model.dyn_user_embedding(-999, seq=seq)                                   # an unknown user with a sequence: the mean row
    assert np.array_equal(oov[:K], uv[nU].cpu().numpy()) and np.array_equal(oov[K:], want[K:])
    with_bias = model.dyn_user_embedding(u, seq=seq, include_bias=True)
    assert with_bias.shape == (2 * K + 1,) and with_bias[2 * K] == 1
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
    model.save(str(tmp_path), "cs")
    full = Caser.load(str(tmp_path), "cs", info)
    assert all(torch.equal(full.net.vars[k], model.net.vars[k]) for k in model.net.vars)
    assert all(torch.equal(full.net.P[k], model.net.P[k]) for k in model.net.P.params)
    b = full.recommend_user(user=some, n_rec=10)
    assert np.array_equal(full.dyn_user_embedding(u, seq=seq), want)
    model.save(str(tmp_path), "cs_inf", inference_only=True)
    assert not os.path.exists(os.path.join(tmp_path, "cs_inf_variables.npz"))
    c = Caser.load(str(tmp_path), "cs_inf", info).recommend_user(user=some, n_rec=10)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with np.load(os.path.join(tmp_path, "cs_variables.npz")) as z:
        assert {"embedding/user_embeds_var", "embedding/seq_embeds_var", "embedding/item_embeds_var", "embedding/item_bias_var",
                "conv1d/kernel", "conv1d_5/bias", "conv1d_6/kernel", "dense/kernel", "dense/bias"} <= set(z.files)
        assert z["embedding/item_bias_var"].shape == (nI,) and z["conv1d/kernel"].shape == (1, 8, 3)
        assert z["conv1d_5/kernel"].shape == (6, 8, 3) and z["conv1d_6/kernel"].shape == (1, 6, 2)
        assert z["dense/kernel"].shape == (6 * 3 + 8 * 2, 8) and z["embedding/item_embeds_var"].shape == (nI, 16)
    # retraining on merged data with added users and items keeps old rows, moments and the step count; both pad rows move
    train2, info2 = DatasetPure.merge_trainset(new, info)
    assert info2.n_items > nI and info2.n_users > nU
    kw = dict(embed_size=8, n_epochs=1, lr=0.01, nh_filters=3, nv_filters=2, recent_num=6, seed=7)
    m2 = Caser("ranking", info2, **kw)
    m2.rebuild_model(str(tmp_path), "cs", full_assign=True)
    V1, V2 = model.net.vars, m2.net.vars
    for k in V1:
        n = nU if k == "user_embeds_var" else nI
        n2 = info2.n_users if k == "user_embeds_var" else info2.n_items
        assert torch.equal(V2[k][:n], V1[k][:n]) and torch.equal(m2.net.m[k][:n], model.net.m[k][:n]), k
        assert not bool(m2.net.m[k][n:n2].any()), k
    for k, n, n2 in (("seq_embeds_var", nI, info2.n_items), ("user_embeds_var", nU, info2.n_users)):
        assert torch.equal(V2[k][n2], V1[k][n]) and torch.equal(m2.net.v[k][n2], model.net.v[k][n]), k
        assert not torch.equal(V2[k][n], V1[k][n]), k                                # a new id's fresh row, not the old pad
    assert all(torch.equal(m2.net.P[k], model.net.P[k]) for k in model.net.P.params)
    assert torch.equal(m2.net.P.m, model.net.P.m) and m2.net.step == model.net.step > 0
    m3 = Caser("ranking", info2, **kw)
    m3.rebuild_model(str(tmp_path), "cs", full_assign=False)
    assert torch.equal(m3.net.vars["item_embeds_var"][:nI], V1["item_embeds_var"]) and m3.net.step == 0
    assert not bool(m3.net.m["item_embeds_var"].any()) and not bool(m3.net.P.m.any())
    m2.fit(train2, neg_sampling=True, verbose=0)
    assert m2.user_embeds.shape[0] == info2.n_users + 1 and m2.net.step > model.net.step
    # the convolution shapes depend on the window: a checkpoint of another `recent_num` is refused, by name
    for other in (4, 9):
        m4 = Caser("ranking", info2, **dict(kw, recent_num=other))
        with pytest.raises(ValueError, match="recent_num"):
            m4.rebuild_model(str(tmp_path), "cs", full_assign=True)


def test_rating_task_and_initialisers(dev, sample):
    old, _, _, info = sample
    train_data, info_r = DatasetPure.build_trainset(old)
    m = Caser("rating", info_r, embed_size=8, n_epochs=1, lr=0.01, nh_filters=12, seed=3)
    m.build_model()
    P = m.net.P
    lim = np.sqrt(6.0 / (3 * 8 + 3 * 12))                                            # Keras' convolution fans
    k2 = P["conv1d_2/kernel"].detach().cpu().numpy()
    assert k2.shape == (3, 8, 12) and np.abs(k2).max() <= lim and np.abs(k2).max() > 0.8 * lim
    assert not P["conv1d_2/bias"].detach().cpu().numpy().any()
    assert P["conv1d_10/kernel"].shape == (1, 10, 4) and P["dense/kernel"].shape == (10 * 12 + 8 * 4, 8)
    assert m.net.loss == "mse" and m.net.vars["seq_embeds_var"].shape == (info_r.n_items + 1, 8)
    assert m.net.vars["item_embeds_var"].shape == (info_r.n_items, 16)
    m.model_built = True
    m.fit(train_data, neg_sampling=False, verbose=0)
    p = m.predict(user=old.user.iloc[:5].tolist(), item=old.item.iloc[:5].tolist())
    assert ((np.asarray(p) >= 1) & (np.asarray(p) <= 5)).all()


def test_unsupported_shapes_raise_at_build(dev, sample):
    _, _, _, info = sample
    with pytest.raises(ValueError, match="1 to 64"):
        Caser("ranking", info, nh_filters=65).build_model()
    with pytest.raises(ValueError, match="1 to 64"):
        Caser("ranking", info, recent_num=65).build_model()
    with pytest.raises(ValueError, match="1 to 128"):
        Caser("ranking", info, embed_size=129).build_model()


def test_multi_rank_fit_raises(dev, sample, monkeypatch):
    _, _, train_data, info = sample
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        Caser("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
