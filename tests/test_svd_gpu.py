"""SVD / SVD++ on the device (csrc/svd.hip, algorithms/svd.py, algorithms/svdpp.py) against the CPU oracle
(tests/svd_oracle.py, f64 variant).  tests/test_svd_cpu.py shows that the oracle equals the reference graph and that the
oracle's own f32 arithmetic passes every tolerance used here on the same inputs."""
import json
import os

import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import SVD, SVDpp
from librecommender_amd.algorithms.svd import SvdNet
from librecommender_amd.data import DatasetPure, split_by_ratio_chrono
from librecommender_amd.evaluation import evaluate

from . import svd_oracle as O

pytestmark = pytest.mark.gpu

CLASSES = {"svd": SVD, "svdpp": SVDpp}


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def _delta_rule(got, want64, want32, what):
    """The project's rule for long f32 sums (test_bpr_gpu._against_oracle): the device within 10 x the oracle's own
    f32 / f64 gap on this very case, and no tighter than one f32 ulp of the largest value compared."""
    delta = O.max_diff([want32], [want64])
    gap = O.max_diff([got], [want64])
    bound = max(10 * delta, _ulp(want64))
    print(f"SVD-FIGURE {what} delta={delta:.3e} device={gap:.3e} bound={bound:.3e}")
    assert gap <= bound, what


class _Info:
    """The least a model needs of a `DataInfo` when the test drives the net itself."""
    global_mean, min_max_rating = 3.0, (1, 5)

    def __init__(self, n_users, n_items, user_consumed):
        self.n_users, self.n_items, self.user_consumed = n_users, n_items, user_consumed


# ---- 1. the history pool -----------------------------------------------------------------
def _check_pool(got, scale, P, Y, ptr, idx, rows, what):
    lens = np.diff(ptr)[np.arange(len(ptr) - 1) if rows is None else rows]
    want64, s64 = O.pool(P, Y, ptr, idx, rows, "f64", want_scale=True)
    want32 = O.pool(P, Y, ptr, idx, rows, "f32")
    short, empty = lens <= 31, lens == 0
    np.testing.assert_allclose(got[short], want64[short], rtol=1e-5, atol=1e-6)
    base = np.zeros_like(got) if P is None else P[np.arange(len(P)) if rows is None else rows]
    assert np.array_equal(got[empty], base[empty])            # an empty history returns P's row bit for bit
    if (~short).any():
        _delta_rule(got[~short], want64[~short], want32[~short], f"pool {what} K={Y.shape[1]} rows={len(lens)} longest={lens.max()}")
    np.testing.assert_allclose(scale, s64, rtol=1e-6, atol=0)


@pytest.mark.parametrize("K", [1, 8, 16, 20, 64, 128])
@pytest.mark.parametrize("n_rows", [1, 37, 1001])
def test_pool(dev, K, n_rows):
    """Histories of 0, 1, 2, 30, 31 and 300 entries (the last one by the delta rule), a repeated item, the last Y row and the
    last user; with P and without, by row list and over all users, and with a device-side row count."""
    P, Y, ptr, idx, rows = O.pool_case(K, n_rows)
    Pd, Yd, ptrd, idxd, rowsd = (_dev(x, dev) for x in (P, Y, ptr, idx, rows))
    for p, pd_ in ((P, Pd), (None, None)):
        got, scale = ops.svdpp_pool(pd_, Yd, ptrd, idxd, rows=rowsd, want_scale=True)
        _check_pool(got.cpu().numpy(), scale.cpu().numpy(), p, Y, ptr, idx, rows, "listed" if p is not None else "listed-noP")
        got, scale = ops.svdpp_pool(pd_, Yd, ptrd, idxd, want_scale=True)
        assert got.shape == (O.POOL_USERS, K)
        _check_pool(got.cpu().numpy(), scale.cpu().numpy(), p, Y, ptr, idx, None, "all" if p is not None else "all-noP")
    if n_rows > 1:                                            # only the leading rows the device-side count names
        k = n_rows // 2
        got = ops.svdpp_pool(Pd, Yd, ptrd, idxd, rows=rowsd, n_rows_dev=torch.tensor([k], dtype=torch.int32, device=dev))
        full = ops.svdpp_pool(Pd, Yd, ptrd, idxd, rows=rowsd)
        assert torch.equal(got[:k], full[:k])


# ---- 2. score, loss and dL/ds ------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 16, 20, 64, 128])
@pytest.mark.parametrize("B", [1, 37, 1001])
@pytest.mark.parametrize("loss", O.LOSSES)
def test_score(dev, K, B, loss):
    """Score, loss, g and the gradient rows against the f64 oracle; s = +-60 K for two samples (everything finite, |g| within
    gscale for the cross entropy); the same samples through a block of rows addressed per sample give the same bits."""
    X, Q, bu, bi, users, items, labels = O.score_case(K, B, loss)
    want = O.score(X, users, Q, bu, bi, users, items, labels, loss, 1.0 / B, "f64")
    Xd, Qd, bud, bid, ud, itd, yd = (_dev(x, dev) for x in (X, Q, bu, bi, users, items, labels))
    out = ops.mf_score(Xd, Qd, bud, bid, ud, itd, yd, loss, mode="grad", gscale=1.0 / B)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("score", "loss", "g"):
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for k in ("gx", "gq"):
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=1e-7, err_msg=k)
    if loss == "cross_entropy":
        assert (np.abs(got["g"]) <= np.float32(1.0 / B)).all()
    if B > 3:
        assert got["score"][0] > 55 * K and got["score"][1] < -55 * K
    plain = ops.mf_score(Xd, Qd, bud, bid, ud, itd, yd, loss, gscale=1.0 / B)
    assert set(plain) == {"score", "loss", "g"} and all(torch.equal(plain[k], out[k]) for k in plain)
    perm = np.random.default_rng(B).permutation(B)
    block, xidx = X[users][perm], np.argsort(perm).astype(np.int32)       # block[xidx[s]] = X[users[s]]
    out2 = ops.mf_score(_dev(block, dev), Qd, bud, bid, ud, itd, yd, loss, xidx=_dev(xidx, dev), mode="grad", gscale=1.0 / B)
    assert all(torch.equal(out2[k], out[k]) for k in out)


@pytest.mark.parametrize("loss", O.LOSSES)
def test_score_bad_ids(dev, loss):
    """u = n_users, i = -1, i = n_items + 5: g = 0, loss = 0 and zero rows; the other samples' outputs are untouched."""
    X, Q, bu, bi, users, items, labels = O.score_case(16, 50, loss)
    Xd, Qd, bud, bid, yd = (_dev(x, dev) for x in (X, Q, bu, bi, labels))
    clean = ops.mf_score(Xd, Qd, bud, bid, _dev(users, dev), _dev(items, dev), yd, loss, mode="grad", gscale=0.02)
    users, items = users.copy(), items.copy()
    users[3], items[7], items[9] = len(X), -1, len(Q) + 5
    out = ops.mf_score(Xd, Qd, bud, bid, _dev(users, dev), _dev(items, dev), yd, loss, mode="grad", gscale=0.02)
    bad = np.zeros(50, dtype=bool)
    bad[[3, 7, 9]] = True
    for k, v in out.items():
        v, c = v.cpu().numpy(), clean[k].cpu().numpy()
        assert not v[bad].any(), k
        assert np.array_equal(v[~bad], c[~bad]), k
    slots = np.arange(50, dtype=np.int32)
    slots[11] = 50                                            # a slot outside the block
    out = ops.mf_score(_dev(X[np.where(bad, 0, users)], dev), Qd, bud, bid, _dev(users, dev), _dev(items, dev), yd, loss,
                       xidx=_dev(slots, dev), mode="grad", gscale=0.02)
    bad[11] = True
    for k, v in out.items():
        v, c = v.cpu().numpy(), clean[k].cpu().numpy()
        assert not v[bad].any() and np.array_equal(v[~bad], c[~bad]), k


# ---- 3. the y gradient -------------------------------------------------------------------
def _hist_device(dev, case):
    ptr, idx, users, gx, Y, m, v = case
    B = len(users)
    seg_u = ops.build_segments(_dev(users, dev), O.HIST_USERS)
    G = ops.embed_segment_sum(_dev(gx, dev), seg_u)           # users occurring 50 times: summed before the fan-out
    _, scale = ops.svdpp_pool(None, _dev(Y, dev), _dev(ptr, dev), _dev(idx, dev), rows=seg_u.rows, n_rows_dev=seg_u.n_seg,
                              n_rows=B, want_scale=True)
    ent_idx, ent_slot, _ = O.entries(ptr, idx, np.unique(users))
    seg_y = ops.build_segments(_dev(ent_idx, dev), O.HIST_ITEMS)
    return G, scale, _dev(ent_slot, dev), seg_y


@pytest.mark.parametrize("K", [16, 64])
def test_hist_grad(dev, K):
    """1,001 distinct users over 200 items, item 0 in a run of 1,001 (longer than any chunk), item 199 in one history, ten empty
    histories, users that occur 50 times: the summed rows and the fused Adam step (non-zero m, v, step 3) by the delta rule;
    rows in no history keep their bits; two calls give equal bits."""
    case = O.hist_case(K)
    Y, m, v = case[4:]
    r64, r32 = O.hist_case_oracle(case, "f64"), O.hist_case_oracle(case, "f32")
    touched = r64[1]
    G, scale, ent_slot, seg_y = _hist_device(dev, case)
    runs = []
    for _ in range(2):
        grows = ops.svdpp_hist_grad(G, scale, ent_slot, seg_y)
        Yd, md, vd = _dev(Y, dev).clone(), _dev(m, dev).clone(), _dev(v, dev).clone()
        assert ops.svdpp_hist_grad(G, scale, ent_slot, seg_y, Y=Yd, m=md, v=vd, hp=ops.adam_hp(0.01, 3, eps=1e-5)) is None
        runs.append((grows, Yd, md, vd))
    ns = seg_y.count()
    assert runs[0][0].shape == (O.HIST_ITEMS, K)              # one row per y row at the most, never one per entry
    assert torch.equal(runs[0][0][:ns], runs[1][0][:ns])      # no float atomics: same bits (rows beyond n_seg are not written)
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))
    rows = seg_y.rows[:ns].cpu().numpy()
    assert np.array_equal(rows, touched) and 0 in rows and O.HIST_ITEMS - 1 in rows
    start = seg_y.start[:ns + 1].cpu().numpy()
    assert (np.diff(start)[rows == 0] == 1001).all() and (np.diff(start)[rows == O.HIST_ITEMS - 1] == 1).all()
    dense = np.zeros((O.HIST_ITEMS, K), dtype=np.float32)
    dense[rows] = runs[0][0][:ns].cpu().numpy()
    _delta_rule(dense, r64[0], r32[0], f"hist-rows K={K}")
    for name, got, i in (("Y", runs[0][1], 2), ("m", runs[0][2], 3), ("v", runs[0][3], 4)):
        _delta_rule(got.cpu().numpy(), r64[i], r32[i], f"hist-adam-{name} K={K}")
    untouched = np.setdiff1d(np.arange(O.HIST_ITEMS), touched)
    assert len(untouched) > 0
    for got, before in ((runs[0][1], Y), (runs[0][2], m), (runs[0][3], v)):
        assert np.array_equal(got.cpu().numpy()[untouched], before[untouched])


# ---- 4. three consecutive training steps -------------------------------------------------
def _stepped_net(dev, model, loss, dense, reg, norm, recent):
    """The net after three steps on the fixed batches, each step checked against the f64 oracle: loss within
    1e-5 max(1, |loss|), every variable within rtol 1e-4 / atol 2e-6 (tests/test_lightgcn_gpu.py:42-43)."""
    S = O.STEP_SHAPE
    hist = O.step_histories(recent)[1] if model == "svdpp" else None
    net = SvdNet(S["nu"], S["ni"], S["K"], S["lr"], 1e-5, reg, norm, dense, 11, dev, loss, with_history=model == "svdpp")
    params = O.step_params(model == "svdpp")
    assert set(params) == set(net.vars)
    for k, val in params.items():
        net.vars[k].copy_(_dev(val, dev).view_as(net.vars[k]))
    if hist is not None:
        net.set_history(*hist)
    adam = O.new_adam(params)
    for step, (u, i, y) in enumerate(O.step_batches(loss), 1):
        want = O.train_step(params, adam, u, i, y, loss, S["lr"], step, 1e-5, reg, norm, dense, hist, "f64")
        got = float(net.train_step(u, i, y))
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (step, got, want)
        for k in params:
            np.testing.assert_allclose(net.vars[k].cpu().numpy().reshape(params[k].shape), params[k], rtol=1e-4, atol=2e-6,
                                       err_msg=f"{k} after step {step}")
    return net, params, hist


def _cfg_id(cfg):
    return "-".join(str(x) for x in cfg)


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=_cfg_id)
def test_training_steps(dev, cfg):
    _stepped_net(dev, *cfg)


def test_training_step_reg_needs_dense(dev):
    with pytest.raises(ValueError, match="dense_adam=True"):
        SvdNet(5, 5, 8, 0.01, 1e-5, 0.01, False, False, 0, dev, "mse")


# ---- 5. the export of SVD++ --------------------------------------------------------------
@pytest.mark.parametrize("recent", [3, None])
def test_svdpp_set_embeddings(dev, recent):
    """After the three steps: user rows [z | bu | 1] with z over ALL users against the oracle (the pool's tolerance: these
    histories hold at most 9 entries), item rows [q | 1 | bi] bit for bit from the variables."""
    net, params, hist = _stepped_net(dev, "svdpp", "cross_entropy", False, None, False, recent)
    S = O.STEP_SHAPE
    model = SVDpp("ranking", _Info(S["nu"], S["ni"], O.step_histories(recent)[0]), embed_size=S["K"], recent_num=recent)
    model.device, model.net = dev, net
    model.set_embeddings()
    K = S["K"]
    dev_params = {k: v.cpu().numpy().reshape(params[k].shape) for k, v in net.vars.items()}
    U, I = O.export(dev_params, hist)
    got_u, got_i = model.user_embeds.cpu().numpy(), model.item_embeds.cpu().numpy()
    assert got_u.shape == (S["nu"], K + 2) and got_i.shape == (S["ni"], K + 2)
    np.testing.assert_allclose(got_u[:, :K], U[:, :K], rtol=1e-5, atol=1e-6)
    assert np.array_equal(got_u[:, K], dev_params["bu"]) and (got_u[:, K + 1] == 1).all()
    assert np.array_equal(got_u[0, :K], dev_params["pu"][0])             # user 0 has no history: z = p exactly
    assert np.array_equal(got_i[:, :K], dev_params["qi"]) and (got_i[:, K] == 1).all()
    assert np.array_equal(got_i[:, K + 1], dev_params["bi"])
    ptr, idx = model._set_sparse_interaction()                            # the model's own CSR is the one the net was given
    assert np.array_equal(ptr, hist[0]) and np.array_equal(idx, hist[1])


# ---- the model on the MovieLens sample ---------------------------------------------------
@pytest.fixture(scope="module")
def movielens():
    df = pd.read_csv(O.DATA, sep="::", engine="python", names=["user", "item", "label", "time"])
    train, evald = split_by_ratio_chrono(df, test_size=0.2)
    train_data, info = DatasetPure.build_trainset(train)
    eval_sets = {task: DatasetPure.build_evalset(evald) for task in ("rating", "ranking")}
    e = eval_sets["rating"]
    # the held-out rows, taken before any evaluation samples negatives into an eval set
    held = (np.array(e.user_indices), np.array(e.item_indices), np.array(e.labels, dtype=np.float64))
    return train, evald, train_data, eval_sets, info, held


@pytest.fixture(scope="module")
def small():
    df = pd.read_csv(O.DATA, sep="::", engine="python", names=["user", "item", "label", "time"]).iloc[:20000]
    train_data, info = DatasetPure.build_trainset(df)
    return train_data, info


# ---- 6. determinism ----------------------------------------------------------------------
@pytest.mark.parametrize("task", ["rating", "ranking"])
@pytest.mark.parametrize("name", ["svd", "svdpp"])
def test_two_fits_give_the_same_bits(dev, small, name, task):
    train_data, info = small
    tables = []
    for _ in range(2):
        m = CLASSES[name](task, info, n_epochs=1, lr=0.01, seed=7)
        m.fit(train_data, neg_sampling=task == "ranking", verbose=0)
        tables.append((m.user_embeds.clone(), m.item_embeds.clone()))
    assert torch.equal(tables[0][0], tables[1][0]) and torch.equal(tables[0][1], tables[1][1])
    assert bool(tables[0][1][:, -1].any())                    # it trained: the item biases moved


# ---- 7. model surface and quality --------------------------------------------------------
@pytest.mark.parametrize("task", ["rating", "ranking"])
@pytest.mark.parametrize("name", ["svd", "svdpp"])
def test_model_surface_and_quality(dev, movielens, tmp_path, name, task):
    train, evald, train_data, eval_sets, info, held = movielens
    eval_data, cls = eval_sets[task], CLASSES[name]
    with open(O.QUALITY) as f:
        q = json.load(f)
    hp = q["hyper"]
    K, sampling = hp["embed_size"], task == "ranking"
    kw = dict(loss_type=hp["loss_type"], embed_size=K, n_epochs=hp["n_epochs"], lr=hp["lr"], batch_size=hp["batch_size"],
              num_neg=hp["num_neg"], seed=42)
    if name == "svdpp":
        kw["recent_num"] = hp["recent_num"]
    model = cls(task, info, **kw)
    model.fit(train_data, neg_sampling=sampling, verbose=0)
    assert model.user_embeds.shape == (info.n_users + 1, K + 2) and model.item_embeds.shape == (info.n_items + 1, K + 2)
    assert model.user_embeds.is_cuda and bool((model.user_embeds[: info.n_users, K + 1] == 1).all())
    assert bool((model.item_embeds[: info.n_items, K] == 1).all())
    assert len(model.default_recs) == min(2000, info.n_items)
    # training learns as the oracle does: its worst seed plus (minus) its own spread over the seeds
    assert len(held[0]) == q["n_eval_pairs"]
    vals = q[f"{name}_{task}"]
    spread = max(vals) - min(vals)
    got = O.quality_metric(task, model.user_embeds_np, model.item_embeds_np, *held, info.n_items, info.min_max_rating)
    print(f"SVD-FIGURE quality model={name} task={task} device={got:.4f} oracle_min={min(vals):.4f} oracle_max={max(vals):.4f} "
          f"spread={spread:.4f}")
    if task == "rating":
        assert got <= max(vals) + spread
    else:
        assert got >= min(vals) - spread
    # predict / recommend
    u, i = train.user.iloc[0], train.item.iloc[0]
    preds = model.predict(user=train.user.iloc[:50].tolist(), item=train.item.iloc[:50].tolist())
    assert len(preds) == 50 and np.isfinite(preds).all()
    oov = model.predict(user=-999, item=i)
    uid, iid = info.n_users, info.item2id[i]
    raw = float(model.user_embeds[uid] @ model.item_embeds[iid])
    if task == "rating":
        lo, hi = info.min_max_rating
        assert (np.asarray(preds) >= lo).all() and (np.asarray(preds) <= hi).all()
        np.testing.assert_allclose(oov, np.clip(raw, lo, hi), rtol=1e-4)
    else:
        np.testing.assert_allclose(oov, 1.0 / (1.0 + np.exp(-raw)), rtol=1e-4)
    recs = model.recommend_user(user=u, n_rec=7)[u]
    assert len(recs) == 7 and not set(recs.tolist()) & set(train.item[train.user == u].tolist())
    cold = model.recommend_user(user=-999, n_rec=7)[-999]
    assert len(cold) == 7 and set(cold.tolist()) <= {info.id2item[j] for j in model.default_recs.tolist()}
    if task == "rating":
        res = evaluate(model, eval_data, neg_sampling=False, metrics=["rmse"])
        assert res["rmse"] < 1.146, res                       # the constant predictor (the training mean) on the held-out rows
    else:
        res = evaluate(model, eval_data, neg_sampling=True, metrics=["roc_auc", "precision"], k=10)
        assert res["roc_auc"] > 0.6, res
    model.init_knn(approximate=False, sim_type="cosine")
    assert len(model.search_knn_items(i, 5)) == 5 and len(model.search_knn_users(u, 5)) == 5
    # checkpoints: full, and the reference's inference layout
    users = train.user.unique()[:20].tolist()
    a = model.recommend_user(user=users, n_rec=10)
    model.save(str(tmp_path), name)
    full = cls.load(str(tmp_path), name, info)
    np.testing.assert_array_equal(full.predict(user=users[:5], item=[i] * 5), model.predict(user=users[:5], item=[i] * 5))
    assert all(torch.equal(full.net.vars[k], model.net.vars[k]) for k in model.net.vars)
    b = full.recommend_user(user=users, n_rec=10)
    model.save(str(tmp_path), name + "_inf", inference_only=True)
    assert not os.path.exists(os.path.join(tmp_path, name + "_inf_variables.npz"))
    with np.load(os.path.join(tmp_path, name + "_inf.npz")) as z:
        assert set(z.files) == {"user_embed", "item_embed"} and z["user_embed"].shape == (info.n_users + 1, K + 2)
    c = cls.load(str(tmp_path), name + "_inf", info).recommend_user(user=users, n_rec=10)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in users)
    with np.load(os.path.join(tmp_path, name + "_variables.npz")) as z:
        want_keys = {"embedding/bu_var", "embedding/pu_var", "embedding/bi_var", "embedding/qi_var"}
        want_keys |= {"embedding/yj_var"} if name == "svdpp" else set()
        assert {k for k in z.files if k.startswith("embedding/")} == want_keys
    # retraining on merged data keeps the old rows and, with `full_assign`, their moments and the step
    new = evald.copy()
    new["user"] = new["user"] + 10_000_000
    train2, info2 = DatasetPure.merge_trainset(new, info)
    m2 = cls(task, info2, **dict(kw, n_epochs=1))
    m2.rebuild_model(str(tmp_path), name, full_assign=True)
    assert torch.equal(m2.net.vars["pu"][: info.n_users], model.net.vars["pu"])
    assert torch.equal(m2.net.vars["bi"][: info.n_items], model.net.vars["bi"])
    assert torch.equal(m2.net.m["qi"][: info.n_items], model.net.m["qi"]) and m2.net.step == model.net.step > 0
    assert m2.net.vars["pu"].shape[0] == info2.n_users > info.n_users and not bool(m2.net.m["pu"][info.n_users:].any())
    if name == "svdpp":
        assert torch.equal(m2.net.vars["yj"][: info.n_items], model.net.vars["yj"])
        m3 = cls(task, info2, **dict(kw, n_epochs=1))
        m3.rebuild_model(str(tmp_path), name)                 # the reference's default: rows without optimiser state
        assert torch.equal(m3.net.vars["yj"][: info.n_items], model.net.vars["yj"]) and m3.net.step == 0
        assert not bool(m3.net.m["yj"].any())
        ptr = m2.net.hist_ptr.cpu().numpy()                   # histories of the new users are in the rebuilt CSR
        assert len(ptr) == info2.n_users + 1
        new_uid = info2.user2id[int(new.user.iloc[0])]
        assert new_uid >= info.n_users
        want = np.asarray(info2.user_consumed[new_uid][-hp["recent_num"]:])
        assert len(want) > 0 and np.array_equal(m2.net.hist_idx.cpu().numpy()[ptr[new_uid]:ptr[new_uid + 1]], want)
    m2.fit(train2, neg_sampling=sampling, verbose=0)
    assert m2.user_embeds.shape[0] == info2.n_users + 1 and m2.net.step > model.net.step


# ---- 8. multi-rank -----------------------------------------------------------------------
def test_multi_rank_fit_raises(dev, small, monkeypatch):
    train_data, info = small
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    for cls in (SVD, SVDpp):
        with pytest.raises(RuntimeError, match="single process"):
            cls("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)


def test_embed_size_limit_is_the_librarys(dev):
    from librecommender_amd.algorithms.svd import max_embed_size

    MAX_EMBED_SIZE = max_embed_size()
    assert ops.svd_supported(1) and ops.svd_supported(256) and ops.svd_supported(MAX_EMBED_SIZE)
    assert not ops.svd_supported(MAX_EMBED_SIZE + 1) and not ops.svd_supported(0)
