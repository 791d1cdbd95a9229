"""SVD / SVD++ without a GPU: the reference's signatures and checks, the history CSR, the oracle (tests/svd_oracle.py) against
the reference graph written literally in torch-CPU f64, and the oracle's own f32 variant inside every tolerance that
tests/test_svd_gpu.py applies on the device.

TensorFlow is not installed here, so the reference graph cannot be run; `graph_step` below is its literal transcription
(`svd.py:103-144`, `svdpp.py:102-135,196-214`, `tfops/loss.py`, `tf.train.AdamOptimizer`) under autograd."""
import inspect

import numpy as np
import pytest
import torch

from librecommender_amd.algorithms import SVD, SVDpp
from librecommender_amd.algorithms.svd import history_csr, max_embed_size

MAX_EMBED_SIZE = max_embed_size()

from . import svd_oracle as O

SVD_SIGNATURE = [
    ("task", inspect.Parameter.empty), ("data_info", inspect.Parameter.empty), ("loss_type", "cross_entropy"), ("embed_size", 16),
    ("norm_embed", False), ("n_epochs", 20), ("lr", 0.001), ("lr_decay", False), ("epsilon", 1e-5), ("reg", None),
    ("batch_size", 256), ("sampler", "random"), ("num_neg", 1), ("seed", 42), ("lower_upper_bound", None),
    ("tf_sess_config", None)]                                                    # svd.py:68-86
SVDPP_SIGNATURE = [
    ("task", inspect.Parameter.empty), ("data_info", inspect.Parameter.empty), ("loss_type", "cross_entropy"), ("embed_size", 16),
    ("n_epochs", 20), ("lr", 0.001), ("lr_decay", False), ("epsilon", 1e-5), ("reg", None), ("batch_size", 256),
    ("sampler", "random"), ("num_neg", 1), ("seed", 42), ("recent_num", 30), ("lower_upper_bound", None),
    ("tf_sess_config", None)]                                                    # svdpp.py:66-84


class Info:
    n_users, n_items, global_mean, min_max_rating = 5, 7, 3.0, (1, 5)
    user_consumed = {0: [1, 2, 2, 3], 1: [], 2: [6], 3: [0, 1, 2, 3, 4, 5], 4: [3, 3]}


# ---- signatures and checks ---------------------------------------------------------------
@pytest.mark.parametrize("cls,sig", [(SVD, SVD_SIGNATURE), (SVDpp, SVDPP_SIGNATURE)])
def test_reference_signature(cls, sig):
    params = list(inspect.signature(cls.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params[: len(sig)]] == sig
    assert [p.name for p in params[len(sig):]] == ["device", "dense_adam"]          # package-only keywords behind them
    assert [(p.name, p.default) for p in params[len(sig):]] == [("device", "cuda"), ("dense_adam", False)]


def test_rebuild_model_defaults():
    assert inspect.signature(SVD.rebuild_model).parameters["full_assign"].default is True
    assert inspect.signature(SVDpp.rebuild_model).parameters["full_assign"].default is False       # svdpp.py:216
    for cls in (SVD, SVDpp):
        assert list(inspect.signature(cls.rebuild_model).parameters) == ["self", "path", "model_name", "full_assign"]


@pytest.mark.parametrize("recent_num", [0, -1, 2.5])
def test_wrong_recent_num(recent_num):
    with pytest.raises(AssertionError, match="`recent_num` must be None or positive int"):
        SVDpp("ranking", Info(), recent_num=recent_num)._set_sparse_interaction()


@pytest.mark.parametrize("cls", [SVD, SVDpp])
def test_constructor_checks(cls):
    with pytest.raises(ValueError, match="unsupported `loss_type`"):
        cls("ranking", Info(), loss_type="bpr")
    with pytest.raises(ValueError, match="dense_adam=True"):
        cls("ranking", Info(), reg=0.01)
    cls("ranking", Info(), reg=0.01, dense_adam=True)
    with pytest.raises(ValueError, match="embed_size"):
        cls("rating", Info(), embed_size=MAX_EMBED_SIZE + 1)
    with pytest.raises(ValueError, match="embed_size"):
        cls("rating", Info(), embed_size=0)
    assert MAX_EMBED_SIZE >= 256
    m = cls("rating", Info(), embed_size=256, tf_sess_config={"anything": 1})
    assert m.embed_size == 256 and m.net is None
    with pytest.raises(ValueError, match="task must either be rating or ranking"):
        cls("other", Info())


# ---- the history CSR ---------------------------------------------------------------------
def test_history_csr_small():
    ptr, idx = history_csr(Info.user_consumed, 5, 2)
    assert ptr.tolist() == [0, 2, 2, 3, 5, 7] and idx.tolist() == [2, 3, 6, 4, 5, 3, 3]       # repeats kept, empty user
    assert ptr.dtype == np.int64 and idx.dtype == np.int32


@pytest.fixture(scope="module")
def movielens():
    return O.movielens()


@pytest.mark.parametrize("recent_num", [30, 1, None])
def test_history_csr_equals_the_reference_loop(movielens, recent_num):
    info = movielens[4]
    ptr, idx = history_csr(info.user_consumed, info.n_users, recent_num)
    rows, vals = O.history_loop(info.user_consumed, info.n_users, recent_num)
    assert np.array_equal(np.repeat(np.arange(info.n_users), np.diff(ptr)), rows) and np.array_equal(idx, vals)
    longest = int(np.diff(ptr).max())
    assert longest == (max(len(v) for v in info.user_consumed.values()) if recent_num is None else recent_num)
    if recent_num is None:
        assert longest > 150          # `recent_num=None` is real input: one user of the training split consumed 186 items


# ---- the oracle against the literal graph ------------------------------------------------
def graph_gradients(params, users, items, labels, loss, reg, norm_embed, hist):
    """The reference graph in torch f64: variables, (for SVD++) the sqrtn pooling of EVERY user's history and the gather,
    the output, the loss, the l2 regulariser on the variables, autograd.  Returns (loss, {name: gradient}, {name: the rows
    the IndexedSlices gradient names})."""
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    iu, ii = torch.as_tensor(np.asarray(users, dtype=np.int64)), torch.as_tensor(np.asarray(items, dtype=np.int64))
    y = torch.as_tensor(np.asarray(labels, dtype=np.float64))
    touched = {"bu": np.unique(users), "pu": np.unique(users), "bi": np.unique(items), "qi": np.unique(items)}
    if hist is not None:
        ptr, idx = hist
        lens = torch.as_tensor(np.diff(ptr))
        bags = torch.nn.functional.embedding_bag(torch.as_tensor(idx.astype(np.int64)), t["yj"], torch.as_tensor(ptr[:-1]),
                                                 mode="sum", include_last_offset=False) if len(idx) else torch.zeros_like(t["pu"])
        uj = bags / torch.sqrt(torch.clamp(lens.double(), min=1.0))[:, None]        # combiner="sqrtn"; empty bags are zero
        all_user_embeds = t["pu"] + uj                                            # svdpp.py:214
        eu = all_user_embeds[iu]
        touched["yj"] = np.unique(np.concatenate([idx[ptr[u]:ptr[u + 1]] for u in np.unique(users)] + [np.zeros(0, np.int32)]))
    else:
        eu = t["pu"][iu]
    eq = t["qi"][ii]
    if norm_embed:
        eu = eu * torch.rsqrt(torch.clamp((eu * eu).sum(1, keepdim=True), min=1e-12))
        eq = eq * torch.rsqrt(torch.clamp((eq * eq).sum(1, keepdim=True), min=1e-12))
    out = t["bu"][iu] + t["bi"][ii] + torch.einsum("ij,ij->i", eu, eq)
    if loss == "mse":
        L = torch.nn.functional.mse_loss(out, y)
    elif loss == "cross_entropy":
        L = torch.nn.functional.binary_cross_entropy_with_logits(out, y)
    else:                                                                         # tfops/loss.py:56-62
        w = y * 0.25 + (1 - y) * 0.75
        p = torch.sigmoid(out)
        p_t = y * p + (1 - y) * (1 - p)
        L = (w * (1 - p_t) ** 2.0 * torch.nn.functional.binary_cross_entropy_with_logits(out, y, reduction="none")).mean()
    total = L + (sum(reg * (x * x).sum() for x in t.values()) if reg else 0.0)
    total.backward()
    return float(L.detach()), {k: v.grad.numpy() for k, v in t.items()}, touched


def graph_step(params, adam, users, items, labels, loss, lr, step, epsilon, reg, norm_embed, dense, hist):
    """`graph_gradients`, then TF1 Adam on the rows the IndexedSlices gradient names (or on every row)."""
    L, grads, touched = graph_gradients(params, users, items, labels, loss, reg, norm_embed, hist)
    lr_t = lr * np.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)
    for name, w_ in params.items():
        g = grads[name]
        m, v = adam[name]
        rows = slice(None) if dense else touched[name]
        m[rows] = (0.9 * m[rows].astype(np.float64) + (1.0 - 0.9) * g[rows]).astype(np.float32)
        v[rows] = (0.999 * v[rows].astype(np.float64) + (1.0 - 0.999) * g[rows] ** 2).astype(np.float32)
        w_[rows] = (w_[rows].astype(np.float64) - lr_t * m[rows] / (np.sqrt(v[rows].astype(np.float64)) + epsilon)).astype(np.float32)
    return L


def _run_steps(stepper, model, loss, dense, reg, norm, recent, **kw):
    hist = O.step_histories(recent)[1] if model == "svdpp" else None
    params = O.step_params(model == "svdpp")
    adam = O.new_adam(params)
    losses = []
    for step, (u, i, y) in enumerate(O.step_batches(loss), 1):
        losses.append(stepper(params, adam, u, i, y, loss, O.STEP_SHAPE["lr"], step, 1e-5, reg, norm, dense, hist, **kw))
    return losses, params, adam


def _ids(cfg):
    return "-".join(str(x) for x in cfg)


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=_ids)
def test_oracle_step_equals_the_literal_graph(cfg):
    """Hand-derived gradients (the pool over the batch's distinct users, G_u summed before the fan-out, |N|^-1/2) against
    autograd through the all-user pooling: three steps, loss to 1e-12 and every variable and moment bit for bit or to
    1e-12 before the f32 store (an f32 store of two f64 values 1e-12 apart can differ by one ulp)."""
    la, pa, aa = _run_steps(O.train_step, *cfg)
    lb, pb, ab = _run_steps(graph_step, *cfg)
    np.testing.assert_allclose(la, lb, rtol=0, atol=1e-12)
    for k in pa:
        ulp = np.spacing(np.abs(pb[k]).max().astype(np.float32))
        assert np.abs(pa[k].astype(np.float64) - pb[k]).max() <= ulp, k
        assert (pa[k] != pb[k]).mean() < 0.01, k
        for x, y in zip(aa[k], ab[k]):
            assert np.abs(x.astype(np.float64) - y).max() <= np.spacing(np.float32(np.abs(y).max())), k


GRAD_CONFIGS = sorted({(m, l, r, n, rc) for m, l, _, r, n, rc in O.STEP_CONFIGS}, key=str)


@pytest.mark.parametrize("cfg", GRAD_CONFIGS, ids=_ids)
def test_oracle_raw_gradients_equal_the_literal_graph(cfg):
    """Before any f32 store: loss, every gradient (the `reg` term and the backward through `norm_embed` included) and the
    touched rows of the hand-derived backward against autograd through the literal graph, to 1e-12, on all three batches."""
    model, loss, reg, norm, recent = cfg
    hist = O.step_histories(recent)[1] if model == "svdpp" else None
    params = O.step_params(model == "svdpp")
    for u, i, y in O.step_batches(loss):
        la, ga, ta = O.gradients(params, u, i, y, loss, reg, norm, hist)
        lb, gb, tb = graph_gradients(params, u, i, y, loss, reg, norm, hist)
        assert abs(la - lb) <= 1e-12 and set(ga) == set(gb) == set(params)
        for k in ga:
            np.testing.assert_allclose(ga[k], gb[k], rtol=0, atol=1e-12, err_msg=k)
            assert np.array_equal(ta[k], tb[k]), k


def test_oracle_gradients_equal_autograd_to_1e12():
    """One step's raw gradients (before any f32 store): the oracle's formulas against autograd, 1e-12."""
    hist = O.step_histories(None)[1]
    params = O.step_params(True)
    u, i, y = O.step_batches("focal")[0]
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    ptr, idx = hist
    z = torch.stack([t["pu"][r] + (t["yj"][idx[ptr[r]:ptr[r + 1]].astype(np.int64)].sum(0) / np.sqrt(max(ptr[r + 1] - ptr[r], 1)))
                     for r in range(len(ptr) - 1)])
    iu, ii = torch.as_tensor(u.astype(np.int64)), torch.as_tensor(i.astype(np.int64))
    out = t["bu"][iu] + t["bi"][ii] + (z[iu] * t["qi"][ii]).sum(1)
    yy = torch.as_tensor(y.astype(np.float64))
    p = torch.sigmoid(out)
    L = ((yy * 0.25 + (1 - yy) * 0.75) * (1 - (yy * p + (1 - yy) * (1 - p))) ** 2
         * torch.nn.functional.binary_cross_entropy_with_logits(out, yy, reduction="none")).mean()
    L.backward()
    du, slot = np.unique(u, return_inverse=True)
    zz, scale = O.pool(params["pu"], params["yj"], ptr, idx, rows=du, want_scale=True)
    res = O.score(zz, slot, params["qi"], params["bu"], params["bi"], u, i, y, "focal", gscale=1.0 / len(u))
    G = np.zeros((len(du), zz.shape[1]))
    np.add.at(G, slot, res["gx"])
    ent_idx, ent_slot, _ = O.entries(ptr, idx, du)
    gy = O.hist_grad(G, scale, ent_idx, ent_slot, len(params["qi"]))
    np.testing.assert_allclose(gy, t["yj"].grad.numpy(), rtol=0, atol=1e-12)
    gq = np.zeros_like(gy)
    np.add.at(gq, i, res["gq"])
    np.testing.assert_allclose(gq, t["qi"].grad.numpy(), rtol=0, atol=1e-12)
    assert abs(res["loss"].mean() - float(L.detach())) < 1e-12


# ---- the f32 variant as a yardstick ------------------------------------------------------
POOL_K, POOL_ROWS = [1, 8, 16, 20, 64, 128], [1, 37, 1001]


@pytest.mark.parametrize("K", POOL_K)
@pytest.mark.parametrize("n_rows", POOL_ROWS)
def test_f32_pool_inside_the_device_tolerance(K, n_rows):
    P, Y, ptr, idx, rows = O.pool_case(K, n_rows)
    for p in (P, None):
        a, b = O.pool(p, Y, ptr, idx, rows, "f64"), O.pool(p, Y, ptr, idx, rows, "f32")
        short = np.diff(ptr)[rows] <= 31
        np.testing.assert_allclose(b[short], a[short], rtol=1e-5, atol=1e-6)
        empty = np.diff(ptr)[rows] == 0
        assert np.array_equal(b[empty], (P[rows] if p is not None else np.zeros_like(b))[empty])
    assert (np.diff(ptr) == 300).sum() == 1 and (n_rows == 1 or (~short).any())


@pytest.mark.parametrize("K", POOL_K)
@pytest.mark.parametrize("B", POOL_ROWS)
@pytest.mark.parametrize("loss", O.LOSSES)
def test_f32_score_inside_the_device_tolerance(K, B, loss):
    X, Q, bu, bi, users, items, labels = O.score_case(K, B, loss)
    a = O.score(X, users, Q, bu, bi, users, items, labels, loss, 1.0 / B, "f64")
    b = O.score(X, users, Q, bu, bi, users, items, labels, loss, 1.0 / B, "f32")
    for k in ("score", "loss", "g"):
        assert np.isfinite(b[k]).all() and np.isfinite(a[k]).all()
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=1e-6, err_msg=k)
    for k in ("gx", "gq"):
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=1e-7, err_msg=k)
    if loss == "cross_entropy":
        assert (np.abs(a["g"]) <= 1.0 / B).all()
    if B > 3:
        assert a["score"][0] > 55 * K and a["score"][1] < -55 * K


@pytest.mark.parametrize("K", [16, 64])
def test_f32_hist_grad_has_a_usable_delta(K):
    """The 10 x delta rule needs a delta: the f32 variant differs from f64 on this case, and by less than 1e-5."""
    case = O.hist_case(K)
    ptr, idx = case[0], case[1]
    assert (idx == 0).sum() == 1001 and (idx == O.HIST_ITEMS - 1).sum() == 1 and (np.diff(ptr) == 0).sum() == 10
    assert np.bincount(case[2], minlength=O.HIST_USERS).min() >= 1 and np.bincount(case[2])[:20].min() >= 50
    a, b = O.hist_case_oracle(case, "f64"), O.hist_case_oracle(case, "f32")
    for x, y in zip(a[2:], b[2:]):
        assert 0 < O.max_diff([x], [y]) < 1e-5
    assert 0 < O.max_diff([a[0]], [b[0]]) < 1e-5
    untouched = np.setdiff1d(np.arange(O.HIST_ITEMS), a[1])
    assert len(untouched) >= 19
    assert np.array_equal(a[2][untouched], case[4][untouched])


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=_ids)
def test_f32_steps_inside_the_device_tolerance(cfg):
    la, pa, _ = _run_steps(O.train_step, *cfg, variant="f64")
    lb, pb, _ = _run_steps(O.train_step, *cfg, variant="f32")
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * max(1.0, abs(x))
    for k in pa:
        np.testing.assert_allclose(pb[k], pa[k], rtol=1e-4, atol=2e-6, err_msg=k)


def test_quality_fixture_is_what_the_oracle_writes():
    """The committed fixture has the oracle's hyper-parameters and one figure per seed; one of them is recomputed."""
    import json

    with open(O.QUALITY) as f:
        q = json.load(f)
    assert q["hyper"] == O.HYPER and q["seeds"] == O.SEEDS
    for key in ("svd_rating", "svd_ranking", "svdpp_rating", "svdpp_ranking"):
        assert len(q[key]) == len(O.SEEDS) and all(np.isfinite(q[key]))
    _, _, train_data, eval_data, info = O.movielens()
    users, items = np.asarray(train_data.user_indices), np.asarray(train_data.item_indices)
    p = O.quality_train("svd", "rating", users, items, np.asarray(train_data.labels, dtype=np.float32), info.n_users, info.n_items,
                        None, O.SEEDS[0])
    U, I = O.export(p)
    got = O.quality_metric("rating", O.with_oov(U), O.with_oov(I), np.asarray(eval_data.user_indices),
                           np.asarray(eval_data.item_indices), np.asarray(eval_data.labels, dtype=np.float64), info.n_items,
                           info.min_max_rating)
    assert abs(got - q["svd_rating"][0]) < 1e-9
