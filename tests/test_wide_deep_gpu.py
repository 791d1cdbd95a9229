"""The FTRL-proximal kernels (csrc/ftrl.hip), `WideDeepNet` and `WideDeep` on the device against the f64 oracle
(tests/wide_deep_oracle.py) on the same seeded f32 inputs.  tests/test_wide_deep_cpu.py shows what the kernel cases hold.

Tolerances are the project's own for a row update against its oracle: rtol 1e-5 / atol 1e-6 where a row's run is short
(tests/test_ops_gpu.py:167-169); rtol 1e-4 / atol 2e-4 on the summed gradient of a long run (tests/test_ops_gpu.py:135),
propagated to `linear` through d linear / d g = 1 - (g / sqrt(new_accum)) / lr * var, |.| <= 1 + |var| / lr, and rtol 1e-4 on
`accum` and `var` of such a row; training steps as tests/test_autoint_gpu.py::test_training_steps."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import WideDeep
from librecommender_amd.data import DatasetFeat
from librecommender_amd.nets import FeatSpec, WideDeepNet
from oracle.make_golden import FEAT_KW, MULTI_KW, synthetic_frame

from . import wide_deep_oracle as O

pytestmark = pytest.mark.gpu

T, C = ops.FTRL_LONG_RUN, ops.FTRL_CHUNK
SLOTS = ("var", "accum", "linear")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run_rows(dev, c, **kw):
    """One `ops.ftrl_rows` call on a case -> (var, accum, linear) as numpy; `var` goes in as [V, 1], the slots as [V]."""
    var, accum, linear = _dev(c["var"].reshape(-1, 1), dev), _dev(c["accum"], dev), _dev(c["linear"], dev)
    ids = _dev(c["ids"], dev)
    seg = ops.build_segments(ids, c["V"])
    ops.ftrl_rows(var, accum, linear, _dev(c["grad"], dev), seg, c["lr"], c["l1"], c["l2"], **kw)
    return var.cpu().numpy().reshape(-1), accum.cpu().numpy(), linear.cpu().numpy()


def _check_rows(got, name):
    """Every element of the three arrays is compared: untouched rows by bits, short runs and long runs by their tolerances."""
    c, want, runs = O.oracle_rows(name, T, C)
    rows = want[3]
    rest = np.setdiff1d(np.arange(c["V"]), rows)
    short, long_ = rows[runs[rows] <= T], rows[runs[rows] > T]
    gsum, _ = O.scatter_sum(c["V"], c["ids"], c["grad"])
    compared = 0
    for k, g, w in zip(SLOTS, got, want[:3]):
        assert np.array_equal(g[rest], c[k][rest]), f"{name}: {k} of a row outside the stream changed"
        np.testing.assert_allclose(g[short], w[short], rtol=1e-5, atol=1e-6, err_msg=f"{name} {k} short runs")
        if k == "linear":
            tol = (1.0 + np.abs(c["var"][long_]) / c["lr"]) * (1e-4 * np.abs(gsum[long_]) + 2e-4) + 1e-5 * np.abs(w[long_]) + 1e-6
            assert (np.abs(g[long_] - w[long_]) <= tol).all(), f"{name} linear long runs"
        else:
            np.testing.assert_allclose(g[long_], w[long_], rtol=1e-4, atol=1e-6, err_msg=f"{name} {k} long runs")
        compared += len(rest) + len(short) + len(long_)
        if len(long_):
            print(f"WIDEDEEP-FIGURE {name} {k}: long runs max |diff| {np.abs(g[long_] - w[long_]).max():.3e}, "
                  f"short {np.abs(g[short] - w[short]).max() if len(short) else 0:.3e}")
    assert compared == 3 * c["V"], "share of compared elements below 100 %"
    return c, want, runs


# ---- 1. the row kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.KERNEL_CASES)
def test_rows_kernel(dev, name):
    c, want, runs = _check_rows(_run_rows(dev, O.kernel_case(name, T, C)), name)
    if name in ("boundaries", "two_valued", "dropped"):
        assert (runs > T).any() and (runs > C).any() or name == "dropped"
    if name == "threshold":
        got = _run_rows(dev, c)[0]
        assert c["var"][:5].all() and not got[:5].any()                    # zero gradient at fresh slots: exactly 0.0
        inside = np.abs(want[2]) <= c["l1"]
        assert inside.any() and (~inside).any() and got.any()


def test_rows_kernel_without_a_workspace(dev):
    """`ws=None`: every run is walked by one lane; the same tolerances (a serial f32 sum of 773 terms is inside them)."""
    _check_rows(_run_rows(dev, O.kernel_case("boundaries", T, C), ws=None), "boundaries")


def test_empty_stream(dev):
    c = O.kernel_case("collide", T, C)
    c = dict(c, ids=c["ids"][:0], grad=c["grad"][:0])
    got = _run_rows(dev, c)
    assert all(np.array_equal(g, c[k]) for k, g in zip(SLOTS, got))


# ---- 2. the dense kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", [0.0, 0.02])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4100])
def test_dense_kernel(dev, n, coef):
    c = O.dense_case(n, coef)
    t = [_dev(c[k], dev) for k in SLOTS]
    ops.ftrl_dense(*t, _dev(c["grad"], dev), c["lr"], c["l1"], c["l2"], l2_grad_coef=coef)
    want = O.ftrl_dense(c["var"], c["accum"], c["linear"], c["grad"], c["lr"], c["l1"], c["l2"], coef)
    for k, g, w in zip(SLOTS, t, want):
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-5, atol=1e-6, err_msg=f"{k} n={n}")


def test_dense_kernel_on_an_unaligned_range(dev):
    """A range that starts 4 bytes off a 16-byte boundary takes the scalar path."""
    c = O.dense_case(1023, 0.0)
    t = [_dev(np.concatenate([[0], c[k]]).astype(np.float32), dev)[1:] for k in SLOTS]
    ops.ftrl_dense(*t, _dev(c["grad"], dev), c["lr"])
    want = O.ftrl_dense(c["var"], c["accum"], c["linear"], c["grad"], c["lr"])
    for k, g, w in zip(SLOTS, t, want):
        np.testing.assert_allclose(g.cpu().numpy(), w, rtol=1e-5, atol=1e-6, err_msg=k)


def test_first_dense_step_with_a_zero_gradient_zeroes_var(dev):
    var = torch.rand(37, device=dev) - 0.5
    accum, linear = torch.full_like(var, ops.FTRL_INIT_ACCUM), torch.zeros_like(var)
    assert bool(var.all())
    ops.ftrl_dense(var, accum, linear, torch.zeros_like(var), 0.01)
    assert not bool(var.any()) and not bool(linear.any()) and bool((accum == ops.FTRL_INIT_ACCUM).all())


# ---- 3. bits, argument errors --------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):
    for name in ("boundaries", "two_valued"):
        c = O.kernel_case(name, T, C)
        a, b = _run_rows(dev, c), _run_rows(dev, c)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
    c = O.dense_case(4100, 0.02)
    runs = []
    for _ in range(2):
        t = [_dev(c[k], dev) for k in SLOTS]
        ops.ftrl_dense(*t, _dev(c["grad"], dev), c["lr"], l2_grad_coef=0.02)
        runs.append([x.cpu().numpy() for x in t])
    assert all(np.array_equal(x, y) for x, y in zip(*runs))


def test_argument_errors(dev):
    c = O.kernel_case("boundaries", T, C)
    with pytest.raises(RuntimeError, match="workspace"):                    # LR_EWORKSPACE
        _run_rows(dev, c, ws=torch.empty(64, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="shape mismatch"):
        _run_rows(dev, dict(c, grad=c["grad"][:-1]))
    with pytest.raises(ValueError, match="shape mismatch"):
        _run_rows(dev, dict(c, accum=c["accum"][:-1]))
    with pytest.raises(ValueError, match="scalar-row"):
        seg = ops.build_segments(_dev(c["ids"], dev), c["V"])
        z = torch.zeros((c["V"], 2), device=dev)
        ops.ftrl_rows(z, z.clone(), z.clone(), _dev(c["grad"], dev), seg, 0.01)
    z = torch.zeros(8, device=dev)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ftrl_dense(z, z.clone(), z.clone(), torch.zeros(7, device=dev), 0.01)
    with pytest.raises(ValueError, match="lr > 0"):
        ops.ftrl_dense(z, z.clone(), z.clone(), z.clone(), 0.0)
    with pytest.raises(ValueError, match="lr_ftrl_dense_f32"):               # LR_EINVAL from the entry point itself
        ops._call("lr_ftrl_dense_f32", z.data_ptr(), z.data_ptr(), z.data_ptr(), 8, z.data_ptr(), 0.0, 0.01, -1.0, 0.0, ops._stream())


# ---- 4. three consecutive training steps against the oracle ----------------------------------------------------------------------
PLAIN_KW = dict(sparse_col=FEAT_KW["sparse_col"], user_col=["sex", "occupation"], item_col=["genre1", "genre2", "genre3"])


def _frame():
    """The synthetic feature frame with its dense columns standardised (raw `profit` reaches 1e4: see tests/test_autoint_gpu.py)."""
    df = synthetic_frame()
    for col in ("age", "profit"):
        df[col] = (df[col] - df[col].mean()) / df[col].std()
    return df


@pytest.fixture(scope="module")
def feat_data():
    out = {}
    for tag, kw in (("plain", PLAIN_KW), ("feat", FEAT_KW), ("multi", MULTI_KW)):
        df = _frame()
        train_data, info = DatasetFeat.build_trainset(df, **kw)
        out[tag] = (df, train_data, info)
    return out


LR = {"wide": 0.01, "deep": 0.01}
# (data, loss, use_bn, dense_adam, reg, l1)
STEP_CONFIGS = [("plain", "cross_entropy", True, False, None, 1e-3), ("multi", "cross_entropy", True, False, None, 1e-3),
                ("multi", "focal", False, False, None, 1e-3), ("feat", "mse", True, False, None, 1e-3),
                ("multi", "cross_entropy", True, True, 0.01, 1e-3), ("feat", "cross_entropy", False, True, None, 1e-3),
                ("multi", "cross_entropy", True, False, None, 0.005)]


def _cfg_id(cfg):
    return "-".join(str(v) for v in cfg)


def _batch(ts, rng, loss, n=48):
    rows = rng.integers(0, len(ts.user_indices), n)
    labels = ts.labels[rows].astype(np.float32) if loss == "mse" else rng.integers(0, 2, n).astype(np.float32)
    return rows, dict(users=ts.user_indices[rows], items=ts.item_indices[rows], labels=labels,
                      sparse=ts.sparse_indices[rows], dense=None if ts.dense_values is None else ts.dense_values[rows],
                      loss_type=loss)


@pytest.mark.parametrize("cfg", STEP_CONFIGS, ids=_cfg_id)
def test_training_steps(dev, feat_data, cfg):
    """The net on the kernels against `WideDeepOracle` from the same weights: the loss to 1e-5, every table, slot, dense parameter
    and BatchNorm statistic to rtol 1e-4 / atol 5e-5 over three steps (`dropout_rate=None`: TF's mask cannot be reproduced)."""
    tag, loss, use_bn, dense_adam, reg, l1 = cfg
    _, ts, info = feat_data[tag]
    spec = FeatSpec.from_data_info(info, "sqrtn" if tag == "multi" else "normal")
    assert (tag == "multi") == bool(spec.pooled) and spec.n_dense_cols == (0 if tag == "plain" else 2)
    hidden = (16, 8)
    net = WideDeepNet(spec, 6, hidden, use_bn, None, LR, 1e-5, 11, dev, bool(dense_adam or reg), reg, l1=l1)
    t, P = net.tables, net.P
    lin0 = t.lin.clone()
    assert bool((t.lin_m == ops.FTRL_INIT_ACCUM).all()) and not bool(t.lin_v.any())
    a, b = net.wide_span
    assert bool((P.m[a:b] == ops.FTRL_INIT_ACCUM).all()) and not bool(P.m[:a].any()) and not bool(P.m[b:].any())
    assert P["wide_term/bias"].storage_offset() + 4 == b and (tag == "plain") == (P["wide_term/kernel"].storage_offset() == a)
    oracle = O.WideDeepOracle(O.export_state(net), spec, len(hidden), use_bn, LR, 1e-5, reg, dense_adam, l1)
    rng = np.random.default_rng(3)
    seen = []
    close = lambda got, want, what: torch.testing.assert_close(got.detach().cpu().double().reshape(want.shape), want, rtol=1e-4,
                                                               atol=5e-5, msg=lambda m: f"{what}: {m}")
    for step in range(1, 4):
        rows, batch = _batch(ts, rng, loss)
        want, got = oracle.train_step(**batch), float(net.train_step(**batch))
        print(f"WIDEDEEP-FIGURE step {_cfg_id(cfg)} {step}: loss {got:.8f} oracle {want:.8f}")
        assert abs(got - want) < 1e-5, (step, got, want)
        for k, ref in oracle.P.items():
            close(P[k], ref, f"{k} after step {step}")
        close(t.embed, oracle.embed, f"embed after step {step}")
        close(t.lin, oracle.lin, f"lin after step {step}")
        close(t.lin_m, oracle.accum["lin"], f"lin accumulator after step {step}")
        close(t.lin_v, oracle.linear["lin"], f"lin linear slot after step {step}")
        for k in oracle.WIDE:
            if k in oracle.P:
                pa = P[k].storage_offset()
                close(P.m[pa:pa + P[k].numel()], oracle.accum[k], f"{k} accumulator after step {step}")
                close(P.v[pa:pa + P[k].numel()], oracle.linear[k], f"{k} linear slot after step {step}")
        idx, fields = oracle._ids(batch["users"], batch["items"], batch["sparse"])
        seen.append(torch.cat([idx.reshape(-1)] + [fi.reshape(-1) for fi, _ in fields]))
    for key, bn in [("bn_in", net.mlp.bn_in)] + [(f"bn{i}", x) for i, x in enumerate(net.mlp.bns, start=1)]:
        if bn is not None:
            close(bn.moving_mean, oracle.bn[key][0], f"{key} moving mean")
            close(bn.moving_var, oracle.bn[key][1], f"{key} moving variance")
    sl = slice(0, 40)
    dense = None if ts.dense_values is None else ts.dense_values[sl]
    close(net.forward(ts.user_indices[sl], ts.item_indices[sl], sparse=ts.sparse_indices[sl], dense=dense),
          oracle.forward(ts.user_indices[sl], ts.item_indices[sl], ts.sparse_indices[sl], dense), "inference logits")
    # Adam left the wide range of the flat buffer to FTRL: its "moments" are an accumulator >= 0.1 and a linear slot
    assert bool((P.m[a:b] >= ops.FTRL_INIT_ACCUM).all())
    touched = torch.unique(torch.cat(seen)).to(dev)
    absent = torch.ones(t.V, dtype=torch.bool, device=dev)
    absent[touched] = False
    assert bool(absent.any())
    if not reg:       # rows of ids absent from the batches: bit-identical to their initial values, slots included
        assert torch.equal(t.lin[absent], lin0[absent]) and bool((t.lin_m[absent] == ops.FTRL_INIT_ACCUM).all())
        assert not bool(t.lin_v[absent].any())
    else:             # under `reg` every row moves every step
        assert bool((t.lin[absent] != lin0[absent]).all())
    if l1 > 1e-3 or tag == "multi":
        # the l1 proximal step is alive: some touched wide rows are exactly zero (|linear| <= l1; with l1 = 1e-3 the pooled
        # field's OOV row, which the stream touches with a zero gradient), others are not
        zero = (t.lin[touched] == 0).reshape(-1)
        print(f"WIDEDEEP-FIGURE step {_cfg_id(cfg)}: {int(zero.sum())} of {zero.numel()} touched wide rows are exactly zero")
        assert bool(zero.any()) and bool((~zero).any())
        assert (oracle.lin[touched.cpu()] == 0).equal(zero.cpu())


# ---- 5. the model --------------------------------------------------------------------------------------------------------------
def _fit(info, train_data, task="ranking", losses=None, **kw):
    model = WideDeep(task, info, **dict(dict(embed_size=8, n_epochs=3, lr=dict(LR), batch_size=64, seed=7, hidden_units=(32, 16)),
                                        **kw))
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
    per_epoch = torch.stack(losses).view(3, -1).mean(1).tolist()
    print(f"WIDEDEEP-FIGURE fit task={task} loss={loss} epoch means {per_epoch}")
    assert per_epoch[2] < per_epoch[0]
    p = np.asarray(model.predict(user=df.user.iloc[:5].tolist(), item=df.item.iloc[:5].tolist()))
    lo, hi = (0, 1) if task == "ranking" else (1, 5)
    assert ((p >= lo) & (p <= hi)).all()


def test_model_surface(dev, feat_data, tmp_path):
    df, train_data, info = feat_data["multi"]                              # plain sparse, multi-sparse and dense columns
    model = _fit(info, train_data, dropout_rate=0.2)
    net = model.net
    assert isinstance(net, WideDeepNet) and model._catalog_scorer() is None and set(model._batch_norms()) == {"mlp/bn_in", "mlp/bn1"}
    u = df.user.iloc[0]
    recs = model.recommend_user(user=u, n_rec=7)[u]
    consumed = {info.id2item[i] for i in info.user_consumed[info.user2id[u]]}
    assert len(recs) == 7 and not consumed & set(recs.tolist())
    cold = model.recommend_user(user="nobody", n_rec=5)["nobody"]
    assert len(cold) == 5
    assert len(model.recommend_user(user=u, n_rec=7, user_feats={"sex": "female", "occupation": "c"})[u]) == 7
    some = df.user.unique()[:10].tolist()
    pa = model.predict(user=df.user.iloc[:20].tolist(), item=df.item.iloc[:20].tolist())
    a = model.recommend_user(user=some, n_rec=5)
    model.save(str(tmp_path), "wd")
    full = WideDeep.load(str(tmp_path), "wd", info)
    assert full.lr == LR and torch.equal(full.net.P.flat, net.P.flat) and torch.equal(full.net.tables.lin, net.tables.lin)
    assert np.array_equal(pa, full.predict(user=df.user.iloc[:20].tolist(), item=df.item.iloc[:20].tolist()))
    b = full.recommend_user(user=some, n_rec=5)
    model.save(str(tmp_path), "wd_inf", inference_only=True)
    c = WideDeep.load(str(tmp_path), "wd_inf", info).recommend_user(user=some, n_rec=5)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with pytest.raises(NotImplementedError):
        model.save_tf_variables(str(tmp_path), "wd")


def test_rebuild_keeps_rows_slots_and_step(dev, tmp_path):
    from oracle.make_golden import retrain_frames

    old, new = retrain_frames()
    train0, info0 = DatasetFeat.build_trainset(old, **FEAT_KW)
    kw = dict(embed_size=8, n_epochs=1, lr=dict(LR), batch_size=64, seed=7, hidden_units=(32, 16))
    m0 = WideDeep("ranking", info0, **kw)
    m0.fit(train0, neg_sampling=True, verbose=0)
    m0.save(str(tmp_path), "m", inference_only=False)
    train1, info1 = DatasetFeat.merge_trainset(new, info0, merge_behavior=True)
    assert info1.n_users > info0.n_users and info1.n_items > info0.n_items
    m1 = WideDeep("ranking", info1, **kw)
    m1.rebuild_model(str(tmp_path), "m", full_assign=True)
    t0, t1, n0 = m0.net.tables, m1.net.tables, info0.n_users
    for name, n in (("user_embeds_var", n0), ("item_embeds_var", info0.n_items), ("user_linear_var", n0)):
        assert torch.equal(t1.variable(name)[:n], t0.variable(name)[:n]), name
    assert torch.equal(t1.lin_m[:n0], t0.lin_m[:n0]) and torch.equal(t1.lin_v[:n0], t0.lin_v[:n0]) and bool((t0.lin_m[:n0] > 0.1).any())
    assert torch.equal(t1.m[:n0], t0.m[:n0])
    # rows the merged data appended: accumulator 0.1 (a zero one would make the quadratic term of an untouched row zero)
    assert bool((t1.lin_m[n0:info1.n_users] == ops.FTRL_INIT_ACCUM).all()) and not bool(t1.lin_v[n0:info1.n_users].any())
    assert bool((t1.lin_m >= ops.FTRL_INIT_ACCUM).all())
    assert torch.equal(m1.net.P.flat, m0.net.P.flat) and torch.equal(m1.net.P.m, m0.net.P.m) and torch.equal(m1.net.P.v, m0.net.P.v)
    assert m1.net.step == m0.net.step > 0
    m2 = WideDeep("ranking", info1, **kw)
    m2.rebuild_model(str(tmp_path), "m", full_assign=False)
    a, b = m2.net.wide_span
    assert m2.net.step == 0 and torch.equal(m2.net.P.flat, m0.net.P.flat) and bool((m2.net.tables.lin_m == ops.FTRL_INIT_ACCUM).all())
    assert bool((m2.net.P.m[a:b] == ops.FTRL_INIT_ACCUM).all()) and not bool(m2.net.P.m[b:].any())
    m1.fit(train1, neg_sampling=True, verbose=0)
    assert m1.net.step > m0.net.step and len(m1.recommend_user(new["user"].iloc[0], 5)[new["user"].iloc[0]]) == 5
    assert bool(torch.isfinite(m1.net.tables.lin).all())


def test_lr_decay_changes_both_rates_on_schedule(dev, feat_data):
    _, train_data, info = feat_data["feat"]
    model = _fit(info, train_data, lr_decay=True, batch_size=128)
    decay_steps = max(1, int(info.data_size / 128))
    f = 0.96 ** ((model.net.step - 1) // decay_steps)                       # the schedule is applied before the step counts up
    assert model.net.step > decay_steps and f < 1.0
    assert model.net.lr == {"wide": LR["wide"] * f, "deep": LR["deep"] * f} and model.lr == LR


def test_multi_rank_fit_raises(dev, feat_data, monkeypatch):
    _, train_data, info = feat_data["feat"]
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        WideDeep("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
