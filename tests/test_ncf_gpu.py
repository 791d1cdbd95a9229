"""The NCF kernels (csrc/ncf.hip), the `K > 0, F = 0` form of `DeepFMTail`, `NCFNet` and `NCF` on the device against the f64 oracle
(tests/ncf_oracle.py) on the same seeded f32 inputs.  tests/test_ncf_cpu.py checks the oracle itself.

Tolerances.  pair_fwd: bits against numpy f32.  pair_bwd: rtol 1e-6 against f64 (two roundings; the case keeps G away from
cancellation).  score: the project's rule for a fused stack forward against its f64 oracle, the delta rule of
tests/test_autoint_gpu.py::test_stack (`delta_bound` of tests/wavenet_oracle.py: 10 x the oracle's own f32 / f64 gap, no tighter
than one f32 ulp of the largest value per layer passed through, the read-out counting as a layer); the gap is taken over the
whole 4,097-pair case a run's pairs are a prefix of, so that a run of one pair is not judged by the luck of one f32 sum.
Tail and training steps: the loss to 1e-5, O(1) quantities to rtol 1e-4 / atol 5e-5 as tests/test_autoint_gpu.py::
test_training_steps and tests/test_feat_block_gpu.py; the per-sample gradients gl and gz1 of a mean loss are of order 1 / B, so
their atol is 5e-5 / B."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import NCF
from librecommender_amd.data import DatasetFeat, DatasetPure
from librecommender_amd.layers.tail import DeepFMTail
from librecommender_amd.nets import NCFNet
from oracle.make_golden import FEAT_KW, retrain_frames, synthetic_frame

from . import ncf_oracle as O
from .wavenet_oracle import delta_bound, max_diff

pytestmark = pytest.mark.gpu

PAD, MARK = 3, 7.0          # rows allocated past the batch and the value they must keep


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the pair kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16, 32, 128])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_pair_kernels(dev, B, K):
    c = O.pair_case(B, K)
    want_x, want_gmf, want_G = O.pair_ref(c)
    if B >= 5:
        ok = (c["idx"] >= 0) & (c["idx"] < c["V"])
        assert (~ok).sum() == 2 and len(np.unique(c["idx"], axis=0)) < B and (c["idx"] == [O.N_USERS, c["V"] - 1]).all(1).any()
    table, idx = _dev(c["table"], dev), _dev(c["idx"], dev)
    x = torch.full((B + PAD, 2 * K), MARK, device=dev)
    gmf = torch.full((B + PAD, K), MARK, device=dev)
    ops.ncf_pair_fwd(table, idx, x, gmf)
    assert np.array_equal(_bits(x[:B].cpu().numpy()), _bits(want_x)), "x differs from the gathered rows"
    assert np.array_equal(_bits(gmf[:B].cpu().numpy()), _bits(want_gmf)), "gmf is not the f32 product, bit for bit"
    assert bool((x[B:] == MARK).all()) and bool((gmf[B:] == MARK).all())
    G = torch.full((B + PAD, 2 * K), MARK, device=dev)
    G[:B] = _dev(c["G"], dev)
    x0 = x.clone()
    ops.ncf_pair_bwd_(x, _dev(c["gl"], dev), _dev(c["wg"], dev), G, B)
    np.testing.assert_allclose(G[:B].cpu().numpy().astype(np.float64), want_G, rtol=1e-6, atol=0)
    assert bool((G[B:] == MARK).all()) and torch.equal(x, x0)
    assert np.array_equal(table.cpu().numpy(), c["table"]), "a table row changed"
    # the allocating form gives the same bits
    x2, gmf2 = ops.ncf_pair_fwd(table, idx)
    assert torch.equal(x2, x[:B]) and torch.equal(gmf2, gmf[:B])


def test_pair_argument_errors(dev):
    c = O.pair_case(64, 16)
    table, idx = _dev(c["table"], dev), _dev(c["idx"], dev)
    with pytest.raises(ValueError, match="K % 4"):
        ops.ncf_pair_fwd(torch.zeros((10, 6), device=dev), idx)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_pair_fwd(table, torch.zeros((4, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_pair_fwd(table, idx, torch.zeros((63, 32), device=dev))
    x, _ = ops.ncf_pair_fwd(table, idx)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_pair_bwd_(x, torch.zeros(65, device=dev), torch.zeros(16, device=dev), torch.zeros_like(x))
    off = torch.zeros(c["V"] * 16 + 1, device=dev)[1:].view(c["V"], 16)          # 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="lr_ncf_pair_fwd_f32"):                  # LR_EINVAL from the entry point itself
        ops.ncf_pair_fwd(off, idx)
    e = torch.zeros((0, 2), dtype=torch.int32, device=dev)
    x0, g0 = ops.ncf_pair_fwd(table, e)                                          # B == 0: nothing is launched
    assert x0.shape == (0, 32) and g0.shape == (0, 16)


# ---- 2. the score kernel -----------------------------------------------------------------------------------------------------
def _score_inputs(dev, c):
    lst = lambda xs: [None if x is None else _dev(x, dev) for x in xs]
    return (_dev(c["table"], dev), _dev(c["users"], dev), _dev(c["items"], dev), lst(c["W"]), lst(c["b"]), lst(c["s"]), lst(c["t"]),
            _dev(c["wg"], dev), _dev(c["wd"], dev), c["c"])


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("K", O.SCORE_KS)
@pytest.mark.parametrize("widths", O.SCORE_STACKS, ids=lambda w: "x".join(map(str, w)))
def test_score(dev, widths, K, affine):
    c = O.score_case(K, widths, affine)
    table, users, items, W, b, s, t, wg, wd, cc = _score_inputs(dev, c)
    assert ops.ncf_score_supported(K, widths) == O.score_envelope(K, widths)
    if not O.score_envelope(K, widths):
        out = torch.full((130,), MARK, device=dev)
        with pytest.raises(ValueError, match="shape not supported"):             # LR_ESHAPE, and nothing is written
            ops.ncf_score(table, users[:130].contiguous(), items[:130].contiguous(), W, b, s, t, wg, wd, cc, out=out)
        assert bool((out == MARK).all())
        return
    assert all((x is not None) == (affine and l < len(widths) - 1) for l, x in enumerate(s))
    want64, want32 = O.score_ref(K, widths, affine, "f64"), O.score_ref(K, widths, affine, "f32")
    bound = delta_bound(want64, want32, len(widths) + 1)
    worst = 0.0
    for n in O.SCORE_NS:
        u, i = users[:n].contiguous(), items[:n].contiguous()
        out = torch.full((n + PAD,), MARK, device=dev)
        ops.ncf_score(table, u, i, W, b, s, t, wg, wd, cc, out=out)
        got = out[:n].cpu().numpy()
        gap = max_diff(got, want64[:n])
        worst = max(worst, gap)
        assert np.isfinite(got).all() and gap <= bound, f"n={n}: largest difference {gap:.3e}, bound {bound:.3e}"
        assert bool((out[n:] == MARK).all()), f"n={n}: wrote past the last pair"
        again = ops.ncf_score(table, u, i, W, b, s, t, wg, wd, cc)
        assert torch.equal(again, out[:n]), f"n={n}: two calls differ"
    print(f"NCF-FIGURE score K={K} widths={widths} affine={affine}: delta={max_diff(want32, want64):.3e} got={worst:.3e} bound={bound:.3e}")
    assert np.array_equal(table.cpu().numpy(), c["table"]), "a table row changed"


def test_score_argument_errors(dev):
    c = O.score_case(16, (32, 16), True)
    table, users, items, W, b, s, t, wg, wd, cc = _score_inputs(dev, c)
    u, i = users[:64].contiguous(), items[:64].contiguous()
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_score(table, u, items[:63].contiguous(), W, b, s, t, wg, wd, cc)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_score(table, u, i, W, b[:1], s, t, wg, wd, cc)
    with pytest.raises(ValueError, match="shape mismatch"):
        ops.ncf_score(table, u, i, W, b, s, t, wg, wd[:-1].contiguous(), cc)
    with pytest.raises(ValueError, match="together"):
        ops.ncf_score(table, u, i, W, b, s, [None, None], wg, wd, cc)
    W24 = [torch.zeros((32, 24), device=dev), torch.zeros((24, 16), device=dev)]
    with pytest.raises(ValueError, match="shape not supported"):
        ops.ncf_score(table, u, i, W24, [torch.zeros(24, device=dev), b[1]], None, None, wg, wd, cc)
    e = users[:0].contiguous()
    assert ops.ncf_score(table, e, e, W, b, s, t, wg, wd, cc).shape == (0,)      # n == 0: nothing is launched
    # `s` / `t` omitted altogether: the identity, the bits of the plain case
    p = O.score_case(16, (32, 16), False)
    args = _score_inputs(dev, p)
    a = ops.ncf_score(*args[:3], args[3], args[4], None, None, *args[7:])
    assert torch.equal(a, ops.ncf_score(*args))


# ---- 3. `DeepFMTail` with K > 0, F = 0 ----------------------------------------------------------------------------------------
def load_state(net, state):
    """Copy an oracle state (tests/ncf_oracle.py: `random_state`) into a net."""
    with torch.no_grad():
        net.tables.embed.copy_(_dev(state["embed"], net.device))
        for k, v in state["P"].items():
            net.P[k].copy_(_dev(v, net.device))
        for k, bn in [("bn_in", net.mlp.bn_in)] + [(f"bn{i}", x) for i, x in enumerate(net.mlp.bns, start=1)]:
            if bn is not None:
                bn.moving_mean.copy_(_dev(state["bn"][k][0], net.device))
                bn.moving_var.copy_(_dev(state["bn"][k][1], net.device))
    return net


@pytest.mark.parametrize("hidden,use_bn", [((128, 64, 32), True), ((64, 32), True), ((128, 64, 32), False)],
                         ids=["128x64x32-bn", "64x32-bn", "128x64x32-plain"])
@pytest.mark.parametrize("B", [64, 65, 200])
def test_tail_with_a_pair_term_and_no_linear_term(dev, B, hidden, use_bn):
    """The head's `[pair | deep]` form without a linear term (lr_mlp_head_f32 with K > 0, F = 0), in the tail's default mode:
    loss, gl, gz1 and the output layer's gradients against the oracle's `tail`."""
    K, L = 16, len(hidden)
    state = O.random_state(21, O.N_USERS, O.N_ITEMS, K, hidden, use_bn)
    net = load_state(NCFNet(O.N_USERS, O.N_ITEMS, K, hidden, use_bn, device=dev), state)
    assert DeepFMTail.supported(net.mlp)
    rng = np.random.default_rng(B)
    z1 = rng.standard_normal((B, hidden[0])).astype(np.float32)
    gmf = rng.uniform(-0.25, 0.25, (B, K)).astype(np.float32)
    labels = rng.integers(0, 2, B).astype(np.float32)
    tail = DeepFMTail(net.P, net.mlp, None, net.out, 0, K, dev)
    print(f"NCF-FIGURE tail B={B} hidden={hidden}: the tail chose its {'one-launch' if tail.fused else 'chain'} form")
    net.P.zero_grad()
    loss, gl, gz1, sgz1 = tail.run(_dev(z1, dev), _dev(gmf, dev), None, _dev(labels, dev))
    tail.check()
    P64 = {k: v.astype(np.float64) for k, v in state["P"].items()}
    want = O.tail(P64, L, use_bn, z1.astype(np.float64), gmf.astype(np.float64), labels.astype(np.float64))
    f = lambda x: x.detach().cpu().numpy().astype(np.float64)
    print(f"NCF-FIGURE tail B={B} hidden={hidden} bn={use_bn}: loss {float(loss):.8f} oracle {want['loss']:.8f}, "
          f"gl {max_diff(f(gl), want['gl']):.3e}, gz1 {max_diff(f(gz1), want['gz1']):.3e}")
    assert abs(float(loss) - want["loss"]) < 1e-5
    np.testing.assert_allclose(f(gl), want["gl"], rtol=1e-4, atol=5e-5 / B, err_msg="gl")
    np.testing.assert_allclose(f(gz1), want["gz1"], rtol=1e-4, atol=5e-5 / B, err_msg="gz1")
    np.testing.assert_allclose(f(sgz1), want["gz1"].sum(0), rtol=1e-4, atol=5e-5, err_msg="sgz1")
    np.testing.assert_allclose(f(net.P["out/kernel"].grad), want["grads"]["out/kernel"], rtol=1e-4, atol=5e-5, err_msg="out.w.grad")
    np.testing.assert_allclose(f(net.P["out/bias"].grad), want["grads"]["out/bias"], rtol=1e-4, atol=5e-5, err_msg="out.b.grad")
    for k in want["grads"]:
        np.testing.assert_allclose(f(net.P[k].grad).reshape(want["grads"][k].shape), want["grads"][k], rtol=1e-4, atol=5e-5, err_msg=k)


# ---- 4. training steps ---------------------------------------------------------------------------------------------------------
def _batches(n_steps, B, seed=3):
    """Pairs with duplicates over users < 30 and items < 45: the rows above stay untouched."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 30, B), rng.integers(0, 45, B), rng.integers(0, 2, B).astype(np.float32)) for _ in range(n_steps)]


def _close(got, want, what):
    torch.testing.assert_close(got.detach().cpu().double().reshape(want.shape), torch.as_tensor(np.asarray(want, dtype=np.float64)),
                               rtol=1e-4, atol=5e-5, msg=lambda m: f"{what}: {m}")


# (K, hidden, use_bn, the step `fused=True` takes)
STEP_CONFIGS = [(16, (128, 64, 32), True, True), (16, (128, 64, 32), False, True), (16, (32, 16), True, False),
                (32, (64, 32), True, True), (8, (128, 64, 32), True, False)]


@pytest.mark.parametrize("cfg", STEP_CONFIGS, ids=lambda c: f"K{c[0]}-{'x'.join(map(str, c[1]))}-{'bn' if c[2] else 'plain'}")
def test_training_steps(dev, cfg):
    """Three steps at B = 200 from one state: the net's default step and the `fused=False` composition against the oracle (the
    loss to 1e-5, the table with both moments, every dense parameter and BatchNorm average to rtol 1e-4 / atol 5e-5), hence
    against each other; rows no sample touched keep their bits and their zero moments."""
    K, hidden, use_bn, takes_fused = cfg
    state, batches = O.step_batches(K, hidden, use_bn)      # (three batches that stay 1e-5 away from every relu kink: see there)
    mk = lambda fused: load_state(NCFNet(O.N_USERS, O.N_ITEMS, K, hidden, use_bn, None, 0.01, 1e-5, 11, dev, fused=fused), state)
    net, comp = mk(True), mk(False)
    assert net.fused == takes_fused and not comp.fused
    oracle = O.NCFOracle(state, K, len(hidden), use_bn, 0.01, 1e-5)
    t = net.tables
    for step, (users, items, labels) in enumerate(batches, start=1):
        rows = np.stack([users + t.user_off, items + t.item_off], axis=1)
        want = oracle.train_step(rows, labels)
        for name, n in (("default", net), ("composition", comp)):
            got = float(n.train_step(users, items, labels))
            print(f"NCF-FIGURE step {cfg} {name} {step}: loss {got:.8f} oracle {want:.8f}")
            assert abs(got - want) < 1e-5, (name, step, got, want)
            for k, ref in oracle.P.items():
                _close(n.P[k], ref, f"{name} {k} after step {step}")
            _close(n.tables.embed, oracle.embed, f"{name} embed after step {step}")
            _close(n.tables.m, oracle.m, f"{name} m after step {step}")
            _close(n.tables.v, oracle.v, f"{name} v after step {step}")
    assert oracle.margin >= O.KINK_MARGIN
    for name, n in (("default", net), ("composition", comp)):
        for key, bn in [("bn_in", n.mlp.bn_in)] + [(f"bn{i}", x) for i, x in enumerate(n.mlp.bns, start=1)]:
            if bn is not None:
                _close(bn.moving_mean, oracle.bn[key][0], f"{name} {key} moving mean")
                _close(bn.moving_var, oracle.bn[key][1], f"{name} {key} moving variance")
        absent = np.r_[30:O.N_USERS + 1, t.item_off + 45:t.V]
        assert np.array_equal(n.tables.embed[absent].cpu().numpy(), state["embed"][absent]), f"{name}: an untouched row moved"
        assert not bool(n.tables.m[absent].any()) and not bool(n.tables.v[absent].any())
        pu, pi = np.arange(O.N_USERS + 1).repeat(2)[:60], np.arange(60) % (O.N_ITEMS + 1)
        assert n.score_kernel == ops.ncf_score_supported(K, hidden)
        _close(n.forward(pu, pi), oracle.forward(np.stack([pu + t.user_off, pi + t.item_off], axis=1)), f"{name} inference logits")
    _close(net.tables.embed, comp.tables.embed.double().cpu().numpy(), "default against composition: embed")
    _close(net.P.flat, comp.P.flat.double().cpu().numpy(), "default against composition: dense parameters")


@pytest.mark.parametrize("loss_type,kw", [("focal", {}), ("mse", {}), ("cross_entropy", dict(reg=0.01)),
                                          ("cross_entropy", dict(dense_adam=True)), ("cross_entropy", dict(dropout_rate=0.3))],
                         ids=["focal", "mse", "reg", "dense_adam", "dropout"])
def test_other_steps_run_and_move_the_parameters(dev, loss_type, kw):
    net = NCFNet(O.N_USERS, O.N_ITEMS, 16, (128, 64, 32), True, kw.get("dropout_rate"), 0.01, 1e-5, 5, dev,
                 kw.get("dense_adam", False), kw.get("reg"))
    assert net.dense_adam == ("reg" in kw or "dense_adam" in kw) and net.fused == (not net.dense_adam)
    e0, p0 = net.tables.embed.clone(), net.P.flat.clone()
    losses = []
    for users, items, labels in _batches(3, 64):
        losses.append(float(net.train_step(users, items, labels * 4 + 1 if loss_type == "mse" else labels, loss_type=loss_type)))
    assert np.isfinite(losses).all() and bool(torch.isfinite(net.tables.embed).all()) and bool(torch.isfinite(net.P.flat).all())
    moved = (net.tables.embed != e0).any(1)
    assert bool(moved[:30].any()) and bool((net.P.flat != p0).any())
    # an untouched row has zero moments and a zero gradient: it moves only under `reg` (2 reg w joins every row's gradient)
    assert bool(moved[30:O.N_USERS + 1].all()) == ("reg" in kw) and bool(moved[30:O.N_USERS + 1].any()) == ("reg" in kw)
    assert torch.isfinite(net.forward(np.arange(10), np.arange(10))).all()


# ---- 5. the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pure_data():
    df = synthetic_frame()[["user", "item", "label"]]
    train_data, info = DatasetPure.build_trainset(df)
    return df, train_data, info


def _fit(info, train_data, task="ranking", losses=None, **kw):
    model = NCF(task, info, **dict(dict(embed_size=16, n_epochs=2, lr=0.01, batch_size=64, seed=7), **kw))
    if losses is not None:
        step = model.train_on_batch
        model.train_on_batch = lambda b: losses.append(step(b)) or losses[-1]
    model.fit(train_data, neg_sampling=task == "ranking", verbose=0)
    return model


def _composition(model, users, items):
    """The torch inference composition on inner ids."""
    net = model.net
    with torch.no_grad():
        rows = ops.embed_gather(net.tables.embed, net.pair_rows(users, items))
        return net._logits(rows[:, 0], rows[:, 1], False).cpu().numpy()


@pytest.mark.parametrize("task", ["ranking", "rating"])
def test_fit_lowers_the_loss_and_predict_is_the_composition(dev, pure_data, task):
    df, train_data, info = pure_data
    losses = []
    model = _fit(info, train_data, task, losses)
    per_epoch = torch.stack(losses).view(2, -1).mean(1).tolist()
    print(f"NCF-FIGURE fit task={task} epoch means {per_epoch}")
    assert per_epoch[1] < per_epoch[0]
    assert model.net.fused and model.net.score_kernel          # (the rating task's mse takes the composition at every step)
    users, items = df.user.iloc[:50].tolist(), df.item.iloc[:50].tolist()
    raw = _composition(model, [info.user2id[u] for u in users], [info.item2id[i] for i in items])
    want = 1 / (1 + np.exp(-raw)) if task == "ranking" else np.clip(raw, model.lower_bound, model.upper_bound)
    np.testing.assert_allclose(model.predict(user=users, item=items), want, rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("hidden,branch", [((128, 64, 32), "pair_mlp"), ((64, 32), "ncf_score")], ids=["pair_mlp", "ncf_score"])
def test_recommend_is_the_brute_force_top_k_of_predict(dev, pure_data, hidden, branch):
    df, train_data, info = pure_data
    model = _fit(info, train_data, hidden_units=hidden)
    sc = model._catalog_scorer()
    (_, _, s, t, *_), _, _ = sc._item_side()
    assert (sc._fused_tail(s, t) is not None) == (branch == "pair_mlp") and model.net.score_kernel
    n_rec, uids = 7, list(range(info.n_users))
    block = sc.scores(uids).cpu().numpy()
    pairs_u, pairs_i = np.repeat(uids, info.n_items), np.tile(np.arange(info.n_items), len(uids))
    fwd = model.net.forward(pairs_u, pairs_i).cpu().numpy().reshape(len(uids), -1)
    print(f"NCF-FIGURE catalogue {branch}: largest difference from net.forward {np.abs(block - fwd).max():.3e}")
    assert np.abs(block - fwd).max() <= 1e-4                                    # the tolerance recommendation/catalog.py states
    users = [info.id2user[u] for u in uids[:8]]
    recs = model.recommend_user(user=users, n_rec=n_rec)
    all_items = [info.id2item[i] for i in range(info.n_items)]
    for u in users:
        uid = info.user2id[u]
        p = np.asarray(model.predict(user=[u] * info.n_items, item=all_items), dtype=np.float64)
        consumed = set(info.user_consumed[uid])
        assert len(recs[u]) == n_rec and not {info.item2id[i] for i in recs[u].tolist()} & consumed
        free = np.array([i not in consumed for i in range(info.n_items)])
        kth = np.sort(p[free])[::-1][n_rec - 1]
        got = p[[info.item2id[i] for i in recs[u].tolist()]]
        # the brute-force top-k of predict over the unconsumed catalogue, up to ties inside the scorer's 1e-4 (in logits; the
        # sigmoid's slope is at most 1 / 4)
        assert (got >= kth - 1e-4).all() and (np.diff(got) <= 1e-4).all(), (u, got, kth)


def test_save_load_rebuild_and_feature_data(dev, pure_data, tmp_path):
    df, train_data, info = pure_data
    model = _fit(info, train_data, n_epochs=1)
    assert set(model._batch_norms()) == {"mlp/bn_in", "mlp/bn1", "mlp/bn2"}
    users, items = df.user.iloc[:30].tolist(), df.item.iloc[:30].tolist()
    pa, ra = model.predict(user=users, item=items), model.recommend_user(user=users[:5], n_rec=5)
    assert len(model.recommend_user(user="nobody", n_rec=5)["nobody"]) == 5      # cold start
    model.save(str(tmp_path), "ncf")
    full = NCF.load(str(tmp_path), "ncf", info)
    assert torch.equal(full.net.P.flat, model.net.P.flat) and torch.equal(full.net.tables.embed, model.net.tables.embed)
    assert np.array_equal(pa, full.predict(user=users, item=items))
    rb = full.recommend_user(user=users[:5], n_rec=5)
    assert all(np.array_equal(ra[u], rb[u]) for u in users[:5])
    with pytest.raises(NotImplementedError):
        model.save_tf_variables(str(tmp_path), "ncf")
    # retraining on merged data with new users and items
    old, new = retrain_frames()
    train0, info0 = DatasetPure.build_trainset(old[["user", "item", "label"]])
    m0 = _fit(info0, train0, n_epochs=1)
    m0.save(str(tmp_path), "m", inference_only=False)
    train1, info1 = DatasetPure.merge_trainset(new[["user", "item", "label"]], info0, merge_behavior=True)
    assert info1.n_users > info0.n_users and info1.n_items > info0.n_items
    m1 = NCF("ranking", info1, embed_size=16, n_epochs=1, lr=0.01, batch_size=64, seed=7)
    m1.rebuild_model(str(tmp_path), "m", full_assign=True)
    t0, t1 = m0.net.tables, m1.net.tables
    for name, n in (("user_embeds_var", info0.n_users), ("item_embeds_var", info0.n_items)):
        assert torch.equal(t1.variable(name)[:n], t0.variable(name)[:n]), name
    assert torch.equal(t1.m[:info0.n_users], t0.m[:info0.n_users]) and not bool(t1.m[info0.n_users:info1.n_users].any())
    assert torch.equal(m1.net.P.flat, m0.net.P.flat) and torch.equal(m1.net.P.m, m0.net.P.m) and m1.net.step == m0.net.step > 0
    assert torch.equal(m1.net.mlp.bn_in.moving_var, m0.net.mlp.bn_in.moving_var)
    m1.fit(train1, neg_sampling=True, verbose=0)
    u_new = new["user"].iloc[0]
    assert m1.net.step > m0.net.step and len(m1.recommend_user(u_new, 5)[u_new]) == 5
    # a `DatasetFeat` trains with its feature columns ignored: no sparse rows, no linear twins
    feat_train, feat_info = DatasetFeat.build_trainset(synthetic_frame(), **FEAT_KW)
    mf = _fit(feat_info, feat_train, n_epochs=1)
    assert feat_info.n_users == info.n_users and feat_info.n_items == info.n_items
    assert mf.net.tables.V == info.n_users + 1 + info.n_items + 1 and mf.net.tables.lin is None
    pf = mf.predict(user=users, item=items)
    assert np.isfinite(pf).all() and len(mf.recommend_user(user=users[0], n_rec=5)[users[0]]) == 5


def test_multi_rank_fit_raises(dev, pure_data, monkeypatch):
    _, train_data, info = pure_data
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        NCF("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
