"""GraphSage on the device (csrc/sage.hip, nets/sage_net.py, bases/sage_base.py) against the CPU oracle (tests/sage_oracle.py):
the integers bit for bit, the tower against the f64 variant by the project's delta rule (10 x the oracle's own f32 / f64 gap on the
case, floored at an ulp per layer).  tests/test_graphsage_cpu.py shows that the oracle equals the reference module's arithmetic
and that its f32 variant passes every tolerance used here."""
import numpy as np
import pandas as pd
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import GraphSage
from librecommender_amd.data import DatasetFeat, DatasetPure
from librecommender_amd.nets.sage_net import SageNet

from . import sage_oracle as O

pytestmark = pytest.mark.gpu

GRAPHS = {"forced": O.forced_graph, "zipf": O.zipf_graph}
SEED, STEP = 42, 3


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _graph(g, dev):
    return ops.SageGraph(_dev(g.item_ptr, dev), _dev(g.item_idx, dev), _dev(g.user_ptr, dev), _dev(g.user_idx, dev))


def _shape_id(s):
    return "x".join(map(str, s))


# ---- 1. integers, bit-exact ------------------------------------------------------------------
@pytest.mark.parametrize("nn", [1, 3, 10])
@pytest.mark.parametrize("n_nodes", [1, 37, 4099])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_neighbors(dev, graph, n_nodes, nn):
    g = GRAPHS[graph]()
    nodes = (np.random.default_rng(n_nodes).integers(0, g.n_items, n_nodes)).astype(np.int32)
    for level in (0, 2):
        got = ops.sage_neighbors(_dev(nodes, dev), _graph(g, dev), nn, SEED, STEP, level).cpu().numpy()
        assert np.array_equal(got, O.neighbors(g, nodes, nn, SEED, STEP, level)), level


def test_neighbors_outside_the_graph(dev):
    """An id outside [0, n_items) and an item nobody consumed return themselves."""
    g = O.forced_graph()
    nodes = np.array([-1, 10, 11, 0], dtype=np.int32)
    got = ops.sage_neighbors(_dev(nodes, dev), _graph(g, dev), 3, SEED, STEP, 0).cpu().numpy()
    assert np.array_equal(got, np.repeat(nodes[:, None], 3, axis=1))


@pytest.mark.parametrize("focus_start", [False, True])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_pairs(dev, graph, focus_start):
    """Walk pairs in ascending (start, walk, step), with starts that have no other reachable item (0 and 10 of the forced graph)."""
    g = GRAPHS[graph]()
    starts = np.concatenate([[0, 10 % g.n_items, 3], np.random.default_rng(1).integers(0, g.n_items, 70)]).astype(np.int32)
    items, pos = ops.sage_pairs(_dev(starts, dev), _graph(g, dev), 4, 5, focus_start, SEED, STEP)
    want = O.pairs(g, starts, 4, 5, focus_start, SEED, STEP)
    assert np.array_equal(items.cpu().numpy(), want[0]) and np.array_equal(pos.cpu().numpy(), want[1])
    if graph == "forced":
        assert (want[0][0], want[1][0]) == (0, 0) and len(want[0]) > 10


@pytest.mark.parametrize("mode", ["random", "unpopular"])
def test_start_nodes(dev, mode):
    g = O.zipf_graph()
    cum = O.unpopular_table(g) if mode == "unpopular" else None
    got = ops.sage_starts(4099, g.n_items, SEED, STEP, dev, cum=None if cum is None else _dev(cum, dev)).cpu().numpy()
    assert np.array_equal(got, O.start_nodes(4099, g.n_items, SEED, STEP, cum))
    if cum is not None:                     # an item nobody consumed is never a start
        assert not np.isin(got, [i for i in range(g.n_items) if not g.item_lists[i]]).any()


@pytest.mark.parametrize("mode", ["random", "popular", "out-batch"])
def test_negatives(dev, mode):
    rng = np.random.default_rng(2)
    n_items, n, num_neg = 11, 300, 3
    items, pos = rng.integers(0, n_items, n).astype(np.int32), rng.integers(0, n_items, n).astype(np.int32)
    cum = np.floor(np.cumsum(np.arange(1, n_items + 1)) / 66.0 * 2.0 ** 32).astype(np.int64) if mode == "popular" else None
    in_batch = None
    if mode == "out-batch":
        in_batch = np.zeros(n_items, dtype=np.uint8)
        in_batch[[0, 1, 2]] = 1
    got = ops.sage_negatives(_dev(items, dev), _dev(pos, dev), num_neg, n_items, mode, SEED, STEP,
                             cum=None if cum is None else _dev(cum, dev), in_batch=None if in_batch is None else _dev(in_batch, dev))
    want = O.negatives(items, pos, num_neg, n_items, mode, SEED, STEP, cum, in_batch)
    assert np.array_equal(got.cpu().numpy(), want)
    if mode == "random":                    # 11 tries at 2 / 11: a clash survives with probability 7e-9
        assert not (want == np.repeat(pos, num_neg)).any() and not (want == np.repeat(items, num_neg)).any()
    if mode == "out-batch":             # 11 tries at 3 / 11: 6e-7 per slot
        assert (want >= 3).all()
    # without `items` (u2i) only the positive is avoided
    if mode == "popular":
        got = ops.sage_negatives(None, _dev(pos, dev), num_neg, n_items, mode, SEED, STEP, cum=_dev(cum, dev))
        assert np.array_equal(got.cpu().numpy(), O.negatives(None, pos, num_neg, n_items, mode, SEED, STEP, cum))


def test_dropout_masks(dev):
    for (n, K, p, layer, level, role) in ((37, 16, 0.5, 0, 1, 0), (4099, 17, 0.1, 2, 3, 1), (1, 64, 0.9, 1, 0, 1)):
        got = ops.sage_dropout_mask(n, K, p, SEED, STEP, layer, level, role, dev).cpu().numpy().astype(bool)
        want = O.dropout_keep(n, K, p, SEED, STEP, layer, level, role)
        assert np.array_equal(got, want)
        if n * K > 1000:
            assert abs(want.mean() - (1 - p)) < 0.02


# ---- 2. the tower ----------------------------------------------------------------------------
def _run(dev, c, rows=None, want_relu=True):
    B, K, T, L, n = c["shape"]
    table, params = _dev(c["table"], dev), _dev(O.pack_params(c["params"]), dev)
    rows_d = _dev(c["rows"] if rows is None else rows, dev)
    scale = _dev(c["scale"], dev)
    kw = dict(dropout=c["p"], seed=c["seed"], step=c["step"])
    rep = ops.sage_fwd(table, rows_d, scale, params, L, n, train=True, **kw)
    grow, gparams, relu = ops.sage_bwd(table, rows_d, scale, params, L, n, _dev(c["grepr"], dev), want_relu=want_relu, **kw)
    return dict(repr=rep, grow=grow, gparams=gparams, relu=relu)


def _np(got):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}


@pytest.mark.parametrize("shape", O.TOWER_SHAPES, ids=_shape_id)
def test_tower(dev, shape):
    """repr against the f64 oracle; the slot-row and parameter gradients against the f64 backward of the device's own ReLU
    pattern (`check_tower`)."""
    c = O.shape_case(shape)
    O.check_tower(_np(_run(dev, c)), c, _shape_id(shape))


def test_tower_wide_batch(dev):
    """A batch at which a workgroup owns several trees and the slab count is at its cap."""
    B, K, T, L, n = O.WIDE_SHAPE
    assert ops.sage_bwd_slabs(B, K, T, L, n) == 256 and B >= 2 * 2 * 256
    test_tower(dev, O.WIDE_SHAPE)


@pytest.mark.parametrize("shape", [(37, 16, 3, 2, 3), (5, 17, 1, 3, 4), (37, 33, 3, 1, 10)], ids=_shape_id)
def test_tower_dropout(dev, shape):
    """p = 0.5: the oracle run on the oracle's own flags (which `test_dropout_masks` shows to be the device's)."""
    c = O.shape_case(shape, p=0.5)
    O.check_tower(_np(_run(dev, c)), c, _shape_id(shape) + " p=0.5")


def test_batch_of_one_has_the_same_bits(dev):
    for shape in ((300, 16, 3, 2, 3), (1100, 16, 3, 2, 3), (40, 33, 1, 3, 4)):
        B, K, T, L, n = shape
        c = O.shape_case(shape)
        whole = _run(dev, c)
        sl = O.level_slices(B, L, n)
        for b in (0, 3, B - 1):
            pick = np.concatenate([np.arange(s.start + b * n ** k, s.start + (b + 1) * n ** k) for k, s in enumerate(sl)])
            one = dict(c, shape=(1, K, T, L, n), rows=c["rows"][pick], scale=c["scale"][pick], grepr=c["grepr"][b:b + 1])
            got = _run(dev, one)
            assert torch.equal(got["repr"][0], whole["repr"][b]), (shape, b)
            assert torch.equal(got["grow"], whole["grow"][torch.from_numpy(pick).to(dev)]), (shape, b)


def test_two_runs_give_the_same_bits(dev):
    for shape, p in ((O.WIDE_SHAPE, 0.0), ((300, 17, 3, 2, 3), 0.5)):
        c = O.shape_case(shape, p=p)
        a, b = _run(dev, c), _run(dev, c)
        for k in ("repr", "grow", "gparams", "relu"):
            assert torch.equal(a[k], b[k]), (shape, k)


def test_inference_equals_training_without_dropout(dev):
    c = O.shape_case((37, 16, 3, 2, 3))
    B, K, T, L, n = c["shape"]
    table, params, rows, scale = (_dev(x, dev) for x in (c["table"], O.pack_params(c["params"]), c["rows"], c["scale"]))
    train = ops.sage_fwd(table, rows, scale, params, L, n, 0.0, c["seed"], c["step"], train=True)
    assert torch.equal(ops.sage_fwd(table, rows, scale, params, L, n, 0.0, c["seed"], c["step"], train=False), train)
    assert torch.equal(ops.sage_fwd(table, rows, scale, params, L, n, 0.5, c["seed"], c["step"], train=False), train)
    # no scale array is a scale of 1
    c1 = O.shape_case((37, 16, 1, 2, 3))
    table, params, rows, scale = (_dev(x, dev) for x in (c1["table"], O.pack_params(c1["params"]), c1["rows"], c1["scale"]))
    assert torch.equal(ops.sage_fwd(table, rows, None, params, L, n), ops.sage_fwd(table, rows, scale, params, L, n))


def test_bad_rows(dev):
    """A row id outside the table is a zero row with exactly zero gradient; the other targets keep their bits."""
    shape = (37, 16, 3, 2, 3)
    B, K, T, L, n = shape
    c = O.shape_case(shape)
    clean = _run(dev, c)
    rows = c["rows"].copy()
    sl = O.level_slices(B, L, n)
    bad = [(sl[0].start + 5, 0), (sl[1].start + 6 * n + 1, 2), (sl[2].start + 6 * n * n + 4, 1)]
    for (node, t), v in zip(bad, (-1, c["V"] + 5, c["V"])):
        rows[node, t] = v
    got = _run(dev, c, rows=rows)
    g = _np(got)
    O.check_tower(g, c, "bad rows", rows=rows)
    for node, t in bad:
        assert not g["grow"][node, t].any() and g["grow"][node, (t + 1) % T].any()
    others = np.setdiff1d(np.arange(B), [5, 6])
    assert np.array_equal(g["repr"][others], clean["repr"].cpu().numpy()[others])
    assert not np.array_equal(g["repr"][[5, 6]], clean["repr"].cpu().numpy()[[5, 6]])


def test_zero_dense_value(dev):
    """A dense value of 0 gives its row a gradient of exactly 0."""
    c = O.shape_case((37, 16, 3, 2, 3))
    c["scale"][::3, 1] = 0.0
    g = _np(_run(dev, c))
    O.check_tower(g, c, "zero dense value")
    assert not g["grow"][::3, 1].any() and g["grow"][1::3, 1].any()


def test_unsupported_shapes(dev):
    assert ops.sage_supported(1, 1, 0, 1) and ops.sage_supported(64, 16, 2, 10) and ops.sage_supported(64, 16, 3, 4)
    table = torch.zeros((4, 16), device=dev)
    with pytest.raises(ValueError, match="unsupported GraphSage shape"):
        ops.sage_fwd(table, torch.zeros((1 + 11 + 121, 1), dtype=torch.int32, device=dev), None, torch.zeros(8, device=dev), 2, 11)
    with pytest.raises(ValueError, match="parameter pack"):
        ops.sage_fwd(table, torch.zeros((13, 1), dtype=torch.int32, device=dev), None, torch.zeros(8, device=dev), 2, 3)
    with pytest.raises(ValueError, match="whole number of trees"):
        ops.sage_fwd(table, torch.zeros((14, 1), dtype=torch.int32, device=dev), None, torch.zeros(8, device=dev), 2, 3)
    params = torch.zeros(ops.sage_param_floats(16, 1, 2), device=dev)
    out = ops.sage_fwd(table, torch.zeros((0, 1), dtype=torch.int32, device=dev), None, params, 2, 3)      # B == 0: nothing launched
    assert out.shape == (0, 16)
    with pytest.raises(ValueError, match="lr_sage_fwd_f32"):            # LR_ESHAPE from the entry point itself
        ops._call("lr_sage_fwd_f32", table.data_ptr(), 4, table.data_ptr(), None, 1, 65, 1, 2, 3, params.data_ptr(), 0.0, 0, 0, 0,
                  table.data_ptr(), ops._stream())


# ---- 3. the net: fused against composed ------------------------------------------------------
def _small_net(dev, paradigm, fused, with_feats, **kw):
    g = O.zipf_graph()
    rng = np.random.default_rng(3)
    feats = {}
    if with_feats:
        feats = dict(n_sparse_rows=9, n_dense_rows=2, item_sparse=rng.integers(0, 9, (g.n_items + 1, 1)),
                     item_dense=rng.standard_normal((g.n_items + 1, 1)).astype(np.float32), item_dense_cols=[1])
        if paradigm == "u2i":
            feats.update(user_sparse=rng.integers(0, 9, (g.n_users + 1, 2)), user_dense=rng.standard_normal((g.n_users + 1, 1)).astype(np.float32),
                         user_dense_cols=[0])
    return SageNet(paradigm, g.n_users, g.n_items, 16, 2, 3, kw.pop("dropout", 0.0), dev, _graph(g, dev), seed=7, lr=0.01, fused=fused,
                   **feats, **kw), g


STEP_CASES = [("i2i", "cross_entropy", False, {}), ("i2i", "focal", True, {}), ("i2i", "bpr", True, dict(dropout=0.5)),
              ("i2i", "max_margin", False, dict(reg=0.01, amsgrad=True)), ("u2i", "cross_entropy", True, {}), ("u2i", "focal", False, {}),
              ("u2i", "bpr", True, dict(reg=0.01, amsgrad=True)), ("u2i", "max_margin", True, dict(dropout=0.5))]


class _Twin64:
    """The step of `SageNet` in f64: the composed tower on f64 copies of the tables and packs (same sampled ids, same dropout
    flags, the net's own loss) under autograd, and torch's own dense Adam."""

    def __init__(self, net):
        self.net, self.step = net, 0
        self.E, self.P = (t.double().clone().requires_grad_(True) for t in (net.E, net.P))
        self.opt = torch.optim.Adam([self.E, self.P], lr=net.lr, eps=net.epsilon, weight_decay=net.reg, amsgrad=net.vmax is not None)

    def _tower(self, side, ids, pack, L, n, p):
        rows, scale = side.slots(ids)
        return self.net.composed(self.E[rows.clamp(min=0).long()], rows, scale, self.P[pack], L, n, p, self.step)

    def train_step(self, loss_type, q, pos, neg):
        net = self.net
        self.step += 1
        if net.paradigm == "u2i":
            qr = self._tower(net.users, q, net.user_pack, 0, 1, 0.0)
            r = self._tower(net.items, net.tree_ids(torch.cat([pos, neg]).contiguous(), self.step), net.item_pack, net.L, net.n, net.dropout)
            loss = net._loss(loss_type, qr, r[:pos.numel()], r[pos.numel():])
        else:
            r = self._tower(net.items, net.tree_ids(torch.cat([q, pos, neg]).contiguous(), self.step), net.item_pack, net.L, net.n,
                            net.dropout)
            nq, npos = q.numel(), pos.numel()
            loss = net._loss(loss_type, r[:nq], r[nq:nq + npos], r[nq + npos:])
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.detach()


def _delta(got, comp32, want64, what):
    """The project's rule with the composed f32 step in the oracle's f32 role: 10 x its own gap to f64 on this
    very case, floored at four f32 ulp of the largest value."""
    want = want64.detach().double()
    floor = 4 * float(np.spacing(np.float32(float(want.abs().max()))))
    own = float((comp32.double() - want).abs().max())
    gap = float((got.double() - want).abs().max())
    bound = max(10 * own, floor)
    print(f"SAGE-FIGURE step {what} delta={own:.3e} got={gap:.3e} bound={bound:.3e}")
    assert np.isfinite(gap) and gap <= bound, what


@pytest.mark.parametrize("paradigm,loss,with_feats,kw", STEP_CASES, ids=[f"{c[0]}-{c[1]}" for c in STEP_CASES])
def test_fused_and_composed_steps_agree(dev, paradigm, loss, with_feats, kw):
    """Three steps of `SageNet` on the fused kernels, composed from torch ops (same ids, same dropout flags) and in f64: the
    loss of every step, the updated tables and packs and their first moments.  The fused step is held to the f64 step by the
    delta rule, with the composed f32 step's own gap to f64 as the measure of what f32 can do on the case.  (Adam turns a
    gradient that is a pure rounding residue, such as the last layer's bias under u2i bpr / max_margin, where it cancels
    between the positive and the negative tower, into a move of about lr in a direction that rounding decides; the composed
    step's own gap shows that where it happens, and a fixed bound would not.)"""
    nets = [_small_net(dev, paradigm, fused, with_feats, **dict(kw))[0] for fused in (True, False)]
    assert nets[0].item_fused and not nets[1].item_fused
    twin = _Twin64(nets[1])
    start = nets[0].E.clone()
    g = O.zipf_graph()
    rng = np.random.default_rng(11)
    what = f"{paradigm} {loss}"
    for s in range(3):
        nq = 50
        q = rng.integers(0, g.n_users if paradigm == "u2i" else g.n_items, nq).astype(np.int32)
        pos, neg = rng.integers(0, g.n_items, nq).astype(np.int32), rng.integers(0, g.n_items, 2 * nq).astype(np.int32)
        args = (loss, _dev(q, dev), _dev(pos, dev), _dev(neg, dev))
        want = twin.train_step(*args)
        fused, comp = (n.train_step(*args) for n in nets)
        _delta(fused, comp, want, f"{what} loss of step {s + 1}")
    assert nets[0].step == nets[1].step == twin.step == 3
    for name, ref in (("E", twin.E), ("P", twin.P), ("m", twin.opt.state[twin.E]["exp_avg"]), ("pm", twin.opt.state[twin.P]["exp_avg"])):
        _delta(getattr(nets[0], name), getattr(nets[1], name), ref, f"{what} {name}")
    assert float((nets[0].E - start).abs().max()) > 1e-3               # it trained


# ---- 4. the model ----------------------------------------------------------------------------
def planted(with_feats):
    """40 items in 4 clusters of 10, 60 users who consume 8 items of their cluster."""
    rng = np.random.default_rng(0)
    rows = []
    for u in range(60):
        c = u % 4
        for i in rng.choice(10, 8, replace=False):
            rows.append((u, c * 10 + int(i), 1, "FM"[u % 2], f"g{c}", float(rng.standard_normal())))
    df = pd.DataFrame(rows, columns=["user", "item", "label", "sex", "genre", "price"])
    price = {i: float(p) for i, p in zip(range(40), np.random.default_rng(1).standard_normal(40))}
    df["price"] = df.item.map(price)
    if with_feats:
        train_data, info = DatasetFeat.build_trainset(df, user_col=["sex"], item_col=["genre", "price"], sparse_col=["sex", "genre"],
                                                      dense_col=["price"])
    else:
        train_data, info = DatasetPure.build_trainset(df[["user", "item", "label"]])
    return df, train_data, info


MODEL_CASES = [("u2i", "bpr", True), ("i2i", "cross_entropy", False), ("i2i", "max_margin", True)]


@pytest.mark.parametrize("paradigm,loss,with_feats", MODEL_CASES, ids=[f"{c[0]}-{c[1]}" for c in MODEL_CASES])
def test_model(dev, tmp_path, paradigm, loss, with_feats):
    df, train_data, info = planted(with_feats)
    kw = dict(loss_type=loss, paradigm=paradigm, embed_size=16, n_epochs=1, lr=0.01, batch_size=64, num_neg=2, num_walks=3,
              sample_walk_len=3, seed=5)
    model = GraphSage("ranking", info, **kw)
    model.fit(train_data, neg_sampling=True, verbose=0)
    first = model.last_epoch_loss
    model.n_epochs = 6
    model.fit(train_data, neg_sampling=True, verbose=0)
    assert np.isfinite(first) and model.last_epoch_loss < first
    assert model.net.item_fused and model.net.items.T == (3 if with_feats else 1)
    assert model.user_embeds.shape == (info.n_users + 1, 16) and model.item_embeds.shape == (info.n_items + 1, 16)
    # two exports give the same bits
    items = model.item_embeds.clone()
    model.set_embeddings()
    assert torch.equal(model.item_embeds, items[:info.n_items])
    model.assign_embedding_oov()
    users, its = df.user.iloc[:30].tolist(), df.item.iloc[:30].tolist()
    U, I = model.user_embeds.cpu().numpy(), model.item_embeds.cpu().numpy()
    raw = (U[[info.user2id[u] for u in users]] * I[[info.item2id[i] for i in its]]).sum(1)
    np.testing.assert_allclose(model.predict(user=users, item=its), 1 / (1 + np.exp(-raw)), rtol=1e-4, atol=1e-6)
    some = df.user.unique()[:20].tolist()
    a = model.recommend_user(user=some, n_rec=5)
    if paradigm == "i2i":       # a user's row is the mean of the consumed items' rows; its cluster's unseen items lead
        u0 = info.user2id[some[0]]
        np.testing.assert_allclose(U[u0], I[info.user_consumed[u0]].mean(0), rtol=1e-5, atol=1e-6)
    assert len(model.recommend_user(user=-999, n_rec=5)[-999]) == 5
    model.save(str(tmp_path), "gs")
    full = GraphSage.load(str(tmp_path), "gs", info)
    assert torch.equal(full.net.E, model.net.E) and torch.equal(full.net.P, model.net.P)
    b = full.recommend_user(user=some, n_rec=5)
    with np.load(tmp_path / "gs_variables.npz") as z:
        assert {"sage/table", "sage/params", "opt::m", "opt::pv", "opt::step"} <= set(z.files) and int(z["opt::step"]) == model.net.step
    model.save(str(tmp_path), "gs_inf", inference_only=True)
    c = GraphSage.load(str(tmp_path), "gs_inf", info).recommend_user(user=some, n_rec=5)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with pytest.raises(NotImplementedError, match="GraphSage"):
        model.rebuild_model(str(tmp_path), "gs")


def test_model_samplers_and_composed_path(dev):
    """Every other sampler, start-node mode and `lr_decay` run a step; outside the fused envelope the composed tower runs."""
    _, train_data, info = planted(False)
    for kw in (dict(paradigm="i2i", sampler="out-batch", start_node="unpopular", focus_start=True, lr_decay=True),
               dict(paradigm="i2i", sampler="popular", dropout_rate=0.3), dict(paradigm="u2i", sampler="unconsumed"),
               dict(paradigm="u2i", sampler="popular", loss_type="focal"), dict(paradigm="i2i", embed_size=72, num_layers=1)):
        model = GraphSage("ranking", info, n_epochs=1, batch_size=128, num_walks=2, sample_walk_len=2, **kw)
        model.fit(train_data, neg_sampling=True, verbose=0)
        assert np.isfinite(model.last_epoch_loss) and model.net.item_fused == (kw.get("embed_size", 16) <= 64)


def test_shapes_outside_both_paths_raise_at_build(dev):
    _, _, info = planted(False)
    for kw in (dict(num_neighbors=11), dict(num_layers=4), dict(embed_size=129), dict(num_neighbors=0)):
        with pytest.raises(ValueError, match="from 0 to 3"):
            GraphSage("ranking", info, **kw).build_model()


def test_multi_rank_fit_raises(dev, monkeypatch):
    _, train_data, info = planted(False)
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        GraphSage("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
