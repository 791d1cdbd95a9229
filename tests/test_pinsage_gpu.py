"""PinSage on the device (csrc/pinsage.hip, nets/pinsage_net.py, algorithms/pinsage.py) against the CPU oracle
(tests/pinsage_oracle.py): the sampler's integers bit for bit, the tower against the f64 variant by the project's delta rule (10 x
the oracle's own f32 / f64 gap on the case, floored at an ulp per layer), with the device's own ReLU flags fed to the f64
backward.  tests/test_pinsage_cpu.py shows that the oracle equals the reference module's arithmetic and that its f32 variant
passes every tolerance used here."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms import PinSage
from librecommender_amd.nets.pinsage_net import PinSageNet

from . import pinsage_oracle as O
from .test_graphsage_gpu import _delta, _dev, _graph, _np, _shape_id, planted

pytestmark = pytest.mark.gpu

GRAPHS = {"forced": O.forced_graph, "zipf": O.zipf_graph}
SEED, STEP = 42, 3
_WANT = {}


def _want(graph, n_nodes, nn, nw, wl, tp, level):
    """The oracle's answer for a sampler case, computed once per session."""
    key = (graph, n_nodes, nn, nw, wl, tp, level)
    if key not in _WANT:
        g = GRAPHS[graph]()
        nodes = (np.random.default_rng(n_nodes).integers(0, g.n_items, n_nodes)).astype(np.int32)
        _WANT[key] = (nodes, O.neighbors(g, nodes, nn, nw, wl, tp, SEED, STEP, level))
    return _WANT[key]


# ---- 1. the sampler, bit-exact ---------------------------------------------------------------
@pytest.mark.parametrize("walks", [(1, 1), (10, 2), (16, 4)], ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("nn", [1, 3, 10])
@pytest.mark.parametrize("n_nodes", [1, 37, 4099])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_neighbors(dev, graph, n_nodes, nn, walks):
    g = GRAPHS[graph]()
    nw, wl = walks
    for tp in (0.0, 0.5, 1.0):
        nodes, (ids, counts) = _want(graph, n_nodes, nn, nw, wl, tp, 0)
        got = ops.pinsage_neighbors(_dev(nodes, dev), _graph(g, dev), nn, nw, wl, tp, SEED, STEP, 0)
        assert np.array_equal(got[0].cpu().numpy(), ids) and np.array_equal(got[1].cpu().numpy(), counts), tp
        assert (counts.sum(1) >= 1).all() and (counts.sum(1) <= nw * wl).all()


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_neighbors_of_a_level_with_an_exclusion(dev, graph):
    """Levels 1 and 2 of 61 trees (other coordinates than level 0), targets that recur in their own trees, every third tree
    without an exclusion; and the same nodes with no exclusion array at all."""
    g = GRAPHS[graph]()
    rng = np.random.default_rng(4)
    nn, nw, wl, B = 3, 10, 2, 61
    target = rng.integers(0, g.n_items, B).astype(np.int32)
    exclude = rng.integers(0, g.n_items, B).astype(np.int32)
    exclude[::3] = -1
    hit = 0
    for level in (0, 1, 2):
        nodes = rng.integers(0, g.n_items, B * nn ** level).astype(np.int32)
        nodes[::2] = np.repeat(target, nn ** level)[::2]
        nodes[5] = -1
        for tgt, exc in ((target, exclude), (None, None)):
            want = O.neighbors(g, nodes, nn, nw, wl, 0.5, SEED, STEP, level, tgt, exc)
            got = ops.pinsage_neighbors(_dev(nodes, dev), _graph(g, dev), nn, nw, wl, 0.5, SEED, STEP, level,
                                        tree_target=None if tgt is None else _dev(tgt, dev),
                                        tree_exclude=None if exc is None else _dev(exc, dev))
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), level
            if tgt is not None:
                plain = O.neighbors(g, nodes, nn, nw, wl, 0.5, SEED, STEP, level)
                hit += int((plain[0] != want[0]).any())
    assert hit > 0                                                      # the exclusion changed something


def test_neighbors_outside_the_graph(dev):
    """An id outside [0, n_items), an item nobody consumed and an item whose only consumer holds nothing else return themselves
    with count 1; a shape outside the envelope is refused."""
    g = O.forced_graph()
    nodes = np.array([-1, 10, 11, 0, 1 << 30], dtype=np.int32)
    ids, counts = ops.pinsage_neighbors(_dev(nodes, dev), _graph(g, dev), 3, 10, 2, 0.5, SEED, STEP, 0)
    assert np.array_equal(ids.cpu().numpy(), np.stack([nodes, np.full(5, -1), np.full(5, -1)], axis=1))
    assert np.array_equal(counts.cpu().numpy(), np.array([[1, 0, 0]] * 5))
    for bad in (dict(nn=11), dict(nw=33, wl=2), dict(wl=0), dict(nw=0), dict(nw=1, wl=65)):
        kw = dict(dict(nn=3, nw=10, wl=2), **bad)
        with pytest.raises(ValueError):
            ops.pinsage_neighbors(_dev(nodes, dev), _graph(g, dev), kw["nn"], kw["nw"], kw["wl"], 0.5, SEED, STEP, 0)
    out = torch.zeros((5, 3), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="lr_pinsage_neighbors_i32"):       # LR_ESHAPE from the entry point itself
        ops._call("lr_pinsage_neighbors_i32", out.data_ptr(), 5, 3, 33, 2, 0.5, None, None, 0, *_graph(g, dev).args(), SEED, STEP, 0,
                  out.data_ptr(), out.data_ptr(), ops._stream())


def test_weights(dev):
    nodes, (ids, counts) = _want("zipf", 4099, 3, 10, 2, 0.5, 0)
    w = ops.pinsage_weights(_dev(counts, dev)).cpu().numpy()
    want = counts.astype(np.float32) / counts.sum(1, keepdims=True).astype(np.float32)
    assert w.dtype == np.float32 and (np.abs(w - want) <= np.spacing(want)).all()
    assert (np.abs(w.sum(1) - 1) <= 1e-6).all() and not w[counts == 0].any() and (counts == 0).any()
    assert np.array_equal(w, O.weights_of(counts))


# ---- 2. the tower ----------------------------------------------------------------------------
def _run(dev, c, rows=None, want_relu=True, train=True):
    B, K, T, L, n = c["shape"]
    table, params = _dev(c["table"], dev), _dev(O.pack_params(c["params"]), dev)
    rows_d = _dev(c["rows"] if rows is None else rows, dev)
    scale, weights = _dev(c["scale"], dev), (_dev(c["weights"], dev) if L else None)
    kw = dict(dropout=c["p"], seed=c["seed"], step=c["step"])
    rep = ops.pinsage_fwd(table, rows_d, scale, weights, params, L, n, train=train, **kw)
    grow, gparams, relu = ops.pinsage_bwd(table, rows_d, scale, weights, params, L, n, _dev(c["grepr"], dev), want_relu=want_relu, **kw)
    return dict(repr=rep, grow=grow, gparams=gparams, relu=relu)


@pytest.mark.parametrize("shape", O.TOWER_SHAPES, ids=_shape_id)
def test_tower(dev, shape):
    """repr against the f64 oracle; the slot-row and parameter gradients against the f64 backward of the device's own ReLU
    patterns (`check_tower`).  The trees are ragged: some children have id -1 and weight 0."""
    assert ops.pinsage_supported(*shape[1:])
    c = O.shape_case(shape)
    O.check_tower(_np(_run(dev, c)), c, _shape_id(shape))


def test_tower_wide_batch(dev):
    """A batch at which a workgroup owns several trees and the slab count is at its cap."""
    B, K, T, L, n = O.WIDE_SHAPE
    assert ops.pinsage_bwd_slabs(B, K, T, L, n) == 256 and B >= 2 * 2 * 256
    test_tower(dev, O.WIDE_SHAPE)


@pytest.mark.parametrize("shape", [(37, 16, 3, 2, 3), (5, 17, 1, 3, 4), (37, 33, 3, 1, 10)], ids=_shape_id)
def test_tower_dropout(dev, shape):
    """p = 0.5 on the neighbour branch: the oracle run on the oracle's own flags (which test_graphsage_gpu.py's
    `test_dropout_masks` shows to be the device's)."""
    c = O.shape_case(shape, p=0.5)
    O.check_tower(_np(_run(dev, c)), c, _shape_id(shape) + " p=0.5")


def test_zero_norm_nodes(dev):
    """A strongly negative bw of layer 0 makes every z of that layer zero: the forward is finite and the gradient through those
    nodes, so every slot-row gradient and the projection's, is exactly 0."""
    c = O.shape_case((37, 16, 3, 2, 3))
    Q, bq, W, bw = c["params"]["layers"][0]
    c["params"]["layers"][0] = (Q, bq, W, np.full_like(bw, -1e4))
    g = _np(_run(dev, c))
    O.check_tower(g, c, "zero norm")
    K, T = 16, 3
    assert np.isfinite(g["repr"]).all() and not g["grow"].any() and not g["gparams"][:T * K * K + K].any()
    assert g["gparams"].any()


def test_bad_rows(dev):
    """A row id outside the table is a zero row with exactly zero gradient; the other targets keep their bits."""
    shape = (37, 16, 3, 2, 3)
    B, K, T, L, n = shape
    c = O.shape_case(shape)
    c["weights"] = O.weights_of(np.random.default_rng(1).integers(1, 5, (B * 12 // n, n))).reshape(-1)      # every child counts
    clean = _run(dev, c)
    rows = c["rows"].copy()
    sl = O.level_slices(B, L, n)
    bad = [(sl[0].start + 5, 0), (sl[1].start + 6 * n + 1, 2), (sl[2].start + 6 * n * n + 4, 1)]
    for (node, t), v in zip(bad, (-1, c["V"] + 5, c["V"])):
        rows[node, t] = v
    g = _np(_run(dev, c, rows=rows))
    O.check_tower(g, c, "bad rows", rows=rows)
    for node, t in bad:
        assert not g["grow"][node, t].any()
    others = np.setdiff1d(np.arange(B), [5, 6])
    assert np.array_equal(g["repr"][others], clean["repr"].cpu().numpy()[others])
    assert not np.array_equal(g["repr"][[5, 6]], clean["repr"].cpu().numpy()[[5, 6]])


def test_batch_of_one_has_the_same_bits(dev):
    for shape in ((300, 16, 3, 2, 3), (1100, 16, 3, 2, 3), (40, 33, 1, 3, 4)):
        B, K, T, L, n = shape
        c = O.shape_case(shape)
        whole = _run(dev, c)
        sl = O.level_slices(B, L, n)
        for b in (0, 3, B - 1):
            pick = np.concatenate([np.arange(s.start + b * n ** k, s.start + (b + 1) * n ** k) for k, s in enumerate(sl)])
            one = dict(c, shape=(1, K, T, L, n), rows=c["rows"][pick], scale=c["scale"][pick], weights=c["weights"][pick[1:] - B],
                       grepr=c["grepr"][b:b + 1])
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
    train = _run(dev, c)["repr"]
    assert torch.equal(_run(dev, c, train=False)["repr"], train)
    assert torch.equal(_run(dev, dict(c, p=0.5), train=False)["repr"], train)
    assert not torch.equal(_run(dev, dict(c, p=0.5), train=True)["repr"], train)


def test_unsupported_shapes(dev):
    table = torch.zeros((4, 16), device=dev)
    rows = lambda n: torch.zeros((n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match="unsupported PinSage shape"):
        ops.pinsage_fwd(table, rows(1 + 11 + 121), None, torch.zeros(132, device=dev), torch.zeros(8, device=dev), 2, 11)
    with pytest.raises(ValueError, match="parameter pack"):
        ops.pinsage_fwd(table, rows(13), None, torch.zeros(12, device=dev), torch.zeros(8, device=dev), 2, 3)
    with pytest.raises(ValueError, match="whole number of trees"):
        ops.pinsage_fwd(table, rows(14), None, torch.zeros(12, device=dev), torch.zeros(8, device=dev), 2, 3)
    params = torch.zeros(ops.pinsage_param_floats(16, 1, 2), device=dev)
    with pytest.raises(ValueError, match="weights must hold"):
        ops.pinsage_fwd(table, rows(13), None, torch.zeros(11, device=dev), params, 2, 3)
    out = ops.pinsage_fwd(table, rows(0), None, torch.zeros(0, device=dev), params, 2, 3)      # B == 0: nothing launched
    assert out.shape == (0, 16)
    for name, tail in (("lr_pinsage_fwd_f32", (0, table.data_ptr(), ops._stream())),
                       ("lr_pinsage_bwd_f32", (table.data_ptr(), table.data_ptr(), table.data_ptr(), None, table.data_ptr(), 1 << 20,
                                               ops._stream()))):
        for K, L, n in ((65, 2, 3), (16, 4, 2), (16, 2, 11), (16, 3, 5)):          # LR_ESHAPE from the entry point itself
            with pytest.raises(ValueError, match=name):
                ops._call(name, table.data_ptr(), 4, table.data_ptr(), None, table.data_ptr(), 1, K, 1, L, n, params.data_ptr(), 0.0,
                          0, 0, *tail)


# ---- 3. the net: the fused and the composed step against an f64 step -------------------------
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
    return PinSageNet(paradigm, g.n_users, g.n_items, 16, 2, 3, kw.pop("dropout", 0.0), dev, _graph(g, dev), seed=7, lr=0.01, fused=fused,
                      **feats, **kw)


STEP_CASES = [("i2i", "cross_entropy", False, {}), ("i2i", "focal", True, dict(remove_edges=True)), ("i2i", "bpr", True, dict(dropout=0.5)),
              ("i2i", "max_margin", False, dict(reg=0.01, amsgrad=True)), ("u2i", "cross_entropy", True, {}),
              ("u2i", "max_margin", True, dict(dropout=0.5, termination_prob=0.2, neighbor_walk_len=3))]


class _Twin64:
    """The step of `PinSageNet` in f64: the composed tower on f64 copies of the tables and packs (same sampled ids, weights and
    dropout flags, the net's own loss) under autograd, and torch's own dense Adam."""

    def __init__(self, net):
        self.net, self.step = net, 0
        self.E, self.P = (t.double().clone().requires_grad_(True) for t in (net.E, net.P))
        self.opt = torch.optim.Adam([self.E, self.P], lr=net.lr, eps=net.epsilon, weight_decay=net.reg, amsgrad=net.vmax is not None)

    def _tower(self, side, ids, weights, pack, L, n, p):
        rows, scale = side.slots(ids)
        return self.net.composed(self.E[rows.clamp(min=0).long()], rows, scale, weights, self.P[pack], L, n, p, self.step)

    def train_step(self, loss_type, q, pos, neg):
        net = self.net
        self.step += 1
        if net.paradigm == "u2i":
            qr = self._tower(net.users, q, None, net.user_pack, 0, 1, 0.0)
            ids, w = net.tree(torch.cat([pos, neg]).contiguous(), self.step)
            r = self._tower(net.items, ids, w, net.item_pack, net.L, net.n, net.dropout)
            loss = net._loss(loss_type, qr, r[:pos.numel()], r[pos.numel():])
        else:
            ids, w = net.tree(torch.cat([q, pos, neg]).contiguous(), self.step, net.i2i_exclude(q, pos, neg))
            r = self._tower(net.items, ids, w, net.item_pack, net.L, net.n, net.dropout)
            nq, npos = q.numel(), pos.numel()
            loss = net._loss(loss_type, r[:nq], r[nq:nq + npos], r[nq + npos:])
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss.detach()


@pytest.mark.parametrize("paradigm,loss,with_feats,kw", STEP_CASES, ids=[f"{c[0]}-{c[1]}" for c in STEP_CASES])
def test_fused_and_composed_steps(dev, paradigm, loss, with_feats, kw):
    """Three steps of `PinSageNet` on the fused kernels, composed from torch ops (same ids, weights and dropout flags) and in
    f64: the loss of every step, the updated tables and packs and their first moments.  The fused step is held to the f64 step
    by the delta rule, with the composed f32 step's own gap to f64 as the measure of what f32 can do on the case (DESIGN §7.11
    says why the two f32 steps are not held to each other by a fixed bound).

    Measured on one MI355X: the hardest case is i2i-bpr (features, dropout 0.5), whose table is 2.187e-06 from f64 against the
    composed step's 3.396e-07, all of it in ONE element whose f64 gradient is 1.7e-07 where its neighbours' are 4e-03 and which
    Adam's lr eps / (|g| + eps)^2 = 3e+03 amplifies; with f32 accumulators in the tower's chains it stood at 3.654e-06 and missed
    the bound, which is why csrc/pinsage.hip accumulates in f64."""
    nets = [_small_net(dev, paradigm, fused, with_feats, **dict(kw)) for fused in (True, False)]
    assert nets[0].item_fused and not nets[1].item_fused and (paradigm == "i2i" or nets[0].user_fused)
    twin = _Twin64(nets[1])
    start = nets[0].E.clone()
    g = O.zipf_graph()
    rng = np.random.default_rng(11)
    what = f"pinsage {paradigm} {loss}"
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


def test_remove_edges_changes_the_query_block_only(dev):
    net = _small_net(dev, "i2i", True, False, remove_edges=True)
    g = O.zipf_graph()
    rng = np.random.default_rng(5)
    q = _dev(rng.integers(0, g.n_items, 200).astype(np.int32), dev)
    pos_np = O.neighbors(g, q.cpu().numpy(), 1, 10, 2, 0.5, 7, 1, 0)[0][:, 0]        # each query's own top neighbour
    pos = _dev(np.where(pos_np >= 0, pos_np, 0).astype(np.int32), dev)
    neg = _dev(rng.integers(0, g.n_items, 200).astype(np.int32), dev)
    targets = torch.cat([q, pos, neg]).contiguous()
    ids, w = net.tree(targets, 1, net.i2i_exclude(q, pos, neg))
    plain, _ = net.tree(targets, 1)
    B = targets.numel()
    lvl1, lvl1_plain = ids[B:B + 3 * B].view(B, 3).cpu().numpy(), plain[B:B + 3 * B].view(B, 3).cpu().numpy()
    assert np.array_equal(lvl1[200:], lvl1_plain[200:]) and not np.array_equal(lvl1[:200], lvl1_plain[:200])
    want = O.neighbors(g, targets.cpu().numpy(), 3, 10, 2, 0.5, 7, 1, 0, targets.cpu().numpy(),
                       net.i2i_exclude(q, pos, neg).cpu().numpy())
    assert np.array_equal(lvl1, want[0]) and np.array_equal(w[:3 * B].view(B, 3).cpu().numpy(), O.weights_of(want[1]))


# ---- 4. the model ----------------------------------------------------------------------------
MODEL_CASES = [("u2i", "bpr", True, {}), ("i2i", "max_margin", False, dict(remove_edges=True, termination_prob=0.3, neighbor_walk_len=3))]


@pytest.mark.parametrize("paradigm,loss,with_feats,extra", MODEL_CASES, ids=[f"{c[0]}-{c[1]}" for c in MODEL_CASES])
def test_model(dev, tmp_path, paradigm, loss, with_feats, extra):
    df, train_data, info = planted(with_feats)
    kw = dict(loss_type=loss, paradigm=paradigm, embed_size=16, n_epochs=1, lr=0.01, batch_size=64, num_neg=2, num_walks=3,
              sample_walk_len=3, seed=5, **extra)
    model = PinSage("ranking", info, **kw)
    model.fit(train_data, neg_sampling=True, verbose=0)
    first = model.last_epoch_loss
    model.n_epochs = 6
    model.fit(train_data, neg_sampling=True, verbose=0)
    assert np.isfinite(first) and model.last_epoch_loss < first
    net = model.net
    assert isinstance(net, PinSageNet) and net.item_fused and net.items.T == (3 if with_feats else 1)
    assert net.remove_edges == (paradigm == "i2i" and bool(extra.get("remove_edges")))
    assert (net.walk_len, net.termination_prob) == (extra.get("neighbor_walk_len", 2), extra.get("termination_prob", 0.5))
    assert model.user_embeds.shape == (info.n_users + 1, 16) and model.item_embeds.shape == (info.n_items + 1, 16)
    items = model.item_embeds.clone()
    model.set_embeddings()                                              # two exports give the same bits
    assert torch.equal(model.item_embeds, items[:info.n_items])
    model.assign_embedding_oov()
    some = df.user.unique()[:20].tolist()
    a = model.recommend_user(user=some, n_rec=5)
    assert len(model.recommend_user(user=-999, n_rec=5)[-999]) == 5
    model.save(str(tmp_path), "ps")
    full = PinSage.load(str(tmp_path), "ps", info)
    assert torch.equal(full.net.E, model.net.E) and torch.equal(full.net.P, model.net.P)
    assert (full.neighbor_walk_len, full.termination_prob) == (model.neighbor_walk_len, model.termination_prob)
    assert (full.net.walk_len, full.net.termination_prob, full.net.remove_edges) == (net.walk_len, net.termination_prob, net.remove_edges)
    b = full.recommend_user(user=some, n_rec=5)
    model.save(str(tmp_path), "ps_inf", inference_only=True)
    inf = PinSage.load(str(tmp_path), "ps_inf", info)
    c = inf.recommend_user(user=some, n_rec=5)
    assert (inf.neighbor_walk_len, inf.termination_prob) == (model.neighbor_walk_len, model.termination_prob)
    assert all(np.array_equal(a[x], b[x]) and np.array_equal(a[x], c[x]) for x in some)
    with pytest.raises(NotImplementedError, match="PinSage"):
        model.rebuild_model(str(tmp_path), "ps")


def test_composed_path_and_envelope_errors(dev, monkeypatch):
    _, train_data, info = planted(False)
    for kw in (dict(paradigm="i2i", embed_size=72, num_layers=1), dict(paradigm="u2i", fused=False, dropout_rate=0.3)):
        model = PinSage("ranking", info, n_epochs=1, batch_size=128, num_walks=2, sample_walk_len=2, **kw)
        model.fit(train_data, neg_sampling=True, verbose=0)
        assert np.isfinite(model.last_epoch_loss) and not model.net.item_fused
    for kw in (dict(num_neighbors=11), dict(num_layers=4), dict(embed_size=129), dict(num_neighbors=0)):
        with pytest.raises(ValueError, match="from 0 to 3"):
            PinSage("ranking", info, **kw).build_model()
    for kw in (dict(num_walks=33), dict(neighbor_walk_len=0), dict(num_walks=8, neighbor_walk_len=9)):
        with pytest.raises(ValueError, match="at most 64"):
            PinSage("ranking", info, **kw).build_model()
    from librecommender_amd import distributed as D

    monkeypatch.setattr(D, "active", lambda group=None: (0, 2))
    with pytest.raises(RuntimeError, match="single process"):
        PinSage("ranking", info, n_epochs=1).fit(train_data, neg_sampling=True, verbose=0)
