"""PinSage without a device: the oracle (tests/pinsage_oracle.py) against the reference module's arithmetic restated with torch
under autograd, the oracle's selection rule on a graph where the answers are forced, the constructor, and the host queries."""
import json
import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import pinsage_oracle as O
from .test_api_signatures_cpu import accepts
from .test_graphsage_cpu import _Info

ROOT = Path(__file__).resolve().parent.parent
SMALL = [s for s in O.TOWER_SHAPES if s[0] <= 37]


def _sid(s):
    return "x".join(map(str, s))


# ---- 1. the oracle's tower is the reference module's ---------------------------------------------
def _torch_tower(c, masks):
    """`PinSageModel.forward` (pinsage_module.py:59-96) in f64: Linear / relu / embedding_bag(sum, per_sample_weights) / cat /
    Linear / relu / norm with the 0 -> 1 rule, the dropout of the neighbour branch as the given flags; `get_raw_features` as a
    gather of slot rows (a row id of -1: a zero row) times the slot's scale."""
    B, K, T, L, n = c["shape"]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    table = t(c["table"]).requires_grad_(True)
    P = c["params"]
    leaf = lambda a: t(a).requires_grad_(True)  # noqa: E731
    Wp, bp = leaf(P["proj_W"]), leaf(P["proj_b"])
    layers = [tuple(leaf(a) for a in lay) for lay in P["layers"]]
    G1, b1, G2 = leaf(P["G1"]), leaf(P["b1"]), leaf(P["G2"])
    rows = torch.tensor(c["rows"].astype(np.int64))
    gathered = table[rows.clamp(min=0)]
    gathered.retain_grad()
    x = gathered * (rows >= 0).unsqueeze(-1) * t(c["scale"]).unsqueeze(-1)
    h0 = F.linear(x.flatten(1), Wp, bp)
    sl = O.level_slices(B, L, n)
    hidden = [h0[s] for s in sl]
    weights = [None] + [t(c["weights"])[s.start - B:s.stop - B] for s in sl[1:]]
    inv_keep = float(np.float32(1.0 / (1.0 - c["p"]))) if c["p"] else 1.0
    for l in range(L):
        Q, bq, W, bw = layers[l]
        nxt = []
        for k in range(L - l):
            nb = F.relu(F.linear(hidden[k + 1], Q, bq))
            if (l, k + 1) in masks:
                nb = torch.where(torch.tensor(masks[(l, k + 1)]), nb * inv_keep, torch.zeros_like(nb))
            agg = F.embedding_bag(torch.arange(len(nb)), nb, offsets=torch.arange(0, len(nb), n), per_sample_weights=weights[k + 1],
                                  mode="sum")
            z = F.relu(F.linear(torch.cat([hidden[k], agg], dim=1), W, bw))
            z_norm = z.norm(dim=1, keepdim=True)
            z_norm = torch.where(z_norm == 0, torch.tensor(1.0).to(z_norm), z_norm)
            nxt.append(z / z_norm)
        hidden = nxt
    rep = F.linear(F.relu(F.linear(hidden[0], G1, b1)), G2)
    rep.backward(t(c["grepr"]))
    g = lambda a: a.grad.numpy() if a.grad is not None else np.zeros(a.shape)  # noqa: E731
    grads = {"proj_W": g(Wp), "proj_b": g(bp), "layers": [tuple(g(a) for a in lay) for lay in layers], "G1": g(G1), "b1": g(b1),
             "G2": g(G2)}
    return rep.detach().numpy(), gathered.grad.numpy(), O.pack_params(grads, np.float64)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, float(np.abs(b).max())))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", SMALL, ids=_sid)
def test_oracle_is_the_reference_module(shape, p):
    c = O.shape_case(shape, p=p)
    assert shape[3] == 0 or ((c["weights"] == 0).any() and (c["rows"][shape[0]:][c["weights"] == 0] == -1).all()) or shape[4] == 1
    got = O.tower(c, "f64")
    rep, gx, gp = _torch_tower(c, O.case_masks(c))
    assert _rel(got["repr"], rep) <= 1e-12 and _rel(got["grow"], gx) <= 1e-12 and _rel(got["gparams"], gp) <= 1e-12


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", O.TOWER_SHAPES + [O.WIDE_SHAPE], ids=_sid)
def test_f32_oracle_passes_the_gpu_tolerances(shape, p):
    c = O.shape_case(shape, p=p)
    O.check_tower(O.oracle_result(c, "f32"), c, _sid(shape))


def test_pack_and_flag_round_trip():
    c = O.shape_case((4, 3, 2, 3, 2))
    B, K, T, L, n = c["shape"]
    flat = O.pack_params(c["params"])
    assert len(flat) == O.param_floats(K, T, L)
    back = O.unpack_params(flat, K, T, L)
    assert np.array_equal(back["proj_W"], c["params"]["proj_W"]) and np.array_equal(back["G2"], c["params"]["G2"])
    assert all(np.array_equal(a, b) for a, b in zip(back["layers"][1], c["params"]["layers"][1]))
    # the device's ReLU flags, tree-major, against the oracle's level-major patterns
    r = O.tower(c, "f64")
    blocks = []
    for l in range(L):
        for kind, levels in (("q", range(1, L - l + 1)), ("w", range(L - l))):
            blocks.append(np.concatenate([np.concatenate([r["relu"][(kind, l, k)].reshape(B, n ** k, K)[b] for k in levels])
                                          for b in range(B)]))
    blocks.append(r["relu"][("head",)])
    back = O.device_relu(np.concatenate(blocks).astype(np.uint8), c)
    assert set(back) == set(r["relu"]) and all(np.array_equal(back[key], r["relu"][key]) for key in back)


def test_zero_norm_node_passes_no_gradient():
    """A strongly negative bw of layer 0 makes every z of that layer zero: the norm counts as 1, the forward stays finite and
    nothing reaches the rows."""
    c = O.shape_case((5, 8, 1, 2, 3))
    Q, bq, W, bw = c["params"]["layers"][0]
    c["params"]["layers"][0] = (Q, bq, W, np.full_like(bw, -1e4))
    r = O.tower(c, "f64")
    assert np.isfinite(r["repr"]).all() and not r["grow"].any() and not r["relu"][("w", 0, 0)].any()


# ---- 2. the selection rule on a forced graph ------------------------------------------------------
def _by_the_rule(g, nodes, nn, num_walks, walk_len, walk, cont, target=None, exclude=None, level=0):
    """`bipartite_neighbors_with_weights` (random_walks.py:74-154) as a plain loop over (walk, step), its one-walk draw given as
    `walk(i, w, s, cur)` and its continue draw as `cont(i, w, s)`; `Counter.most_common` and the two removals."""
    out = []
    for i, node in enumerate(nodes):
        if g.no_neighbor(node):
            out.append(([node], [1]))
            continue
        lst = []
        for w in range(num_walks):
            one = []
            for s in range(walk_len):
                if not one:
                    one.append(walk(i, w, s, node))
                elif cont(i, w, s):
                    one.append(walk(i, w, s, one[-1]))
                else:
                    break
            lst.extend(one)
        lst = O.remove_target(lst, node)
        if exclude is not None:
            t = i // nn ** level
            if exclude[t] >= 0 and target[t] == node:
                lst = O.remove_target(lst, exclude[t])
        if len(lst) == 1:
            out.append((lst, [1]))
        else:
            common = Counter(lst).most_common(nn)
            out.append(([x for x, _ in common], [w for _, w in common]))
    return out


def _draws(g, seed, step, level, walk_len, tp):
    a = np.uint64(step * 8 + level)

    def walk(i, w, s, cur):
        return int(g.one_walk(np.array([cur]), seed, O.PIN_WALK, a, np.array([O.coord(i, w, s, walk_len)], dtype=np.uint64))[0])

    def cont(i, w, s):
        return int(O.H(seed, O.PIN_WALK, a, O.coord(i, w, s, walk_len) + np.uint64(2)) >> np.uint64(32)) >= O.threshold(tp)

    return walk, cont


def _same(got, want, nn):
    ids, counts = got
    for i, (it, cn) in enumerate(want):
        assert ids[i, :len(it)].tolist() == it and counts[i, :len(it)].tolist() == cn, i
        assert (ids[i, len(it):] == -1).all() and (counts[i, len(it):] == 0).all(), i


@pytest.mark.parametrize("tp", [0.0, 0.5, 1.0])
def test_selection_is_the_reference_loop(tp):
    g = O.forced_graph()
    nodes = [0, 10, 1, 2, 3, 4, 3, 9]
    for seed in range(6):
        for nn, nw, wl in ((3, 10, 2), (10, 16, 4), (1, 1, 1)):
            walk, cont = _draws(g, seed, 2, 0, wl, tp)
            want = _by_the_rule(g, nodes, nn, nw, wl, walk, cont)
            got = O.neighbors(g, nodes, nn, nw, wl, tp, seed, 2, 0)
            _same(got, want, nn)
            ids, counts = got
            assert ids[0].tolist()[:1] == [0] and counts[0, 0] == 1 and ids[1, 0] == 10 and counts[1, 0] == 1
            assert set(ids[2]) <= {1, 2, -1} and set(ids[3]) <= {1, 2, -1} and (ids[2, 1:] == -1).all()
            if nw >= 10:                      # items 1 / 2 return each other unless all ten or more visits stayed at home
                assert ids[2, 0] == 2 and ids[3, 0] == 1
            hub = ids[4][ids[4] >= 0]
            assert set(hub) <= ({4, 5, 6, 7, 8, 9} if nw >= 10 else {3, 4, 5, 6, 7, 8, 9}) and len(hub) >= 1
            assert (np.diff(counts[4][counts[4] > 0]) <= 0).all()
            total = O.visits(g, nodes, nw, wl, tp, seed, 2, 0)
            length = (total[4] != -2).sum()
            if tp == 0.0:
                assert length == nw * wl
            if tp == 1.0:
                assert length == nw


def test_ties_keep_the_first_visit_order():
    assert O.select([7, 5, 5, 7, 9, 4, 4], 3) == ([7, 5, 4], [2, 2, 2])
    assert [x for x, _ in Counter([7, 5, 5, 7, 9, 4, 4]).most_common(3)] == [7, 5, 4]
    assert O.select([4], 3) == ([4], [1]) and O.remove_target([3, 3], 3) == [3] and O.remove_target([3, 4, 3], 3) == [4]


def test_exclusion_removes_the_positive_unless_nothing_else_is_left():
    g = O.forced_graph()
    seed, nn, nw, wl = 3, 3, 10, 2
    # tree 0: target 1, whose only neighbour is 2: excluding 2 leaves 2 (all that is left); tree 1: the hub without item 4
    target, exclude = np.array([1, 3, 3], dtype=np.int32), np.array([2, 4, -1], dtype=np.int32)
    ids, counts = O.neighbors(g, target, nn, nw, wl, 0.5, seed, 1, 0, target, exclude)
    assert ids[0].tolist() == [2, -1, -1] and counts[0].tolist() == [1, 0, 0]
    plain = O.neighbors(g, target, nn, nw, wl, 0.5, seed, 1, 0)
    assert 4 not in ids[1] and np.array_equal(ids[2], plain[0][2]) and np.array_equal(ids[0][:1], plain[0][0][:1])
    assert 4 in O.neighbors(g, target, 10, nw, wl, 0.5, seed, 1, 0)[0][1]                      # 4 was among the visited items
    walk, cont = _draws(g, seed, 1, 0, wl, 0.5)
    _same((ids, counts), _by_the_rule(g, target.tolist(), nn, nw, wl, walk, cont, target, exclude), nn)
    # level 1: the exclusion holds wherever the node equals its tree's target
    lvl1 = np.array([3, 5, 1, 3, 3, 4, 3, 3, 3], dtype=np.int32)
    walk, cont = _draws(g, seed, 1, 1, wl, 0.5)
    got = O.neighbors(g, lvl1, nn, nw, wl, 0.5, seed, 1, 1, target, exclude)
    _same(got, _by_the_rule(g, lvl1.tolist(), nn, nw, wl, walk, cont, target, exclude, level=1), nn)
    assert 4 not in got[0][3] and 4 not in got[0][4]


def test_first_steps_follow_the_walk_probabilities():
    """Step 0 of the walks from the hub of the forced graph over fixed seeds against the exact two-step probabilities: the hub has
    four consumers of three items each, so P(3) = 1/3, P(4) = P(9) = 1/6, P(5) = P(6) = P(7) = P(8) = 1/12.  Chi-square with 6
    degrees of freedom; the 99.9 % quantile is 22.458."""
    g = O.forced_graph()
    nodes = np.full(500, 3, dtype=np.int32)
    draws = np.concatenate([O.visits(g, nodes, 1, 1, 0.5, seed, 1, 0)[:, 0] for seed in range(8)])
    prob = {3: 1 / 3, 4: 1 / 6, 9: 1 / 6, 5: 1 / 12, 6: 1 / 12, 7: 1 / 12, 8: 1 / 12}
    assert set(draws) <= set(prob)
    chi2 = sum((np.sum(draws == i) - len(draws) * p) ** 2 / (len(draws) * p) for i, p in prob.items())
    print(f"PINSAGE-FIGURE chi2={chi2:.3f}")
    assert chi2 < 22.458


def test_weights():
    w = O.weights_of(np.array([[3, 2, 0], [1, 0, 0], [7, 7, 7]], dtype=np.int32))
    assert w.dtype == np.float32 and w[0].tolist() == [np.float32(3) / np.float32(5), np.float32(2) / np.float32(5), 0.0]
    assert w[1].tolist() == [1.0, 0.0, 0.0] and abs(float(w[2].sum()) - 1) <= 1e-6


# ---- 3. the constructor ---------------------------------------------------------------------------
def _model(**kw):
    from librecommender_amd.algorithms import PinSage

    return PinSage(kw.pop("task", "ranking"), _Info(), **kw)


def test_constructor_accepts_the_reference_signature():
    from librecommender_amd.algorithms import PinSage

    golden = json.loads((ROOT / "tests" / "golden" / "pinsage_signature.json").read_text())["algorithms.PinSage.__init__"]
    problem = accepts(golden, PinSage.__init__)
    assert problem is None, problem
    assert len(golden) == 29 and [g[0] for g in golden][19:22] == ["neighbor_walk_len", "sample_walk_len", "termination_prob"]
    import inspect

    mine = list(inspect.signature(PinSage.__init__).parameters)
    assert mine[:29] == [g[0] for g in golden] and mine[29:] == ["fused"]


def test_check_params_errors():
    with pytest.raises(ValueError, match="`PinSage` is only suitable for ranking"):
        _model(task="rating")
    with pytest.raises(ValueError, match="`paradigm` must either be `u2i` or `i2i`"):
        _model(paradigm="u2u")
    with pytest.raises(ValueError, match="unsupported `loss_type`: softmax"):
        _model(loss_type="softmax")
    with pytest.raises(ValueError, match="`PinSage` must use negative sampling"):
        _model(sampler=None)
    with pytest.raises(ValueError, match=re.escape("`sampler` must be one of (`random`, `out-batch`, `popular`) for i2i, got unconsumed")):
        _model(sampler="unconsumed")._check_trainer_params()
    m = _model(remove_edges=True, neighbor_walk_len=4, termination_prob=0.25, num_walks=7, fused=False)
    assert (m.loss_type, m.remove_edges, m.neighbor_walk_len, m.termination_prob, m.num_walks, m.fused) == ("max_margin", True, 4, 0.25, 7, False)
    assert m.all_args["neighbor_walk_len"] == 4 and m.all_args["termination_prob"] == 0.25
    with pytest.raises(NotImplementedError, match="PinSage does not support retraining"):
        m.rebuild_model("nowhere", "ps")
    for kw in (dict(num_walks=33, neighbor_walk_len=2), dict(neighbor_walk_len=0), dict(num_walks=0)):
        with pytest.raises(ValueError, match="at most 64"):
            _model(**kw).net_class()


def test_exports_and_structure():
    import librecommender_amd.algorithms as A
    import librecommender_amd.bases as B
    import librecommender_amd.nets as Nn

    assert "PinSage" in A.__all__ and "PinSageNet" in Nn.__all__
    assert issubclass(A.PinSage, B.SageBase) and issubclass(Nn.PinSageNet, Nn.SageNet) and not issubclass(A.PinSage, A.GraphSage)


# ---- 4. the C ABI ---------------------------------------------------------------------------------
SYMBOLS = ["lr_pinsage_supported", "lr_pinsage_params_bytes", "lr_pinsage_bwd_slabs", "lr_pinsage_bwd_ws_bytes",
           "lr_pinsage_neighbors_i32", "lr_pinsage_fwd_f32", "lr_pinsage_bwd_f32"]


def test_header_and_host_queries():
    from librecommender_amd import _lib, ops

    header = (ROOT / "include" / "libreco_hip.h").read_text()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\(", header), s
        assert s in _lib.SIGNATURES, s
    ok = ops.pinsage_supported
    # the envelope the issue asks for: K 1 .. 64, T 1 .. 16, 0 .. 3 layers, 1 .. 10 neighbours wherever a tree fits in LDS
    assert ok(1, 1, 0, 1) and ok(64, 16, 3, 4) and ok(64, 16, 2, 10) and ok(16, 1, 2, 3) and ok(64, 16, 1, 10) and ok(64, 16, 0, 0)
    for bad in ((0, 1, 2, 3), (65, 1, 2, 3), (16, 0, 2, 3), (16, 17, 2, 3), (16, 1, -1, 3), (16, 1, 4, 2), (16, 1, 2, 0), (16, 1, 2, 11),
                (16, 1, 3, 5)):
        assert not ok(*bad), bad
    assert ops.pinsage_param_floats(16, 3, 2) == O.param_floats(16, 3, 2) == 3 * 256 + 16 + 2 * (3 * 256 + 32) + 2 * 256 + 16
    assert ops.pinsage_param_floats(16, 2, 0) == 2 * 256 + 16 + 2 * 256 + 16
    assert ops.pinsage_param_floats(65, 1, 1) == 0 and ops.pinsage_bwd_slabs(10, 16, 1, 2, 11) == 0
    assert ops.pinsage_bwd_slabs(1, 16, 1, 2, 3) == 1 and ops.pinsage_bwd_slabs(37, 16, 1, 2, 3) == 37
    assert ops.pinsage_bwd_slabs(100000, 16, 1, 2, 3) == 256
    lib = _lib.load()
    assert lib.lr_pinsage_bwd_ws_bytes(37, 16, 1, 2, 3) >= 37 * ops.pinsage_param_floats(16, 1, 2) * 4
    assert lib.lr_pinsage_bwd_ws_bytes(37, 16, 1, 2, 11) == 0
    assert ops.pinsage_relu_rows(2, 3) == (12 + 4) + (3 + 1) + 1 and ops.pinsage_relu_rows(0, 1) == 1
