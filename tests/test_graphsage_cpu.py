"""GraphSage without a device: the oracle (tests/sage_oracle.py) against the reference module's arithmetic restated with torch
under autograd, the oracle's sampling rules on a graph where the answers are forced, the constructor, and the host queries."""
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import sage_oracle as O
from .test_api_signatures_cpu import accepts

ROOT = Path(__file__).resolve().parent.parent
SMALL = [s for s in O.TOWER_SHAPES if s[0] <= 37]


def _sid(s):
    return "x".join(map(str, s))


# ---- 1. the oracle's tower is the reference module's ---------------------------------------------
def _torch_tower(c, masks):
    """`GraphSageModel.forward` (graphsage_module.py:104-140) in f64: embedding_bag(mean) / cat / Linear, the dropout of each role
    as the given flags; `get_raw_features` as a gather of slot rows times the slot's scale."""
    B, K, T, L, n = c["shape"]
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    table = t(c["table"]).requires_grad_(True)
    P = c["params"]
    Wp, bp = t(P["proj_W"]).requires_grad_(True), t(P["proj_b"]).requires_grad_(True)
    layers = [(t(W).requires_grad_(True), t(b).requires_grad_(True)) for W, b in P["layers"]]
    rows = torch.tensor(c["rows"].astype(np.int64))
    gathered = table[rows]                                             # [nodes, T, K]
    gathered.retain_grad()
    x = gathered * t(c["scale"]).unsqueeze(-1)
    h0 = F.linear(x.flatten(1), Wp, bp)
    hidden = [h0[s] for s in O.level_slices(B, L, n)]
    inv_keep = float(np.float32(1.0 / (1.0 - c["p"]))) if c["p"] else 1.0

    def drop(h, key):
        return h if key not in masks else torch.where(torch.tensor(masks[key]), h * inv_keep, torch.zeros_like(h))

    for l in range(L):
        W, b = layers[l]
        nxt = []
        for k in range(L - l):
            cur, nb = drop(hidden[k], (l, k, 0)), drop(hidden[k + 1], (l, k + 1, 1))
            offsets = torch.arange(0, len(nb), n)
            mean = F.embedding_bag(torch.arange(len(nb)), nb, offsets=offsets, mode="mean")
            h = F.linear(torch.cat([cur, mean], dim=1), W, b)
            nxt.append(h if l == L - 1 else F.relu(h))
        hidden = nxt
    rep = hidden[0]
    rep.backward(t(c["grepr"]))
    grads = {"proj_W": Wp.grad.numpy(), "proj_b": bp.grad.numpy(), "layers": [(W.grad.numpy(), b.grad.numpy()) for W, b in layers]}
    return rep.detach().numpy(), gathered.grad.numpy(), O._pack64(grads)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, float(np.abs(b).max())))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", SMALL, ids=_sid)
def test_oracle_is_the_reference_module(shape, p):
    c = O.shape_case(shape, p=p)
    got = O.tower(c, "f64")
    rep, gx, gp = _torch_tower(c, O.case_masks(c))
    assert _rel(got["repr"], rep) <= 1e-12 and _rel(got["grow"], gx) <= 1e-12 and _rel(got["gparams"], gp) <= 1e-12
    if shape[3] > 1:
        assert got["pre"] > 0


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", O.TOWER_SHAPES + [O.WIDE_SHAPE], ids=_sid)
def test_f32_oracle_passes_the_gpu_tolerances(shape, p):
    c = O.shape_case(shape, p=p)
    O.check_tower(O.oracle_result(c, "f32"), c, _sid(shape))


def test_pack_round_trip():
    c = O.shape_case((3, 5, 2, 2, 3))
    flat = O.pack_params(c["params"])
    back = O.unpack_params(flat, 5, 2, 2)
    assert np.array_equal(back["proj_W"], c["params"]["proj_W"]) and np.array_equal(back["layers"][1][0], c["params"]["layers"][1][0])
    assert np.array_equal(back["layers"][0][1], c["params"]["layers"][0][1])
    # the device's ReLU flags, tree-major, against the oracle's level-major pattern
    c = O.shape_case((4, 3, 1, 3, 2))
    r = O.tower(c, "f64")
    B, K, T, L, n = c["shape"]
    blocks = []
    for l in range(L - 1):
        per_tree = [np.concatenate([r["relu"][(l, k)].reshape(B, n ** k, K)[b] for k in range(L - l)]) for b in range(B)]
        blocks.append(np.concatenate(per_tree))
    back = O.device_relu(np.concatenate(blocks).astype(np.uint8), c)
    assert all(np.array_equal(back[key], r["relu"][key]) for key in r["relu"])


# ---- 2. the sampling rules on a forced graph ------------------------------------------------------
def test_forced_neighbors():
    g = O.forced_graph()
    for seed in range(20):
        nb = O.neighbors(g, np.array([0, 1, 2, 3, 10], dtype=np.int32), 4, seed, 1, 0)
        assert (nb[0] == 0).all() and (nb[4] == 10).all()          # only itself is reachable
        # exactly one other reachable item: slot 0 takes it whenever one of its six conditional draws hits it (1 - 2^-6 per
        # draw that must differ from the node); the later slots fall through the ladder to "not the node itself"
        assert set(nb[1]) <= {1, 2} and set(nb[2]) <= {1, 2}
        hub = nb[3]
        assert set(hub) <= {3, 4, 5, 6, 7, 8, 9}
    many = np.stack([O.neighbors(g, np.array([1], dtype=np.int32), 3, seed, 1, 0)[0] for seed in range(200)])
    assert (many[:, 0] == 2).mean() > 0.95 and (many[:, 1:] == 2).mean() > 0.95      # 1 - 2^-11 each
    hubs = np.stack([O.neighbors(g, np.array([3], dtype=np.int32), 3, seed, 1, 0)[0] for seed in range(200)])
    distinct = np.mean([len(set(r)) == 3 and 3 not in r for r in hubs])
    assert distinct > 0.85              # six reachable others; a draw fits the third slot with probability >= 1/3, six draws


def test_first_draws_follow_the_walk_probabilities():
    """Attempt-0 draws from the hub of the forced graph over fixed seeds against the exact two-step probabilities: the hub has
    four consumers of three items each, so P(3) = 1/3, P(4) = P(9) = 1/6, P(5) = P(6) = P(7) = P(8) = 1/12.  Chi-square with 6
    degrees of freedom; the 99.9 % quantile is 22.458."""
    g = O.forced_graph()
    nodes = np.full(500, 3, dtype=np.int32)
    draws = np.concatenate([O.neighbors(g, nodes, 1, seed, 1, 0, first_only=True)[:, 0] for seed in range(8)])
    prob = {3: 1 / 3, 4: 1 / 6, 9: 1 / 6, 5: 1 / 12, 6: 1 / 12, 7: 1 / 12, 8: 1 / 12}
    assert set(draws) <= set(prob)
    chi2 = sum((np.sum(draws == i) - len(draws) * p) ** 2 / (len(draws) * p) for i, p in prob.items())
    print(f"SAGE-FIGURE chi2={chi2:.3f}")
    assert chi2 < 22.458


def _pairs_by_the_rule(g, starts, num_walks, walk_length, focus_start, walk):
    """The rule of `pairs_from_random_walk` (random_walks.py:21-41) as a plain loop over (start, walk, step), its one-walk draw
    given as `walk(w, s, cur)`: a step emits (source, next) where they differ, the source being the start node with
    `focus_start` and the current node without; a start that can reach nothing else emits (start, start) first."""
    out = []
    for si, start in enumerate(starts):
        if g.no_neighbor(start):
            out.append((start, start))
        for wi in range(num_walks):
            at = start
            for s in range(walk_length):
                nxt = walk(si * num_walks + wi, s, at)
                src = start if focus_start else at
                if nxt != src:
                    out.append((src, nxt))
                at = nxt
    return np.array([x for x, _ in out]), np.array([y for _, y in out])


@pytest.mark.parametrize("focus_start", [False, True])
def test_pair_order_is_the_reference_loop(focus_start):
    g = O.forced_graph()
    starts = [0, 3, 1, 10, 4, 3]

    def walk(w, s, cur):
        return int(g.one_walk(np.array([cur]), 9, O.WALK, np.uint64(2), np.array([(w * 5 + s) * 2], dtype=np.uint64))[0])

    want = _pairs_by_the_rule(g, starts, 3, 5, focus_start, walk)
    got = O.pairs(g, starts, 3, 5, focus_start, 9, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0][0], got[1][0]) == (0, 0) and (10, 10) in set(zip(got[0].tolist(), got[1].tolist()))


def test_negative_and_start_rules():
    g = O.forced_graph()
    cum = O.unpopular_table(g)
    assert cum[-1] == 1 << 32 and (np.diff(cum) >= 0).all() and cum[10] == cum[9]       # item 10: nobody consumed it
    s = O.start_nodes(5000, g.n_items, 1, 1, cum)
    assert 10 not in s and np.mean(s == 3) < np.mean(s == 0)                               # the hub is the least likely start
    neg = O.negatives([1] * 400, [2] * 400, 2, 11, "random", 1, 1)
    assert not np.isin(neg, [1, 2]).any()
    keep = O.dropout_keep(2000, 16, 0.25, 1, 1, 0, 1, 0)
    assert abs(keep.mean() - 0.75) < 0.01 and not np.array_equal(keep, O.dropout_keep(2000, 16, 0.25, 1, 1, 0, 1, 1))


# ---- 3. the constructor ---------------------------------------------------------------------------
_NO_COLS = SimpleNamespace(name=[], index=[])


class _Info:
    global_mean, min_max_rating = 3.0, (1, 5)
    n_users, n_items = 3, 6
    user_consumed = {0: [0, 1, 2], 1: [3], 2: [4, 5]}
    item_consumed = {0: [0], 1: [0], 2: [0], 3: [1], 4: [2], 5: [2]}
    sparse_col = dense_col = user_sparse_col = user_dense_col = item_sparse_col = item_dense_col = _NO_COLS
    user_sparse_unique = user_dense_unique = item_sparse_unique = item_dense_unique = None


def _model(**kw):
    from librecommender_amd.algorithms import GraphSage

    return GraphSage(kw.pop("task", "ranking"), _Info(), **kw)


def test_constructors_accept_the_reference_signatures():
    from librecommender_amd.algorithms import GraphSage
    from librecommender_amd.bases import SageBase

    golden = json.loads((ROOT / "tests" / "golden" / "graphsage_signature.json").read_text())
    for key, fn in (("algorithms.GraphSage.__init__", GraphSage.__init__), ("bases.SageBase.__init__", SageBase.__init__)):
        problem = accepts(golden[key], fn)
        assert problem is None, (key, problem)
    assert len(golden["algorithms.GraphSage.__init__"]) == 27 and golden["bases.SageBase.__init__"][-1][0] == "full_inference"


def test_check_params_errors():
    with pytest.raises(ValueError, match="`GraphSage` is only suitable for ranking"):
        _model(task="rating")
    with pytest.raises(ValueError, match="`paradigm` must either be `u2i` or `i2i`"):
        _model(paradigm="u2u")
    with pytest.raises(ValueError, match="unsupported `loss_type`: softmax"):
        _model(loss_type="softmax")
    with pytest.raises(ValueError, match="`start_nodes` must either be `random` or `unpopular`"):
        _model(start_node="popular")
    with pytest.raises(ValueError, match="`GraphSage` must use negative sampling"):
        _model(sampler=None)
    _model(paradigm="u2i", start_node="anything")                    # checked for i2i only, as in the reference
    with pytest.raises(AssertionError, match="`num_neg` should be positive and smaller than total items, got 6, 6"):
        _model(num_neg=6)._check_trainer_params()
    with pytest.raises(ValueError, match=re.escape("`sampler` must be one of (`random`, `unconsumed`, `popular`) for u2i, got out-batch")):
        _model(paradigm="u2i", sampler="out-batch")._check_trainer_params()
    with pytest.raises(ValueError, match=re.escape("`sampler` must be one of (`random`, `out-batch`, `popular`) for i2i, got unconsumed")):
        _model(sampler="unconsumed")._check_trainer_params()
    m = _model(remove_edges=True, num_layers=3, num_neighbors=4, fused=False)
    assert (m.remove_edges, m.num_layers, m.num_neighbors, m.fused, m.full_inference) == (True, 3, 4, False, False)
    with pytest.raises(NotImplementedError, match="GraphSage does not support retraining"):
        m.rebuild_model("nowhere", "gs")


def test_exports_and_structure():
    import librecommender_amd.algorithms as A
    import librecommender_amd.bases as B
    import librecommender_amd.nets as Nn

    assert "GraphSage" in A.__all__ and "SageBase" in B.__all__ and "SageNet" in Nn.__all__
    assert issubclass(A.GraphSage, B.SageBase) and issubclass(B.SageBase, B.EmbedBase)
    assert "predict" not in vars(B.SageBase) and "recommend_user" not in vars(B.SageBase) and "save" not in vars(B.SageBase)


def test_cumulative_table():
    from librecommender_amd.nets.sage_net import cumulative_table

    cum = cumulative_table(np.array([0.0, 1.0, 3.0, 0.0]))
    assert cum.tolist() == [0, 1 << 30, 1 << 32, 1 << 32]
    g = O.forced_graph()
    freq = np.array([len(set(x)) for x in g.item_lists], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = freq / g.n_users
        w = np.where(prob > 0, (np.sqrt(prob / 1e-3) + 1) * (1e-3 / prob), 0.0)
    assert np.array_equal(cumulative_table(w), O.unpopular_table(g))


# ---- 4. the C ABI ---------------------------------------------------------------------------------
SYMBOLS = ["lr_sage_supported", "lr_sage_params_bytes", "lr_sage_bwd_slabs", "lr_sage_bwd_ws_bytes", "lr_sage_neighbors_i32",
           "lr_sage_pairs_i32", "lr_sage_starts_i32", "lr_sage_negatives_i32", "lr_sage_dropout_u8", "lr_sage_fwd_f32", "lr_sage_bwd_f32"]


def test_header_and_host_queries():
    from librecommender_amd import _lib, ops

    header = (ROOT / "include" / "libreco_hip.h").read_text()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\(", header), s
        assert s in _lib.SIGNATURES, s
    ok = ops.sage_supported
    # the edges of the envelope
    assert ok(1, 1, 0, 1) and ok(64, 16, 3, 4) and ok(64, 16, 2, 10) and ok(16, 1, 2, 3) and ok(64, 16, 1, 10) and ok(64, 16, 0, 0)
    for bad in ((0, 1, 2, 3), (65, 1, 2, 3), (16, 0, 2, 3), (16, 17, 2, 3), (16, 1, -1, 3), (16, 1, 4, 2), (16, 1, 2, 0), (16, 1, 2, 11),
                (16, 1, 3, 5)):
        assert not ok(*bad), bad
    assert ops.sage_param_floats(16, 3, 2) == 3 * 16 * 16 + 16 + 2 * (2 * 16 * 16 + 16)
    assert ops.sage_param_floats(65, 1, 1) == 0 and ops.sage_bwd_slabs(10, 16, 1, 2, 11) == 0
    assert ops.sage_bwd_slabs(1, 16, 1, 2, 3) == 1 and ops.sage_bwd_slabs(37, 16, 1, 2, 3) == 37
    assert ops.sage_bwd_slabs(100000, 16, 1, 2, 3) == 256
    lib = _lib.load()
    assert lib.lr_sage_bwd_ws_bytes(37, 16, 1, 2, 3) >= 37 * ops.sage_param_floats(16, 1, 2) * 4
    assert lib.lr_sage_bwd_ws_bytes(37, 16, 1, 2, 11) == 0
    assert ops.sage_tree_nodes(2, 3) == 13 and ops.sage_tree_nodes(0, 5) == 1 and ops.sage_tree_nodes(3, 4) == 85
