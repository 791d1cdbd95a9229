"""NCF without a device: the constructor against the reference's recorded signature and checks, the refused TF-variable IO, the
f64 oracle (tests/ncf_oracle.py) against an independent torch f64 autograd model of the same graph, the inference fold against
BatchNorm in evaluation mode, the reason for the product kernel of csrc/ncf.hip (the FM identity is not u * i in f32), and the
host-side envelope query of the score kernel."""
import itertools
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from librecommender_amd import algorithms, nets, ops
from librecommender_amd.algorithms import NCF

from . import ncf_oracle as O
from .test_api_signatures_cpu import accepts

ROOT = Path(__file__).resolve().parent.parent


def _info():
    col = lambda: SimpleNamespace(name=[], index=[])
    return SimpleNamespace(n_users=5, n_items=7, user_consumed={}, sparse_col=col(), dense_col=col(), data_size=100)


def test_constructor_accepts_the_reference_signature():
    golden = json.loads((ROOT / "tests" / "golden" / "ncf_signature.json").read_text())
    problem = accepts(golden["algorithms.NCF.__init__"], NCF.__init__)
    assert problem is None, problem
    assert "NCF" in algorithms.__all__ and "NCFNet" in nets.__all__
    m = NCF("ranking", _info())
    assert (m.embed_size, m.n_epochs, m.lr, m.epsilon, m.batch_size, m.num_neg, m.use_bn) == (16, 20, 0.01, 1e-5, 256, 1, True)
    assert m.hidden_units == [128, 64, 32] and m.multi_sparse_combiner == "normal" and not m.dense_adam


def test_constructor_checks_as_the_reference():
    assert NCF("ranking", _info(), hidden_units=64).hidden_units == [64]
    assert NCF("ranking", _info(), hidden_units=[32, 16]).hidden_units == [32, 16]
    for bad in ("128,64", (), (64, 32.0)):
        with pytest.raises(ValueError, match="hidden_units"):
            NCF("ranking", _info(), hidden_units=bad)
    assert NCF("ranking", _info()).dropout_rate == 0.0 and NCF("ranking", _info(), dropout_rate=0.3).dropout_rate == 0.3
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="dropout_rate"):
            NCF("ranking", _info(), dropout_rate=bad)
    assert NCF("ranking", _info()).reg is None and NCF("ranking", _info(), reg=0.0).reg is None
    m = NCF("ranking", _info(), reg=0.01)
    assert m.reg == 0.01 and m.dense_adam                                       # `reg` selects the dense update
    for bad in (1, -0.5):
        with pytest.raises(ValueError, match="reg"):
            NCF("ranking", _info(), reg=bad)
    with pytest.raises(ValueError, match="loss_type"):
        NCF("ranking", _info(), loss_type="bpr")
    NCF("ranking", _info(), tf_sess_config={"intra_op_parallelism_threads": 1})   # accepted and ignored


def test_tf_variable_io_is_refused():
    m = NCF("ranking", _info())
    with pytest.raises(NotImplementedError):
        m.save_tf_variables("x", "y")
    with pytest.raises(NotImplementedError):
        m.load_tf_variables("x", "y")


# ---- the oracle against torch autograd -------------------------------------------------------------------------------------
def _torch_model(state, rows, labels, K, hidden, use_bn, loss_type):
    """The same graph from torch ops in f64 under autograd: (loss, d loss / d gathered rows, {name: gradient})."""
    dd = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    P = {k: dd(v) for k, v in state["P"].items()}
    e = dd(state["embed"][rows])                                                # [B, 2, K]
    u, i = e[:, 0], e[:, 1]
    bn = lambda x, key: torch.nn.functional.batch_norm(x, None, None, P[f"mlp/{key}/gamma"], P[f"mlp/{key}/beta"], True, 0.0, O.BN_EPS)
    h = torch.cat([u, i], dim=1)
    if use_bn:
        h = bn(h, "bn_in")
    for l in range(1, len(hidden) + 1):
        h = h @ P[O.kernel(l)] + P[O.bias(l)]
        if l < len(hidden):
            h = torch.relu(h)
            if use_bn:
                h = bn(h, f"bn{l}")
    logits = (torch.cat([u * i, h], dim=1) @ P["out/kernel"]).squeeze(1) + P["out/bias"]
    y = torch.tensor(labels, dtype=torch.float64)
    loss = (torch.nn.functional.binary_cross_entropy_with_logits(logits, y) if loss_type == "cross_entropy"
            else torch.nn.functional.mse_loss(logits, y))
    loss.backward()
    return float(loss.detach()), e.grad.numpy(), {k: p.grad.numpy() for k, p in P.items()}


@pytest.mark.parametrize("loss_type", ["cross_entropy", "mse"])
@pytest.mark.parametrize("K,hidden,use_bn", [(8, (16, 16, 8), True), (4, (16,), True), (6, (12, 8), False)])
def test_oracle_gradients_equal_torch_autograd(K, hidden, use_bn, loss_type):
    state = O.random_state(3, O.N_USERS, O.N_ITEMS, K, hidden, use_bn)
    rng = np.random.default_rng(5)
    B = 33
    rows = np.stack([rng.integers(0, O.N_USERS + 1, B), O.N_USERS + 1 + rng.integers(0, O.N_ITEMS + 1, B)], axis=1)
    rows[:3] = rows[0]                                                           # duplicates
    labels = rng.integers(0, 2, B).astype(np.float64) if loss_type == "cross_entropy" else rng.uniform(1, 5, B)
    oracle = O.NCFOracle(state, K, len(hidden), use_bn, 0.01)
    loss, ge, grads, stats = oracle.gradients(rows, labels, loss_type)
    want_loss, want_ge, want = _torch_model(state, rows, labels, K, hidden, use_bn, loss_type)
    assert abs(loss - want_loss) < 1e-12
    np.testing.assert_allclose(ge, want_ge, rtol=1e-9, atol=1e-13)
    assert set(grads) == set(want)
    for k in want:
        np.testing.assert_allclose(grads[k].reshape(want[k].shape), want[k], rtol=1e-9, atol=1e-13, err_msg=k)
    assert set(stats) == set(state["bn"])


def test_oracle_step_is_adam_on_touched_rows_with_duplicates_summed():
    K, hidden = 4, (16, 8)
    state = O.random_state(4, O.N_USERS, O.N_ITEMS, K, hidden, True)
    oracle = O.NCFOracle(state, K, 2, True, 0.01)
    rows = np.array([[1, 40], [1, 40], [2, 41]])
    labels = np.array([1.0, 0.0, 1.0])
    _, ge, grads, stats = oracle.gradients(rows, labels)
    before = oracle.embed.copy()
    oracle.train_step(rows, labels)
    moved = np.flatnonzero((oracle.embed != before).any(1))
    assert list(moved) == [1, 2, 40, 41] and oracle.step == 1
    # first Adam step from zero moments: w -= lr_t (1-b1) g / (sqrt((1-b2) g^2) + eps), g = the sum over the duplicates
    g = ge[0, 0] + ge[1, 0]
    lr_t = 0.01 * np.sqrt(1 - O.B2) / (1 - O.B1)
    np.testing.assert_allclose(oracle.embed[1], before[1] - lr_t * (1 - O.B1) * g / (np.sqrt((1 - O.B2) * g * g) + 1e-5), rtol=1e-12)
    mean, var = stats["bn_in"]
    mm0, mv0 = (np.asarray(a, dtype=np.float64) for a in state["bn"]["bn_in"])
    np.testing.assert_allclose(oracle.bn["bn_in"][0], mm0 * 0.99 + mean * 0.01, rtol=1e-12)
    np.testing.assert_allclose(oracle.bn["bn_in"][1], mv0 * 0.99 + var * 0.01, rtol=1e-12)


# ---- the inference fold ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,use_bn", [((16, 16, 8), True), ((16,), True), ((32, 16), False)])
def test_inference_fold_equals_batchnorm_in_evaluation_mode(hidden, use_bn):
    """(W1', b1', s_l, t_l) applied as the score kernel applies them against the oracle's own evaluation-mode forward in f64, and
    `NCFNet.inference_fold` against the net's torch composition in inference mode."""
    K, L = 8, len(hidden)
    state = O.random_state(9, O.N_USERS, O.N_ITEMS, K, hidden, use_bn)
    rng = np.random.default_rng(2)
    rows = np.stack([rng.integers(0, O.N_USERS + 1, 50), O.N_USERS + 1 + rng.integers(0, O.N_ITEMS + 1, 50)], axis=1)

    def folded(W, b, s, t, wg, wd, c, e):
        u, i = e[:, 0], e[:, 1]
        h = np.concatenate([u, i], axis=1)
        for l in range(L):
            h = h @ W[l] + b[l]
            if l < L - 1:
                h = np.maximum(h, 0)
                if s[l] is not None:
                    h = h * s[l] + t[l]
        return (u * i) @ wg + h @ wd + c

    W, b, s, t, wg, wd, c = O.inference_fold(state, K, L, use_bn)
    assert all((x is None) == (not use_bn) for x in s[:L - 1]) and s[L - 1] is None
    want = O.NCFOracle(state, K, L, use_bn, 0.01).forward(rows)
    np.testing.assert_allclose(folded(W, b, s, t, wg, wd, c, state["embed"][rows].astype(np.float64)), want, rtol=1e-12, atol=1e-13)
    # the net's own fold, f32 on the host
    net = nets.NCFNet(O.N_USERS, O.N_ITEMS, K, hidden, use_bn, device=torch.device("cpu"))
    with torch.no_grad():
        net.tables.embed.copy_(torch.from_numpy(state["embed"]))
        for k, v in state["P"].items():
            net.P[k].copy_(torch.from_numpy(v))
        for k, bn in [("bn_in", net.mlp.bn_in)] + [(f"bn{i}", x) for i, x in enumerate(net.mlp.bns, start=1)]:
            if bn is not None:
                bn.moving_mean.copy_(torch.from_numpy(state["bn"][k][0]))
                bn.moving_var.copy_(torch.from_numpy(state["bn"][k][1]))
        e = net.tables.embed[torch.from_numpy(rows)]
        got = net._logits(e[:, 0], e[:, 1], False).numpy()
        Wn, bn_, sn, tn, wgn, wdn, cn = net.inference_fold()
    tonp = lambda xs: [None if x is None else x.numpy() for x in xs]
    mine = folded(tonp(Wn), tonp(bn_), tonp(sn), tonp(tn), wgn.numpy(), wdn.numpy(), cn, e.numpy())
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(mine, want, rtol=1e-4, atol=5e-5)


# ---- why the GMF product has its own kernel -----------------------------------------------------------------------------------
def test_fm_identity_is_not_the_product_in_f32():
    """For two fields the DeepFM kernels' 0.5((u+i)^2 - u^2 - i^2) equals u * i only up to an error of order eps * u^2: on this
    pair the identity is off by more than 1 % while the f32 product is the correctly rounded one."""
    u, i = np.float32(1000.0), np.float32(1.0e-3)
    s = np.float32(u + i)
    fm = np.float32(0.5) * np.float32(np.float32(s * s) - np.float32(u * u) - np.float32(i * i))
    exact = float(u) * float(i)
    prod = np.float32(u * i)
    assert prod == np.float32(exact)
    assert abs(float(fm) - exact) > 1e-2 * exact and abs(float(fm) - exact) < 2.0 ** -23 * float(u) ** 2 * 2
    assert fm != prod


# ---- the envelope ----------------------------------------------------------------------------------------------------------
def test_supported_query_on_the_corners_of_the_envelope():
    yes = [(4, (16,)), (128, (16,)), (16, (128, 64, 32)), (16, (256, 32)), (16, (16, 16, 16, 16)), (64, (64, 64, 64, 16)),
           (4, (256, 16)), (16, (256, 16)), (8, (48, 16))]
    no = [(0, (16,)), (2, (16,)), (6, (16,)), (132, (16,)), (16, ()), (16, (16,) * 5), (16, (8,)), (16, (24,)), (16, (272,)),
          (16, (128, 0)), (64, (256, 16)), (64, (128, 64, 32)), (128, (256, 256))]
    for K, w in yes:
        assert O.score_envelope(K, w) and ops.ncf_score_supported(K, w), (K, w)
    for K, w in no:
        assert not O.score_envelope(K, w) and not ops.ncf_score_supported(K, w), (K, w)
    # the LDS boundary, from the layout the header states: one width step across 160 KB flips the answer
    assert O.score_lds_bytes(16, (128, 64, 32)) == 4 * (32 * 128 + 128 * 64 + 64 * 32 + 68 * (64 + 128)) == 109568
    flips = 0
    for K, w1 in itertools.product((16, 32, 64, 96, 128), range(16, 257, 16)):
        for w in ((w1,), (w1, 64), (w1, w1)):
            assert ops.ncf_score_supported(K, w) == O.score_envelope(K, w), (K, w)
            flips += O.score_lds_bytes(K, w) > 160 * 1024
    assert 0 < flips < 5 * 16 * 3
    for K, w in itertools.product(O.SCORE_KS, O.SCORE_STACKS):
        assert ops.ncf_score_supported(K, w) == O.score_envelope(K, w), (K, w)
    assert sum(O.score_envelope(K, w) for K, w in itertools.product(O.SCORE_KS, O.SCORE_STACKS)) == 13
