"""The oracle of Caser's convolutions (tests/caser_oracle.py) against torch's own `conv1d`, `amax` and autograd, the oracle's
f32 arithmetic against every tolerance tests/test_caser_gpu.py uses, and the host-side surface of `Caser`.  No device."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import caser_oracle as O
from .test_api_signatures_cpu import accepts

SMALL = [s for s in O.STACK_SHAPES if s[0] * s[1] * s[1] * s[2] * s[3] <= 37 * 50 * 50 * 64 * 16]


def _sid(s):
    return "x".join(map(str, s))


def _torch_convs(c, x):
    """The convolutions from torch ops in f64: F.conv1d + relu, torch.max(dim) -> (feat, arg, parameters)."""
    L = c["shape"][1]
    t, hs, args = [], [], []
    for W, b in c["layers"]:
        t.append(tuple(torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (W, b)))
    for i in range(1, L + 1):
        z = torch.relu(F.conv1d(x.transpose(1, 2), t[i - 1][0].permute(2, 1, 0), t[i - 1][1]))
        h, a = z.max(dim=2)
        hs.append(h)
        args.append(a)
    v = torch.relu(F.conv1d(x, t[L][0].permute(2, 1, 0), t[L][1])).transpose(1, 2).reshape(x.shape[0], -1)
    return torch.cat(hs + [v], dim=1), torch.cat(args, dim=1), t


@pytest.mark.parametrize("shape", SMALL, ids=_sid)
def test_forward_equals_torch_conv1d(shape):
    c = O.stack_case(*shape)
    L, nh = shape[1], shape[3]
    feat, arg, zs = O.forward_oracle(c, "f64")
    with torch.no_grad():
        t_feat, t_arg, _ = _torch_convs(c, torch.tensor(O.case_input(c), dtype=torch.float64))
    np.testing.assert_allclose(feat, t_feat.numpy(), rtol=0, atol=1e-12)
    # the first maximum, torch's rule: equal to torch's own arg wherever the maximum leads by more than the two sums' rounding
    for i in range(1, L + 1):
        sl = slice((i - 1) * nh, i * nh)
        assert np.array_equal(arg[:, sl], torch.tensor(zs[i - 1]).max(dim=1).indices.numpy())
        if L - i + 1 > 1:
            clear = feat[:, sl] - np.sort(zs[i - 1], axis=1)[:, -2] > 1e-12
            assert np.array_equal(arg[:, sl][clear], t_arg.numpy()[:, sl][clear])


def test_arg_is_the_first_maximum():
    """Windows whose last positions repeat one id give equal positions: the oracle's arg is the first of them, like torch.max."""
    c = O.stack_case(37, 10, 16, 2, 4)
    c["custom"] = True
    c["ids"][:, 5:] = c["V"] - 1
    feat, arg, zs = O.forward_oracle(c, "f64")
    hit = False
    for i in range(1, 6):                                      # kernel size i: the positions 5 .. 10 - i see only the pad row
        z, a = zs[i - 1], arg[:, (i - 1) * 2: i * 2]
        assert (z[:, 5:] == z[:, 5:6]).all() and (a <= 5).all()
        v, at = torch.tensor(z).max(dim=1)
        assert np.array_equal(at.numpy(), a) and np.array_equal(v.numpy(), feat[:, (i - 1) * 2: i * 2])
        hit = hit or bool((a == 5).any())
    assert hit


@pytest.mark.parametrize("shape", [(37, 2, 3, 2, 1), (37, 10, 16, 2, 4), (300, 10, 20, 3, 4), (5, 64, 8, 1, 64)], ids=_sid)
def test_analytic_backward_equals_autograd(shape):
    c = O.stack_case(*shape)
    ids = c["ids"].copy()
    ids[2 % shape[0], 0], ids[4 % shape[0], shape[1] - 1] = -1, c["V"] + 5          # bad ids are zero input rows
    x = O.case_input(c, ids)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    t_feat, t_arg, t = _torch_convs(c, xt)
    t_feat.backward(torch.tensor(c["gfeat"], dtype=torch.float64))
    gx, grads = O.conv_backward(x, c["layers"], t_feat.detach().numpy() > 0, t_arg.numpy(), c["gfeat"], "f64")
    np.testing.assert_allclose(gx, xt.grad.numpy(), rtol=0, atol=1e-11)
    for j, (gW, gb) in enumerate(grads):
        np.testing.assert_allclose(gW, t[j][0].grad.numpy(), rtol=0, atol=1e-11, err_msg=f"gW[{j}]")
        np.testing.assert_allclose(gb, t[j][1].grad.numpy(), rtol=0, atol=1e-11, err_msg=f"gb[{j}]")


@pytest.mark.parametrize("shape", O.STACK_SHAPES + O.WIDE_SHAPES, ids=_sid)
def test_f32_oracle_passes_the_gpu_tolerances(shape):
    """The f32 variant handed to the very checker the device results go through."""
    c = O.stack_case(*shape)
    O.check_caser(O.oracle_result(c, "f32"), c, f"cpu {_sid(shape)}")


def test_every_case_has_live_units():
    """A case whose units are all dead would compare zeros: every seeded case has live horizontal and vertical units."""
    for shape in O.STACK_SHAPES + O.WIDE_SHAPES:
        feat, _, _ = O.forward_oracle(O.stack_case(*shape), "f64")
        H = shape[1] * shape[3]
        assert (feat[:, :H] > 0).any() and (feat[:, H:] > 0).any(), shape


def test_params_round_trip_and_layout():
    c = O.stack_case(37, 2, 3, 2, 1)
    flat = O.pack_params(c["layers"])
    assert flat.size == 8 + 4 + 12 + 4 + 4 + 4                    # 1*3*2 -> 8, 2 -> 4, 2*3*2 -> 12, 2 -> 4, 1*2*1 -> 4, 1 -> 4
    layers, gaps = O.unpack_params(flat, 2, 3, 2, 1)
    assert not gaps.any() and all(np.array_equal(a, b) for p, q in zip(layers, c["layers"]) for a, b in zip(p, q))


# ---- the training step ----------------------------------------------------------------------
def _twin(cfg):
    loss, dense, reg, norm, _ = cfg
    S = O.STEP_SHAPE
    return O.NetTwin(O.step_weights(O.step_seed(cfg)), S["L"], loss, S["lr"], dense=dense, reg=reg, norm_embed=norm)


def _batches(cfg):
    return O.step_batches(seed=O.step_seed(cfg), num_neg=cfg[4])


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_step_batches_stay_clear_of_relu_and_pool_flips(cfg):
    """Adam turns a flipped ReLU or a flipped argmax into an O(lr) difference of the variables, which no tolerance of the
    step test could absorb.  So at every step of the seeded batches the twin's smallest non-zero |pre-activation| (the
    convolutions' and the Dense layer's) and its smallest pool lead (exact ties aside) exceed 100 x the forward bound measured
    on that batch."""
    twin = _twin(cfg)
    for step, batch in enumerate(_batches(cfg), 1):
        w = {k: v.numpy() for k, v in twin.w.items()}
        bound = O.step_forward_bound(w, batch["seqs"])
        z, lead = twin.margins(batch["users"], batch["seqs"])
        print(f"CASER-FIGURE margins {cfg} step {step}: |z| {z:.3e} lead {lead:.3e} bound {bound:.3e}")
        assert z > 100 * bound and lead > 100 * bound, (step, z, lead, bound)
        twin.train_step(**batch)


def test_twin_step_tolerances_hold_for_an_f32_twin():
    """The training-step tolerances of the GPU file (loss 1e-5, variables rtol 1e-4 / atol 5e-5) are met by the steps of the
    twin whose weights are rounded to f32 after every step."""
    for cfg in (O.STEP_CONFIGS[0], O.STEP_CONFIGS[3], O.STEP_CONFIGS[5]):
        a, b = _twin(cfg), _twin(cfg)
        for batch in _batches(cfg):
            la, lb = a.train_step(**batch), b.train_step(**batch)
            b.w = {k: v.float().double() for k, v in b.w.items()}
            assert abs(la - lb) < 1e-5
            for k in a.w:
                np.testing.assert_allclose(b.w[k].numpy(), a.w[k].numpy(), rtol=1e-4, atol=5e-5, err_msg=k)


def test_twin_user_side_equals_the_numpy_convolutions():
    cfg = O.STEP_CONFIGS[5]
    twin = _twin(cfg)
    batch = _batches(cfg)[0]
    w = {k: v.numpy() for k, v in twin.w.items()}
    layers = [(w[f"{n}/kernel"], w[f"{n}/bias"]) for n in O.conv_names(O.STEP_SHAPE["L"])]
    feat, _, _ = O.conv_forward(w["seq_embeds_var"][batch["seqs"]], layers, "f64")
    want = np.concatenate([w["user_embeds_var"][batch["users"]], np.maximum(feat @ w["dense/kernel"] + w["dense/bias"], 0)], axis=1)
    np.testing.assert_allclose(twin.user_vectors(twin.w, batch["users"], batch["seqs"]).numpy(), want, rtol=0, atol=1e-12)


# ---- the host-side surface of the model ----------------------------------------------------
L, N = 4, 6
_NO_COLS = SimpleNamespace(name=[], index=[])


class _Info:                                                     # the stub of tests/test_dyn_embed_base_cpu.py
    global_mean, min_max_rating = 3.0, (1, 5)
    n_users, n_items = 3, N
    user_consumed = {0: [0, 1, 2, 3, 4, 5], 1: [3], 2: []}
    user2id = {"a": 0, "b": 1, "c": 2}
    item2id = {10 * (i + 1): i for i in range(N)}            # raw 10, 20, .. 60 -> 0 .. 5
    item_col = []
    user_sparse_col = user_dense_col = item_sparse_col = item_dense_col = _NO_COLS
    user_sparse_unique = user_dense_unique = None


def _model(**kw):
    from librecommender_amd.algorithms import Caser

    return Caser("ranking", _Info(), **dict(dict(recent_num=L), **kw))


def test_constructor_accepts_the_reference_signature():
    from librecommender_amd.algorithms import Caser

    golden = json.loads((Path(__file__).parent / "golden" / "caser_signature.json").read_text())
    problem = accepts(golden["algorithms.Caser.__init__"], Caser.__init__)
    assert problem is None, problem


def test_check_params_errors():
    with pytest.raises(ValueError, match="`loss_type` must be one of"):
        _model(loss_type="bpr")
    with pytest.raises(ValueError, match="dense_adam=True"):
        _model(reg=0.01)
    with pytest.raises(ValueError, match="`nh_filters` must be a positive integer"):
        _model(nh_filters=0)
    with pytest.raises(ValueError, match="`nv_filters` must be a positive integer"):
        _model(nv_filters=1.5)
    with pytest.raises(ValueError, match="dropout_rate"):
        _model(dropout_rate=1.5)
    m = _model(use_bn=True, dropout_rate=0.3, nh_filters=3, recent_num=10)
    assert m.use_bn is True and m.dropout_rate == 0.3 and m.uses_sequence and m.max_seq_len == 10
    assert (m.nh_filters, m.nv_filters, m.n_epochs) == (3, 4, 20)
    assert m.recent_seqs.shape == (4, 10) and (m.recent_seqs[2] == N).all()      # no history: the window of pad ids


def test_class_structure():
    from librecommender_amd.algorithms import Caser
    from librecommender_amd.bases import DynEmbedBase, EmbedBase

    assert issubclass(Caser, DynEmbedBase) and issubclass(DynEmbedBase, EmbedBase)
    assert "convert_array_id" not in vars(Caser) and "recommend_user" not in vars(Caser)
    assert Caser.convert_array_id is DynEmbedBase.convert_array_id and Caser.recommend_user is DynEmbedBase.recommend_user
    assert "dyn_user_embedding" in vars(Caser) and vars(Caser)["takes_user_feats"] is False


@pytest.mark.parametrize("seq", [None, [10, 20]], ids=["no-seq", "seq"])
def test_user_feats_are_rejected_by_name(seq):
    m = _model()
    for call in (lambda: m.recommend_user("a", 3, user_feats={"age": 1}, seq=seq),
                 lambda: m.dyn_user_embedding("a", user_feats={"age": 1}, seq=seq)):
        with pytest.raises(ValueError, match="`Caser` has no user features: `user_feats`"):
            call()


def test_window_of_a_given_sequence():
    m = _model()
    assert m.max_seq_len == L and m.n_items == N
    for seq, inner_id, want in (([10, 20, 30, 40, 50, 60], False, [[2, 3, 4, 5]]), ([30, 10], False, [[2, 0, N, N]]),
                                ([10, 999, 20], False, [[0, N, 1, N]]), ([1, -1, 6, 2], True, [[1, N, N, 2]])):
        got = m._window(0, seq, inner_id)
        assert got.shape == (1, L) and got.dtype == np.int32
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("seq", [None, []], ids=["none", "empty"])
def test_window_fallbacks(seq):
    """No `seq`: the cached recent window; the OOV user's window is all pad."""
    m = _model()
    want = {0: [[2, 3, 4, 5]], 1: [[3, N, N, N]], 2: [[N, N, N, N]], m.n_users: [[N, N, N, N]]}
    for uid, w in want.items():
        got = m._window(uid, seq, False)
        assert got.shape == (1, L) and got.dtype == np.int32
        np.testing.assert_array_equal(got, w, err_msg=f"user {uid}")
    np.testing.assert_array_equal(m._window(1, seq, True), m.recent_seqs[[1]])


def test_sequence_models_default_names_caser():
    from librecommender_amd.recommendation import check_dynamic_rec_feats

    check_dynamic_rec_feats("Caser", 1, None, [1, 2])


def test_conv_param_names_and_exports():
    import librecommender_amd.algorithms as A
    import librecommender_amd.nets as Nn
    from librecommender_amd.nets.caser_net import conv_param_names

    assert "Caser" in A.__all__ and "CaserNet" in Nn.__all__
    names = conv_param_names(3)
    assert names[0] == ("conv1d/kernel", "conv1d/bias") and names[-1] == ("conv1d_3/kernel", "conv1d_3/bias") and len(names) == 4
