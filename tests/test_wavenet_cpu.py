"""The oracle of the WaveNet stack (tests/wavenet_oracle.py) against torch's own `conv1d`, `max` and autograd, the oracle's f32
arithmetic against every tolerance tests/test_wavenet_gpu.py uses, and the host-side surface of `WaveNet`.  No device."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import wavenet_oracle as O
from .test_api_signatures_cpu import accepts

SMALL = [s for s in O.STACK_SHAPES if s[0] * s[1] * s[3] <= 37 * 50 * 64]


def _sid(s):
    return "x".join(map(str, s))


def _torch_stack(c, x):
    """The stack from torch ops in f64: F.conv1d on a left-padded input + relu, torch.max(dim) -> (acts, pooled, arg)."""
    t = {}
    a = x.transpose(1, 2)
    acts = []
    for j, (K, b) in enumerate(c["layers"]):
        Kt, bt = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (K, b))
        t[j] = (Kt, bt)
        d = O.dilation(j, c["npb"]) if K.shape[0] == 2 else 1
        a = torch.relu(F.conv1d(F.pad(a, ((K.shape[0] - 1) * d, 0)), Kt.permute(2, 1, 0), bt, dilation=d))
        acts.append(a.transpose(1, 2))
    pooled, arg = a.max(dim=2)
    return acts, pooled, arg, t


@pytest.mark.parametrize("shape", SMALL, ids=_sid)
def test_forward_equals_torch_conv1d(shape):
    c = O.stack_case(*shape)
    acts, pooled, arg = O.forward_oracle(c, "f64")
    with torch.no_grad():
        t_acts, t_pooled, t_arg, _ = _torch_stack(c, torch.tensor(O.case_input(c), dtype=torch.float64))
    for a, b in zip(acts, t_acts):
        np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(pooled, t_pooled.numpy(), rtol=0, atol=1e-12)
    # the first maximum, torch's rule: equal to torch's own arg wherever the maximum leads by more than the two sums' rounding
    last = acts[-1]
    assert np.array_equal(arg, torch.tensor(last).max(dim=1).indices.numpy())
    if shape[1] > 1:
        clear = pooled - np.sort(last, axis=1)[:, -2] > 1e-12
        assert np.array_equal(arg[clear], t_arg.numpy()[clear])


def test_arg_is_the_first_maximum():
    """Windows whose last positions repeat one id give equal columns: the oracle's arg is the first of them, like torch.max."""
    c = O.stack_case(37, 10, 16, 16, 1, 1)
    c["custom"] = True
    c["ids"][:, 5:] = c["V"] - 1
    acts, pooled, arg = O.forward_oracle(c, "f64")
    assert (acts[-1][:, 6:] == acts[-1][:, 6:7]).all() and (arg <= 6).all()
    v, i = torch.tensor(acts[-1]).max(dim=1)
    assert np.array_equal(i.numpy(), arg) and np.array_equal(v.numpy(), pooled)


@pytest.mark.parametrize("shape", [(37, 2, 3, 5, 1, 2), (37, 10, 16, 16, 1, 4), (300, 10, 20, 16, 2, 2), (5, 128, 8, 128, 1, 8)], ids=_sid)
def test_analytic_backward_equals_autograd(shape):
    c = O.stack_case(*shape)
    ids = c["ids"].copy()
    ids[2 % shape[0], 0], ids[4 % shape[0], shape[1] - 1] = -1, c["V"] + 5          # bad ids are zero input rows
    x = O.case_input(c, ids)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    t_acts, t_pooled, t_arg, t = _torch_stack(c, xt)
    t_pooled.backward(torch.tensor(c["gpooled"], dtype=torch.float64))
    acts = [a.detach().numpy() for a in t_acts]
    gx, grads = O.stack_backward(x, c["layers"], c["npb"], acts, [a > 0 for a in acts], t_arg.numpy(), c["gpooled"], "f64")
    np.testing.assert_allclose(gx, xt.grad.numpy(), rtol=0, atol=1e-11)
    for j, (gK, gb) in enumerate(grads):
        np.testing.assert_allclose(gK, t[j][0].grad.numpy(), rtol=0, atol=1e-11, err_msg=f"gK[{j}]")
        np.testing.assert_allclose(gb, t[j][1].grad.numpy(), rtol=0, atol=1e-11, err_msg=f"gb[{j}]")


@pytest.mark.parametrize("shape", O.STACK_SHAPES + O.WIDE_SHAPES, ids=_sid)
def test_f32_oracle_passes_the_gpu_tolerances(shape):
    """The f32 variant handed to the very checker the device results go through."""
    c = O.stack_case(*shape)
    O.check_stack(O.oracle_result(c, "f32"), c, f"cpu {_sid(shape)}")


def test_params_round_trip_and_layout():
    c = O.stack_case(37, 2, 3, 5, 1, 2)
    flat = O.pack_params(c["layers"])
    assert flat.size == 32 + 8 + 52 + 8 + 28 + 8                 # 2*3*5 -> 32, 5 -> 8, 2*5*5 -> 52, 5 -> 8, 25 -> 28, 5 -> 8
    layers, gaps = O.unpack_params(flat, 3, 5, 1, 2)
    assert not gaps.any() and all(np.array_equal(a, b) for p, q in zip(layers, c["layers"]) for a, b in zip(p, q))


# ---- the training step ----------------------------------------------------------------------
def _twin(cfg, seed=None):
    loss, dense, reg, norm, nb, npb = cfg
    w = O.step_weights(nb, npb, seed)
    return O.NetTwin(w, nb, npb, loss, O.STEP_SHAPE["lr"], dense=dense, reg=reg, norm_embed=norm)


@pytest.mark.parametrize("cfg", O.STEP_CONFIGS, ids=lambda c: "-".join(map(str, c)))
def test_step_batches_stay_clear_of_relu_and_pool_flips(cfg):
    """Adam turns a flipped ReLU or a flipped argmax into an O(lr) difference of the variables, which no tolerance of the
    step test could absorb.  So at every step of the seeded batches the twin's smallest non-zero |pre-activation| and its
    smallest pool lead (exact ties aside) exceed 100 x the forward bound measured on that batch."""
    twin = _twin(cfg)
    for step, batch in enumerate(O.step_batches(), 1):
        w = {k: v.numpy() for k, v in twin.w.items()}
        bound = O.step_forward_bound(w, cfg[4], cfg[5], batch["seqs"])
        z, lead = twin.margins(batch["seqs"])
        print(f"WAVENET-FIGURE margins {cfg} step {step}: |z| {z:.3e} lead {lead:.3e} bound {bound:.3e}")
        assert z > 100 * bound and lead > 100 * bound, (step, z, lead, bound)
        twin.train_step(**batch)


def test_twin_step_tolerances_hold_for_an_f32_twin():
    """The training-step tolerances of the GPU file (loss 1e-5, variables rtol 1e-4 / atol 5e-5) are met by three steps of
    the twin whose weights are rounded to f32 after every step."""
    for cfg in (O.STEP_CONFIGS[0], O.STEP_CONFIGS[3], O.STEP_CONFIGS[5]):
        a, b = _twin(cfg), _twin(cfg)
        for batch in O.step_batches():
            la, lb = a.train_step(**batch), b.train_step(**batch)
            b.w = {k: v.float().double() for k, v in b.w.items()}
            assert abs(la - lb) < 1e-5
            for k in a.w:
                np.testing.assert_allclose(b.w[k].numpy(), a.w[k].numpy(), rtol=1e-4, atol=5e-5, err_msg=k)


def test_twin_user_side_equals_the_numpy_stack():
    cfg = O.STEP_CONFIGS[5]
    twin = _twin(cfg)
    batch = O.step_batches()[0]
    w = {k: v.numpy() for k, v in twin.w.items()}
    layers = [(w[f"{n}/kernel"], w[f"{n}/bias"]) for n in O.conv_names(cfg[4], cfg[5])]
    _, pooled, _ = O.stack_forward(w["seq_embeds_var"][batch["seqs"]], layers, cfg[5], "f64")
    want = np.concatenate([w["user_embeds_var"][batch["users"]], pooled @ w["dense/kernel"] + w["dense/bias"]], axis=1)
    np.testing.assert_allclose(twin.user_vectors(twin.w, batch["users"], batch["seqs"]).numpy(), want, rtol=0, atol=1e-12)


# ---- the host-side surface of the model ----------------------------------------------------
class _Info:
    global_mean, min_max_rating = 3.0, (1, 5)
    n_users, n_items = 3, 5
    user_consumed = {0: [1, 2], 1: [3], 2: []}


def test_constructor_accepts_the_reference_signature():
    from librecommender_amd.algorithms import WaveNet

    golden = json.loads((Path(__file__).parent / "golden" / "wavenet_signature.json").read_text())
    problem = accepts(golden["algorithms.WaveNet.__init__"], WaveNet.__init__)
    assert problem is None, problem


def test_check_params_errors():
    from librecommender_amd.algorithms import WaveNet

    with pytest.raises(ValueError, match="`loss_type` must be one of"):
        WaveNet("ranking", _Info(), loss_type="bpr")
    with pytest.raises(ValueError, match="dense_adam=True"):
        WaveNet("ranking", _Info(), reg=0.01)
    with pytest.raises(ValueError, match="`n_filters` must be a positive integer"):
        WaveNet("ranking", _Info(), n_filters=0)
    with pytest.raises(ValueError, match="dropout_rate"):
        WaveNet("ranking", _Info(), dropout_rate=1.5)
    m = WaveNet("ranking", _Info(), use_bn=True, dropout_rate=0.3, n_blocks=2, n_layers_per_block=3)
    assert m.use_bn is True and m.dropout_rate == 0.3 and m.uses_sequence and m.max_seq_len == 10
    assert (m.n_filters, m.n_blocks, m.n_layers_per_block) == (16, 2, 3)
    assert m.recent_seqs.shape == (4, 10) and (m.recent_seqs[2] == 5).all()      # no history: the window of pad ids


def test_glorot_uniform_uses_the_convolution_fans():
    """Keras' `glorot_uniform` on a Conv1D kernel [k, C_in, C_out]: fans k * C_in and k * C_out."""
    from librecommender_amd.layers.dense import DenseParams

    P = DenseParams(torch.device("cpu"), 3)
    P.add("conv1d/kernel", (2, 40, 24), "glorot_uniform")
    P.add("dense/kernel", (40, 24), "glorot_uniform")
    P.finalize()
    lim3, lim2 = np.sqrt(6.0 / (2 * 40 + 2 * 24)), np.sqrt(6.0 / (40 + 24))
    k3, k2 = P["conv1d/kernel"].detach().abs().max().item(), P["dense/kernel"].detach().abs().max().item()
    assert 0.95 * lim3 < k3 <= lim3 and 0.95 * lim2 < k2 <= lim2


def test_sequence_models_default_names_wavenet():
    from librecommender_amd.recommendation import check_dynamic_rec_feats

    check_dynamic_rec_feats("WaveNet", 1, None, [1, 2])
    with pytest.raises(ValueError):
        check_dynamic_rec_feats("SVD", 1, None, [1, 2])
