"""The oracle of the recurrent layers (tests/rnn_oracle.py) against torch's own cells and autograd, the oracle's f32
arithmetic against every tolerance tests/test_rnn_gpu.py uses, and the host-side surface of `RNN4Rec`.  No device."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from . import rnn_oracle as O
from .test_api_signatures_cpu import accepts

CELLS = ("gru", "lstm")
SMALL = [s for s in O.LAYER_SHAPES if s[0] * s[1] * s[3] <= 37 * 50 * 64]


def _torch_cell(cell, c, D, H):
    """torch.nn.GRU / LSTM carrying the case's weights: Keras' z, r, h columns permuted to torch's r, z, n; the LSTM's gate
    order is the same, with b_hh = 0."""
    W, U, b = (torch.tensor(c[k], dtype=torch.float64) for k in ("W", "U", "b"))
    net = (torch.nn.GRU if cell == "gru" else torch.nn.LSTM)(D, H, batch_first=True).double()
    with torch.no_grad():
        if cell == "gru":
            perm = torch.cat([torch.arange(H, 2 * H), torch.arange(0, H), torch.arange(2 * H, 3 * H)])
            net.weight_ih_l0.copy_(W[:, perm].t())
            net.weight_hh_l0.copy_(U[:, perm].t())
            net.bias_ih_l0.copy_(b[0][perm])
            net.bias_hh_l0.copy_(b[1][perm])
        else:
            net.weight_ih_l0.copy_(W.t())
            net.weight_hh_l0.copy_(U.t())
            net.bias_ih_l0.copy_(b)
            net.bias_hh_l0.zero_()
    return net


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cell", CELLS)
def test_final_state_equals_torch_cells_on_packed_sequences(cell, shape):
    B, L, D, H = shape
    c = O.layer_case(cell, B, L, D, H)
    valid = O.valid_steps(c["lens"], L)
    x = c["table"][c["ids"]]
    hs, _ = O.layer_forward(cell, x, valid, c["W"], c["U"], c["b"], True, variant="f64")
    keep = np.flatnonzero(c["lens"] > 0)
    assert not hs[c["lens"] == 0].any()                       # len 0: every output is 0
    if len(keep) == 0:
        return
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.tensor(x[keep], dtype=torch.float64), torch.tensor(c["lens"][keep]).long(),
                                                     batch_first=True, enforce_sorted=False)
    with torch.no_grad():
        _, state = _torch_cell(cell, c, D, H)(packed)
    final = (state[0] if cell == "lstm" else state)[0].numpy()
    np.testing.assert_allclose(hs[keep, L - 1], final, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("cell", CELLS)
def test_analytic_backward_equals_autograd(cell, act, dropout):
    B, L, D, H = 37, 10, 16, 16
    c = O.layer_case(cell, B, L, D, H, dropout)
    ids = c["ids"].copy()
    ids[5, 0], ids[6, 1] = -1, c["V"] + 5                     # bad ids at valid steps are masked steps
    inside = (ids >= 0) & (ids < c["V"])
    valid = O.valid_steps(c["lens"], L, inside)
    x = np.nan_to_num(c["table"])[np.where(inside, ids, 0)]
    t = {k: torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in ("W", "U", "b")}
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    masks = [None if c[k] is None else torch.tensor(c[k], dtype=torch.float64) for k in ("in_mask", "rec_mask")]
    hs_t = O.layer_forward_torch(cell, xt, torch.as_tensor(valid), t["W"], t["U"], t["b"], act, *masks)
    hs_t.backward(torch.tensor(c["ghs"], dtype=torch.float64))
    want = O.layer_oracle(cell, c, act, "f64", ids)
    for name, got, ref in zip(O.OUTPUTS, want, (hs_t, xt.grad, t["W"].grad, t["U"].grad, t["b"].grad)):
        np.testing.assert_allclose(got, ref.detach().numpy(), rtol=0, atol=1e-11, err_msg=name)
    assert not want[1][~valid].any()


@pytest.mark.parametrize("shape", O.LAYER_SHAPES + O.WIDE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("cell", CELLS)
def test_f32_oracle_passes_the_gpu_tolerances(cell, act, shape):
    """The f32 variant handed to the very checker the device results go through."""
    c = O.layer_case(cell, *shape)
    O.check_layer(O.layer_oracle(cell, c, act, "f32"), cell, c, act, f"cpu {cell} act={act} {shape}")
    if shape in ((37, 10, 16, 16), (300, 7, 16, 128)):
        c = O.layer_case(cell, *shape, dropout=0.5)
        O.check_layer(O.layer_oracle(cell, c, act, "f32"), cell, c, act, f"cpu-dropout {cell} act={act} {shape}")


def test_twin_step_tolerances_hold_for_an_f32_twin():
    """The training-step tolerances of the GPU file (loss 1e-5, variables rtol 1e-4 / atol 5e-5) are met by three steps of
    the twin whose weights are rounded to f32 after every step."""
    for cfg in (("gru", (16, 8), True, "cross_entropy", False, None), ("lstm", (16,), False, "bpr", True, 0.01)):
        cell, hidden, ln, loss, dense, reg = cfg
        w = O.step_weights(cell, hidden, ln)
        a = O.NetTwin(w, cell, len(hidden), ln, loss, O.STEP_SHAPE["lr"], dense=dense, reg=reg)
        b = O.NetTwin(w, cell, len(hidden), ln, loss, O.STEP_SHAPE["lr"], dense=dense, reg=reg)
        for batch in O.step_batches(loss):
            la, lb = a.train_step(**batch), b.train_step(**batch)
            b.w = {k: v.float().double() for k, v in b.w.items()}
            assert abs(la - lb) < 1e-5
            for k in a.w:
                np.testing.assert_allclose(b.w[k].numpy(), a.w[k].numpy(), rtol=1e-4, atol=5e-5, err_msg=k)


def test_stack_with_layer_norm_equals_the_twin():
    cell, hidden = "gru", (16, 8)
    w = O.step_weights(cell, hidden, True)
    batch = O.step_batches("cross_entropy")[0]
    twin = O.NetTwin(w, cell, 2, True, "cross_entropy", 0.01)
    names = O.layer_param_names(cell, 2, True)
    layers = [tuple(w[n] for n in ns) for ns in names]
    valid = O.valid_steps(batch["lens"], batch["seqs"].shape[1])
    last = O.stack_forward(cell, w["seq_embeds_var"][batch["seqs"]], valid, layers, use_ln=True)
    want = twin.user_vectors(twin.w, batch["seqs"], batch["lens"]).numpy()
    np.testing.assert_allclose(last @ w["dense/kernel"].astype(np.float64) + w["dense/bias"], want, rtol=0, atol=1e-12)


# ---- the host-side surface of the model ----------------------------------------------------
class _Info:
    global_mean, min_max_rating = 3.0, (1, 5)
    n_users, n_items = 3, 5
    user_consumed = {0: [1, 2], 1: [3], 2: []}


def test_constructor_accepts_the_reference_signature():
    from librecommender_amd.algorithms import RNN4Rec

    golden = json.loads((Path(__file__).parent / "golden" / "rnn4rec_signature.json").read_text())
    problem = accepts(golden["algorithms.RNN4Rec.__init__"], RNN4Rec.__init__)
    assert problem is None, problem


def test_check_params_errors():
    from librecommender_amd.algorithms import RNN4Rec

    with pytest.raises(ValueError, match="`rnn_type` must either be `lstm` or `gru`"):
        RNN4Rec("ranking", _Info(), rnn_type="rnn")
    with pytest.raises(ValueError, match="`loss_type` must be one of"):
        RNN4Rec("ranking", _Info(), loss_type="mse")
    with pytest.raises(ValueError, match="dense_adam=True"):
        RNN4Rec("ranking", _Info(), reg=0.01)
    m = RNN4Rec("ranking", _Info(), rnn_type="LSTM", hidden_units=[16, 8])
    assert m.rnn_type == "lstm" and m.hidden_units == [16, 8] and m.uses_sequence and m.max_seq_len == 10
    assert m.recent_seqs.shape == (4, 10) and m.recent_seq_lens.tolist() == [2, 1, 0, 1]


def test_sequence_models_default_names_rnn4rec():
    from librecommender_amd.recommendation import check_dynamic_rec_feats

    check_dynamic_rec_feats("RNN4Rec", 1, None, [1, 2])
    with pytest.raises(ValueError):
        check_dynamic_rec_feats("SVD", 1, None, [1, 2])
