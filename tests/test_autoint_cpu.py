"""The oracle of AutoInt's stack (tests/autoint_oracle.py) against `seq_nets.multi_head_attention` and torch autograd, the oracle's
f32 arithmetic against every tolerance tests/test_autoint_gpu.py uses, and the host-side surface of `AutoInt`.  No device."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.algorithms.autoint import AutoInt, attention_config
from librecommender_amd.layers import DenseParams
from librecommender_amd.nets.autoint_net import MHA_KERNELS, mha_layer_names
from librecommender_amd.nets.seq_nets import multi_head_attention

from . import autoint_oracle as O
from .test_api_signatures_cpu import accepts

ALL_SHAPES = O.SHAPES + O.WIDE_SHAPES
GOLDEN = Path(__file__).parent / "golden" / "autoint_signature.json"


def _torch_stack(c):
    """The stack in torch f64 under autograd: `multi_head_attention` per layer, a matmul read-out."""
    _, _, _, H, _, residual = c["shape"]
    t64 = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True)
    x, w, b = t64(c["x"]), t64(c["w"]), t64(c["c"])
    layers = [tuple(t64(m) for m in layer) for layer in c["layers"]]
    a, acts = x, []
    for Wq, Wk, Wv, Wo in layers:
        y = multi_head_attention(a, a, Wq, Wk, Wv, Wo, H, None)
        a = a + y if residual else y
        acts.append(a)
    return x, layers, w, b, acts, a.flatten(1) @ w + b


@pytest.mark.parametrize("shape", O.SHAPES, ids=O.sid)
def test_oracle_equals_multi_head_attention_and_autograd(shape):
    c = O.stack_case(*shape)
    o = O.oracle(c, "f64")
    x, layers, w, b, acts, logits = _torch_stack(c)
    for mine, ref in zip(o["acts"], acts):
        np.testing.assert_allclose(mine, ref.detach().numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(o["logits"], logits.detach().numpy(), rtol=0, atol=1e-11)
    logits.backward(torch.tensor(c["glogits"], dtype=torch.float64))
    np.testing.assert_allclose(o["gx"], x.grad.numpy(), rtol=0, atol=1e-10)
    for l, (mine, ref) in enumerate(zip(o["grads"], layers)):
        for name, g, t in zip(MHA_KERNELS, mine, ref):
            np.testing.assert_allclose(g, t.grad.numpy(), rtol=0, atol=1e-10, err_msg=f"{name}[{l}]")
    np.testing.assert_allclose(o["gw"], w.grad.numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(o["gc"], b.grad.numpy(), rtol=0, atol=1e-10)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=O.sid)
def test_f32_oracle_passes_the_delta_rule(shape):
    """The oracle's own f32 arithmetic is inside the bound at every shape the device is tested at."""
    c = O.stack_case(*shape)
    O.check_stack(O.oracle_result(c, "f32"), c, O.sid(shape))


def test_f32_oracle_passes_the_delta_rule_saturated():
    c = O.saturated_case()
    first = O._layer(c["x"].astype(np.float64), c["layers"][0], c["shape"][3], np.float64)[1]
    scores = np.log(np.maximum(first[3], 1e-300))                    # log-softmax: its spread is the scores' spread
    assert (scores.max(-1) - scores.min(-1)).max() > 80
    O.check_stack(O.oracle_result(c, "f32"), c, "saturated")


def test_softmax_of_one_field_is_one():
    c = O.stack_case(5, 1, 6, 2, (4,), True)
    for variant in ("f64", "f32"):
        p = O._layer(c["x"].astype(O._dt(variant)), c["layers"][0], 2, O._dt(variant))[1][3]
        assert (p == 1).all()


# ---- the constructor -------------------------------------------------------------------------------------------------
def test_constructor_accepts_the_reference_signature():
    sig = json.loads(GOLDEN.read_text())["algorithms.AutoInt.__init__"]
    assert [s[0] for s in sig][:4] == ["self", "task", "data_info", "loss_type"] and len(sig) == 22
    assert accepts(sig, AutoInt.__init__) is None, accepts(sig, AutoInt.__init__)


def test_att_embed_size_validation():
    assert attention_config(None) == (8, 8, 8) and attention_config(()) == (8, 8, 8)
    assert attention_config(4) == (4,) and attention_config(np.int64(4)) == (4,)
    assert attention_config([8, 4]) == (8, 4) and attention_config((16,)) == (16,)
    for bad in ("8", 8.0, {8}, [8, 0], [8, "4"], (8, 4.0)):
        with pytest.raises(ValueError):
            attention_config(bad)


# ---- the parameter layout (a host-only call of the library) -----------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 16, 2, (8, 8, 8)), (3, 6, 3, (1, 5)), (1, 1, 1, (1,)), (17, 7, 2, (8, 4)), (64, 64, 8, (8,) * 8)],
                         ids=O.sid)
def test_parameter_layout_is_dense_params(shape):
    """`lr_autoint_params_bytes` is the length `DenseParams` gives the net's tensors, `pack_params` lays them out alike, and
    the 3-D Keras shapes get Keras' fans."""
    T, D, H, head_dims = shape
    assert ops.autoint_supported(T, D, H, head_dims)
    P = DenseParams(torch.device("cpu"), 3)
    for name, hd in zip(mha_layer_names(len(head_dims)), head_dims):
        for w in MHA_KERNELS[:3]:
            P.add(f"{name}/{w}/kernel", (D, H, hd), "glorot_uniform")
        P.add(f"{name}/attention_output/kernel", (H, hd, D), "glorot_uniform")
    P.add("dense/kernel", (T * D, 1), "glorot_uniform")
    P.add("dense/bias", (1,), "zeros")
    P.finalize()
    assert ops.autoint_param_floats(T, D, H, head_dims) == P.flat.numel()
    names = list(P.params)
    layers = [tuple(P[n].detach().numpy().reshape(s) for n, s in zip(names[4 * l:4 * l + 4], O.param_shapes(T, D, H, head_dims)[4 * l:]))
              for l in range(len(head_dims))]
    packed = O.pack_params(layers, P["dense/kernel"].detach().numpy(), P["dense/bias"].detach().numpy()[0])
    assert np.array_equal(packed, P.flat.numpy())
    back, w, c, gaps = O.unpack_params(packed, T, D, H, head_dims)
    assert all(np.array_equal(a, b) for la, lb in zip(back, layers) for a, b in zip(la, lb)) and not gaps.any()
    hd = head_dims[0]
    for n, fans in ((names[0], D * H + D * hd), (names[3], H * hd + H * D)):
        lim = np.sqrt(6.0 / fans)
        top = float(P[n].detach().abs().max())
        assert top <= lim and (P[n].numel() < 50 or top > 0.8 * lim), n


def test_unsupported_shapes_are_reported():
    for bad in ((65, 16, 2, (8,)), (8, 65, 2, (8,)), (8, 16, 2, (33,)), (8, 16, 9, (4,)), (8, 16, 2, (8,) * 9), (8, 16, 2, ()),
                (0, 16, 2, (8,)), (8, 0, 2, (8,)), (8, 16, 0, (8,)), (8, 16, 2, (8, 0))):
        assert not ops.autoint_supported(*bad), bad
        assert ops.autoint_param_floats(*bad) == 0, bad
