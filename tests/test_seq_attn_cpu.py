"""The sequence-attention oracle (tests/seq_attn_oracle.py) against torch autograd in fp64 of the two compositions the kernels
replace (`seq_nets.multi_head_attention`'s core and `feat_nets.dot_attention_torch`), the f32 semantics of a row with nothing
allowed, the host queries of csrc/seq_attn.hip, and the argument errors of `ops.seq_attn` that need no device."""
import math

import numpy as np
import pytest
import torch

from librecommender_amd import _lib, ops
from librecommender_amd.nets.feat_nets import dot_attention_torch
from librecommender_amd.nets.seq_nets import multi_head_attention

from . import seq_attn_oracle as O


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)


@pytest.mark.parametrize("args", [c for c in O.CASES if not c[7] and c[0] <= 6], ids=O.sid)
def test_oracle_equals_autograd_of_multi_head_attention(args):
    """Identity projections leave the core (the function projects k and v from one input, so the case's keys serve as values
    and that input's gradient is gk + gv): out and the gradients to 1e-12.  No row of these cases is without an allowed key,
    where the composition in fp64 would not round -1e9 + S to f32."""
    c = O.case(*args)
    B, Tq, Tk, H, hd = c["shape"]
    ok = O.allowed(B, Tq, Tk, c["key_ok"], c["lens"], c["causal_or"])
    assert ok.any(-1).all() and c["scale"] == 1.0 / math.sqrt(hd)
    q, kv, eye = _t(c["q"]), _t(c["k"]), torch.eye(H * hd, dtype=torch.float64)
    out = multi_head_attention(q, kv, eye, eye, eye, eye, H, torch.from_numpy(ok.copy()))
    out.backward(torch.from_numpy(c["gout"].astype(np.float64)))
    o, P = O.forward(c["q"], c["k"], c["k"], H, c["scale"], c["key_ok"], c["lens"], c["causal_or"])
    gq, gk, gv = O.backward(c["q"], c["k"], c["k"], H, c["scale"], P, c["gout"])
    assert O.max_diff(out.detach().numpy(), o) <= 1e-12
    assert O.max_diff(q.grad.numpy(), gq) <= 1e-12 and O.max_diff(kv.grad.numpy(), gk + gv) <= 1e-12


@pytest.mark.parametrize("args", [O.CASES[3], O.CASES[4], O.CASES[5]], ids=O.sid)
def test_oracle_gk_and_gv_apart(args):
    """Values that are not the keys: the same composition written out with three inputs, so gk and gv are pinned one by one."""
    c = O.case(*args)
    B, Tq, Tk, H, hd = c["shape"]
    q, k, v = _t(c["q"]), _t(c["k"]), _t(c["v"])
    heads = lambda x, T: x.view(B, T, H, hd).transpose(1, 2)
    s = (heads(q, Tq) * c["scale"]) @ heads(k, Tk).transpose(2, 3)
    ok = torch.from_numpy(O.allowed(B, Tq, Tk, c["key_ok"], c["lens"], c["causal_or"]).copy())
    s = s - 1e9 * (~ok[:, None]).to(s.dtype)
    out = (torch.softmax(s, dim=-1) @ heads(v, Tk)).transpose(1, 2).reshape(B, Tq, H * hd)
    out.backward(torch.from_numpy(c["gout"].astype(np.float64)))
    want = O.run(c, "f64")
    for name, got in (("out", out.detach()), ("gq", q.grad), ("gk", k.grad), ("gv", v.grad)):
        assert O.max_diff(got.numpy(), want[name]) <= 1e-12, name


@pytest.mark.parametrize("args", [c for c in O.CASES if c[7] and c[0] <= 6], ids=O.sid)
def test_oracle_equals_autograd_of_dot_attention(args):
    c = O.case(*args)
    q, keys = _t(c["q"][:, 0]), _t(c["k"])
    out = dot_attention_torch(q, keys, torch.from_numpy(c["lens"]))
    out.backward(torch.from_numpy(c["gout"][:, 0].astype(np.float64)))
    want = O.run(c, "f64")
    assert O.max_diff(out.detach().numpy(), want["out"][:, 0]) <= 1e-12
    assert O.max_diff(q.grad.numpy(), want["gq"][:, 0]) <= 1e-12
    assert O.max_diff(keys.grad.numpy(), want["gk"] + want["gv"]) <= 1e-12


@pytest.mark.parametrize("variant", ["f64", "f32"])
def test_row_with_nothing_allowed_is_uniform(variant):
    """-1e9 + S rounds to -1e9 in f32 for |S| < 32: uniform weights, the mean of v, and the gradient still reaches q and k
    (through dS of the other rows it is 0 here only if gout is orthogonal to v's spread, which it is not)."""
    c = O.all_masked_case()
    B, Tq, Tk, H, hd = c["shape"]
    out, P = O.forward(c["q"], c["k"], c["v"], H, c["scale"], c["key_ok"], None, False, variant)
    s = np.einsum("bihc,bjhc->bhij", c["q"].reshape(B, Tq, H, hd), c["k"].reshape(B, Tk, H, hd)) * c["scale"]
    assert np.abs(s[1]).max() < 32
    assert np.array_equal(P[1], np.full_like(P[1], 1.0 / Tk))
    want = c["v"][1].astype(np.float64).mean(0, keepdims=True).repeat(Tq, 0)
    assert O.max_diff(out[1], want) <= (1e-12 if variant == "f64" else 1e-6)
    gq, gk, _ = O.backward(c["q"], c["k"], c["v"], H, c["scale"], P, c["gout"], variant)
    assert np.abs(gq[1]).max() > 1e-3 and np.abs(gk[1]).max() > 1e-3
    assert not np.array_equal(P[0], np.full_like(P[0], 1.0 / Tk))


def test_f32_oracle_passes_its_own_rule():
    """The rule is not vacuous: the f32 variant is inside it on every case (it is the rule's own yardstick)."""
    for args in O.CASES:
        if args[0] <= 6:
            c = O.case(*args)
            O.check(O.run(c, "f32"), c, O.sid(args))


def test_host_queries():
    lib = _lib.load()
    S = ops.seq_attn_supported
    assert S(1, 1, 1, 1) and S(64, 64, 8, 32) and S(64, 64, 2, 128) and S(50, 50, 1, 80) and S(10, 10, 1, 33)
    assert S(64, 1, 1, 8) and not S(65, 1, 1, 8) and S(1, 64, 1, 8) and not S(1, 65, 1, 8)          # T 64 / 65
    assert S(4, 4, 1, 128) and not S(4, 4, 1, 129)                                                    # hd 128 / 129
    assert S(4, 4, 8, 8) and not S(4, 4, 9, 8)                                                        # H 8 / 9
    assert S(4, 4, 8, 32) and S(4, 4, 4, 64) and not S(4, 4, 8, 33) and not S(4, 4, 3, 86)            # M 256 / 257+
    assert not S(0, 4, 1, 8) and not S(4, 0, 1, 8) and not S(4, 4, 0, 8) and not S(4, 4, 1, 0)
    for ok, bad in (((64, 4, 1, 8), (65, 4, 1, 8)), ((4, 64, 1, 8), (4, 65, 1, 8)), ((4, 4, 1, 128), (4, 4, 1, 129)),
                    ((4, 4, 8, 8), (4, 4, 9, 8)), ((4, 4, 8, 32), (4, 4, 8, 33))):
        assert lib.lr_seq_attn_saved_bytes(3, *ok) > 0 and lib.lr_seq_attn_saved_bytes(3, *bad) == 0
    assert lib.lr_seq_attn_saved_bytes(0, 4, 4, 1, 8) == 0 and lib.lr_seq_attn_saved_bytes(-1, 4, 4, 1, 8) == 0


def test_cpu_tensors_raise_no_cpu_fallback():
    q, k = torch.zeros(2, 3, 8), torch.zeros(2, 5, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seq_attn(q, k, k, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.seq_attn_fwd(q, k, k.clone(), 1, 1.0, lens=torch.ones(2, dtype=torch.int32))


@pytest.mark.parametrize("shape", [(1, 1, 65, 1, 8), (1, 1, 4, 1, 129), (1, 65, 65, 1, 8), (2, 3, 3, 9, 8), (2, 3, 3, 8, 33)], ids=str)
def test_unsupported_shapes_raise_before_any_device_work(shape):
    """The shape is judged by the host query first: a ValueError even for CPU tensors, which a supported shape refuses with
    'no CPU fallback'."""
    B, Tq, Tk, H, hd = shape
    q, k = torch.zeros(B, Tq, H * hd), torch.zeros(B, Tk, H * hd)
    with pytest.raises(ValueError, match="unsupported sequence-attention shape"):
        ops.seq_attn(q, k, k, H, 1.0)
    with pytest.raises(ValueError, match="unsupported sequence-attention shape"):
        ops.seq_attn_bwd(q, k, k, H, 1.0, None, None, False, torch.zeros(0, dtype=torch.uint8), q)
    with pytest.raises(ValueError):
        ops.seq_attn(q, k, k, 3 if (H * hd) % 3 else 7, 1.0)               # M is no multiple of the heads
