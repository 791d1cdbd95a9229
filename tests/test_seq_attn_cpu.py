"""The sequence-attention oracle (tests/seq_attn_oracle.py) against torch autograd in fp64 of the two compositions the kernels
replace (`seq_nets.multi_head_attention`'s core and `feat_nets.dot_attention_torch`), the f32 semantics of a row with nothing
allowed, the host queries of csrc/seq_attn.hip (the launch plan among them: its invariants over the whole envelope, the plan
of every case written for a branch, and that the cases reach every branch), and the argument errors of `ops.seq_attn` that
need no device."""
import ctypes as C
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


@pytest.mark.parametrize("args", [O.CASES[3], O.CASES[4], O.CASES[5], O.CASES[25]], ids=O.sid)
def test_oracle_gk_and_gv_apart(args):
    """Values that are not the keys: the same composition written out with three inputs, so gk and gv are pinned one by one
    (also where the case's values are its keys, on several heads with a u8 mask: no pooling form)."""
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


@pytest.mark.parametrize("args", [c for c in O.CASES if c[7] and c[0] <= 6 and c[1] == c[3] == 1 and c[5] == "lens"], ids=O.sid)
def test_oracle_equals_autograd_of_dot_attention(args):
    """The pooling form: one query, one head, a length mask."""
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


# ---- the launch plan (`lr_seq_attn_plan_params`, `ops.seq_attn_plan`): what the launches themselves derive ------------
def _plan(lib, B, Tq, Tk, H, hd, bwd, aligned=1):
    out = (C.c_int32 * 8)()
    assert lib.lr_seq_attn_plan_params(B, Tq, Tk, H, hd, bwd, aligned, out) == 0, (B, Tq, Tk, H, hd, bwd)
    return tuple(out)


def test_plan_invariants_over_the_whole_envelope():
    """Every Tq = Tk in 1 .. 64 and hd in 1 .. 128, forward and backward, one head, a batch of one sample and one that asks
    for the cap of 64 units per workgroup: the tile fits 64 KB, the chunks cover the head's columns exactly once, chunks start
    on a multiple of 4 columns, the strides are what the kernels' bank-conflict reasoning assumes, and G is Tk's alone."""
    lib = _lib.load()
    up4 = lambda n: (n + 3) & ~3
    tiled = chunked = 0
    for T in range(1, 65):
        groups = set()
        for hd in range(1, 129):
            for B in (1, 40000):
                for bwd in (0, 1):
                    TB, nch, CW, CS, ST, G, vec, lds = _plan(lib, B, T, T, 1, hd, bwd)
                    what = (B, T, hd, bwd)
                    assert lds <= 65536 and 1 <= TB <= 64, what
                    assert (nch - 1) * CW < hd <= nch * CW, what
                    assert nch == 1 or CW % 4 == 0, what
                    assert CS % 4 == 0 and (CS // 4) % 2 == 1 and CS >= up4(CW), what
                    assert ST == T | 1 and vec == (hd % 4 == 0), what
                    assert _plan(lib, B, T, T, 1, hd, bwd, 0)[:6] == (TB, nch, CW, CS, ST, G), what    # alignment moves `vec` alone
                    assert TB == 1 or (B > 1 and nch == 1), what       # a unit that needs two chunks leaves no room for a second
                    groups.add(G)
                    tiled += TB > 1
                    chunked += nch > 1
        assert groups == {1 if T <= 8 else 2 if T <= 16 else 4 if T <= 32 else 8}, T
    assert tiled and chunked


def test_plan_errors():
    lib = _lib.load()
    out = (C.c_int32 * 8)(*([7] * 8))
    for bad in ((65, 4, 1, 8), (4, 65, 1, 8), (4, 4, 1, 129), (4, 4, 9, 8), (4, 4, 8, 33), (0, 4, 1, 8), (4, 4, 1, 0)):
        assert lib.lr_seq_attn_plan_params(3, *bad, 0, 1, out) == _lib.LR_ESHAPE, bad
        with pytest.raises(ValueError, match="lr_seq_attn_plan_params"):
            ops.seq_attn_plan(3, *bad, False)
    for B in (0, -1):
        assert lib.lr_seq_attn_plan_params(B, 4, 4, 1, 8, 0, 1, out) == _lib.LR_EINVAL
        assert lib.lr_seq_attn_plan_params(B, 4, 4, 1, 8, 1, 1, out) == _lib.LR_EINVAL
    assert lib.lr_seq_attn_plan_params(3, 4, 4, 1, 8, 0, 1, None) == _lib.LR_EINVAL
    assert list(out) == [7] * 8                                            # an error writes nothing
    assert lib.lr_seq_attn_plan_params(3, 4, 4, 1, 8, 0, 1, out) == 0 and out[0] == 1
    with pytest.raises(ValueError, match="lr_seq_attn_plan_params"):
        ops.seq_attn_plan(0, 4, 4, 1, 8, True)
    p = ops.seq_attn_plan(3, 4, 9, 2, 8, True)
    assert list(p) == ["TB", "nch", "CW", "CS", "ST", "G", "vec", "lds_bytes"] and p["vec"] == 1 and p["ST"] == 9 and p["G"] == 2
    assert ops.seq_attn_plan(3, 4, 9, 2, 8, True, aligned=False)["vec"] == 0 and ops.seq_attn_plan(3, 4, 9, 2, 7, True)["vec"] == 0


# (TB, nch, CW) forward and backward of every case appended to `O.CASES` for its plan: a change to the heuristics or to the
# number of compute units they assume that moves a case off the branch it was written for fails here, by name
PLANS = {
    (345, 3, 3, 3, 4, "lens", False, False): ((2, 1, 4), (2, 1, 4)),
    (345, 4, 9, 3, 8, "u8", False, False): ((2, 1, 8), (2, 1, 8)),
    (345, 6, 6, 3, 8, "lens", True, False): ((2, 1, 8), (2, 1, 8)),
    (4099, 5, 5, 8, 4, "lens", False, False): ((64, 1, 4), (64, 1, 4)),
    (4099, 1, 7, 8, 4, "lens", False, True): ((64, 1, 4), (64, 1, 4)),
    (1537, 40, 40, 1, 32, "lens", False, False): ((3, 1, 32), (2, 1, 32)),
    (1300, 1, 20, 1, 16, "lens", False, True): ((2, 1, 16), (2, 1, 16)),
    (3, 20, 20, 1, 8, "lens", False, False): ((1, 1, 8), (1, 1, 8)),
    (2, 64, 64, 1, 64, "lens", True, False): ((1, 1, 64), (1, 2, 32)),
    (2, 64, 64, 1, 128, "lens", False, False): ((1, 2, 64), (1, 3, 44)),
    (2, 64, 64, 1, 99, "lens", False, False): ((1, 2, 52), (1, 2, 52)),
    (2, 64, 64, 1, 61, "lens", False, False): ((1, 1, 61), (1, 2, 32)),
    (1, 64, 64, 2, 128, "u8", False, True): ((1, 2, 64), (1, 3, 44)),
    (2, 63, 61, 1, 128, "lens", False, False): ((1, 2, 64), (1, 2, 64)),
}
# what else the cases were written for: G, and the units of the last tile (forward) where it is ragged
PLAN_G = {(345, 4, 9, 3, 8, "u8", False, False): 2, (1537, 40, 40, 1, 32, "lens", False, False): 8,
          (1300, 1, 20, 1, 16, "lens", False, True): 4, (3, 20, 20, 1, 8, "lens", False, False): 4}
PLAN_TAIL = {(345, 3, 3, 3, 4, "lens", False, False): 1, (4099, 5, 5, 8, 4, "lens", False, False): 24}


def test_the_appended_cases_are_the_planned_ones():
    assert list(PLANS) == O.CASES[13:] and len(O.CASES) == 27
    assert O.CASES[3][6] and O.CASES[5][1:3] == (4, 9) and O.WIDE[0] == O.CASES[11][0] == 131       # the cases used by index


@pytest.mark.parametrize("args", list(PLANS), ids=O.sid)
def test_pinned_plan(args):
    B, Tq, Tk, H, hd = args[:5]
    fwd, bwd = ops.seq_attn_plan(B, Tq, Tk, H, hd, False), ops.seq_attn_plan(B, Tq, Tk, H, hd, True)
    assert ((fwd["TB"], fwd["nch"], fwd["CW"]), (bwd["TB"], bwd["nch"], bwd["CW"])) == PLANS[args]
    assert fwd["G"] == bwd["G"] == PLAN_G.get(args, fwd["G"])
    if args in PLAN_TAIL:
        assert (B * H) % fwd["TB"] == PLAN_TAIL[args]


def test_the_cases_reach_every_branch_of_the_plan():
    """The union over `O.CASES` of what `O.plan_class` finds.  More than one unit per workgroup together with more than one
    chunk is not asked for: it cannot occur (`test_plan_invariants_over_the_whole_envelope` asserts so)."""
    reached = set().union(*(O.plan_class(args) for args in O.CASES))
    wanted = {"TB=1", "1<TB<64", "TB=64", "TB fwd!=bwd", "nch=1", "nch=2", "nch=3", "nch fwd!=bwd", "last chunk cw%4!=0",
              "G=1", "G=2", "G=4", "G=8", "shared, nch>1", "ragged last tile"}
    assert wanted <= reached, sorted(wanted - reached)
    assert O.plan_class(O.CASES[0]) == {"TB=1", "nch=1", "G=1"}
    assert {"1<TB<64", "TB fwd!=bwd", "ragged last tile", "G=8"} <= O.plan_class(O.TILE_CLAMPED)


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
