"""The sequence-attention kernels (csrc/seq_attn.hip, `ops.seq_attn`) against the CPU oracle (tests/seq_attn_oracle.py, f64
variant) by the delta rule, their bit contracts and argument errors, and the three nets that use them (`FeatTransformerNet`,
`FeatSIMNet`, `FeatDINNet(use_tf_attention=True)`) against the same nets composed from torch ops (`fused_attention=False`).
tests/test_seq_attn_cpu.py pins the oracle to torch autograd; tests/test_din_tower_models_gpu.py pins the nets, kernels
included, to the fp64 restatement of the reference's graphs."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops
from librecommender_amd.nets import FeatDINNet, FeatSpec
from librecommender_amd.nets.seq_nets import FeatSIMNet, FeatTransformerNet

from . import seq_attn_oracle as O
from .test_din_tower_models_gpu import din_batch, din_call

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, c):
    """Forward + backward of one case through the entry points -> {out, gq, gk, gv} (torch)."""
    q, k, gout = _dev(c["q"], dev), _dev(c["k"], dev), _dev(c["gout"], dev)
    v = k if c["shared"] else _dev(c["v"], dev)
    key_ok, lens = _dev(c["key_ok"], dev), _dev(c["lens"], dev)
    out, saved = ops.seq_attn_fwd(q, k, v, c["H"], c["scale"], key_ok, lens, c["causal_or"])
    gq, gk, gv = ops.seq_attn_bwd(q, k, v, c["H"], c["scale"], key_ok, lens, c["causal_or"], saved, gout)
    return dict(out=out, gq=gq, gk=gk, gv=gv)


def _np(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


# ---- 1. the kernels against the oracle -------------------------------------------------------
@pytest.mark.parametrize("args", O.CASES, ids=O.sid)
def test_kernel_case(dev, args):
    """out, gq, gk and gv of every shape class by the delta rule; the autograd form gives the entry points' bits, with
    gk + gv as the key gradient where the keys are the values."""
    c = O.case(*args)
    got = _run(dev, c)
    O.check(_np(got), c, O.sid(args), key=args + (0, 1.0))
    q, k = _dev(c["q"], dev).requires_grad_(True), _dev(c["k"], dev).requires_grad_(True)
    v = k if c["shared"] else _dev(c["v"], dev).requires_grad_(True)
    out = ops.seq_attn(q, k, v, c["H"], c["scale"], _dev(c["key_ok"], dev), _dev(c["lens"], dev), c["causal_or"])
    out.backward(_dev(c["gout"], dev))
    assert torch.equal(out.detach(), got["out"]) and torch.equal(q.grad, got["gq"])
    if c["shared"]:
        assert torch.equal(k.grad, got["gk"] + got["gv"])
    else:
        assert torch.equal(k.grad, got["gk"]) and torch.equal(v.grad, got["gv"])


def test_saturated_scores(dev):
    """Scores of +-80 and beyond: finite and inside the rule (the row maximum is subtracted before exp)."""
    c = O.saturated_case()
    O.check(_np(_run(dev, c)), c, "saturated")


def test_row_with_nothing_allowed(dev):
    """One sample of the batch has no valid key: uniform weights there (the f32 sum -1e9 + S is -1e9), inside the rule
    everywhere, and the gradient reaches that sample's q and k."""
    c = O.all_masked_case()
    got = _np(_run(dev, c))
    O.check(got, c, "all-masked")
    Tq = c["shape"][1]
    assert O.max_diff(got["out"][1], c["v"][1].astype(np.float64).mean(0, keepdims=True).repeat(Tq, 0)) <= 1e-6
    assert np.abs(got["gq"][1]).max() > 1e-3 and np.abs(got["gk"][1]).max() > 1e-3


def test_inference_form_writes_the_same_output(dev):
    """Without `saved` (no gradient asked for) the output has the training forward's bits."""
    c = O.case(*O.CASES[3])
    q, k, v, lens = (_dev(c[n], dev) for n in ("q", "k", "v", "lens"))
    a, saved = ops.seq_attn_fwd(q, k, v, c["H"], c["scale"], None, lens, True)
    b, none = ops.seq_attn_fwd(q, k, v, c["H"], c["scale"], None, lens, True, want_saved=False)
    assert none is None and saved.numel() == 4 * 2 * 6 * 2 * 4 and torch.equal(a, b)
    with torch.no_grad():
        assert torch.equal(ops.seq_attn(q, k, v, c["H"], c["scale"], None, lens, True), a)


# ---- 2. bits, the empty batch, errors --------------------------------------------------------
def test_empty_batch(dev):
    q, k = torch.zeros((0, 3, 16), device=dev), torch.zeros((0, 5, 16), device=dev)
    lens = torch.zeros(0, dtype=torch.int32, device=dev)
    out, saved = ops.seq_attn_fwd(q, k, k, 2, 0.5, None, lens)
    assert out.shape == (0, 3, 16) and saved.numel() == 0
    gq, gk, gv = ops.seq_attn_bwd(q, k, k, 2, 0.5, None, lens, False, saved, out)
    assert gq.shape == (0, 3, 16) and gk.shape == gv.shape == (0, 5, 16)


def test_two_runs_give_the_same_bits(dev):
    """One unit per workgroup, and 64 with a ragged last tile."""
    for args in (O.WIDE, O.TILE_CAP):
        c = O.case(*args)
        a, b = _run(dev, c), _run(dev, c)
        for name in O.OUTPUTS:
            assert torch.equal(a[name], b[name]), (args, name)


def _plans(shape, aligned=True):
    """(forward, backward) plan of a call, from the launches' own arithmetic."""
    return ops.seq_attn_plan(*shape, False, aligned), ops.seq_attn_plan(*shape, True, aligned)


TILED = [O.TILE_MIXED, O.TILE_CAP, O.TILE_CAP_POOLED, O.TILE_CLAMPED]


@pytest.mark.parametrize("args", [O.WIDE, O.CASES[11]] + TILED, ids=O.sid)
def test_sample_alone_has_the_bits_it_has_in_the_batch(dev, args):
    """Samples of a batch against their own B = 1 runs, and a slice.  In the B = 131 cases every workgroup holds one unit (one
    sample's head), so they compare grids only.  In the `TILED` cases a workgroup holds 2, 3 or 64 units, of several samples
    with their own masks (and, in one, 3 units forward and 2 backward), and the B = 1 run holds one: the first sample, a
    sample from the middle of a tile, the first sample of the last (ragged) tile in either direction, and the last sample."""
    c = O.case(*args)
    B, _, _, H, _ = c["shape"]
    fwd, bwd = _plans(c["shape"])
    assert (fwd["TB"] > 1 and bwd["TB"] > 1) == (args in TILED) and (fwd["TB"] == 1 and bwd["TB"] == 1) == (args not in TILED)
    assert all(p["TB"] == 1 for p in _plans((1,) + tuple(c["shape"][1:])))
    samples = {0, B // 2, B - 1, max(1, fwd["TB"] // 2 // H)}
    samples |= {(B * H - 1) // p["TB"] * p["TB"] // H for p in (fwd, bwd)}               # the owner of the last tile's first unit
    whole = _run(dev, c)
    for b in sorted(samples):
        one = _run(dev, O.slice_case(c, b, b + 1))
        for name in O.OUTPUTS:
            assert torch.equal(one[name], whole[name][b:b + 1]), (name, b)
    part = _run(dev, O.slice_case(c, 3, 30))
    for name in O.OUTPUTS:
        assert torch.equal(part[name], whole[name][3:30]), name


def _padded(c, hd2):
    """A one-head case with q, k, v and gout zero-padded to `hd2` columns, and the same scale."""
    B, Tq, Tk, H, hd = c["shape"]
    assert H == 1 and hd2 > hd and not c["shared"]
    out = dict(c)
    for name in ("q", "k", "v", "gout"):
        out[name] = np.concatenate([c[name], np.zeros(c[name].shape[:2] + (hd2 - hd,), np.float32)], axis=2)
    out["shape"] = (B, Tq, Tk, 1, hd2)
    return out


@pytest.mark.parametrize("widths", [(64, 128), (32, 64)], ids=str)
def test_zero_columns_leave_the_bits(dev, widths):
    """Padding every row with zero columns (same `scale`) moves the case to another chunking -- forward from 1 chunk to 2 and
    backward from 2 to 3, or backward from 1 to 2 -- and only appends fmaf(0, 0, acc) to every score's chain: out, gq, gk and gv
    keep their bits on the first columns and are 0 beyond.  This is what sees a partial sum that is carried from chunk to
    chunk in another order, or the backward re-deriving P from a chunking that is not the forward's."""
    hd, hd2 = widths
    c = O.case(2, 64, 64, 1, hd, "lens", True, False)
    wide = _padded(c, hd2)
    nch = lambda shape: tuple(p["nch"] for p in _plans(shape))
    assert (nch(c["shape"]), nch(wide["shape"])) == {(64, 128): ((1, 2), (2, 3)), (32, 64): ((1, 1), (1, 2))}[widths]
    a, b = _run(dev, c), _run(dev, wide)
    for name in O.OUTPUTS:
        assert torch.equal(b[name][..., :hd], a[name]), name
        assert bool((b[name][..., hd:] == 0).all()), name


def _off_boundary(a, dev):
    """The array as a contiguous device tensor that begins 4 bytes past a 16-byte boundary."""
    if a is None:
        return None
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    t = flat[1:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("args", [O.CHUNKED, O.U8_TILED], ids=O.sid)
def test_rows_off_a_16_byte_boundary_give_the_same_bits(dev, args):
    """hd % 4 == 0 with q, k, v and gout 4 bytes off a 16-byte boundary: the float-by-float path (`vec` 0), in two chunks and
    in tiles of two units, has the bits of the 16-byte path."""
    c = O.case(*args)
    assert c["shape"][4] % 4 == 0 and all(p["vec"] == 1 for p in _plans(c["shape"]))
    assert all(p["vec"] == 0 for p in _plans(c["shape"], aligned=False))
    want = _run(dev, c)
    q, k, v, gout = (_off_boundary(c[n], dev) for n in ("q", "k", "v", "gout"))
    key_ok, lens = _dev(c["key_ok"], dev), _dev(c["lens"], dev)
    out, saved = ops.seq_attn_fwd(q, k, v, c["H"], c["scale"], key_ok, lens, c["causal_or"])
    gq, gk, gv = ops.seq_attn_bwd(q, k, v, c["H"], c["scale"], key_ok, lens, c["causal_or"], saved, gout)
    for name, got in zip(O.OUTPUTS, (out, gq, gk, gv)):
        assert torch.equal(got, want[name]), name


def test_sample_with_nothing_allowed_inside_a_tile(dev):
    """lens[5] = 0 in the case whose tiles of two units mix samples (the units of samples 4 and 5 share one): inside the rule
    everywhere, the mean of v's rows for sample 5, and samples 4 and 6 keep the bits they have with lens[5] = 1."""
    c1, c0 = dict(O.case(*O.TILE_MIXED)), dict(O.case(*O.TILE_MIXED))
    B, Tq, Tk, H, hd = c0["shape"]
    assert _plans(c0["shape"])[0]["TB"] == 2 and (4 * H + H - 1) // 2 == (5 * H) // 2      # sample 4's last unit, 5's first
    for c, n in ((c1, 1), (c0, 0)):
        c["lens"] = c["lens"].copy()
        c["lens"][5] = n
    s = np.einsum("ihc,jhc->hij", c0["q"][5].reshape(Tq, H, hd).astype(np.float64), c0["k"][5].reshape(Tk, H, hd)) * c0["scale"]
    assert np.abs(s).max() < 32                               # -1e9 + S is -1e9 in f32: uniform weights
    got0, got1 = _run(dev, c0), _run(dev, c1)
    got = _np(got0)
    O.check(got, c0, "all-masked-in-tile")
    want = c0["v"][5].astype(np.float64).mean(0, keepdims=True).repeat(Tq, 0)
    assert O.max_diff(got["out"][5], want) <= 1e-6
    for name in O.OUTPUTS:
        for b in (4, 6):
            assert torch.equal(got0[name][b], got1[name][b]), (name, b)
    assert not torch.equal(got0["out"][5], got1["out"][5])


def test_argument_errors(dev):
    c = O.case(*O.CASES[5])                                   # Tq = 4, Tk = 9
    q, k, v = (_dev(c[n], dev) for n in ("q", "k", "v"))
    lens, key_ok = _dev(c["lens"], dev), torch.ones((3, 9), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="lr_seq_attn_fwd_f32"):                       # LR_EINVAL: both masks
        ops.seq_attn_fwd(q, k, v, 2, 1.0, key_ok, lens)
    with pytest.raises(ValueError, match="lr_seq_attn_fwd_f32"):                       # LR_EINVAL: causal_or with Tq != Tk
        ops.seq_attn_fwd(q, k, v, 2, 1.0, None, lens, True)
    out, saved = ops.seq_attn_fwd(q, k, v, 2, 1.0, None, lens)
    with pytest.raises(ValueError, match="lr_seq_attn_bwd_f32"):
        ops.seq_attn_bwd(q, k, v, 2, 1.0, key_ok, lens, False, saved, out)
    with pytest.raises(ValueError, match="lr_seq_attn_bwd_f32"):
        ops.seq_attn_bwd(q, k, v, 2, 1.0, None, lens, True, saved, out)
    with pytest.raises(ValueError, match="saved must be"):
        ops.seq_attn_bwd(q, k, v, 2, 1.0, None, lens, False, saved[:8], out)
    with pytest.raises(ValueError, match="key_ok must be"):
        ops.seq_attn_fwd(q, k, v, 2, 1.0, key_ok[:, :4].contiguous())
    with pytest.raises(TypeError):
        ops.seq_attn_fwd(q, k, v, 2, 1.0, None, lens.long())


@pytest.mark.parametrize("shape", [(1, 1, 65, 1, 8), (1, 1, 4, 1, 129)], ids=str)
def test_unsupported_shapes_leave_the_outputs_untouched(dev, shape):
    """`ValueError` from the wrappers, LR_ESHAPE from the entry points themselves, and nothing written."""
    B, Tq, Tk, H, hd = shape
    q, k = torch.zeros((B, Tq, H * hd), device=dev), torch.zeros((B, Tk, H * hd), device=dev)
    with pytest.raises(ValueError, match="unsupported sequence-attention shape"):
        ops.seq_attn(q, k, k, H, 1.0)
    with pytest.raises(ValueError, match="unsupported sequence-attention shape"):
        ops.seq_attn_fwd(q, k, k.clone(), H, 1.0)
    out, gk, gv = torch.full_like(q, 7.0), torch.full_like(k, 7.0), torch.full_like(k, 7.0)
    saved = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="lr_seq_attn_fwd_f32"):
        ops._call("lr_seq_attn_fwd_f32", q.data_ptr(), k.data_ptr(), k.data_ptr(), B, Tq, Tk, H, hd, 1.0, 0, 0, 0, out.data_ptr(),
                  saved.data_ptr(), saved.numel(), ops._stream())
    with pytest.raises(ValueError, match="lr_seq_attn_bwd_f32"):
        ops._call("lr_seq_attn_bwd_f32", q.data_ptr(), k.data_ptr(), k.data_ptr(), B, Tq, Tk, H, hd, 1.0, 0, 0, 0, saved.data_ptr(),
                  q.data_ptr(), out.data_ptr(), gk.data_ptr(), gv.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((gk == 7).all()) and bool((gv == 7).all()) and bool((saved == 7).all())


# ---- 3. the nets: kernels against the torch composition, three training steps ----------------
NU, NI, VOCAB = 40, 60, 7
# the configurations and sizes of tests/test_din_tower_models_gpu.py: (K, item_side, mode, heads, layers, pos, causal)
TFM_CONFIGS = [(16, False, "concat", 1, 1, "trainable", False), (16, True, "concat", 2, 2, "sinusoidal", True),
               (16, True, "elementwise", 4, 1, "trainable", False)]
SIM_CONFIGS = [(False, 2, 1.0, 1.0), (True, 4, 0.3, 0.8)]        # (item_side, heads, alpha, beta)
MODEL_CASES = [("tfm",) + c for c in TFM_CONFIGS] + [("sim",) + c for c in SIM_CONFIGS] + [("din_tf",)]


def _side(rng, item_side, n_sp, n_dense):
    if not item_side:   # last sparse column and last dense column are item features
        return {}
    isu = rng.integers(0, VOCAB, (NI + 1, 1)) + (n_sp - 1) * (VOCAB + 1)
    idu = rng.standard_normal((NI + 1, 1)).astype(np.float32)
    return dict(item_sparse_unique=isu, item_dense_unique=idu, item_dense_cols=[n_dense - 1])


def _sim_batch(rng, B, Lg, S, n_sp, n_dense):
    """Long windows of 0 .. Lg distinct items (no ties in the top-k search; fewer valid items than `search_topk` included) and
    short windows of 0 .. S items."""
    users, items = rng.integers(0, NU, B), rng.integers(0, NI, B)
    seqs = np.full((B, Lg + S), NI, dtype=np.int64)
    lens = np.ones((B, 2), dtype=np.int64)
    for b in range(B):
        nl, ns = rng.integers(0, Lg + 1), rng.integers(0, S + 1)
        seqs[b, :nl] = rng.permutation(NI)[:nl]
        seqs[b, Lg:Lg + ns] = rng.integers(0, NI, ns)
        lens[b] = max(nl, 1), max(ns, 1)
    sparse = rng.integers(0, VOCAB, (B, n_sp)) + np.arange(n_sp) * (VOCAB + 1)
    dense = rng.standard_normal((B, n_dense)).astype(np.float32)
    return users, items, sparse, dense, seqs, lens, rng.integers(0, 2, B).astype(np.float32)


def build_model_case(dev, case, L=6):
    """-> (make(fused_attention) -> net, batch() -> the tuple of `din_batch`)."""
    kind, cfg = case[0], case[1:]
    if kind == "tfm":
        K, item_side, mode, heads, layers, pos, causal = cfg
        rng = np.random.default_rng(8)
        n_sp, n_dense = (3, 2) if item_side else (2, 1)
        kw = _side(rng, item_side, n_sp, n_dense)
        spec = FeatSpec(NU, NI, n_sp, n_sp * (VOCAB + 1), n_dense)
        make = lambda fused: FeatTransformerNet(spec, K, (32, 16), use_bn=True, max_seq_len=L, num_heads=heads, num_tfm_layers=layers,
                                                positional_embedding=pos, use_causal_mask=causal, feat_agg_mode=mode, lr=1e-2,
                                                device=dev, dense_adam=True, fused_attention=fused, **kw)
        return make, lambda: din_batch(rng, 48, NU, NI, L, n_sp, VOCAB, n_dense)
    if kind == "sim":
        item_side, heads, alpha, beta = cfg
        rng = np.random.default_rng(13)
        n_sp, n_dense = (3, 2) if item_side else (2, 1)
        kw = _side(rng, item_side, n_sp, n_dense)
        spec = FeatSpec(NU, NI, n_sp, n_sp * (VOCAB + 1), n_dense)
        make = lambda fused: FeatSIMNet(spec, 16, (32, 16), use_bn=True, alpha=alpha, beta=beta, search_topk=5, long_max_len=9,
                                        short_max_len=4, num_heads=heads, lr=1e-2, device=dev, dense_adam=True,
                                        fused_attention=fused, **kw)
        return make, lambda: _sim_batch(rng, 48, 9, 4, n_sp, n_dense)
    rng = np.random.default_rng(0)
    spec = FeatSpec(NU, NI, 2, 2 * (VOCAB + 1), 1)
    make = lambda fused: FeatDINNet(spec, 16, (32, 16), use_bn=True, max_seq_len=L, lr=1e-2, device=dev, dense_adam=True,
                                    use_tf_attention=True, fused_attention=fused)
    return make, lambda: din_batch(rng, 48, NU, NI, L, 2, VOCAB, 1)


def _case_id(case):
    return "-".join(str(x) for x in case)


@pytest.mark.parametrize("case", MODEL_CASES, ids=_case_id)
def test_training_steps(dev, case):
    """Two nets from one seed, one on the kernels and one composed from torch ops under autograd: the loss to 1e-5, every
    table, moment and dense parameter to rtol 1e-4 / atol 5e-5 over three steps, then the inference forward (the figures of
    tests/test_autoint_gpu.py::test_training_steps)."""
    make, batch = build_model_case(dev, case)
    fused, composed = make(True), make(False)
    assert fused.fused_attention and not composed.fused_attention
    assert torch.equal(fused.P.flat, composed.P.flat) and torch.equal(fused.tables.embed, composed.tables.embed)
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-4, atol=5e-5, msg=lambda m: f"{what}: {m}")
    for step in range(1, 4):
        b = batch()
        want = float(composed.train_step(labels=b[-1], **din_call(b)))
        got = float(fused.train_step(labels=b[-1], **din_call(b)))
        print(f"SEQATTN-FIGURE step {_case_id(case)} {step}: loss {got:.8f} composed {want:.8f}")
        assert abs(got - want) < 1e-5, (step, got, want)
        for k, ref in composed.P.params.items():
            close(fused.P[k], ref, f"{k} after step {step}")
        for name in ("m", "v"):
            close(getattr(fused.P, name), getattr(composed.P, name), f"dense moment {name} after step {step}")
            close(getattr(fused.tables, name), getattr(composed.tables, name), f"table moment {name} after step {step}")
        close(fused.tables.embed, composed.tables.embed, f"tables after step {step}")
    b = batch()
    close(fused.forward(**din_call(b)), composed.forward(**din_call(b)), "inference forward")


# ---- 4. routing ------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of `ops.seq_attn`."""
    seen, real = [], ops.seq_attn

    def counting(q, k, v, *args, **kwargs):
        seen.append((tuple(q.shape), tuple(k.shape), v is k))
        return real(q, k, v, *args, **kwargs)

    monkeypatch.setattr(ops, "seq_attn", counting)
    return seen


def test_routing(dev, calls):
    """One Transformer forward: a call per layer and one for the read-out; SIM: the exact search unit and the short window; DIN
    with `use_tf_attention`: one; none with `fused_attention=False`."""
    for case, n in ((MODEL_CASES[1], 3), (MODEL_CASES[0], 2), (MODEL_CASES[3], 2), (MODEL_CASES[5], 1)):
        make, batch = build_model_case(dev, case)
        b = batch()
        del calls[:]
        make(True).forward(**din_call(b))
        assert len(calls) == n, (case, calls)
        if case[0] == "tfm":
            assert calls[-1][0][1] == 1 and calls[-1][2] and not calls[0][2]          # the read-out is the pooling form
        if case[0] == "sim":
            assert calls[0][:2] == ((48, 1, 16), (48, 5, 16)) and calls[1][1] == (48, 4, 16) and calls[1][2]
        del calls[:]
        net = make(False)
        net.forward(**din_call(b))
        net.train_step(labels=b[-1], **din_call(b))
        assert not calls, case


def test_window_past_the_kernels_takes_the_composition(dev, calls):
    """max_seq_len = 65: no kernel call in a forward or a training step, and the composed net's results: the same op
    sequence, so the same logits and loss."""
    make, _ = build_model_case(dev, MODEL_CASES[1], L=65)
    rng = np.random.default_rng(2)
    b = din_batch(rng, 16, NU, NI, 65, 3, VOCAB, 2)
    fused, composed = make(True), make(False)
    assert fused.fused_attention and not ops.seq_attn_supported(65, 65, 2, 32)
    assert torch.equal(fused.forward(**din_call(b)), composed.forward(**din_call(b)))
    la, lb = fused.train_step(labels=b[-1], **din_call(b)), composed.train_step(labels=b[-1], **din_call(b))
    assert not calls and torch.equal(la, lb)
    torch.testing.assert_close(fused.P.flat, composed.P.flat, rtol=1e-4, atol=5e-5)
