"""The DIN attention kernels (csrc/din_attention.hip, csrc/din_mfma.hpp) where they branch, against the fp64 oracle of
tests/din_oracle.py (`-m gpu`): lengths at every edge of the 16-key tiles, waves that take a second and a third sample (the
forward's cross-sample prefetch), ids outside the table, sharp logits and ties, the limits of the supported (K, L) region, and
— last — the shuffle kernels that sequences beyond 2,048 keys run on.  Cases, properties and tolerances are the oracle
module's (tests/test_din_cpu.py runs the f32 oracle through the same checks)."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops

from . import din_oracle as D

pytestmark = pytest.mark.gpu

ARGS = ("table", "item", "seq", "lens", "W1", "b1", "W2", "b2")
GRADS = ("gq", "gkey", "gW1", "gb1", "gW2", "gb2")
SENTINEL = 123.0


def dev_args(c, dev):
    return [torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ARGS]


def as_np(names, tensors):
    return {k: v.detach().cpu().numpy() for k, v in zip(names, tensors)}


def run(c, dev, form="plain"):
    """Forward + backward of a case in one of the forms: plain (recomputing), order (plain, balanced walk), hid, hid+order.
    -> dict of the eight outputs as device tensors, plus `hid` / `order` where the form has them."""
    args = dev_args(c, dev)
    B, L, K = c["B"], c["L"], c["K"]
    with_hid, with_order = "hid" in form, "order" in form
    hid = torch.full((ops.din_hid_floats(B, L, K, with_order),), SENTINEL, device=dev) if with_hid else None
    order = torch.full((B,), -1, dtype=torch.int32, device=dev) if with_order else None
    out, attn = ops.din_attn_pool_fwd(*args, hid=hid, order_out=order)
    gout = torch.from_numpy(c["gout"]).to(dev)
    grads = ops.din_attn_pool_bwd(*args, attn, gout, hid=hid, order=order)
    r = dict(zip(D.OUTPUTS, (out, attn, *grads)))
    r["hid"], r["order"] = hid, order
    return r


def run_dense(c, dev):
    q, keys, _ = D.gathered(c)
    q, keys = torch.from_numpy(q).to(dev), torch.from_numpy(keys).to(dev)
    args = dev_args(c, dev)
    out, attn = ops.din_attn_dense_fwd(q, keys, *args[3:])
    grads = ops.din_attn_dense_bwd(q, keys, *args[3:], attn, torch.from_numpy(c["gout"]).to(dev))
    return dict(zip(D.OUTPUTS, (out, attn, *grads)))


def check(r, c, what):
    D.check({k: r[k].cpu().numpy() for k in D.OUTPUTS if k in r}, c, what)


def same_bits(a, b, names, what):
    for k in names:
        assert torch.equal(a[k].view(-1), b[k].view(-1)), f"{what}: {k} differs"


def check_hid(r, c):
    """Positions l >= len keep the sentinel; the others hold h = sigmoid(z) in (0, 1)."""
    B, L = c["B"], c["L"]
    h = r["hid"][:B * L * 16].view(B, L, 16).cpu().numpy()
    pad = ~D.valid_steps(c["lens"], L)
    assert (h[pad] == SENTINEL).all() and ((h[~pad] > 0) & (h[~pad] < 1)).all()


# ---- 1. tile edges, one sample per wave ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 32, 64, 128])
@pytest.mark.parametrize("L", [1, 15, 16, 17, 32, 33, 49])
def test_tile_edges(dev, L, K):
    c = D.get_case(f"edge-L{L}-K{K}")
    assert c["B"] == 45 and ops.din_path(K, L) == 2
    plain = run(c, dev)
    check(plain, c, f"{c['name']} plain")
    saved = run(c, dev, "hid")
    check(saved, c, f"{c['name']} hid")
    same_bits(plain, saved, ("out", "attn"), "keeping h changes nothing in the forward")
    check_hid(saved, c)


# ---- 2. waves that take two and three samples ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trips-L18-K16", "trips-L18-K32", "trips-L18-K64", "trips-L18-K128", "trips-L50-K64"])
def test_waves_take_two_and_three_samples(dev, name):
    c = D.get_case(name)
    assert c["B"] == 4133 and ops.din_path(c["K"], c["L"], backward=True) == 2
    r = {form: run(c, dev, form) for form in ("plain", "order", "hid", "hid+order")}
    for form in ("plain", "hid", "hid+order"):
        check(r[form], c, f"{name} {form}")
    check_hid(r["hid"], c)
    check_hid(r["hid+order"], c)
    for form in ("order", "hid", "hid+order"):
        same_bits(r["plain"], r[form], ("out", "attn"), f"forward of {form}")
    # each sample is computed by one wave from its own rows: the walk order does not change its bits
    same_bits(r["plain"], r["order"], ("gq", "gkey"), "identity / balanced order")
    same_bits(r["hid"], r["hid+order"], ("gq", "gkey"), "identity / balanced order, saved h")
    n = D.clamp_lens(c["lens"], c["L"])
    tiles = np.where(n == 0, 1, (n + 15) // 16)
    np.testing.assert_array_equal(r["order"]["order"].cpu().numpy(), np.argsort(-tiles, kind="stable").astype(np.int32))
    assert torch.equal(r["order"]["order"], r["hid+order"]["order"])
    same_bits(r["plain"], run_dense(c, dev), D.OUTPUTS, "dense rows against the gather form")
    for form in ("plain", "hid+order"):
        same_bits(r[form], run(c, dev, form), D.OUTPUTS, f"two runs, {form}")


# ---- 3. ids outside the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 128])
def test_bad_ids(dev, K):
    c = D.get_case(f"bad-L18-K{K}")
    clean = D.get_case(f"trips-L18-K{K}")
    bad = c["bad"]
    assert len(bad["item"]) == 2 and [l for _, l in bad["seq"]] == [0, 16, 17]
    got = run(c, dev)
    check(got, c, f"{c['name']} plain")
    check(run(c, dev, "hid+order"), c, f"{c['name']} hid+order")
    # a bad id is a row of zeros: the same bits as a zero row of the table under a valid id, at every position
    same_bits(got, run(D.remapped(c), dev), D.OUTPUTS, "bad ids against a zero row")
    same_bits(run(c, dev, "hid+order"), run(D.remapped(c), dev, "hid+order"), D.OUTPUTS, "bad ids against a zero row, saved h")
    # and nobody else's business: every other sample keeps the bits of the clean run
    ref = run(clean, dev)
    others = np.ones(c["B"], bool)
    others[bad["item"] + [b for b, _ in bad["seq"]]] = False
    keep = torch.from_numpy(others).to(dev)
    for k in ("out", "attn", "gq", "gkey"):
        assert torch.equal(got[k][keep], ref[k][keep]), f"{k} of an untouched sample changed"
        assert not torch.equal(got[k][~keep], ref[k][~keep])
    # lengths outside [0, L] are their clamped values
    assert (c["lens"] < 0).any() and (c["lens"] > c["L"]).any()
    same_bits(got, run(D.clamped(c), dev), D.OUTPUTS, "clamped lengths")


# ---- 6. sharp logits and ties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 128])
def test_sharp_logits_and_ties(dev, K):
    """Scores that span 160: exp() underflows in the online softmax's rescale on both sides of a tile boundary.
    This case found the forward forming its denominator from UNROUNDED scores (the product with 1 / sqrt(K) contracted into
    the subtraction of the maximum) while `attn` came from the rounded ones: at K = 128 the rows of attn missed 1 by up to
    7.2e-6 and gq stood at 4.046e-03 against a bound of 3.639e-03 (measured on an MI355X); with the product rounded
    (`din_mul_rounded`) the rows sum to 1 within 1.5e-7 and gq stands at 2.308e-04."""
    c = D.get_case(f"sharp-L33-K{K}")
    assert c["B"] == 45 and c["L"] == 33
    for form in ("plain", "hid"):
        r = run(c, dev, form)
        check(r, c, f"{c['name']} {form}")
        attn = r["attn"].cpu().numpy()
        n = D.clamp_lens(c["lens"], c["L"])
        for b in c["ties"]:                              # all valid keys equal: uniform attention
            np.testing.assert_allclose(attn[b, :n[b]], 1.0 / n[b], rtol=1e-5, atol=1e-6)


# ---- 5. the supported region is one statement --------------------------------------------------------------------------
def _refused(c, dev, backward, K, L):
    """The call raises a ValueError that names the shape, before anything is launched: the output buffers keep a sentinel."""
    args = dev_args(c, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    B = c["B"]
    if not backward:
        out, attn = torch.full((B, K), SENTINEL, **f32), torch.full((B, L), SENTINEL, **f32)
        with pytest.raises(ValueError, match=rf"K = {K}, L = {L}\b"):
            ops.din_attn_pool_fwd(*args, out=out, attn=attn)
        bufs = (out, attn)
    else:
        attn = torch.full((B, L), 1.0 / L, **f32)
        gq, gkey = torch.full((B, K), SENTINEL, **f32), torch.full((B, L, K), SENTINEL, **f32)
        pout = tuple(torch.full_like(a, SENTINEL) for a in args[4:])
        with pytest.raises(ValueError, match=rf"K = {K}, L = {L}\b"):
            ops.din_attn_pool_bwd(*args, attn, torch.from_numpy(c["gout"]).to(dev), gq_out=gq, gkey_out=gkey, param_out=pout)
        q, keys, _ = D.gathered(c)
        with pytest.raises(ValueError, match=rf"K = {K}, L = {L}\b"):
            ops.din_attn_dense_bwd(torch.from_numpy(q).to(dev), torch.from_numpy(keys).to(dev), *args[3:], attn,
                                   torch.from_numpy(c["gout"]).to(dev))
        bufs = (gq, gkey, *pout)
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)


def test_forward_without_a_backward_is_refused_in_python(dev):
    K, L = 128, 2049
    assert ops.din_path(K, L) == 1 and ops.din_path(K, L, backward=True) == 0
    assert ops._lib.load().lr_din_attn_ws_bytes(2, L, K, 16) == 0
    c = D.limit_case(K, L)
    args = dev_args(c, dev)
    out, attn = ops.din_attn_pool_fwd(*args)
    check(dict(out=out, attn=attn), c, f"{c['name']} forward")
    _refused(c, dev, True, K, L)


def test_longest_sequences_of_each_dispatcher(dev):
    K = 64
    Lb, Lf = D.max_len(ops.din_path, K, backward=True), D.max_len(ops.din_path, K, backward=False)
    assert (Lb, Lf) == (6108, 9216)                      # the figures of the LDS formulas (160 KB a workgroup)
    c = D.limit_case(K, Lb)
    check(run(c, dev), c, f"{c['name']} both")
    _refused(D.limit_case(K, Lb + 1), dev, True, K, Lb + 1)
    c = D.limit_case(K, Lf)
    out, attn = ops.din_attn_pool_fwd(*dev_args(c, dev))
    check(dict(out=out, attn=attn), c, f"{c['name']} forward")
    _refused(c, dev, True, K, Lf)
    _refused(D.limit_case(K, Lf + 1), dev, False, K, Lf + 1)


# ---- 4. the shuffle kernels: sequences beyond 2,048 keys (last in the file) -------------------------------------------
@pytest.mark.parametrize("K", [16, 32, 64])
@pytest.mark.parametrize("L", [2049, 2100])
def test_shuffle_kernels(dev, L, K):
    c = D.get_case(f"long-L{L}-K{K}")
    assert c["B"] == 9 and ops.din_path(K, L) == 1 and ops.din_path(K, L, backward=True) == 1
    got = run(c, dev)
    check(got, c, f"{c['name']} gather")
    dense = run_dense(c, dev)
    check(dense, c, f"{c['name']} dense")
    same_bits(got, run(c, dev), D.OUTPUTS, "two runs")
    same_bits(dense, run_dense(c, dev), D.OUTPUTS, "two runs, dense")
    # the saved activations and the balanced order belong to the MFMA kernels: refused before anything is launched
    args = dev_args(c, dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out, attn = torch.full((9, K), SENTINEL, **f32), torch.full((9, L), SENTINEL, **f32)
    hid = torch.full((ops.din_hid_floats(9, L, K),), SENTINEL, **f32)
    order = torch.full((9,), -1, dtype=torch.int32, device=dev)
    gq, gkey = torch.full((9, K), SENTINEL, **f32), torch.full((9, L, K), SENTINEL, **f32)
    gout = torch.from_numpy(c["gout"]).to(dev)
    for kw in (dict(hid=hid), dict(order_out=order), dict(hid=hid, order_out=order)):
        with pytest.raises(ValueError):
            ops.din_attn_pool_fwd(*args, out=out, attn=attn, **kw)
    for kw in (dict(hid=hid), dict(order=order), dict(hid=hid, order=order)):
        with pytest.raises(ValueError):
            ops.din_attn_pool_bwd(*args, got["attn"], gout, gq_out=gq, gkey_out=gkey, **kw)
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in (out, attn, hid, gq, gkey)) and bool((order == -1).all())
