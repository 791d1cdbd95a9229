"""The DIN attention oracle (tests/din_oracle.py) against `oracle/ops_np.din_attention` and plain torch autograd, its chunked
form against the unchunked one, the properties its case builders promise, and the f32 oracle inside every tolerance of
tests/test_din_kernels_gpu.py on every case of that file (the case list is the oracle module's).  CPU only."""
import numpy as np
import pytest
import torch

from librecommender_amd import ops
from oracle import ops_np
from . import din_oracle as D


def plain_autograd(c):
    """fp64 autograd of the reference's arithmetic in one piece (no chunks, no edge semantics: for ordinary cases)."""
    d = torch.float64
    q, keys, valid = D.gathered(c)
    q = torch.tensor(q, dtype=d, requires_grad=True)
    keys = torch.tensor(np.where(valid[:, :, None], keys, 0), dtype=d, requires_grad=True)
    P = [torch.tensor(c[k], dtype=d, requires_grad=True) for k in ("W1", "b1", "W2", "b2")]
    B, L, K = keys.shape
    qt = q[:, None, :].expand(-1, L, -1)
    h = torch.sigmoid(torch.cat([qt, keys, qt - keys, qt * keys], dim=2) @ P[0] + P[1])
    s = ((h @ P[2]).reshape(B, L) + P[3]) / np.sqrt(K)
    s = torch.where(torch.from_numpy(valid), s, torch.full_like(s, -(2.0 ** 32) + 1))
    a = torch.softmax(s, dim=1)
    out = (a[:, None, :] @ keys).reshape(B, K)
    out.backward(torch.tensor(c["gout"], dtype=d))
    return (out.detach().numpy(), a.detach().numpy(), q.grad.numpy(), keys.grad.numpy(), *[p.grad.numpy() for p in P])


def ordinary_case():
    rng = np.random.default_rng(0)
    return D.case(700, 21, 32, seed=9, lens=rng.integers(1, 22, 700), name="ordinary")


def test_f64_oracle_is_the_reference_arithmetic():
    c = ordinary_case()
    got = D.backward_oracle(c, "f64")
    q, keys, valid = D.gathered(c)
    keys = np.where(valid[:, :, None], keys, 0)
    o_np, a_np = ops_np.din_attention(q.astype(np.float64), keys.astype(np.float64), c["lens"], *(c[k].astype(np.float64)
                                                                                                 for k in ("W1", "b1", "W2", "b2")))
    np.testing.assert_allclose(got[0], o_np, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[1], a_np, rtol=1e-9, atol=1e-9)
    for g, w, name in zip(got, plain_autograd(c), D.OUTPUTS):
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-9, err_msg=name)
    fo = D.forward_oracle(c, "f64")
    np.testing.assert_array_equal(fo[0], got[0])
    np.testing.assert_array_equal(fo[1], got[1])


@pytest.mark.parametrize("name", ["ordinary", "edge-L17-K16", "bad-L18-K16"])
def test_chunked_oracle_equals_unchunked(name):
    c = ordinary_case() if name == "ordinary" else D.get_case(name)
    whole = D.backward_oracle(c, "f64", chunk=10 ** 9)
    for chunk in (512, 37):
        for g, w, out in zip(D.backward_oracle(c, "f64", chunk=chunk), whole, D.OUTPUTS):
            np.testing.assert_allclose(g, w, rtol=1e-11, atol=1e-11, err_msg=f"{out} chunk {chunk}")


def test_edge_semantics_of_the_oracle():
    c = D.get_case("bad-L18-K16")
    o = D.oracles(c)["f64"]
    n = D.clamp_lens(c["lens"], c["L"])
    zero = n == 0
    assert zero.any() and not o["out"][zero].any() and not o["attn"][zero].any()
    assert not o["gq"][zero].any() and not o["gkey"][zero].any()            # len == 0: no gradient from that sample
    assert not o["gkey"][~D.valid_steps(c["lens"], c["L"])].any()
    for b, l in c["bad"]["seq"]:                                             # a bad key still has a weight and a gradient value
        assert o["attn"][b, l] > 0 and np.abs(o["gkey"][b, l]).max() > 0
    for b in c["bad"]["item"]:
        assert np.abs(o["gq"][b]).max() > 0
    # the same mathematics as a zero row under a valid id, and as the clamped lengths
    for other in (D.remapped(c), D.clamped(c)):
        for g, w in zip(D.backward_oracle(other, "f64"), D.backward_oracle(c, "f64")):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_builder_keeps_its_promises(name):
    c = D.get_case(name)
    B, L, V = c["B"], c["L"], c["V"]
    assert np.isnan(c["table"][0]).all() and np.isnan(c["table"][V - 1]).all() and np.isfinite(c["table"][1:V - 1]).all()
    valid = D.valid_steps(c["lens"], L)
    assert (c["seq"][~valid] == V - 1).all()
    inside = (c["seq"] >= 1) & (c["seq"] <= V - 2)
    bad_seq = {tuple(x) for x in c["bad"].get("seq", [])}
    assert {tuple(x) for x in np.argwhere(valid & ~inside)} == bad_seq       # bad ids at the promised places, valid steps only
    ok_item = (c["item"] >= 1) & (c["item"] <= V - 2)
    assert sorted(np.flatnonzero(~ok_item)) == sorted(c["bad"].get("item", []))
    for b, l in bad_seq:
        assert not 0 <= c["seq"][b, l] < V
    if name.startswith("long"):
        assert {0, 1, 2048, 2049, L, L + 3}.issubset(set(c["lens"].tolist()))
    elif B >= 45:
        assert set(D.len_members(L)).issubset(set(c["lens"].tolist())), "every edge length is in every batch"
        for x in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49):
            assert (x in c["lens"]) == (x <= L)
        assert {L - 1, L, L + 3, -2}.issubset(set(c["lens"].tolist()))
    assert len(D.len_cycle(L)) % 2 == 1                                      # coprime to 2,048
    if B > D.STRIDE:
        succ = D.successions(c["lens"], L)
        assert {("full", "zero"), ("zero", "full"), ("one", "gt16")}.issubset(succ)
        assert B > 2 * D.STRIDE                                               # some waves take a third sample
    if name.startswith("bad"):
        (lo, hi), seqs = c["bad"]["item"], c["bad"]["seq"]
        assert lo < D.STRIDE <= hi and c["item"][lo] == -1 and c["item"][hi] == V + 5
        assert [l for _, l in seqs] == [0, 16, 17] and all(b >= D.STRIDE for b, _ in seqs)
        assert len({lo, hi, *[b for b, _ in seqs]}) == 5


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_f32_oracle_is_inside_every_tolerance(name):
    c = D.get_case(name)
    D.check({k: v.astype(np.float32) for k, v in D.oracles(c)["f32"].items()}, c, f"f32-oracle {name}")


@pytest.mark.parametrize("K", [16, 128])
def test_sharp_case_spreads_its_scores(K):
    c = D.get_case(f"sharp-L33-K{K}")
    s = D.scores64(c)
    n = D.clamp_lens(c["lens"], c["L"])
    span = np.array([np.nanmax(r) - np.nanmin(r) if k else 0.0 for r, k in zip(s, n)])
    assert span.max() > 100 and (span > 50).sum() >= 10
    up, down = D.tile_steps(c)                   # exp() underflows on both sides of a tile boundary, in both directions
    assert up >= 1 and down >= 1
    o = D.oracles(c)["f64"]
    assert all(np.isfinite(v).all() for v in o.values())
    for b in c["ties"]:
        assert len(set(c["seq"][b, :n[b]].tolist())) == 1 and n[b] >= 2
        np.testing.assert_allclose(o["attn"][b, :n[b]], 1.0 / n[b], rtol=1e-12)


def test_limit_shapes_follow_the_library():
    """The supported region is one statement (`lr_din_attn_path`): the figures of its LDS formulas, and the f32 oracle on the
    cases the GPU file runs at those limits."""
    assert [ops.din_path(K, 2048) for K in (16, 32, 64, 128, 24)] == [2, 2, 2, 2, 0]
    assert ops.din_path(128, 2049) == 1 and ops.din_path(128, 2049, backward=True) == 0
    assert D.max_len(ops.din_path, 64, backward=True) == 6108 and D.max_len(ops.din_path, 64, backward=False) == 9216
    assert D.max_len(ops.din_path, 128, backward=False) == 8192 and D.max_len(ops.din_path, 128, backward=True) == 2048
    lib = ops._lib.load()
    assert lib.lr_din_attn_ws_bytes(2, 2049, 128, 16) == 0 and lib.lr_din_attn_ws_bytes(2, 2049, 64, 16) > 0
    assert lib.lr_din_attn_ws_bytes(2, 6108, 64, 16) > 0 and lib.lr_din_attn_ws_bytes(2, 6109, 64, 16) == 0
    for K, L in ((128, 2049), (64, 6108), (64, 9216)):
        c = D.limit_case(K, L)
        D.check({k: v.astype(np.float32) for k, v in D.oracles(c)["f32"].items()}, c, f"f32-oracle {c['name']}")
