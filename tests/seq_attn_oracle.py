"""CPU oracle of the sequence-attention core (csrc/seq_attn.hip, `ops.seq_attn`), numpy, written from the formulas of
include/libreco_hip.h.

The arithmetic is the reference's: `libreco/layers/attention.py:5-25` (`tf_attention`: keras `Attention(use_scale=False)`
with a value mask, the keys are the values), `:67-126` (the Keras `MultiHeadAttention` branch: scores of the scaled query,
`_masked_softmax`) and `libreco/algorithms/transformer.py:281-328` (the sequence mask ORed with the causal one).

  forward / backward   "f64" or "f32" arithmetic; the backward is hand-derived (tests/test_seq_attn_cpu.py pins it to torch
                       autograd).  In BOTH variants a masked score is first rounded to f32 and -1e9 is added in f32, because
                       that rounding is the reference's semantics (its graph is f32): a row with nothing allowed is the softmax
                       of the rounded values, uniform while |S| < 32 (the f32 spacing at 1e9 is 64).
  case, saturated_case, all_masked_case   the seeded inputs shared by the CPU, the GPU and the guarded file
  check                the tolerance they share: `delta_bound` of tests/wavenet_oracle.py with 2 stages (scores -> output)
"""
from __future__ import annotations

import functools

import numpy as np

from .wavenet_oracle import delta_bound, max_diff

F32 = np.float32
NEG = F32(-1e9)
OUTPUTS = ("out", "gq", "gk", "gv")


def _dt(variant):
    return np.float64 if variant == "f64" else F32


def allowed(B, Tq, Tk, key_ok=None, lens=None, causal_or=False):
    """[B, Tq, Tk] bool: key_ok(b, j) || (causal_or && j <= i); `key_ok` [B, Tk] any pattern, or `lens` [B] (j < lens[b]),
    or neither: every key valid."""
    if key_ok is not None:
        ok = np.asarray(key_ok).astype(bool)
    elif lens is not None:
        ok = np.arange(Tk)[None, :] < np.asarray(lens)[:, None]
    else:
        ok = np.ones((B, Tk), dtype=bool)
    a = np.broadcast_to(ok[:, None, :], (B, Tq, Tk))
    if causal_or:
        assert Tq == Tk
        a = a | np.tril(np.ones((Tq, Tk), dtype=bool))[None]
    return a


def _heads(x, H, dt):
    B, T, M = x.shape
    return x.astype(dt).reshape(B, T, H, M // H).transpose(0, 2, 1, 3)


def forward(q, k, v, H, scale, key_ok=None, lens=None, causal_or=False, variant="f64"):
    """q [B, Tq, M], k, v [B, Tk, M] -> (out [B, Tq, M], P [B, H, Tq, Tk])."""
    dt = _dt(variant)
    B, Tq, M = q.shape
    Tk = k.shape[1]
    qh, kh, vh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt)
    s = (qh * dt(scale)) @ kh.transpose(0, 1, 3, 2)
    ok = allowed(B, Tq, Tk, key_ok, lens, causal_or)[:, None]
    s = np.where(ok, s, (s.astype(F32) + NEG).astype(dt))                  # the f32 addition, in both variants
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    return (P @ vh).transpose(0, 2, 1, 3).reshape(B, Tq, M), P


def backward(q, k, v, H, scale, P, gout, variant="f64"):
    """Hand-derived: gv = P^T gO, dP = gO v^T, dS = P (dP - rowsum(dP P)), gq = (dS k) scale, gk = dS^T (q scale).  The mask
    is an added constant: it does not appear.  -> (gq, gk, gv); with the keys as values the key gradient is gk + gv."""
    dt = _dt(variant)
    B, Tq, M = q.shape
    Tk = k.shape[1]
    qh, kh, vh, gh = _heads(q, H, dt), _heads(k, H, dt), _heads(v, H, dt), _heads(gout, H, dt)
    P = P.astype(dt)
    gv = P.transpose(0, 1, 3, 2) @ gh
    dP = gh @ vh.transpose(0, 1, 3, 2)
    dS = P * (dP - (dP * P).sum(-1, keepdims=True))
    gq = (dS @ kh) * dt(scale)
    gk = dS.transpose(0, 1, 3, 2) @ (qh * dt(scale))
    back = lambda x, T: x.transpose(0, 2, 1, 3).reshape(B, T, M)
    return back(gq, Tq), back(gk, Tk), back(gv, Tk)


def run(c, variant):
    """{out, gq, gk, gv} of a case in one arithmetic."""
    out, P = forward(c["q"], c["k"], c["v"], c["H"], c["scale"], c["key_ok"], c["lens"], c["causal_or"], variant)
    gq, gk, gv = backward(c["q"], c["k"], c["v"], c["H"], c["scale"], P, c["gout"], variant)
    return dict(out=out, gq=gq, gk=gk, gv=gv)


# ---- seeded cases ----------------------------------------------------------------------------------------------------
# (B, Tq, Tk, H, hd, mask, causal_or, shared): mask is None, "lens" or "u8"; `shared`: v is k and scale 1 (the pooling form),
# otherwise scale 1 / sqrt(hd)
CASES = [
    (3, 1, 1, 1, 1, "lens", False, False),           # the smallest shape
    (5, 1, 7, 1, 16, "lens", False, True),           # pooled, v is k, lens include 1 and 7
    (4, 6, 6, 2, 8, "lens", False, False),
    (4, 6, 6, 2, 8, "lens", True, False),            # lens = 1 (the causal part alone admits keys) and lens = 6
    (3, 1, 5, 4, 4, "u8", False, False),             # a mask that is no prefix
    (3, 4, 9, 2, 8, "lens", False, False),           # Tq != Tk
    (2, 50, 50, 1, 33, "lens", False, False),        # an odd head width
    (2, 64, 64, 1, 5, "lens", True, False),          # the top of the T range
    (1, 9, 9, 1, 128, "lens", False, False),         # the top of the hd range
    (2, 3, 3, 8, 32, "lens", False, False),          # M = 256
    (131, 10, 10, 1, 32, "lens", False, False),      # a batch that is no multiple of any tile
    (131, 1, 10, 1, 32, "lens", False, True),        # the same for the pooling form
    (6, 5, 5, 2, 8, None, False, False),             # no mask at all
    # Appended (CASES[3], [5], [10] and [11] are used by index): the launch plans past one unit per workgroup and one chunk per
    # head.  tests/test_seq_attn_cpu.py pins the plan of each (`PLANS`) and asks the union of `plan_class` for every branch.
    (345, 3, 3, 3, 4, "lens", False, False),         # TB 2: tiles that mix two samples (H odd), a last tile of one unit
    (345, 4, 9, 3, 8, "u8", False, False),           # TB 2, G 2: Tq != Tk, a per-sample u8 mask inside a tile
    (345, 6, 6, 3, 8, "lens", True, False),          # TB 2: causal OR lens inside a tile
    (4099, 5, 5, 8, 4, "lens", False, False),        # TB 64 (the cap), a last tile of 24 units
    (4099, 1, 7, 8, 4, "lens", False, True),         # TB 64, the pooling form: the key chunk serves as the values
    (1537, 40, 40, 1, 32, "lens", False, False),     # the LDS clamp: TB 3 forward, 2 backward; G 8
    (1300, 1, 20, 1, 16, "lens", False, True),       # TB 2, G 4, the pooling form
    (3, 20, 20, 1, 8, "lens", False, False),         # G 4 with Tq > 1
    (2, 64, 64, 1, 64, "lens", True, False),         # one chunk forward, two of 32 backward
    (2, 64, 64, 1, 128, "lens", False, False),       # two chunks of 64 forward; 44, 44, 40 backward
    (2, 64, 64, 1, 99, "lens", False, False),        # the scalar path, chunks of 52 and 47
    (2, 64, 64, 1, 61, "lens", False, False),        # scalar, chunked only backward: 32 and 29
    (1, 64, 64, 2, 128, "u8", False, True),          # v is k with more than one chunk (no reuse), the second head at M = 256
    (2, 63, 61, 1, 128, "lens", False, False),       # an unpaired row in `sa_apply`, a clamped key tile in `sa_dots`
]
WIDE = CASES[10]
TILE_MIXED, TILE_CAP, TILE_CAP_POOLED, TILE_CLAMPED = CASES[13], CASES[16], CASES[17], CASES[18]
U8_TILED, CHUNKED = CASES[14], CASES[22]


def sid(c):
    return "x".join("-" if x is None else str(int(x)) if isinstance(x, bool) else str(x) for x in c)


def plan_class(args):
    """The branches of csrc/seq_attn.hip that a case of `CASES` runs, from the launches' own plan (`ops.seq_attn_plan`, a
    host query), as a set of names.  More than one unit per workgroup together with more than one chunk cannot occur: a unit
    that needs two chunks takes more than half the LDS budget, so no second unit fits beside it."""
    from librecommender_amd import ops

    B, Tq, Tk, H, hd, _, _, shared = args
    fwd, bwd = ops.seq_attn_plan(B, Tq, Tk, H, hd, False), ops.seq_attn_plan(B, Tq, Tk, H, hd, True)
    out = {f"G={fwd['G']}"}
    for p in (fwd, bwd):
        out.add("TB=1" if p["TB"] == 1 else "TB=64" if p["TB"] == 64 else "1<TB<64")
        out.add(f"nch={p['nch']}")
        if (B * H) % p["TB"]:
            out.add("ragged last tile")
        if p["nch"] > 1 and (hd - (p["nch"] - 1) * p["CW"]) % 4:
            out.add("last chunk cw%4!=0")
        if p["nch"] > 1 and shared:
            out.add("shared, nch>1")
    if fwd["TB"] != bwd["TB"]:
        out.add("TB fwd!=bwd")
    if fwd["nch"] != bwd["nch"]:
        out.add("nch fwd!=bwd")
    return out


@functools.lru_cache(maxsize=None)
def _case(B, Tq, Tk, H, hd, mask, causal_or, shared, seed, mul):
    rng = np.random.default_rng([seed, B, Tq, Tk, H, hd])
    M = H * hd
    q = (rng.standard_normal((B, Tq, M)) * mul).astype(F32)
    k = (rng.standard_normal((B, Tk, M)) * mul).astype(F32)
    v = k if shared else (rng.standard_normal((B, Tk, M)) * mul).astype(F32)
    key_ok = lens = None
    if mask == "lens":
        lens = rng.integers(1, Tk + 1, B).astype(np.int32)
        lens[0] = 1
        lens[-1] = Tk
    elif mask == "u8":
        key_ok = (rng.random((B, Tk)) < 0.5).astype(np.uint8)
        key_ok[:, -1] = 1                              # every row keeps a key: the last one, so no pattern is a prefix ...
        key_ok[:, 0] = 0                               # ... because the first key is never valid
    scale = 1.0 if shared else 1.0 / np.sqrt(hd)
    return dict(q=q, k=k, v=v, H=H, scale=scale, key_ok=key_ok, lens=lens, causal_or=causal_or, shared=shared,
                gout=rng.standard_normal((B, Tq, M)).astype(F32), shape=(B, Tq, Tk, H, hd))


def case(B, Tq, Tk, H, hd, mask="lens", causal_or=False, shared=False, seed=0, mul=1.0):
    """dict of f32 / int32 / uint8 arrays; the same arrays for the same arguments (do not write into them)."""
    return _case(B, Tq, Tk, H, hd, mask, causal_or, shared, seed, mul)


def saturated_case():
    """Inputs x 9 (scores x 81, as `autoint_oracle.saturated_case`): the exponentials underflow unless the row maximum is
    subtracted."""
    return case(7, 6, 6, 2, 8, "lens", False, False, seed=1, mul=9.0)


def all_masked_case():
    """A u8 mask whose sample 1 allows no key: |S| < 32 there, so its weights are uniform."""
    c = dict(case(4, 3, 5, 2, 8, "u8", False, False, seed=2))
    ok = c["key_ok"].copy()
    ok[1] = 0
    c["key_ok"] = ok
    return c


def slice_case(c, lo, hi):
    """Samples lo .. hi - 1 of a case as a case of their own."""
    out = dict(c)
    for name in ("q", "k", "v", "gout", "key_ok", "lens"):
        if c[name] is not None:
            out[name] = np.ascontiguousarray(c[name][lo:hi])
    if c["shared"]:
        out["v"] = out["k"]
    out["shape"] = (hi - lo,) + tuple(c["shape"][1:])
    return out


# ---- the tolerance shared by the CPU and the GPU file ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cached(args, variant):
    return run(case(*args), variant)


def oracle(c, variant, key=None):
    """The oracle's result for a case; computed once per variant for a case named by its `case(...)` arguments."""
    return _cached(key, variant) if key is not None else run(c, variant)


def check(got, c, what, key=None):
    """`got` = {out, gq, gk, gv} (numpy) of a case against the f64 oracle by the delta rule, two stages."""
    w64, w32 = oracle(c, "f64", key), oracle(c, "f32", key)
    for name in OUTPUTS:
        g = np.asarray(got[name])
        assert g.shape == w64[name].shape, (what, name, g.shape)
        bound = delta_bound(w64[name], w32[name], 2)
        gap = max_diff(g, w64[name])
        print(f"SEQATTN-FIGURE {what} {name} delta={max_diff(w32[name], w64[name]):.3e} got={gap:.3e} bound={bound:.3e}")
        assert np.isfinite(g).all() and gap <= bound, (what, name, gap, bound)
