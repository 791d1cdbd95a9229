"""CPU oracle of the DIN attention kernels (csrc/din_attention.hip, csrc/din_mfma.hpp) and the cases that put every edge of
those kernels into every batch.

The arithmetic is `oracle/ops_np.din_attention` (layers/attention.py:28-64 of the reference) with the semantics the kernels
add at the edges, all read from their code:
  * `len` is clamped to [0, L];
  * `len == 0` gives out = 0 and attn = 0 (the reference's softmax over an all-masked row would be uniform) and the sample
    sends no gradient anywhere;
  * an id outside [0, V), in `item` or in `seq`, is a row of zeros: it still takes part in the softmax and still receives a
    gradient value (gq / gkey), which the caller drops;
  * gkey is exactly 0 at l >= len.

  forward_oracle / backward_oracle   torch (autograd) in "f64" or "f32", in chunks of at most 512 samples; the parameter
                                     gradients of the chunks are summed in f64
  case, with_bad_ids, remapped,      the seeded inputs shared by tests/test_din_cpu.py and tests/test_din_kernels_gpu.py
  clamped, sharp_case, CASES
  check                              the properties and tolerances both files use
"""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32
H = 16                                 # hidden units of the attention MLP (the reference's fixed value)
CHUNK = 512
STRIDE = 2048                          # waves of the attention kernels' persistent grid: one wave takes samples b, b + 2048, ...
EDGE_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49)
OUTPUTS = ("out", "attn", "gq", "gkey", "gW1", "gb1", "gW2", "gb2")
PER_SAMPLE_TOL = {"out": (1e-5, 2e-6), "attn": (1e-5, 1e-6), "gq": (1e-4, 1e-5), "gkey": (1e-4, 1e-5)}   # rtol, atol


def max_diff(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max()) if np.size(a) else 0.0


def clamp_lens(lens, L):
    return np.clip(np.asarray(lens), 0, L)


def valid_steps(lens, L):
    return np.arange(L)[None, :] < clamp_lens(lens, L)[:, None]


# ---- the cases -------------------------------------------------------------------------------------------------------
def len_members(L):
    """The lengths every case holds: the tile edges that fit L, and L - 1, L, L + 3 and -2 (the last two are clamped)."""
    m = [x for x in EDGE_LENS if x <= L] + [L - 1, L, L + 3, -2]
    return list(dict.fromkeys(m))


def len_cycle(L):
    """A fixed cycle of lengths that holds every member of `len_members(L)`.  Its length P is odd, hence coprime to 2,048,
    so the samples b, b + 2048, b + 4096 that one forward wave takes run through different combinations: stepping the cycle
    by 2048 % P visits every position.  Laid out ALONG that orbit, so that these successions occur (wave-wise, sample b then
    b + 2048):  full length -> len 0,  len 0 -> full length (L + 3, clamped),  len 1 -> a length above 16 (L, where L > 16)."""
    members = len_members(L)
    chain = [L, 0, L + 3, 1, L] + [x for x in members if x not in (L, 0, L + 3, 1)]
    if len(chain) % 2 == 0:
        chain.append(L - 1)
    P = len(chain)
    d = STRIDE % P
    cyc = [None] * P
    for k, x in enumerate(chain):
        cyc[(k * d) % P] = x
    assert None not in cyc and set(cyc) == set(members)
    return cyc


def successions(lens, L, stride=STRIDE):
    """{(kind of sample b, kind of sample b + stride)} over the batch; kinds: 'zero', 'one', 'full', 'gt16', 'other'."""
    n = clamp_lens(lens, L)

    def kinds(x):
        k = {"zero"} if x == 0 else ({"one"} if x == 1 else set())
        if x == L:
            k.add("full")
        if x > 16:
            k.add("gt16")
        return k or {"other"}

    out = set()
    for b in range(len(n) - stride):
        out |= {(a, c) for a in kinds(n[b]) for c in kinds(n[b + stride])}
    return out


def case(B, L, K, V=None, seed=0, lens=None, table_scale=0.5, name=None):
    """dict of f32 / int32 arrays.  The table has V rows; rows 0 and V - 1 are NaN and no valid position names them; valid
    ids are Zipf-like with repeats from [1, V - 2].  Every position l >= len holds id V - 1, so a single masked row that reaches
    arithmetic turns the output NaN — row 0 too, which the MFMA kernels read as the stand-in of a masked row.  `lens` follows
    `len_cycle(L)` (or is given)."""
    V = V or 61
    rng = np.random.default_rng([seed, B, L, K])
    table = (rng.standard_normal((V, K)) * table_scale).astype(F32)
    table[0] = np.nan
    table[V - 1] = np.nan
    if lens is None:
        cyc = len_cycle(L)
        lens = np.array([cyc[b % len(cyc)] for b in range(B)], dtype=np.int32)
    lens = np.asarray(lens, dtype=np.int32)
    assert lens.shape == (B,)
    item = (1 + rng.zipf(1.3, B) % (V - 2)).astype(np.int32)
    seq = (1 + rng.zipf(1.3, (B, L)) % (V - 2)).astype(np.int32)
    seq[~valid_steps(lens, L)] = V - 1
    return dict(name=name or f"B{B}-L{L}-K{K}", B=B, L=L, K=K, V=V, table=table, item=item, seq=seq, lens=lens,
                W1=(rng.standard_normal((4 * K, H)) / np.sqrt(4 * K)).astype(F32),
                b1=(rng.standard_normal(H) * 0.1).astype(F32),
                W2=(rng.standard_normal((H, 1)) * 0.5).astype(F32),
                b2=(rng.standard_normal(1) * 0.1).astype(F32),
                gout=rng.standard_normal((B, K)).astype(F32), sharp=False, bad={})


def with_bad_ids(c, seq_steps=(0, 16, 17)):
    """A copy with ids outside [0, V):  item[b] = -1 for one b in the first wave trip (b < 2048 where the batch has a second
    trip, else the first half), item[b] = V + 5 for one b of a later trip (a query the previous sample's last tile
    prefetches), and for each l of `seq_steps` that fits one seq[b, l] at a VALID step of a sample of a later trip, all on
    different samples.  `bad` = {"item": [b, b], "seq": [(b, l), ...]}."""
    B, L, V = c["B"], c["L"], c["V"]
    half = STRIDE if B > STRIDE else B // 2
    n = clamp_lens(c["lens"], L)
    d = dict(c, item=c["item"].copy(), seq=c["seq"].copy(), name=c["name"] + "-bad")
    lo = next(b for b in range(3, half) if n[b] > 0)
    hi = next(b for b in range(half + 3, B) if n[b] > 0)
    d["item"][lo], d["item"][hi] = -1, V + 5
    used, bad_seq = {lo, hi}, []
    for l in seq_steps:
        if l >= L:
            continue
        b = next(b for b in range(half, B) if n[b] > l and b not in used)
        used.add(b)
        d["seq"][b, l] = -7 if l % 2 else V
        bad_seq.append((b, l))
    d["bad"] = {"item": [lo, hi], "seq": bad_seq}
    return d


def remapped(c):
    """The bad-id case with a row of zeros appended to the table and every bad id renamed to it: the same mathematics."""
    V = c["V"]
    table = np.concatenate([c["table"], np.zeros((1, c["K"]), F32)])
    item, seq = c["item"].copy(), c["seq"].copy()
    item[(item < 0) | (item >= V)] = V
    seq[(seq < 0) | (seq >= V)] = V
    return dict(c, table=table, item=item, seq=seq, V=V + 1, name=c["name"] + "-remapped")


def clamped(c):
    return dict(c, lens=clamp_lens(c["lens"], c["L"]).astype(np.int32), name=c["name"] + "-clamped")


def scores64(c):
    """The f64 scores after the 1 / sqrt(K) scaling, NaN at l >= len."""
    q, keys, valid = gathered(c)
    q, keys = q.astype(np.float64), np.where(valid[:, :, None], keys, 0).astype(np.float64)
    qt = np.broadcast_to(q[:, None, :], keys.shape)
    z = np.concatenate([qt, keys, qt - keys, qt * keys], axis=2) @ c["W1"].astype(np.float64) + c["b1"]
    s = ((1 / (1 + np.exp(-z))) @ c["W2"].astype(np.float64).reshape(-1) + float(c["b2"][0])) / np.sqrt(c["K"])
    return np.where(valid, s, np.nan)


SHARP_SPAN = 160.0
EXP_UNDERFLOW = 88.0                   # exp(-88) is below the smallest normal f32


def tile_steps(c):
    """(up, down): the numbers of (sample, key) pairs whose f64 score lies more than `EXP_UNDERFLOW` above / below the score
    16 keys earlier — one lane's consecutive keys in the MFMA forward, on the two sides of a tile boundary.  Up: the rescale
    exp(m - m_new) of the running sums underflows; down: the new key's own term exp(s - m) does."""
    s = scores64(c)
    d = s[:, 16:] - s[:, :-16]
    return int(np.nansum(d > EXP_UNDERFLOW)), int(np.nansum(d < -EXP_UNDERFLOW))


def sharp_case(B, L, K, seed=0):
    """Sharp logits: W2 is scaled until the f64 scores of the widest sample span `SHARP_SPAN` (> 100) after the 1 / sqrt(K)
    scaling, so the online softmax's rescale exp(m - m_new) underflows to 0 on both sides of a tile boundary (`tile_steps`); the
    table is louder (2.0) so the hidden units saturate differently from key to key and the scaling stays moderate.  The samples
    `ties` (four with at least two keys, of different lengths where the cycle has them) repeat ONE id over all their valid
    steps: their attention is uniform, 1 / len."""
    c = case(B, L, K, seed=seed, table_scale=2.0, name=f"sharp-B{B}-L{L}-K{K}")
    n = clamp_lens(c["lens"], L)
    c["ties"] = [b for b in range(B) if n[b] >= 2][1::7][:4]
    assert len(c["ties"]) == 4
    for b in c["ties"]:
        c["seq"][b, :n[b]] = c["seq"][b, 0]
    s = scores64(c)
    span = np.nanmax(np.where(np.isnan(s), -np.inf, s), axis=1) - np.nanmin(np.where(np.isnan(s), np.inf, s), axis=1)
    span = span[clamp_lens(c["lens"], L) > 0]
    c["W2"] = (c["W2"] * (SHARP_SPAN / span.max())).astype(F32)
    c["sharp"] = True
    return c


def gathered(c):
    """(q [B, K], keys [B, L, K], valid [B, L]) as the dense entry points take them: rows gathered on the host, a row of zeros
    for an id outside [0, V); positions l >= len keep what the table holds there (NaN: the pad id names a NaN row)."""
    V, L = c["V"], c["L"]
    okq = (c["item"] >= 0) & (c["item"] < V)
    oks = (c["seq"] >= 0) & (c["seq"] < V)
    q = np.where(okq[:, None], c["table"][np.where(okq, c["item"], 1)], 0).astype(F32)
    keys = np.where(oks[:, :, None], c["table"][np.where(oks, c["seq"], 1)], 0).astype(F32)
    return q, keys, valid_steps(c["lens"], L)


def _cases():
    out = {}
    for L in (1, 15, 16, 17, 32, 33, 49):                                   # group 1: tile edges, one sample per wave
        for K in (16, 32, 64, 128):
            out[f"edge-L{L}-K{K}"] = lambda L=L, K=K: case(45, L, K, seed=1, name=f"edge-L{L}-K{K}")
    for K in (16, 32, 64, 128):                                             # group 2: waves that take two and three samples
        out[f"trips-L18-K{K}"] = lambda K=K: case(4133, 18, K, seed=2, name=f"trips-L18-K{K}")
    out["trips-L50-K64"] = lambda: case(4133, 50, 64, seed=2, name="trips-L50-K64")
    for K in (16, 128):                                                     # group 3: bad ids
        out[f"bad-L18-K{K}"] = lambda K=K: with_bad_ids(case(4133, 18, K, seed=2, name=f"trips-L18-K{K}"))
    for L in (2049, 2100):                                                  # group 4: the shuffle path
        for K in (16, 32, 64):
            out[f"long-L{L}-K{K}"] = lambda L=L, K=K: long_case(L, K)
    for K in (16, 128):                                                     # group 6: sharp logits and ties
        out[f"sharp-L33-K{K}"] = lambda K=K: sharp_case(45, 33, K, seed=6)
    return out


def long_case(L, K, B=9, seed=4):
    """The shuffle kernels' case (L > 2048): lens 0, 1, 2048, 2049, L, L + 3, -2, 17 and L - 1, one bad id at a valid step."""
    lens = [0, 1, 2048, 2049, L, L + 3, -2, 17, L - 1][:B]
    c = case(B, L, K, seed=seed, lens=lens, name=f"long-L{L}-K{K}")
    c["seq"][4, 2047] = c["V"] + 1
    c["item"][7] = -3
    c["bad"] = {"item": [7], "seq": [(4, 2047)]}
    return c


def limit_case(K, L):
    """Two samples at a sequence length where a dispatcher stops: a full one and one a key short, a bad id in the last tile."""
    c = case(2, L, K, seed=5, lens=[L, L - 1], name=f"limit-L{L}-K{K}")
    c["seq"][0, L - 2] = -1
    c["bad"] = {"item": [], "seq": [(0, L - 2)]}
    return c


def max_len(din_path, K, backward, start=2048, stop=20000):
    """The largest L one dispatcher accepts at width K, READ from the library's predicate (`ops.din_path`): the region is an
    interval of L, walked upward from the MFMA kernels' limit."""
    L = start
    while L < stop and din_path(K, L + 1, backward) != 0:
        L += 1
    return L


CASES = _cases()                     # name -> builder (both test files take their cases from here)
_BUILT: dict = {}
_ORACLES: dict = {}


def get_case(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _chunk_forward(c, lo, hi, dt):
    """torch forward of samples [lo, hi) in dtype `dt` -> (out, attn, q leaf, keys leaf, parameter leaves)."""
    q, keys, valid = gathered(dict(c, item=c["item"][lo:hi], seq=c["seq"][lo:hi], lens=c["lens"][lo:hi]))
    L, K = c["L"], c["K"]
    n = clamp_lens(c["lens"][lo:hi], L)
    keys = np.where(valid[:, :, None], keys, 0)                  # a masked position never reaches arithmetic
    q = torch.tensor(q, dtype=dt, requires_grad=True)
    keys = torch.tensor(keys, dtype=dt, requires_grad=True)
    P = [torch.tensor(c[k], dtype=dt, requires_grad=True) for k in ("W1", "b1", "W2", "b2")]
    qt = q[:, None, :].expand(-1, L, -1)
    cross = torch.cat([qt, keys, qt - keys, qt * keys], dim=2)              # attention.py:47-49
    h = torch.sigmoid(cross @ P[0] + P[1])
    s = (h @ P[2]).reshape(hi - lo, L) + P[3]
    s = s * torch.tensor(1.0 / np.sqrt(np.asarray(K, dtype=np.float64)), dtype=dt)      # attention.py:58
    mask = torch.from_numpy(valid)
    s = torch.where(mask, s, torch.full_like(s, -(2.0 ** 32) + 1))          # attention.py:59-60
    a = torch.softmax(s, dim=1) * torch.tensor((n > 0).astype(np.float64), dtype=dt)[:, None]   # len == 0: no attention
    # (a reduction, not a matrix product: torch sums a reduced axis in a cascade, so the f32 variant's error over the up to
    # 9,216 keys of the longest cases stays a few ulps on any machine; a BLAS product's depends on its blocking and threads)
    out = (a[:, :, None] * keys).sum(1)
    return out, a, q, keys, P


def backward_oracle(c, variant="f64", chunk=CHUNK):
    """-> (out, attn, gq, gkey, gW1, gb1, gW2, gb2) as f64 arrays (values of `variant` arithmetic)."""
    dt = torch.float64 if variant == "f64" else torch.float32
    B = c["B"]
    per = [[], [], [], []]
    gp = [np.zeros(c[k].shape, np.float64) for k in ("W1", "b1", "W2", "b2")]
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        out, a, q, keys, P = _chunk_forward(c, lo, hi, dt)
        out.backward(torch.tensor(c["gout"][lo:hi], dtype=dt))
        for dst, x in zip(per, (out.detach(), a.detach(), q.grad, keys.grad)):
            dst.append(x.numpy().astype(np.float64))
        for g, p in zip(gp, P):
            g += p.grad.numpy().astype(np.float64)
    return tuple(np.concatenate(x) for x in per) + tuple(gp)


def forward_oracle(c, variant="f64", chunk=CHUNK):
    """-> (out, attn) as f64 arrays."""
    dt = torch.float64 if variant == "f64" else torch.float32
    outs, attns = [], []
    with torch.no_grad():
        for lo in range(0, c["B"], chunk):
            out, a, *_ = _chunk_forward(c, lo, min(c["B"], lo + chunk), dt)
            outs.append(out.numpy().astype(np.float64))
            attns.append(a.numpy().astype(np.float64))
    return np.concatenate(outs), np.concatenate(attns)


def oracles(c):
    """{"f64": dict, "f32": dict} of a case's eight outputs, computed once per case name and left unchanged."""
    key = c["name"]
    if key not in _ORACLES:
        _ORACLES[key] = {v: dict(zip(OUTPUTS, backward_oracle(c, v))) for v in ("f64", "f32")}
        for v in _ORACLES[key].values():
            for a in v.values():
                a.setflags(write=False)
    return _ORACLES[key]


# ---- the properties and tolerances shared by the CPU and the GPU file -----------------------------------------------
def _bound(name, want64, want32, sharp):
    """Elementwise bound of |got - want64| and the f32 oracle's own gap `delta`.
    Per-sample outputs: the project's fixed figures (tests/test_din_gpu.py).  Parameter gradients are sums over B x L terms:
    the larger of that file's atol = 1e-4 * max(1, |want|max) with rtol 1e-4 and the delta rule (`delta_rule` of
    tests/rnn_oracle.py), 10 x the f32 oracle's own gap to f64 on this very case.
    The sharp-logit case takes the delta rule for every output, with the fixed figures as the floor: its W2 is in the
    hundreds, the scores reach ~100 where one f32 ulp is 8e-6, and the f32 oracle itself then stands 1e-5 (out) and 1e-4 to
    3e-4 (gq, gkey) from f64 — f32 arithmetic cannot meet the fixed figures there, so the reference's own error sets the bar."""
    delta = max_diff(want32, want64)
    if name in PER_SAMPLE_TOL:
        rtol, atol = PER_SAMPLE_TOL[name]
        bound = atol + rtol * np.abs(want64)
        if sharp:
            bound = np.maximum(bound, 10 * delta)
    else:
        bound = 1e-4 * max(1.0, float(np.abs(want64).max())) + 1e-4 * np.abs(want64)
        bound = np.maximum(bound, 10 * delta)
    return bound, delta


def check(got, c, what):
    """`got` = {output name: array} (any subset of OUTPUTS) of case `c` against its f64 oracle: everything finite; attn and
    gkey exactly 0 at l >= clamp(len); rows of attn sum to 1, or to 0 for len == 0; then the tolerances of `_bound`, one
    DIN-FIGURE line per output (delta = the f32 oracle's own largest gap, got / bound = the gap and the bound at the element
    nearest to its bound)."""
    o = oracles(c)
    L = c["L"]
    n = clamp_lens(c["lens"], L)
    pad = ~valid_steps(c["lens"], L)
    for name, g in got.items():
        g = np.asarray(g, dtype=np.float64).reshape(o["f64"][name].shape)
        assert np.isfinite(g).all(), f"{what} {name}: not finite"
        if name == "attn":
            assert not g[pad].any(), f"{what} attn: not 0 past the length"
            # (the weights are exp(s_l - max) / den with den the f32 sum of the same L exponentials: whatever the scores'
            # own error, the row misses 1 only by the roundings of that sum, L half-ulps at the worst, and by the few ulps of
            # exp, the reciprocal and the product in every weight — 8 ulps.  Half an ulp of a SCORE near 190, 8e-6, is
            # outside it at every L below 250: that is what a denominator formed from other scores than the weights shows.)
            np.testing.assert_allclose(g.sum(1), (n > 0).astype(np.float64), rtol=0, atol=(8 + L / 2) * 2.0 ** -24,
                                       err_msg=f"{what} attn rows")
        if name == "gkey":
            assert not g[pad].any(), f"{what} gkey: not 0 past the length"
    failed = []
    for name, g in got.items():
        want64, want32 = o["f64"][name], o["f32"][name]
        g = np.asarray(g, dtype=np.float64).reshape(want64.shape)
        bound, delta = _bound(name, want64, want32, c["sharp"])
        err = np.abs(g - want64)
        at = np.unravel_index(np.argmax(err / bound), err.shape)         # the element nearest to (or furthest past) its bound
        print(f"DIN-FIGURE {what} {name} delta={delta:.3e} got={err[at]:.3e} bound={float(np.broadcast_to(bound, err.shape)[at]):.3e}")
        if not (err <= bound).all():
            failed.append(name)
    assert not failed, f"{what}: {failed} outside their bounds"
