"""CPU oracle of the recurrent layers and of RNN4Rec (csrc/rnn.hip, layers/recurrent.py, nets/rnn_nets.py).

The arithmetic is the reference's TF2 branch, `libreco/layers/recurrent.py:27-45`: Keras `GRU` (v2, reset_after=True, gate
order z, r, h, bias [2, 3H]) and `LSTM` (gate order i, f, c, o) with `return_sequences=True` under
`tf.sequence_mask(lengths, maxlen)`, `activation=None` when a `LayerNormalization` (epsilon 1e-3) + tanh follows each layer,
and `output[:, -1, :]` as the result; the graph around it is `libreco/algorithms/rnn4rec.py:151-237`.

  layer_forward / layer_backward   numpy, "f64" or "f32" arithmetic, with the masking rule (a step t >= len, or one the caller
                                   marks invalid, carries h and c and repeats the carried h in the output), the dropout
                                   masks and the `act` flag; the backward is hand-derived
  layer_forward_torch              the same forward on torch tensors (autograd checks the hand-derived backward; the twin)
  stack_forward                    numpy stack with layer norm + tanh between the layers -> the last step's output
  NetTwin                          torch-CPU f64 autograd twin of `RNN4RecNet.train_step` with TF1 Adam
  layer_case, step_*               the seeded inputs shared by tests/test_rnn_cpu.py and tests/test_rnn_gpu.py
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32
B1, B2 = 0.9, 0.999
LN_EPS = 1e-3
DATA = os.path.join(os.path.dirname(__file__), "golden", "sample_movielens_rating.dat")
GATES = {"gru": 3, "lstm": 4}


def _dt(variant):
    return np.float64 if variant == "f64" else F32


def max_diff(a, b):
    return max(float(np.abs(np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)).max()) for x, y in zip(a, b))


def _sig(x):
    return 1 / (1 + np.exp(-x))


def valid_steps(lens, L, extra=None):
    """[B, L] bool: t < clip(len, 0, L), and `extra` (the table path: the step's id is inside the table)."""
    v = np.arange(L)[None, :] < np.clip(np.asarray(lens), 0, L)[:, None]
    return v if extra is None else v & extra


# ---- one layer, numpy ------------------------------------------------------------------------------------------------
def layer_forward(cell, x, valid, W, U, b, act=True, in_mask=None, rec_mask=None, variant="f64"):
    """-> (hs [B, L, H], cache).  `x` [B, L, D] (its values at invalid steps are never used), `valid` [B, L] bool."""
    dt = _dt(variant)
    B, L, D = x.shape
    H = U.shape[0]
    W, U, b = W.astype(dt), U.astype(dt), b.astype(dt)
    xm = np.where(valid[:, :, None], x, 0).astype(dt)
    if in_mask is not None:
        xm = xm * in_mask.astype(dt)[:, None, :]
    rm = np.ones((B, H), dtype=dt) if rec_mask is None else rec_mask.astype(dt)
    h, c = np.zeros((B, H), dtype=dt), np.zeros((B, H), dtype=dt)
    hs = np.zeros((B, L, H), dtype=dt)
    steps = []
    for t in range(L):
        v = valid[:, t, None]
        hm = h * rm
        if cell == "gru":
            mx, mh = xm[:, t] @ W + b[0], hm @ U + b[1]
            z, r = _sig(mx[:, :H] + mh[:, :H]), _sig(mx[:, H:2 * H] + mh[:, H:2 * H])
            pre = mx[:, 2 * H:] + r * mh[:, 2 * H:]
            cand = np.tanh(pre) if act else pre
            hn = z * h + (1 - z) * cand
            steps.append(dict(h_prev=h, hm=hm, z=z, r=r, cand=cand, mhh=mh[:, 2 * H:]))
        else:
            a = xm[:, t] @ W + hm @ U + b
            i, f, o = _sig(a[:, :H]), _sig(a[:, H:2 * H]), _sig(a[:, 3 * H:])
            g = np.tanh(a[:, 2 * H:3 * H]) if act else a[:, 2 * H:3 * H]
            cn = f * c + i * g
            tc = np.tanh(cn) if act else cn
            hn = o * tc
            steps.append(dict(h_prev=h, hm=hm, c_prev=c, i=i, f=f, g=g, o=o, tc=tc))
            c = np.where(v, cn, c)
        h = np.where(v, hn, h)
        hs[:, t] = h
    return hs, dict(xm=xm, rm=rm, steps=steps, valid=valid, in_mask=in_mask)


def layer_backward(cell, cache, ghs, W, U, act=True, variant="f64"):
    """Hand-derived backward of `layer_forward` -> (gx [B, L, D], gW, gU, gb); gx is exactly 0 at invalid steps."""
    dt = _dt(variant)
    W, U, ghs = W.astype(dt), U.astype(dt), ghs.astype(dt)
    xm, rm, valid = cache["xm"], cache["rm"], cache["valid"]
    B, L, D = xm.shape
    H = U.shape[0]
    G = GATES[cell]
    gx = np.zeros((B, L, D), dtype=dt)
    gW, gU = np.zeros((D, G * H), dtype=dt), np.zeros((H, G * H), dtype=dt)
    gb = np.zeros((2, G * H) if cell == "gru" else (G * H,), dtype=dt)
    dh, dc = np.zeros((B, H), dtype=dt), np.zeros((B, H), dtype=dt)
    for t in range(L - 1, -1, -1):
        s, v = cache["steps"][t], valid[:, t, None]
        g = ghs[:, t] + dh
        if cell == "gru":
            z, r, cand = s["z"], s["r"], s["cand"]
            dpre = g * (1 - z) * ((1 - cand * cand) if act else 1)
            da_z = g * (s["h_prev"] - cand) * z * (1 - z)
            da_r = dpre * s["mhh"] * r * (1 - r)
            dax = np.where(v, np.concatenate([da_z, da_r, dpre], axis=1), 0)
            dah = np.where(v, np.concatenate([da_z, da_r, dpre * r], axis=1), 0)
            direct = g * z
            gb[0] += dax.sum(0)
            gb[1] += dah.sum(0)
        else:
            i, f, gg, o, tc = s["i"], s["f"], s["g"], s["o"], s["tc"]
            dcell = dc + g * o * ((1 - tc * tc) if act else 1)
            da = np.concatenate([dcell * gg * i * (1 - i), dcell * s["c_prev"] * f * (1 - f),
                                 dcell * i * ((1 - gg * gg) if act else 1), g * tc * o * (1 - o)], axis=1)
            dax = dah = np.where(v, da, 0)
            dc = np.where(v, dcell * f, dc)
            direct = np.zeros_like(g)
            gb += dax.sum(0)
        gW += xm[:, t].T @ dax
        gU += s["hm"].T @ dah
        gxt = dax @ W.T
        if cache["in_mask"] is not None:
            gxt = gxt * cache["in_mask"].astype(dt)
        gx[:, t] = np.where(v, gxt, 0)
        dh = np.where(v, direct + (dah @ U.T) * rm, g)
    return gx, gW, gU, gb


def layer_norm(x, gamma, beta):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(LN_EPS)) * gamma.astype(x.dtype) + beta.astype(x.dtype)


def stack_forward(cell, x, valid, layers, use_ln=False, masks=None, variant="f64"):
    """`layers` = [(W, U, b) or (W, U, b, gamma, beta)] -> the last step's output [B, H_last] (`recurrent.py:30-45`)."""
    out = x
    for i, p in enumerate(layers):
        im, rm = masks[i] if masks is not None else (None, None)
        out, _ = layer_forward(cell, out, valid, p[0], p[1], p[2], not use_ln, im, rm, variant)
        if use_ln:
            out = np.tanh(layer_norm(out, p[3], p[4]))
    return out[:, -1]


# ---- one layer, torch (autograd) -------------------------------------------------------------------------------------
def layer_forward_torch(cell, x, valid, W, U, b, act=True, in_mask=None, rec_mask=None):
    """`layer_forward` on torch tensors of one dtype; `valid` a bool tensor [B, L]."""
    B, L, _ = x.shape
    H = U.shape[0]
    xm = torch.where(valid[:, :, None], x, torch.zeros_like(x))
    if in_mask is not None:
        xm = xm * in_mask[:, None, :]
    h = torch.zeros((B, H), dtype=x.dtype)
    c = torch.zeros((B, H), dtype=x.dtype)
    out = []
    for t in range(L):
        v = valid[:, t, None]
        hm = h if rec_mask is None else h * rec_mask
        if cell == "gru":
            mx, mh = xm[:, t] @ W + b[0], hm @ U + b[1]
            z, r = torch.sigmoid(mx[:, :H] + mh[:, :H]), torch.sigmoid(mx[:, H:2 * H] + mh[:, H:2 * H])
            pre = mx[:, 2 * H:] + r * mh[:, 2 * H:]
            cand = torch.tanh(pre) if act else pre
            hn = z * h + (1 - z) * cand
        else:
            a = xm[:, t] @ W + hm @ U + b
            i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
            g = torch.tanh(a[:, 2 * H:3 * H]) if act else a[:, 2 * H:3 * H]
            cn = f * c + i * g
            hn = o * (torch.tanh(cn) if act else cn)
            c = torch.where(v, cn, c)
        h = torch.where(v, hn, h)
        out.append(h)
    return torch.stack(out, dim=1)


# ---- seeded layer cases ----------------------------------------------------------------------------------------------
LAYER_SHAPES = [(1, 1, 1, 1), (37, 2, 3, 5), (37, 10, 16, 16), (300, 10, 20, 16), (37, 50, 64, 64), (37, 10, 128, 128),
                (300, 7, 16, 128), (300, 7, 128, 16)]
# batches large enough for the kernels' four-samples-per-lane form (a workgroup for every compute unit at four per lane)
WIDE_SHAPES = [(2100, 3, 4, 128), (16400, 2, 3, 16)]
TABLE_ROWS = 50


def layer_case(cell, B, L, D, H, dropout=0.0, seed=0):
    """dict of f32 / int32 arrays: a table of 50 rows + a NaN pad row and Zipf ids with repeats, lens holding L, 0, 1 and L - 1
    (as many of them as B allows) and random ones, weights, an upstream gradient for every step, and for `dropout` the two
    masks (Bernoulli(1 - p) / (1 - p))."""
    rng = np.random.default_rng([seed, B, L, D, H, GATES[cell]])
    G, V = GATES[cell], TABLE_ROWS
    table = rng.standard_normal((V + 1, D)).astype(F32)
    table[V] = np.nan                                            # the pad row: no id of the case names it
    ids = (rng.zipf(1.5, (B, L)) % V).astype(np.int32)
    lens = rng.integers(0, L + 1, B).astype(np.int32)
    lens[:4] = np.array([L, 0, 1, L - 1], dtype=np.int32)[:min(B, 4)]
    lens = np.clip(lens, 0, L)
    c = dict(table=table, ids=ids, lens=lens, V=V + 1,
             W=(rng.standard_normal((D, G * H)) / np.sqrt(D)).astype(F32),
             U=(rng.standard_normal((H, G * H)) / np.sqrt(H)).astype(F32),
             b=(rng.standard_normal((2, G * H) if cell == "gru" else (G * H,)) * 0.1).astype(F32),
             ghs=rng.standard_normal((B, L, H)).astype(F32), in_mask=None, rec_mask=None)
    if dropout:
        keep = 1.0 - dropout
        c["in_mask"] = ((rng.random((B, D)) < keep) / keep).astype(F32)
        c["rec_mask"] = ((rng.random((B, H)) < keep) / keep).astype(F32)
    return c


def layer_oracle(cell, c, act, variant, ids=None):
    """(hs, gx, gW, gU, gb) of a case in one arithmetic; `ids` replaces the case's (bad ids make their steps invalid)."""
    ids = c["ids"] if ids is None else ids
    L = ids.shape[1]
    inside = (ids >= 0) & (ids < c["V"])
    valid = valid_steps(c["lens"], L, inside)
    x = c["table"][np.where(inside, ids, 0)]
    hs, cache = layer_forward(cell, x, valid, c["W"], c["U"], c["b"], act, c["in_mask"], c["rec_mask"], variant)
    return (hs, *layer_backward(cell, cache, c["ghs"], c["W"], c["U"], act, variant))


# ---- the net's training step, torch f64 ------------------------------------------------------------------------------
def layer_param_names(cell, n_layers, use_ln):
    out = []
    for i in range(n_layers):
        sfx = "" if i == 0 else f"_{i}"
        scope = f"{cell}{sfx}/{cell}_cell{sfx}"
        names = [f"{scope}/kernel", f"{scope}/recurrent_kernel", f"{scope}/bias"]
        if use_ln:
            names += [f"layer_normalization{sfx}/gamma", f"layer_normalization{sfx}/beta"]
        out.append(names)
    return out


TABLE_NAMES = ("seq_embeds_var", "item_embeds_var", "item_bias_var")


class NetTwin:
    """`RNN4RecNet` in torch-CPU f64 with autograd: `weights` = {name: f32 array} of the three tables (`item_bias_var`
    [n_items, 1]) and of every dense parameter under the net's names.  TF1 Adam: the rows a batch touches (or, `dense`, every
    row, with the l2 term 2 * reg * w of `tf.keras.regularizers.l2` on the three tables); dense parameters always whole."""

    def __init__(self, weights, cell, n_layers, use_ln, loss, lr, epsilon=1e-5, dense=False, reg=None, norm_embed=False):
        self.w = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in weights.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.cell, self.use_ln, self.loss, self.lr, self.eps = cell, use_ln, loss, lr, epsilon
        self.dense, self.reg, self.norm_embed, self.step = dense, reg or 0.0, norm_embed, 0
        self.layers = layer_param_names(cell, n_layers, use_ln)

    def user_vectors(self, w, seqs, lens, masks=None):
        seqs, L = torch.as_tensor(np.asarray(seqs)).long(), np.asarray(seqs).shape[1]
        valid = torch.as_tensor(valid_steps(lens, L))
        out = w["seq_embeds_var"][seqs]
        for i, names in enumerate(self.layers):
            im, rm = (torch.tensor(a, dtype=torch.float64) for a in masks[i]) if masks is not None else (None, None)
            out = layer_forward_torch(self.cell, out, valid, w[names[0]], w[names[1]], w[names[2]], not self.use_ln, im, rm)
            if self.use_ln:
                out = torch.tanh(F.layer_norm(out, (out.shape[-1],), w[names[3]], w[names[4]], LN_EPS))
        return out[:, -1] @ w["dense/kernel"] + w["dense/bias"]

    def loss_of(self, w, seqs, lens, items=None, labels=None, pos=None, neg=None, masks=None):
        u = self.user_vectors(w, seqs, lens, masks)
        Q, bias = w["item_embeds_var"], w["item_bias_var"].view(-1)
        if self.loss == "bpr":                                    # rnn4rec.py:169-195 (the raw user vector, line 191)
            p, n = (torch.as_tensor(np.asarray(a)).long() for a in (pos, neg))
            qp, qn = Q[p], Q[n]
            if self.norm_embed:
                qp, qn = F.normalize(qp, dim=1, eps=1e-12), F.normalize(qn, dim=1, eps=1e-12)
            return -F.logsigmoid(bias[p] - bias[n] + (u * (qp - qn)).sum(1)).mean()
        it = torch.as_tensor(np.asarray(items)).long()
        y = torch.tensor(np.asarray(labels), dtype=torch.float64)
        q = Q[it]
        if self.norm_embed:
            u, q = F.normalize(u, dim=1, eps=1e-12), F.normalize(q, dim=1, eps=1e-12)
        s = (u * q).sum(1) + bias[it]
        if self.loss == "mse":
            return F.mse_loss(s, y)
        bce = F.binary_cross_entropy_with_logits(s, y, reduction="none")
        if self.loss == "focal":                                  # tfops/loss.py:56-62
            p = torch.sigmoid(s)
            bce = (y * 0.25 + (1 - y) * 0.75) * (1 - (y * p + (1 - y) * (1 - p))) ** 2.0 * bce
        return bce.mean()

    def train_step(self, seqs, lens, items=None, labels=None, pos=None, neg=None, masks=None):
        self.step += 1
        w = {k: v.clone().requires_grad_(True) for k, v in self.w.items()}
        loss = self.loss_of(w, seqs, lens, items, labels, pos, neg, masks)
        loss.backward()
        seqs = np.asarray(seqs)
        touched_seq = np.unique(seqs[valid_steps(lens, seqs.shape[1])])
        touched_item = np.unique(np.concatenate([np.asarray(pos), np.asarray(neg)]) if self.loss == "bpr" else np.asarray(items))
        lr_t = self.lr * np.sqrt(1.0 - B2 ** self.step) / (1.0 - B1 ** self.step)
        for k, p in self.w.items():
            g = w[k].grad if w[k].grad is not None else torch.zeros_like(p)
            if k in TABLE_NAMES and not self.dense:
                rows = torch.as_tensor(touched_seq if k == "seq_embeds_var" else touched_item).long()
            else:
                rows = slice(None)
                if k in TABLE_NAMES and self.reg:
                    g = g + 2.0 * self.reg * p
            m, v = self.m[k], self.v[k]
            m[rows] = B1 * m[rows] + (1 - B1) * g[rows]
            v[rows] = B2 * v[rows] + (1 - B2) * g[rows] ** 2
            p[rows] = p[rows] - lr_t * m[rows] / (torch.sqrt(v[rows]) + self.eps)
        return float(loss.detach())


# ---- seeded training-step cases --------------------------------------------------------------------------------------
STEP_SHAPE = dict(n_items=40, K=8, L=6, B=33, lr=0.01)
STEP_CONFIGS = [(cell, hidden, ln, loss, dense, reg)
                for cell in ("gru", "lstm") for hidden in ((16,), (16, 8)) for ln in (False, True)
                for loss in ("cross_entropy", "focal", "bpr") for dense, reg in ((False, None), (True, 0.01))]


def step_batches(loss, n=3):
    """n batches of (seqs [B, L] with the pad id n_items beyond the length, lens >= 1 holding 1 and L, a no-history row [pad],
    then items + labels or pos + neg)."""
    S = STEP_SHAPE
    N, L, B = S["n_items"], S["L"], S["B"]
    rng = np.random.default_rng(5)
    out = []
    for _ in range(n):
        lens = rng.integers(1, L + 1, B).astype(np.int32)
        lens[:3] = (1, L, 1)
        seqs = (rng.zipf(1.5, (B, L)) % N).astype(np.int32)
        seqs[np.arange(L)[None, :] >= lens[:, None]] = N
        seqs[2, 0] = N                                           # a user without history: the one-step sequence [pad]
        if loss == "bpr":
            out.append(dict(seqs=seqs, lens=lens, pos=rng.integers(0, N, B).astype(np.int32),
                            neg=rng.integers(0, N, B).astype(np.int32)))
        else:
            out.append(dict(seqs=seqs, lens=lens, items=(rng.zipf(1.5, B) % N).astype(np.int32),
                            labels=rng.integers(0, 2, B).astype(F32)))
    return out


def step_weights(cell, hidden, ln, seed=3):
    """Seeded f32 weights under the net's parameter names (shared with tests/test_rnn_gpu.py)."""
    S, G = STEP_SHAPE, GATES[cell]
    rng = np.random.default_rng(seed)
    N, K = S["n_items"], S["K"]
    w = {"seq_embeds_var": rng.standard_normal((N + 1, hidden[0])) * 0.3, "item_embeds_var": rng.standard_normal((N, K)) * 0.3,
         "item_bias_var": rng.standard_normal((N, 1)) * 0.1}
    dims = [hidden[0], *hidden]
    for names, d, h in zip(layer_param_names(cell, len(hidden), ln), dims[:-1], dims[1:]):
        w[names[0]] = rng.standard_normal((d, G * h)) / np.sqrt(d)
        w[names[1]] = rng.standard_normal((h, G * h)) / np.sqrt(h)
        w[names[2]] = rng.standard_normal((2, G * h) if cell == "gru" else (G * h,)) * 0.1
        if ln:
            w[names[3]], w[names[4]] = 1 + rng.standard_normal(h) * 0.1, rng.standard_normal(h) * 0.1
    w["dense/kernel"], w["dense/bias"] = rng.standard_normal((hidden[-1], K)) * 0.3, rng.standard_normal(K) * 0.1
    return {k: v.astype(F32) for k, v in w.items()}


# ---- the tolerance shared by the CPU and the GPU file ----------------------------------------------------------------
def delta_rule(got, want64, want32, what):
    """The project's rule for long f32 sums (`_delta_rule` of tests/test_svd_gpu.py): `got` within 10 x the oracle's own
    f32 / f64 gap on this very case, and no tighter than one f32 ulp of the largest value compared."""
    delta = max_diff([want32], [want64])
    gap = max_diff([got], [want64])
    bound = max(10 * delta, float(np.spacing(F32(np.abs(want64).max()))))
    print(f"RNN-FIGURE {what} delta={delta:.3e} got={gap:.3e} bound={bound:.3e}")
    assert gap <= bound, what


OUTPUTS = ("hs", "gx", "gW", "gU", "gb")


def check_layer(got, cell, case, act, what, ids=None):
    """`got` = (hs, gx, gW, gU, gb) of a case against its f64 oracle by the delta rule; all finite, gx exactly 0 at every
    invalid step."""
    want64, want32 = layer_oracle(cell, case, act, "f64", ids), layer_oracle(cell, case, act, "f32", ids)
    ids = case["ids"] if ids is None else ids
    valid = valid_steps(case["lens"], ids.shape[1], (ids >= 0) & (ids < case["V"]))
    for name, g, w64, w32 in zip(OUTPUTS, got, want64, want32):
        g = np.asarray(g)
        assert g.shape == w64.shape and np.isfinite(g).all(), (what, name)
        delta_rule(g, w64, w32, f"{what} {name}")
    assert not np.asarray(got[1])[~valid].any(), what
