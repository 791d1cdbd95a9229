"""CPU oracle of AutoInt's interaction stack (csrc/autoint.hip, nets/autoint_net.py).

The arithmetic is `libreco/algorithms/autoint.py:146-168` with the Keras branch of `layers/attention.py:67-101`: per layer
bias-free query / key / value projections, per head softmax((Q_h / sqrt(hd)) Kx_h^T) V_h, a bias-free output projection and an
optional residual; then Dense(1) of the flattened result.  No mask, no activation, no normalisation.

  stack_forward / stack_backward   numpy, "f64" or "f32" arithmetic; the backward is hand-derived
  pack_params / unpack_params      the flat parameter buffer of `lr_autoint_*` (the layout of `DenseParams`)
  stack_case, SHAPES               the seeded inputs shared by tests/test_autoint_cpu.py and tests/test_autoint_gpu.py
  check_stack                      the tolerance both files use: `delta_bound` of tests/wavenet_oracle.py, the project's rule
"""
from __future__ import annotations

import functools

import numpy as np

from .wavenet_oracle import delta_bound, max_diff

F32 = np.float32


def _dt(variant):
    return np.float64 if variant == "f64" else F32


def _heads(a, H):
    """[B, T, H hd] -> [B, H, T, hd]"""
    B, T, M = a.shape
    return a.reshape(B, T, H, M // H).transpose(0, 2, 1, 3)


def _merge(a):
    """[B, H, T, hd] -> [B, T, H hd]"""
    B, H, T, hd = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B, T, H * hd)


def _layer(a, layer, H, dt):
    """One attention layer on a [B, T, D] -> (Y, what the backward needs)."""
    Wq, Wk, Wv, Wo = (w.astype(dt) for w in layer)
    hd = Wq.shape[1] // H
    scale = dt(1.0 / np.sqrt(hd))
    q, k, v = _heads(a @ Wq, H) * scale, _heads(a @ Wk, H), _heads(a @ Wv, H)
    s = q @ k.transpose(0, 1, 3, 2)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    o = _merge(p @ v)
    return o @ Wo, (q, k, v, p, o, scale)


def stack_forward(x, layers, w, c, H, residual, variant="f64"):
    """x [B, T, D]; `layers` = [(Wq, Wk, Wv [D, H hd], Wo [H hd, D])]; w [T D], c scalar -> (acts: A_l of every layer, logits)."""
    dt = _dt(variant)
    a, acts = x.astype(dt), []
    for layer in layers:
        y, _ = _layer(a, layer, H, dt)
        a = a + y if residual else y
        acts.append(a)
    return acts, a.reshape(len(x), -1) @ w.astype(dt) + dt(c)


def stack_backward(x, layers, w, H, residual, glogits, variant="f64"):
    """Hand-derived backward from glogits [B] -> (gx [B, T, D], [(gWq, gWk, gWv, gWo)] per layer, gw [T D], gc)."""
    dt = _dt(variant)
    B, T, D = x.shape
    ins, a = [], x.astype(dt)
    for layer in layers:
        ins.append(a)
        y, _ = _layer(a, layer, H, dt)
        a = a + y if residual else y
    g = glogits.astype(dt)
    gw, gc = a.reshape(B, -1).T @ g, g.sum()
    da = (g[:, None] * w.astype(dt)[None, :]).reshape(B, T, D)
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        Wq, Wk, Wv, Wo = (m.astype(dt) for m in layers[l])
        a_in = ins[l]
        _, (q, k, v, p, o, scale) = _layer(a_in, layers[l], H, dt)
        flat = lambda t: t.reshape(B * T, -1)
        gWo = flat(o).T @ flat(da)
        do = _heads(da @ Wo.T, H)
        dp = do @ v.transpose(0, 1, 3, 2)
        dv = p.transpose(0, 1, 3, 2) @ do
        ds = p * (dp - (dp * p).sum(axis=-1, keepdims=True))
        dq = _merge(ds @ k) * scale                       # q is the scaled query
        dk = _merge(ds.transpose(0, 1, 3, 2) @ q)
        dv = _merge(dv)
        grads[l] = (flat(a_in).T @ flat(dq), flat(a_in).T @ flat(dk), flat(a_in).T @ flat(dv), gWo)
        prev = dq @ Wq.T + dk @ Wk.T + dv @ Wv.T
        da = prev + da if residual else prev
    return da, grads, gw, gc


# ---- the parameter buffer --------------------------------------------------------------------------------------------
def _pad(flat):
    flat = np.asarray(flat, dtype=F32).reshape(-1)
    return np.concatenate([flat, np.zeros(-flat.size % 4, dtype=F32)])


def pack_params(layers, w, c):
    """query, key, value, attention_output kernels per layer, dense/kernel, dense/bias; every tensor padded to 4 floats."""
    return np.concatenate([_pad(t) for layer in layers for t in layer] + [_pad(w), _pad([c])])


def param_shapes(T, D, H, head_dims):
    out = []
    for hd in head_dims:
        out += [(D, H * hd)] * 3 + [(H * hd, D)]
    return out + [(T * D,), (1,)]


def unpack_params(flat, T, D, H, head_dims):
    """-> ([(Wq, Wk, Wv, Wo)], w, c [1], the gap elements concatenated)."""
    ts, gaps, off = [], [], 0
    for s in param_shapes(T, D, H, head_dims):
        n = int(np.prod(s))
        ts.append(flat[off:off + n].reshape(s))
        gaps.append(flat[off + n: off + n + (-n % 4)])
        off += n + (-n % 4)
    assert off == flat.size
    n = len(head_dims)
    return [tuple(ts[4 * l:4 * l + 4]) for l in range(n)], ts[4 * n], ts[4 * n + 1], np.concatenate(gaps)


# ---- seeded cases: (B, T, D, H, head_dims, residual) -----------------------------------------------------------------
# T = 1 (a softmax of one element), T = 3, T = 17, D = 1, D = 6, hd = 1, H = 1, H hd != D, differing head dimensions, one and
# three layers, no residual, B = 1, and the envelope's corners (64 fields, width 64, 8 heads of 8, one head of 64, 8 layers)
SHAPES = [(5, 1, 6, 2, (4,), True), (7, 3, 1, 1, (1,), True), (1, 8, 16, 2, (8, 8, 8), True), (37, 17, 16, 2, (8, 8, 8), True),
          (37, 8, 16, 2, (8, 4), True), (37, 10, 6, 3, (5,), False), (3, 64, 64, 8, (8,), True), (3, 64, 64, 1, (64, 64), False),
          (2, 40, 32, 4, (8,) * 8, True)]
# batches past 2 x 512 samples, where a workgroup owns several samples: a last tile that is not full, and more tiles than the
# backward has workgroups (some of them walk over two tiles, and 512 partial slabs are reduced)
WIDE_SHAPES = [(1025, 3, 6, 2, (3,), True), (4100, 8, 16, 2, (8, 8, 8), True)]
SATURATED = (37, 8, 16, 2, (8, 8, 8), True)


def sid(s):
    return "x".join(str(v) if not isinstance(v, tuple) else "_".join(map(str, v)) for v in s)


def stack_case(B, T, D, H, head_dims, residual, seed=0, x_scale=1.0):
    """dict of f32 arrays: fields, weights of unit output variance, an upstream gradient for the logits."""
    rng = np.random.default_rng([seed, B, T, D, H, *head_dims, int(residual)])
    layers = []
    for hd in head_dims:
        M = H * hd
        layers.append(tuple((rng.standard_normal(s) / np.sqrt(s[0])).astype(F32) for s in [(D, M)] * 3 + [(M, D)]))
    return dict(x=(rng.standard_normal((B, T, D)) * x_scale).astype(F32), layers=layers,
                w=(rng.standard_normal(T * D) / np.sqrt(T * D)).astype(F32), c=F32(rng.standard_normal() * 0.1),
                glogits=rng.standard_normal(B).astype(F32), shape=(B, T, D, H, tuple(head_dims), residual), seed=seed,
                x_scale=x_scale)


def saturated_case():
    """Fields scaled by 9: the scores of the first layer (unit variance at scale 1) reach about +-80 times a few."""
    return stack_case(*SATURATED, x_scale=9.0)


@functools.lru_cache(maxsize=None)
def _cached(shape, seed, x_scale, variant):
    c = stack_case(*shape, seed=seed, x_scale=x_scale)
    _, _, _, H, _, residual = shape
    acts, logits = stack_forward(c["x"], c["layers"], c["w"], c["c"], H, residual, variant)
    gx, grads, gw, gc = stack_backward(c["x"], c["layers"], c["w"], H, residual, c["glogits"], variant)
    return dict(acts=acts, logits=logits, gx=gx, grads=grads, gw=gw, gc=gc)


def oracle(c, variant):
    """Forward and backward of a case in one arithmetic, computed once per case and variant and never changed."""
    return _cached(c["shape"], c["seed"], c["x_scale"], variant)


def oracle_result(c, variant):
    """What a device run returns, from the oracle in one arithmetic."""
    o = oracle(c, variant)
    return dict(acts=np.stack(o["acts"]), logits=o["logits"], gx=o["gx"], gparams=pack_params(o["grads"], o["gw"], o["gc"]))


# ---- the tolerance shared by the CPU and the GPU file ----------------------------------------------------------------
def delta_rule(got, want64, want32, n_layers, what):
    bound = delta_bound(want64, want32, n_layers)
    gap = max_diff(got, want64)
    print(f"AUTOINT-FIGURE {what} delta={max_diff(want32, want64):.3e} got={gap:.3e} bound={bound:.3e}")
    assert np.isfinite(np.asarray(got)).all() and gap <= bound, what
    return bound


def check_stack(got, c, what):
    """`got` = dict(acts [n, B, T, D], logits [B], gx [B, T, D], gparams (flat)) of a case: every layer of acts, the logits, gx
    and every parameter gradient against f64 by the delta rule (10 x the oracle's own f32 / f64 gap on this case, no tighter
    than one f32 ulp of the largest value per layer passed through; the read-out counts as a layer); the gaps of gparams are 0."""
    B, T, D, H, head_dims, _ = c["shape"]
    n = len(head_dims)
    o64, o32 = oracle(c, "f64"), oracle(c, "f32")
    acts = np.asarray(got["acts"])
    assert acts.shape == (n, B, T, D)
    for l in range(n):
        delta_rule(acts[l], o64["acts"][l], o32["acts"][l], l + 1, f"{what} acts[{l}]")
    delta_rule(got["logits"], o64["logits"], o32["logits"], n + 1, f"{what} logits")
    delta_rule(got["gx"], o64["gx"], o32["gx"], n + 1, f"{what} gx")
    grads, gw, gc, gaps = unpack_params(np.asarray(got["gparams"]), T, D, H, head_dims)
    assert not gaps.any(), f"{what} gaps"
    for l in range(n):
        for name, g, w64, w32 in zip(("gWq", "gWk", "gWv", "gWo"), grads[l], o64["grads"][l], o32["grads"][l]):
            delta_rule(g, w64, w32, n + 1, f"{what} {name}[{l}]")
    delta_rule(gw, o64["gw"], o32["gw"], n + 1, f"{what} gw")
    delta_rule(gc, np.asarray([o64["gc"]]), np.asarray([o32["gc"]]), n + 1, f"{what} gc")
