"""CPU oracle of Caser's convolutions and of Caser's training step (csrc/caser.hip, nets/caser_net.py).

The arithmetic is the reference's, `libreco/algorithms/caser.py:177-221` with `layers/convolutional.py`: for i = 1 .. L a
`Conv1D(nh, kernel_size=i, padding="valid", activation=relu)` over the window followed by a max pool over all L - i + 1
positions, a `Conv1D(nv, kernel_size=1, activation=relu)` over the transposed window (the "vertical" layer: it mixes the L
positions per embedding channel) flattened [c][g], and relu(Dense(K)) of their concatenation; there is no sequence mask.

  conv_forward / conv_backward     numpy, "f64" or "f32" arithmetic.  The backward is hand-derived and takes the ReLU pattern
                                   (feat > 0) and the pools' `arg` as inputs: a unit within rounding of 0 and a near-tie in a
                                   pool are legitimate subgradients either way, so a result is judged against the backward of
                                   ITS OWN pattern
  NetTwin                          torch-CPU f64 autograd twin of `CaserNet.train_step` (F.conv1d, amax) with TF1 Adam
  stack_case, step_*               the seeded inputs shared by tests/test_caser_cpu.py and tests/test_caser_gpu.py
  check_caser                      the tolerance both files use: `delta_bound` of tests/wavenet_oracle.py
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from .wavenet_oracle import B1, B2, DATA, F32, delta_bound, max_diff  # noqa: F401  (DATA: the MovieLens sample)

TABLE_ROWS = 50


def _dt(variant):
    return np.float64 if variant == "f64" else F32


# ---- the convolutions, numpy -----------------------------------------------------------------------------------------
def conv_forward(x, layers, variant="f64"):
    """x [B, L, K]; `layers` = [(Wh_i [i, K, nh], bh_i [nh]) for i = 1 .. L] + [(Wv [1, L, nv], bv [nv])] ->
    (feat [B, L nh + K nv], arg int32 [B, L nh]: the smallest t that attains each maximum, zs: the post-ReLU [B, L - i + 1, nh]
    of every horizontal layer)."""
    dt = _dt(variant)
    x = x.astype(dt)
    B, L, K = x.shape
    hs, args, zs = [], [], []
    for i in range(1, L + 1):
        W, b = (v.astype(dt) for v in layers[i - 1])
        P = L - i + 1
        z = np.zeros((B, P, W.shape[2]), dtype=dt) + b
        for tau in range(i):
            z = z + x[:, tau:tau + P] @ W[tau]
        z = np.maximum(z, 0)
        zs.append(z)
        hs.append(z.max(axis=1))
        args.append(z.argmax(axis=1).astype(np.int32))
    Wv, bv = (v.astype(dt) for v in layers[L])
    v = np.maximum(np.einsum("btc,tg->bcg", x, Wv[0]) + bv, 0)
    return np.concatenate(hs + [v.reshape(B, -1)], axis=1), np.concatenate(args, axis=1), zs


def conv_backward(x, layers, pattern, arg, gfeat, variant="f64"):
    """Hand-derived backward from gfeat [B, L nh + K nv] -> (gx [B, L, K], [(gW, gb)] per layer).  `pattern` bool [B, width]:
    where ReLU passes the gradient (its derivative at 0 is 0); `arg` [B, L nh]: the position each pool's gradient goes to."""
    dt = _dt(variant)
    x = x.astype(dt)
    B, L, K = x.shape
    nh = layers[0][0].shape[2]
    g_all = gfeat.astype(dt) * pattern
    gx = np.zeros((B, L, K), dtype=dt)
    bi = np.arange(B)[:, None]
    grads = []
    for i in range(1, L + 1):
        W = layers[i - 1][0].astype(dt)
        g = g_all[:, (i - 1) * nh: i * nh]                       # [B, nh]
        a = np.asarray(arg)[:, (i - 1) * nh: i * nh].astype(np.int64)
        gW = np.zeros_like(W)
        for tau in range(i):
            gW[tau] = np.einsum("bfc,bf->cf", x[bi, a + tau], g)
            np.add.at(gx, (bi, a + tau), g[:, :, None] * W[tau].T[None])
        grads.append((gW, g.sum(0)))
    Wv = layers[L][0].astype(dt)
    gv = g_all[:, L * nh:].reshape(B, K, -1)
    grads.append((np.einsum("btc,bcg->tg", x, gv)[None], gv.sum((0, 1))))
    gx += np.einsum("bcg,tg->btc", gv, Wv[0])
    return gx, grads


# ---- seeded cases ----------------------------------------------------------------------------------------------------
# (B, L, K, nh, nv).  The tiling of csrc/caser.hip: filter tiles of 1, 2 and 4 (nh = 1, 2, more), a row stride of K rounded up
# to 4 that gains 4 more floats when that is a multiple of 8 (K = 16, 64, 128, 8 do, K = 1, 3, 20, 4 do not), 4 waves taking
# (kernel size, filter tile) items in turn (L nh / tile = 1, 2, 5, 10, 200, 64, 7, 112 items), one sample per workgroup
# below 1024 samples.  (37, 9, 5, 5, 3): two filter tiles with the second cut short, 18 items (not a multiple of 4 waves).
STACK_SHAPES = [(1, 1, 1, 1, 1), (37, 2, 3, 2, 1), (37, 10, 16, 2, 4), (300, 10, 20, 3, 4), (37, 50, 64, 16, 8), (5, 64, 8, 1, 64),
                (300, 7, 128, 4, 2), (37, 7, 16, 64, 3), (37, 9, 5, 5, 3)]
# a workgroup owns B // 512 samples: 4 (2100 = 4 * 525), 32 with the last workgroup holding 16 (16400 = 32 * 512 + 16), 2 with
# the last holding one (1025), 33 (16900: 99, 66 and 33 (sample, position) pairs per item, so a second, partly filled pass of
# the wave's 64 lanes).  The slab count is at its cap of 128: slabs of 17 samples of which the last four are empty and the
# one before holds 9 (2100), of 129 with 17 in the last (16400), of 133 with 9 in the last (16900); 65 slabs of 16 at 1025
WIDE_SHAPES = [(2100, 3, 4, 2, 2), (16400, 2, 3, 1, 1), (1025, 3, 4, 2, 2), (16900, 3, 5, 3, 2)]
# seed 0 unless named here: the only horizontal unit of the single-element case is dead at seed 0 (its gradients would all be 0)
CASE_SEEDS = {(1, 1, 1, 1, 1): 1}


def layer_shapes(L, K, nh, nv):
    return [((i, K, nh), (nh,)) for i in range(1, L + 1)] + [((1, L, nv), (nv,))]


def pack_params(layers):
    """The flat parameter buffer of `lr_caser_*`: kernel, bias, kernel, ... every tensor padded to a multiple of 4 floats."""
    out = []
    for W, b in layers:
        for t in (W, b):
            flat = np.asarray(t, dtype=F32).reshape(-1)
            out.append(np.concatenate([flat, np.zeros(-flat.size % 4, dtype=F32)]))
    return np.concatenate(out)


def unpack_params(flat, L, K, nh, nv):
    """-> ([(W, b)], the gap elements concatenated)."""
    out, gaps, off = [], [], 0
    for ks, bs in layer_shapes(L, K, nh, nv):
        pair = []
        for s in (ks, bs):
            n = int(np.prod(s))
            pair.append(flat[off:off + n].reshape(s))
            gaps.append(flat[off + n: off + n + (-n % 4)])
            off += n + (-n % 4)
        out.append(tuple(pair))
    assert off == flat.size
    return out, np.concatenate(gaps)


def stack_case(B, L, K, nh, nv, seed=None):
    """dict of f32 / int32 arrays: a table of 50 rows + the pad row (id 50, an ordinary row: it takes part), Zipf ids with
    repeats, the first windows ending in 0, 1, L - 1 and L pad ids (as many of them as B allows), weights, an upstream
    gradient for feat."""
    if seed is None:
        seed = CASE_SEEDS.get((B, L, K, nh, nv), 0)
    rng = np.random.default_rng([seed, B, L, K, nh, nv])
    V = TABLE_ROWS
    table = rng.standard_normal((V + 1, K)).astype(F32)
    ids = (rng.zipf(1.5, (B, L)) % V).astype(np.int32)
    for i, n_pad in enumerate([0, 1, L - 1, L][:B]):
        ids[i, L - n_pad:] = V
    layers = []
    for ks, bs in layer_shapes(L, K, nh, nv):
        layers.append(((rng.standard_normal(ks) / np.sqrt(ks[0] * ks[1])).astype(F32), (rng.standard_normal(bs) * 0.1).astype(F32)))
    return dict(table=table, ids=ids, V=V + 1, layers=layers, shape=(B, L, K, nh, nv), seed=seed, custom=False,
                gfeat=rng.standard_normal((B, L * nh + K * nv)).astype(F32))


def inside(c, ids=None):
    """[B, L, 1] bool: the id names a table row.  Any other id is never dereferenced: a zero input row whose gradient is 0."""
    ids = c["ids"] if ids is None else ids
    return ((ids >= 0) & (ids < c["V"]))[:, :, None]


def case_input(c, ids=None):
    """x [B, L, K]: the rows the ids name, zeros for an id outside [0, V)."""
    ids = c["ids"] if ids is None else ids
    ok = (ids >= 0) & (ids < c["V"])
    return np.where(ok[:, :, None], c["table"][np.where(ok, ids, 0)], 0).astype(F32)


@functools.lru_cache(maxsize=None)
def _cached_forward(shape, seed, variant):
    c = stack_case(*shape, seed=seed)
    return conv_forward(case_input(c), c["layers"], variant)


def forward_oracle(c, variant, ids=None):
    """The forward of a case in one arithmetic; computed once per (shape, seed, variant) for the case's own ids and weights
    (a test that edits a case sets `custom`)."""
    if ids is None and not c["custom"]:
        return _cached_forward(c["shape"], c["seed"], variant)
    return conv_forward(case_input(c, ids), c["layers"], variant)


# ---- the tolerance shared by the CPU and the GPU file ----------------------------------------------------------------
def delta_rule(got, want64, want32, what):
    """`delta_rule` of tests/wavenet_oracle.py with one layer passed through (every output of Caser's convolutions is one
    layer deep): 10 x the oracle's own f32 / f64 gap on this very case, floored at one f32 ulp of the largest value."""
    bound = delta_bound(want64, want32, 1)
    gap = max_diff(got, want64)
    print(f"CASER-FIGURE {what} delta={max_diff(want32, want64):.3e} got={gap:.3e} bound={bound:.3e}")
    assert np.isfinite(np.asarray(got)).all() and gap <= bound, what
    return bound


def check_caser(got, c, what, ids=None):
    """`got` = dict(feat [B, L nh + K nv], arg [B, L nh], gx [B, L, K], gparams (flat)) of a case.
    Forward: feat against f64 by the delta rule.  arg: the f64 value at the device's arg is within feat's bound of the f64
    maximum, and where the f64 maximum leads the runner-up by more than the bound, arg is the f64 first argmax.  Backward: gx
    and every parameter gradient against the f64 backward run with the result's own ReLU pattern and arg; the alignment gaps
    of gparams are 0; gx at ids outside the table is exactly 0."""
    B, L, K, nh, nv = c["shape"]
    x = case_input(c, ids)
    f64, arg64, z64 = forward_oracle(c, "f64", ids)
    f32, _, _ = forward_oracle(c, "f32", ids)
    feat, arg = np.asarray(got["feat"]), np.asarray(got["arg"])
    assert feat.shape == (B, L * nh + K * nv) and feat.dtype == F32
    bound = delta_rule(feat, f64, f32, f"{what} feat")
    assert arg.shape == (B, L * nh) and arg.dtype == np.int32 and (arg >= 0).all()
    bi, fi = np.meshgrid(np.arange(B), np.arange(nh), indexing="ij")
    for i in range(1, L + 1):
        sl = slice((i - 1) * nh, i * nh)
        z, a = z64[i - 1], arg[:, sl]
        assert (a <= L - i).all(), f"{what} arg range, kernel size {i}"
        assert (f64[:, sl] - z[bi, a, fi] <= bound).all(), f"{what} arg value, kernel size {i}"
        if L - i + 1 > 1:
            rest = z.copy()
            rest[bi, arg64[:, sl], fi] = -np.inf
            clear = f64[:, sl] - rest.max(axis=1) > bound
            assert np.array_equal(a[clear], arg64[:, sl][clear]), f"{what} arg, kernel size {i}"
    pattern = feat > 0
    gx64, g64 = conv_backward(x, c["layers"], pattern, arg, c["gfeat"], "f64")
    gx32, g32 = conv_backward(x, c["layers"], pattern, arg, c["gfeat"], "f32")
    delta_rule(got["gx"], gx64 * inside(c, ids), gx32 * inside(c, ids), f"{what} gx")
    assert not np.asarray(got["gx"])[~inside(c, ids)[:, :, 0]].any(), f"{what} gx at ids outside the table"
    grads, gaps = unpack_params(np.asarray(got["gparams"]), L, K, nh, nv)
    assert not gaps.any(), f"{what} gaps"
    for j in range(L + 1):
        delta_rule(grads[j][0], g64[j][0], g32[j][0], f"{what} gW[{j}]")
        delta_rule(grads[j][1], g64[j][1], g32[j][1], f"{what} gb[{j}]")


def oracle_result(c, variant, ids=None):
    """What a device run returns, from the oracle in one arithmetic (its own pattern and arg)."""
    x = case_input(c, ids)
    feat, arg, _ = forward_oracle(c, variant, ids)
    gx, grads = conv_backward(x, c["layers"], feat > 0, arg, c["gfeat"], variant)
    return dict(feat=feat.astype(F32), arg=arg, gx=(gx * inside(c, ids)).astype(F32), gparams=pack_params(grads))


# ---- the net's training step, torch f64 ------------------------------------------------------------------------------
TABLE_NAMES = ("user_embeds_var", "seq_embeds_var", "item_embeds_var", "item_bias_var")
REG_NAMES = TABLE_NAMES[:3]                  # caser.py:162-192: `item_bias_var` has no regulariser


def conv_names(L):
    return [f"conv1d{'' if i == 0 else f'_{i}'}" for i in range(L + 1)]


class NetTwin:
    """`CaserNet` in torch-CPU f64 with autograd: `weights` = {name: f32 array} of the four tables (`item_bias_var`
    [n_items, 1]) and of every dense parameter under the net's names.  TF1 Adam: the rows a batch touches (every id of the
    window, the pad id included) or, `dense`, every row, with the l2 term 2 * reg * w of `tf.keras.regularizers.l2` on the three
    embedding tables; dense parameters always whole."""

    def __init__(self, weights, L, loss, lr, epsilon=1e-5, dense=False, reg=None, norm_embed=False):
        self.w = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in weights.items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.w.items()}
        self.L, self.loss, self.lr, self.eps = L, loss, lr, epsilon
        self.dense, self.reg, self.norm_embed, self.step = dense, reg or 0.0, norm_embed, 0

    def features(self, w, seqs, pre=None, post=None):
        """-> feat [B, L nh + K nv]; `pre` (a list) collects every convolution's pre-activation, `post` the horizontal
        layers' post-ReLU [B, nh, L - i + 1]."""
        x = w["seq_embeds_var"][torch.as_tensor(np.asarray(seqs)).long()]                           # [B, L, K]
        names, out = conv_names(self.L), []
        for name in names[:-1]:
            z = F.conv1d(x.transpose(1, 2), w[f"{name}/kernel"].permute(2, 1, 0), w[f"{name}/bias"])
            if pre is not None:
                pre.append(z.detach())
            a = torch.relu(z)
            if post is not None:
                post.append(a.detach())
            out.append(a.amax(dim=2))
        z = F.conv1d(x, w[f"{names[-1]}/kernel"].permute(2, 1, 0), w[f"{names[-1]}/bias"])             # [B, nv, K]
        if pre is not None:
            pre.append(z.detach())
        out.append(torch.relu(z).transpose(1, 2).reshape(x.shape[0], -1))
        return torch.cat(out, dim=1)

    def user_vectors(self, w, users, seqs, pre=None):
        z = self.features(w, seqs, pre) @ w["dense/kernel"] + w["dense/bias"]
        if pre is not None:
            pre.append(z.detach())
        return torch.cat([w["user_embeds_var"][torch.as_tensor(np.asarray(users)).long()], torch.relu(z)], dim=1)

    def loss_of(self, w, users, seqs, items, labels):
        u = self.user_vectors(w, users, seqs)
        it = torch.as_tensor(np.asarray(items)).long()
        y = torch.tensor(np.asarray(labels), dtype=torch.float64)
        q = w["item_embeds_var"][it]
        if self.norm_embed:
            u, q = F.normalize(u, dim=1, eps=1e-12), F.normalize(q, dim=1, eps=1e-12)
        s = (u * q).sum(1) + w["item_bias_var"].view(-1)[it]
        if self.loss == "mse":
            return F.mse_loss(s, y)
        bce = F.binary_cross_entropy_with_logits(s, y, reduction="none")
        if self.loss == "focal":                                  # tfops/loss.py:56-62
            p = torch.sigmoid(s)
            bce = (y * 0.25 + (1 - y) * 0.75) * (1 - (y * p + (1 - y) * (1 - p))) ** 2.0 * bce
        return bce.mean()

    def margins(self, users, seqs):
        """(the smallest non-zero |pre-activation| of any convolution and of the Dense layer, the smallest lead of a pooled
        maximum over the values of its column that differ from it) at the current weights: how far the batch is from a
        flipped ReLU / a flipped argmax."""
        pre, post = [], []
        self.features(self.w, seqs, None, post)
        self.user_vectors(self.w, users, seqs, pre)
        z = np.abs(np.concatenate([p.numpy().reshape(-1) for p in pre]))
        lead = np.concatenate([(a.amax(dim=2, keepdim=True) - a).numpy().reshape(-1) for a in post])
        return float(z[z > 0].min()), float(lead[lead > 0].min()) if (lead > 0).any() else np.inf

    def train_step(self, users, seqs, items, labels):
        self.step += 1
        w = {k: v.clone().requires_grad_(True) for k, v in self.w.items()}
        loss = self.loss_of(w, users, seqs, items, labels)
        loss.backward()
        touched = {"user_embeds_var": np.unique(users), "seq_embeds_var": np.unique(seqs), "item_embeds_var": np.unique(items),
                   "item_bias_var": np.unique(items)}
        lr_t = self.lr * np.sqrt(1.0 - B2 ** self.step) / (1.0 - B1 ** self.step)
        for k, p in self.w.items():
            g = w[k].grad if w[k].grad is not None else torch.zeros_like(p)
            if k in TABLE_NAMES and not self.dense:
                rows = torch.as_tensor(touched[k]).long()
            else:
                rows = slice(None)
                if k in REG_NAMES and self.reg:
                    g = g + 2.0 * self.reg * p
            m, v = self.m[k], self.v[k]
            m[rows] = B1 * m[rows] + (1 - B1) * g[rows]
            v[rows] = B2 * v[rows] + (1 - B2) * g[rows] ** 2
            p[rows] = p[rows] - lr_t * m[rows] / (torch.sqrt(v[rows]) + self.eps)
        return float(loss.detach())


# ---- seeded training-step cases --------------------------------------------------------------------------------------
# small on purpose: Adam turns a flipped ReLU into an O(lr) difference, so the batches must keep every pre-activation and
# every pool lead well away from the forward's rounding (test_caser_cpu.py asserts a factor of 100), which only a net with
# few units can promise.  K, nh and nv are no multiples of 4: almost every tensor of the parameter buffer is followed by a gap.
STEP_SHAPE = dict(n_users=12, n_items=20, K=6, nh=3, nv=2, L=4, B=6, lr=0.01)
N_STEPS = 2
# (loss, dense_adam, reg, norm_embed, num_neg)
STEP_CONFIGS = [("cross_entropy", False, None, False, 0), ("focal", False, None, False, 0), ("mse", False, None, False, 0),
                ("cross_entropy", True, 0.01, False, 0), ("cross_entropy", False, None, True, 0), ("cross_entropy", False, None, False, 2)]
# the seed of the batches and weights per configuration, chosen on the CPU (tests/test_caser_cpu.py asserts the margins):
# 50 unless named here
CASER_SEEDS = {}


def step_seed(cfg):
    return CASER_SEEDS.get(tuple(cfg), 50)


def step_batches(n=N_STEPS, seed=50, num_neg=0):
    """n batches of (users, seqs [B, L] padded with the pad id n_items: windows ending in 0, 1, L - 1 and L pad ids, items,
    labels).  `num_neg` > 0: every sample is followed by that many copies of itself with a drawn item and label 0, as the
    trainer's negative sampling lays a batch out."""
    S = STEP_SHAPE
    N, L, B = S["n_items"], S["L"], S["B"]
    rng = np.random.default_rng([5, seed])
    out = []
    for _ in range(n):
        seqs = (rng.zipf(1.5, (B, L)) % N).astype(np.int32)
        for i, n_pad in enumerate([0, 1, L - 1, L]):
            seqs[i, L - n_pad:] = N
        users = (rng.zipf(1.5, B) % S["n_users"]).astype(np.int32)
        items = (rng.zipf(1.5, B) % N).astype(np.int32)
        labels = rng.integers(0, 2, B).astype(F32)
        if num_neg:
            r = 1 + num_neg
            users, seqs = np.repeat(users, r), np.repeat(seqs, r, axis=0)
            items = np.repeat(items, r)
            neg = np.arange(B * r) % r != 0
            items[neg] = rng.integers(0, N, int(neg.sum()))
            labels = np.where(neg, 0, 1).astype(F32)
        out.append(dict(users=users, seqs=seqs, items=items, labels=labels))
    return out


def step_weights(seed=50):
    """Seeded f32 weights under the net's parameter names (shared with tests/test_caser_gpu.py)."""
    S = STEP_SHAPE
    rng = np.random.default_rng([7, seed])
    N, K, nh, nv, L = S["n_items"], S["K"], S["nh"], S["nv"], S["L"]
    w = {"user_embeds_var": rng.standard_normal((S["n_users"] + 1, K)) * 0.3, "seq_embeds_var": rng.standard_normal((N + 1, K)) * 0.5,
         "item_embeds_var": rng.standard_normal((N, 2 * K)) * 0.3, "item_bias_var": rng.standard_normal((N, 1)) * 0.1}
    for name, (ks, bs) in zip(conv_names(L), layer_shapes(L, K, nh, nv)):
        w[f"{name}/kernel"] = rng.standard_normal(ks) / np.sqrt(ks[0] * ks[1]) * 1.5
        w[f"{name}/bias"] = rng.standard_normal(bs) * 0.1
    w["dense/kernel"], w["dense/bias"] = rng.standard_normal((L * nh + K * nv, K)) * 0.3, rng.standard_normal(K) * 0.1
    return {k: v.astype(F32) for k, v in w.items()}


def step_forward_bound(w, seqs):
    """The forward bound of `check_caser` measured on a step batch at the weights `w`."""
    L = STEP_SHAPE["L"]
    layers = [(np.asarray(w[f"{n}/kernel"]), np.asarray(w[f"{n}/bias"])) for n in conv_names(L)]
    x = np.asarray(w["seq_embeds_var"])[seqs]
    f64, _, _ = conv_forward(x, layers, "f64")
    f32, _, _ = conv_forward(x, layers, "f32")
    return delta_bound(f64, f32, 1)
